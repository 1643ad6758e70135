// Device-side helpers shared by the kernel files (wave64 reductions, first-index argmin keys, row dot).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"

#include <mutex>
#include <set>
#include <utility>

namespace gomilp {

// Raise a kernel's dynamic-LDS limit once per (device, kernel): the attribute is per device, and launches come from many host
// threads (flat contexts, pool workers, the two batch schedules).
inline void lds_attr_once(const void *fn, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<int, const void *>> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(mu);
    if (done.insert(std::make_pair(dev, fn)).second) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// workgroups for a wave-per-row kernel over `rows` rows (at most kMaxPartials: one argmin partial per workgroup)
static inline int grid_for_rows(int rows) {
    int g = (rows + kWavesPerBlock - 1) / kWavesPerBlock;
    if (g > kMaxPartials) g = kMaxPartials;
    if (g < 1) g = 1;
    return g;
}

// ------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------

// Order-preserving map double -> u64 for floats.MinIdx semantics (floats/floats.go:458-474):
// NaN never wins (largest key), -0 == +0, ties resolved by the smaller index.
__device__ __forceinline__ unsigned long long ordkey(double v) {
    if (v != v) return ~0ull;
    v = v + 0.0;  // -0 -> +0
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// inverse of ordkey (exact; -0 comes back as +0, NaN as NaN)
__device__ __forceinline__ double orddecode(unsigned long long k) {
    if (k == ~0ull) return __builtin_nan("");
    const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double((long long)b);
}

__device__ __forceinline__ void amin_take(unsigned long long &k, unsigned int &i, unsigned long long k2,
                                          unsigned int i2) {
    if (k2 < k || (k2 == k && i2 < i)) { k = k2; i = i2; }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void wave_argmin(unsigned long long &k, unsigned int &i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long k2 = __shfl_xor(k, o, 64);
        unsigned int i2 = __shfl_xor(i, o, 64);
        amin_take(k, i, k2, i2);
    }
}

// argmin over the 4 waves of a 256-thread workgroup; result valid in every thread
__device__ __forceinline__ void block_argmin(unsigned long long &k, unsigned int &i, unsigned long long *sk,
                                             unsigned int *si) {
    wave_argmin(k, i);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sk[w] = k; si[w] = i; }
    __syncthreads();
    k = sk[0]; i = si[0];
#pragma unroll
    for (int t = 1; t < kWavesPerBlock; t++) amin_take(k, i, sk[t], si[t]);
    __syncthreads();
}

// reduce the per-workgroup partials of the previous kernel (every workgroup does it redundantly:
// <= 1024 entries out of L2, cheaper than another kernel boundary)
__device__ __forceinline__ unsigned int reduce_partials(const unsigned long long *pk, const unsigned int *pi,
                                                        int nparts, unsigned long long *sk, unsigned int *si,
                                                        unsigned long long *key_out) {
    unsigned long long k = ~0ull;
    unsigned int i = 0xFFFFFFFFu;
    for (int t = threadIdx.x; t < nparts; t += kBlock) amin_take(k, i, pk[t], pi[t]);
    block_argmin(k, i, sk, si);
    if (key_out) *key_out = k;
    return i;
}

// Guard mode of the revised-simplex kernels (LPArgs::guard): the first-index argmin and, beside it, the second smallest key of the
// same set (an exact tie: the minimum twice).  (k2, i2, s2): the winner and runner-up of another set (~0ull: none).  The same
// winning index on both sides is the same element (the lanes of a wave carry identical copies of their wave's winner): no tie.
__device__ __forceinline__ void amin2_take(unsigned long long &k, unsigned int &i, unsigned long long &s, unsigned long long k2,
                                           unsigned int i2, unsigned long long s2) {
    s = s2 < s ? s2 : s;
    if (i2 == i) return;
    const bool take = k2 < k || (k2 == k && i2 < i);
    const unsigned long long lose = take ? k : k2;
    s = lose < s ? lose : s;
    if (take) { k = k2; i = i2; }
}

// block_argmin with the runner-up key; result valid in every thread
__device__ __forceinline__ void block_argmin2(unsigned long long &k, unsigned int &i, unsigned long long &s, unsigned long long *sk,
                                              unsigned int *si, unsigned long long *ss) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long k2 = __shfl_xor(k, o, 64), s2 = __shfl_xor(s, o, 64);
        const unsigned int i2 = __shfl_xor(i, o, 64);
        amin2_take(k, i, s, k2, i2, s2);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sk[w] = k; si[w] = i; ss[w] = s; }
    __syncthreads();
    k = sk[0]; i = si[0]; s = ss[0];
#pragma unroll
    for (int t = 1; t < kWavesPerBlock; t++) amin2_take(k, i, s, sk[t], si[t], ss[t]);
    __syncthreads();
}

// reduce_partials with the runner-up key (pk2: the workgroups' runner-up keys)
__device__ __forceinline__ unsigned int reduce_partials2(const unsigned long long *pk, const unsigned int *pi, const unsigned long long *pk2,
                                                         int nparts, unsigned long long *sk, unsigned int *si, unsigned long long *ss,
                                                         unsigned long long *key_out, unsigned long long *key2_out) {
    unsigned long long k = ~0ull, s = ~0ull;
    unsigned int i = 0xFFFFFFFFu;
    for (int t = threadIdx.x; t < nparts; t += kBlock) amin2_take(k, i, s, pk[t], pi[t], pk2[t]);
    block_argmin2(k, i, s, sk, si, ss);
    *key_out = k; *key2_out = s;
    return i;
}

// argmin with two payload words travelling with the winner (fused pipeline: saves the dependent
// global loads that would otherwise follow the reduction)
struct ArgMinP {
    unsigned long long k;
    unsigned int i;
    unsigned int u;  // payload: variable id
    double d;        // payload: d'_i
};
__device__ __forceinline__ void aminp_take(ArgMinP &a, const ArgMinP &b) {
    if (b.k < a.k || (b.k == a.k && b.i < a.i)) a = b;
}
__device__ __forceinline__ void wave_argminp(ArgMinP &a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ArgMinP b;
        b.k = __shfl_xor(a.k, o, 64); b.i = __shfl_xor(a.i, o, 64); b.u = __shfl_xor(a.u, o, 64); b.d = __shfl_xor(a.d, o, 64);
        aminp_take(a, b);
    }
}
__device__ __forceinline__ void block_argminp(ArgMinP &a, ArgMinP *sm) {
    wave_argminp(a);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sm[w] = a;
    __syncthreads();
    a = sm[0];
#pragma unroll
    for (int t = 1; t < kWavesPerBlock; t++) aminp_take(a, sm[t]);
    __syncthreads();
}

// ---- (key, index) candidates and DPP reductions for the single-workgroup kernels (bt_kernels.hip, lu_compressed.hip)
struct BtCand {   // (sort key, index): payloads (pivot element, x_B[p]) are published through LDS by the owner of the
    unsigned long long k;   // winning row after the reduction, so the reduction moves 3 dwords instead of 5
    unsigned int i;
};
__device__ __forceinline__ void bt_take(BtCand &a, const BtCand &b) {
    if (b.k < a.k || (b.k == a.k && b.i < a.i)) a = b;
}
// ---- DPP reductions.  A ds_bpermute-based __shfl_xor butterfly costs ~400 cycles per round (5 dwords through the
// LDS crossbar); the two workgroup-wide argmins per pivot were 2/3 of the inner kernel's time.  DPP row shifts are
// plain VALU moves: 4 row_shr steps leave each 16-lane row's result in its last lane, v_readlane combines the rows.
template <int CTRL>
__device__ __forceinline__ unsigned int dpp_u32(unsigned int v) {
    return (unsigned int)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);  // lanes without a source keep v
}
template <int CTRL>
__device__ __forceinline__ BtCand dpp_cand(const BtCand &a) {
    BtCand b;
    const unsigned int klo = dpp_u32<CTRL>((unsigned int)a.k), khi = dpp_u32<CTRL>((unsigned int)(a.k >> 32));
    b.k = ((unsigned long long)khi << 32) | klo;
    b.i = dpp_u32<CTRL>(a.i);
    return b;
}
__device__ __forceinline__ BtCand readlane_cand(const BtCand &a, int lane) {
    BtCand b;
    const unsigned int klo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)a.k, lane);
    const unsigned int khi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(a.k >> 32), lane);
    b.k = ((unsigned long long)khi << 32) | klo;
    b.i = (unsigned int)__builtin_amdgcn_readlane((int)a.i, lane);
    return b;
}
// reduce within each row of 16 lanes: afterwards lane 15 of every row holds that row's argmin
__device__ __forceinline__ void row_argmin(BtCand &a) {
    bt_take(a, dpp_cand<0x111>(a));  // row_shr:1
    bt_take(a, dpp_cand<0x112>(a));  // row_shr:2
    bt_take(a, dpp_cand<0x114>(a));  // row_shr:4
    bt_take(a, dpp_cand<0x118>(a));  // row_shr:8
}
// argmin over the whole 1024-thread workgroup; result (uniform) in every thread.  `sm` is double buffered by the
// caller (sm + 16*parity) so that one barrier per reduction is enough.
template <int NW>
__device__ __forceinline__ void bt_block_argmin(BtCand &a, BtCand *sm) {
    row_argmin(a);
    BtCand w = readlane_cand(a, 15);
    bt_take(w, readlane_cand(a, 31));
    bt_take(w, readlane_cand(a, 47));
    bt_take(w, readlane_cand(a, 63));
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) sm[wv] = w;
    __syncthreads();
    BtCand c;
    c.k = ~0ull; c.i = 0xFFFFFFFFu;
    if (lane < NW) c = sm[lane];
    row_argmin(c);  // NW <= 16: one row
    a = readlane_cand(c, 15);
}

// ---- value reductions without index payloads (bt_kernels.hip k_bt_inner2, lu_compressed.hip k_luc_panel)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned int lo = dpp_u32<CTRL>((unsigned int)b), hi = dpp_u32<CTRL>((unsigned int)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)b, lane);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// v_min_f64 directly: minnum semantics in hardware (a NaN operand loses); __builtin_fmin would add a v_max_f64 x,x
// canonicalisation per operand, doubling the instruction count of the reductions
__device__ __forceinline__ double vmin_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// min over each 16-lane row (NaN operands lose: minnum)
// rotations (row_ror) have a source in every lane, so the DPP move needs no `old` operand (one v_mov less per
// dword and step than row_shr with old = own value); afterwards EVERY lane of a row holds the row's minimum
template <int CTRL>
__device__ __forceinline__ unsigned int ror_u32(unsigned int v) {
    return (unsigned int)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ double ror_f64(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned int lo = ror_u32<CTRL>((unsigned int)b), hi = ror_u32<CTRL>((unsigned int)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double row_min_f64(double x) {
    x = vmin_f64(x, ror_f64<0x121>(x));  // row_ror:1
    x = vmin_f64(x, ror_f64<0x122>(x));  // row_ror:2
    x = vmin_f64(x, ror_f64<0x124>(x));  // row_ror:4
    x = vmin_f64(x, ror_f64<0x128>(x));  // row_ror:8
    return x;
}
// rows combined with the gfx9 broadcast forms of DPP instead of 4 x v_readlane pairs: row_bcast15 hands lane 15 of a row to
// the next row (row_mask 0xA: rows 1 and 3 take it), row_bcast31 hands lane 31 to rows 2 and 3 (row_mask 0xC); lane 63 then
// holds the minimum of the wave — 6 VALU + 2 v_readlane instead of 19 instructions
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double bcast_f64(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned int lo = (unsigned int)__builtin_amdgcn_update_dpp((int)(unsigned int)b, (int)(unsigned int)b, CTRL, ROWMASK, 0xF, false);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_update_dpp((int)(unsigned int)(b >> 32), (int)(unsigned int)(b >> 32), CTRL, ROWMASK, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double wave_min_f64(double x) {
    x = row_min_f64(x);                               // every lane of a row holds the row's minimum
    x = vmin_f64(x, bcast_f64<0x142, 0xA>(x));        // row_bcast:15 -> rows 1, 3: min(r0, r1), min(r2, r3)
    x = vmin_f64(x, bcast_f64<0x143, 0xC>(x));        // row_bcast:31 -> rows 2, 3: row 3 = min of the wave
    return readlane_f64(x, 63);
}
__device__ __forceinline__ unsigned int row_min_u32(unsigned int x) {
    x = min(x, ror_u32<0x121>(x));
    x = min(x, ror_u32<0x122>(x));
    x = min(x, ror_u32<0x124>(x));
    x = min(x, ror_u32<0x128>(x));
    return x;
}

// x / d for d > 0 and operands in the normal range (|x| / d far from overflow and underflow: ratios of the ratio test):
// reciprocal + two Newton steps + one residual correction — the instruction sequence of the compiler's IEEE division without
// its scaling and fix-up stages (8 instead of 13 instructions), the same correctly rounded quotient where those stages are idle
__device__ __forceinline__ double div_pos(double x, double d) {
    double r = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    double q = x * r;
    const double rem = __builtin_fma(-d, q, x);
    return __builtin_fma(rem, r, q);
}

// element (i, j) of the tableau T in either layout: row-major, or the 4x4 tiles of the blocked pipeline (bt_kernels.hip:
// tile (I, J) at ((I * ldt/4) + J) * 16, element (i&3)*4 + (j&3))
__device__ __forceinline__ size_t tab_idx(int i, int j, int ldt, int tiled) {
    return tiled ? ((size_t)(i >> 2) * (size_t)(ldt >> 2) + (size_t)(j >> 2)) * 16u + (size_t)(((i & 3) << 2) + (j & 3))
                 : (size_t)i * ldt + j;
}

// ------------------------------------------------------------------------------------------------
// Row dot products against LDS-staged vectors.  Rows and vectors come through loaders: load2(c) gives double2 c of a padded row
// (ld2 double2, 16-byte aligned) — PlainCol where the row lies in memory, ChildCol (rev_child_col.h) where it is synthesised.
// One pass stages the whole vector; the chunked form (vectors longer than the LDS window) stages it in chunks of
// ck2 double2 (a multiple of 256) and carries the four accumulators of wave_dot_chunk from chunk to chunk.  A chunk [c0, c1)
// that is not the last one holds whole 256-wide steps of the main loop, so every lane adds the same terms into the same
// accumulator in the same order as one pass over [0, ld2): the result is bit-identical.
// ------------------------------------------------------------------------------------------------

// a padded row that lies in memory (rows of At and B^-1, the vectors y / rho / b)
struct PlainCol {
    const double2 *p;
    __host__ __device__ __forceinline__ PlainCol() : p(nullptr) {}   // (the slot of a row a group does not have)
    __host__ __device__ __forceinline__ explicit PlainCol(const double *row) : p(reinterpret_cast<const double2 *>(row)) {}
    __host__ __device__ __forceinline__ double2 load2(int c) const { return p[c]; }
};

struct DotAcc {
    double a0, a1, a2, a3;
};

// the part of the dots of one row with NV staged vectors that falls into the chunk [c0, c1): vector v at svec + v * sstride,
// element c0 at offset 0.  The row is read once for all NV vectors.
template <int NV, class Row>
__device__ __forceinline__ void wave_dot_chunk(const Row &row, const double2 *__restrict__ svec, int sstride, int c0, int c1, int ld2, int lane,
                                               DotAcc (&acc)[NV]) {
    int c = c0 + lane;
    for (; c + 192 < c1; c += 256) {
        const double2 v0 = row.load2(c), v1 = row.load2(c + 64), v2 = row.load2(c + 128), v3 = row.load2(c + 192);
#pragma unroll
        for (int v = 0; v < NV; v++) {
            const double2 *s = svec + v * sstride + (c - c0);
            const double2 s0 = s[0], s1 = s[64], s2 = s[128], s3 = s[192];
            acc[v].a0 += v0.x * s0.x + v0.y * s0.y;
            acc[v].a1 += v1.x * s1.x + v1.y * s1.y;
            acc[v].a2 += v2.x * s2.x + v2.y * s2.y;
            acc[v].a3 += v3.x * s3.x + v3.y * s3.y;
        }
    }
    if (c1 == ld2) {   // the last chunk: the tail
        for (; c < ld2; c += 64) {
            const double2 v0 = row.load2(c);
#pragma unroll
            for (int v = 0; v < NV; v++) {
                const double2 s0 = svec[v * sstride + (c - c0)];
                acc[v].a0 += v0.x * s0.x + v0.y * s0.y;
            }
        }
    }
}

__device__ __forceinline__ double wave_dot_finish(const DotAcc &acc) { return wave_sum((acc.a0 + acc.a1) + (acc.a2 + acc.a3)); }

// NV vectors whole into LDS, ld2 double2 apart; one barrier behind
template <int NV, class Vec>
__device__ __forceinline__ void stage_vec(double2 *__restrict__ svec, const Vec (&src)[NV], int ld2) {
    for (int c = threadIdx.x; c < ld2; c += kBlock) {
#pragma unroll
        for (int v = 0; v < NV; v++) svec[v * ld2 + c] = src[v].load2(c);
    }
    __syncthreads();
}

// chunk [c0, c1) of NV vectors into LDS (vector v at svec + v * sstride).  Every thread of the workgroup: a barrier in front, so
// that the previous chunk is no longer read, and one behind.
template <int NV, class Vec>
__device__ __forceinline__ void stage_chunk(double2 *__restrict__ svec, int sstride, const Vec (&src)[NV], int c0, int c1) {
    __syncthreads();
    for (int c = threadIdx.x; c < c1 - c0; c += kBlock) {
#pragma unroll
        for (int v = 0; v < NV; v++) svec[v * sstride + c] = src[v].load2(c0 + c);
    }
    __syncthreads();
}

// The chunked kernels take a wave's rows kCkRows at a time, and the workgroup streams the vectors through LDS once per such group.
constexpr int kCkRows = 4;

// one group of up to kCkRows rows: dot[r][v] = rows[r] . vec[v], valid where has[r]; the NV vectors are staged ck2 double2 apart.
// Every thread of the workgroup (stage_chunk's barriers).
template <int NV, class Row, class Vec>
__device__ __forceinline__ void dot_group(const Row (&rows)[kCkRows], const bool (&has)[kCkRows], int ld, const Vec (&vec)[NV], double2 *svec,
                                          int ck2, int lane, double (&dot)[kCkRows][NV]) {
    const int ld2 = ld >> 1;
    DotAcc acc[kCkRows][NV];
#pragma unroll
    for (int r = 0; r < kCkRows; r++)
#pragma unroll
        for (int v = 0; v < NV; v++) acc[r][v].a0 = acc[r][v].a1 = acc[r][v].a2 = acc[r][v].a3 = 0;
    for (int c0 = 0; c0 < ld2; c0 += ck2) {
        const int c1 = min(c0 + ck2, ld2);
        stage_chunk<NV>(svec, ck2, vec, c0, c1);
#pragma unroll
        for (int r = 0; r < kCkRows; r++)
            if (has[r]) wave_dot_chunk<NV>(rows[r], svec, ck2, c0, c1, ld2, lane, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kCkRows; r++)
#pragma unroll
        for (int v = 0; v < NV; v++) dot[r][v] = has[r] ? wave_dot_finish(acc[r][v]) : 0.0;
}

// The row loop of every kernel that dots rows with staged vectors: the rows at positions first, first + step, ... < rows, row_of(pos)
// the loader of the row at a position, each dotted with the NV vectors vec[]; per_row(pos, dot) gets a row's NV dots (in all lanes).
//   CK = false: the vectors staged whole, ld2 apart, then one row at a time.
//   CK = true:  the rows kCkRows at a time (dot_group), the vectors streamed ck2 double2 at a time per group.  The loop runs to the
//               bound (rows + step - 1) / step, which is uniform wherever step is: every thread of the workgroup reaches every barrier.
// Every thread of the workgroup calls it (first = the wave's own position).  The two forms give a row the same bits.
template <bool CK, int NV, class RowOf, class Vec, class PerRow>
__device__ __forceinline__ void sweep_rows(RowOf row_of, const Vec (&vec)[NV], int rows, int first, int step, int ld, double2 *svec, int ck2,
                                           int lane, PerRow per_row) {
    if constexpr (CK) {
        const int kmax = (rows + step - 1) / step;
        for (int k0 = 0; k0 < kmax; k0 += kCkRows) {
            decltype(row_of(0)) row[kCkRows];
            bool has[kCkRows];
#pragma unroll
            for (int r = 0; r < kCkRows; r++) {
                const int pos = first + (k0 + r) * step;
                has[r] = pos < rows;
                if (has[r]) row[r] = row_of(pos);
            }
            double dot[kCkRows][NV];
            dot_group<NV>(row, has, ld, vec, svec, ck2, lane, dot);
#pragma unroll
            for (int r = 0; r < kCkRows; r++)
                if (has[r]) per_row(first + (k0 + r) * step, dot[r]);
        }
    } else {
        const int ld2 = ld >> 1;
        stage_vec<NV>(svec, vec, ld2);
        for (int pos = first; pos < rows; pos += step) {
            DotAcc acc[NV];
#pragma unroll
            for (int v = 0; v < NV; v++) acc[v].a0 = acc[v].a1 = acc[v].a2 = acc[v].a3 = 0;
            wave_dot_chunk<NV>(row_of(pos), svec, ld2, 0, ld2, ld2, lane, acc);
            double dot[NV];
#pragma unroll
            for (int v = 0; v < NV; v++) dot[v] = wave_dot_finish(acc[v]);
            per_row(pos, dot);
        }
    }
}

// the workgroup's first-index argmin into the per-workgroup partials that the next kernel reduces (reduce_partials)
__device__ __forceinline__ void publish_partials(unsigned long long &bk, unsigned int &bi, unsigned long long *sk, unsigned int *si,
                                                 unsigned long long *pk, unsigned int *pi) {
    block_argmin(bk, bi, sk, si);
    if (threadIdx.x == 0) { pk[blockIdx.x] = bk; pi[blockIdx.x] = bi; }
}

// guard mode: the runner-up key too, into pk2 (reduce_partials2)
__device__ __forceinline__ void publish_partials2(unsigned long long &bk, unsigned int &bi, unsigned long long &b2, unsigned long long *sk,
                                                  unsigned int *si, unsigned long long *ss, unsigned long long *pk, unsigned int *pi,
                                                  unsigned long long *pk2) {
    block_argmin2(bk, bi, b2, sk, si, ss);
    if (threadIdx.x == 0) { pk[blockIdx.x] = bk; pi[blockIdx.x] = bi; pk2[blockIdx.x] = b2; }
}

}  // namespace gomilp
