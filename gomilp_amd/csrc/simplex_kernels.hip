// gfx950 (CDNA4, wave64) kernels of the revised-simplex inner loop that replaces the per-pivot
// work of gonum's lp.Simplex (reference: vendor/gonum.org/v1/gonum/optimize/convex/lp/simplex.go:233-293).
//
// Data layout in HBM (all fp64, row-major, rows padded to `ld` doubles with zeros):
//   At    (ncols x ld)  row j = column j of the standard-form A  -> pricing and FTRAN read contiguous rows
//   Binv  (m x ld)      explicit basis inverse, two copies (ping-pong target of the rank-1 update)
// Every hot kernel is a streaming kernel: one 64-lane wave per matrix row, 16-byte loads per lane
// (1 KiB per wave instruction), the shared vector staged once per workgroup in LDS, and the
// arg-reductions (entering column, leaving row) fused into the epilogue as first-index argmins.
// Kernels communicate only across kernel boundaries; nothing depends on dispatch order.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "device_types.h"
#include "kernels_common.h"
#include "simplex_helpers.h"

namespace gomilp {

// K1-K3: the pivot rules, the per-element work and the commit are the helpers of simplex_helpers.h (shared with batch_revised.hip).

// Template parameter CK (every kernel that stages an m-long vector): false stages the vector whole (ld up to the 64 KB LDS window, the
// kernel's ck2 unused), true streams it through LDS ck2 double2 at a time (ld > 8192, or wherever the context knob row_chunk forces it).
// The staging and the row loop of either form are sweep_rows of kernels_common.h; everything around them is written once.

// ------------------------------------------------------------------------------------------------
// K1  pricing:  r[pos] = cost[j] - At[j,:].y   (simplex.go:242-243), fused first-index argmin (:247)
//     algorithmic traffic: m*(n-m)*8 bytes read (A_N once)
// ------------------------------------------------------------------------------------------------
template <bool G, bool CK>
__global__ __launch_bounds__(kBlock) void k_price(LPArgs a, int ck2) {
    extern __shared__ __attribute__((aligned(16))) double2 svec[];
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int si[kWavesPerBlock];
    __shared__ unsigned long long ss[G ? kWavesPerBlock : 1];
    if (!price_gate(a.st)) return;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlock;
    unsigned long long bk = ~0ull, b2 = ~0ull;
    unsigned int bi = 0xFFFFFFFFu;
    sweep_rows<CK, 1>([&](int pos) { return PlainCol(a.At + (size_t)a.nonbasic[pos] * a.ld); }, {PlainCol(a.y)}, a.nn, wave, nwaves, a.ld, svec, ck2, lane,
                      [&](int pos, const double (&dot)[1]) { price_elem<G>(a.cost, a.rvec, pos, a.nonbasic[pos], dot[0], lane, bk, bi, b2); });
    publish<G>(bk, bi, b2, sk, si, ss, a.pk_price, a.pi_price);
}

// ------------------------------------------------------------------------------------------------
// K2  FTRAN + ratio test:  d' = Binv a_q ; move_i = x_B[i]/|d_i| for d_i = -d'_i < 0 (simplex.go:306-342),
//     fused first-index argmin of move (:268).   traffic: m*m*8 bytes read (B^-1 once)
//     entering variable: pick_entering
// ------------------------------------------------------------------------------------------------
template <bool G, bool CK>
__global__ __launch_bounds__(kBlock) void k_ftran(LPArgs a, int nparts_price, int forced_pos, int forced_var, int ck2) {
    extern __shared__ __attribute__((aligned(16))) double2 svec[];
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int si[kWavesPerBlock];
    __shared__ unsigned long long ss[G ? kWavesPerBlock : 1];
    int var;
    if (!pick_entering<G>(a.st, a.pk_price, a.pi_price, nparts_price, a.rvec, a.nonbasic, a.tol, a.guard, forced_pos, forced_var, sk, si, ss, var)) return;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlock;
    unsigned long long bk = ~0ull, b2 = ~0ull;
    unsigned int bi = 0xFFFFFFFFu;
    sweep_rows<CK, 1>([&](int i) { return PlainCol(a.binv_cur + (size_t)i * a.ld); }, {PlainCol(a.At + (size_t)var * a.ld)}, a.m, wave, nwaves, a.ld, svec, ck2, lane,
                      [&](int i, const double (&dot)[1]) { ratio_elem<G>(a.xb, a.dvec, a.move, i, dot[0], lane, bk, bi, b2); });
    publish<G>(bk, bi, b2, sk, si, ss, a.pk_ratio, a.pi_ratio);
}

// ------------------------------------------------------------------------------------------------
// K3  basis change: rank-1 update of B^-1 (ping-pong), x_B, y, index swap (simplex.go:280-292 without
//     the three fresh LU factorizations).   traffic: m*m*8 read + m*m*8 written
//     leaving row: pick_leaving.  no_swap: setup pivot (indices managed by the host).
//     Elementwise: the chunks of CK are only bounds, and the commit reads old row p where CK left it (LDS, or B^-1 itself:
//     binv_cur is only read here).
// ------------------------------------------------------------------------------------------------
template <bool G, bool CK>
__global__ __launch_bounds__(kBlock) void k_update(LPArgs a, int nparts_ratio, int forced_p, int no_swap, int bland, int ck2) {
    extern __shared__ __attribute__((aligned(16))) double2 svec[];
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int si[kWavesPerBlock];
    __shared__ unsigned long long ss[G ? kWavesPerBlock : 1];
    int p;
    if (!pick_leaving<G>(a.st, a.pk_ratio, a.pi_ratio, nparts_ratio, a.move, a.dvec, a.guard, forced_p, sk, si, ss, p)) return;
    const double dpv = a.dvec[p];
    const double *rowp_g = a.binv_cur + (size_t)p * a.ld;   // old row p
    update_rows<CK>(a.binv_cur, a.binv_next, a.ld, a.dvec, a.m, p, dpv, rowp_g, svec, ck2);
    if (blockIdx.x == 0)
        commit_pivot(a.st, a.xb, a.y, a.dvec, a.move, a.basic, a.nonbasic, a.trace, a.trace_cap, a.phase, a.m, a.ld, p, dpv,
                     CK ? rowp_g : reinterpret_cast<const double *>(svec), no_swap, bland);
}

// ------------------------------------------------------------------------------------------------
// set-up / refresh kernels (outside the per-pivot path)
// ------------------------------------------------------------------------------------------------

// At[j*ld + i] = A[i*lda + j]   (32x32 LDS tile transpose; block = 32x8)
__global__ void k_transpose_in(const double *__restrict__ A, int64_t lda, int m, int n, double *__restrict__ At, int ld) {
    __shared__ double tile[32][33];
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int i = i0 + r, j = j0 + threadIdx.x;
        if (i < m && j < n) tile[r][threadIdx.x] = A[(size_t)i * lda + j];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int j = j0 + r, i = i0 + threadIdx.x;
        if (i < m && j < n) At[(size_t)j * ld + i] = tile[threadIdx.x][r];
    }
}

// per column j of A (row of At): nnz, row of the last non-zero, all non-zeros equal to 1 ; and mark non-empty rows
// range (optional): [0] = bits of max |a_ij|, [1] = bits of the smallest non-zero |a_ij| (positive doubles order like their bit patterns)
__global__ __launch_bounds__(kBlock) void k_col_stats(const double *__restrict__ At, int ld, int m, int n, int32_t *nnz,
                                                      int32_t *lastrow, int32_t *allone, int32_t *rowflag, unsigned long long *range) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlock;
    for (int j = wave; j < n; j += nwaves) {
        const double *row = At + (size_t)j * ld;
        int cnt = 0, last = -1, one = 1;
        unsigned long long hi = 0ull, lo = ~0ull;
        for (int i = lane; i < m; i += 64) {
            const double v = row[i];
            if (v != 0) {
                cnt++; last = i; if (v != 1.0) one = 0; rowflag[i] = 1;
                const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(v));
                hi = bits > hi ? bits : hi; lo = bits < lo ? bits : lo;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            cnt += __shfl_xor(cnt, o, 64);
            last = max(last, __shfl_xor(last, o, 64));
            one &= __shfl_xor(one, o, 64);
            const unsigned long long h2 = __shfl_xor(hi, o, 64), l2 = __shfl_xor(lo, o, 64);
            hi = h2 > hi ? h2 : hi; lo = l2 < lo ? l2 : lo;
        }
        if (lane == 0) {
            nnz[j] = cnt; lastrow[j] = last; allone[j] = one;
            if (range && cnt) { atomicMax(range, hi); atomicMin(range + 1, lo); }
        }
    }
}

// Child relaxation of a B&B node assembled in HBM from the resident root (subproblem.go:81-139, :245-255):
//   child A = [[A0, 0], [G#, I_K]],  G# row k = sign_k * e_{var_k}.  In the transposed layout every root column keeps
//   its m0 entries and gains K entries; K unit columns are appended; the last row is the (zeroed) artificial slot.
__global__ __launch_bounds__(kBlock) void k_child_assemble(const double *__restrict__ At0, int ld0, int m0, int n0,
                                                           double *__restrict__ At1, int ld1, int K,
                                                           const int32_t *__restrict__ var, const double *__restrict__ sign) {
    const int j = blockIdx.x;  // child column
    double *dst = At1 + (size_t)j * ld1;
    if (j < n0) {
        const double *src = At0 + (size_t)j * ld0;
        for (int i = threadIdx.x; i < ld1; i += kBlock) {
            double v = 0.0;
            if (i < m0) v = src[i];
            else if (i < m0 + K && var[i - m0] == j) v = sign[i - m0];
            dst[i] = v;
        }
    } else {
        const int unit = (j < n0 + K) ? m0 + (j - n0) : -1;
        for (int i = threadIdx.x; i < ld1; i += kBlock) dst[i] = (i == unit) ? 1.0 : 0.0;
    }
}

// Binv = permutation: Binv[pos, rho[pos]] = 1 (buffer pre-zeroed)
__global__ void k_set_binv_perm(double *binv, int ld, int m, const int32_t *rho) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos < m) binv[(size_t)pos * ld + rho[pos]] = 1.0;
}

// out[i] = M[i,:].vec   (x_B = Binv b refresh)
template <bool CK>
__global__ __launch_bounds__(kBlock) void k_matvec_rows(const double *__restrict__ M, int ld, int m, const double *__restrict__ vec,
                                                        double *__restrict__ out, int ck2) {
    extern __shared__ __attribute__((aligned(16))) double2 svec[];
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlock;
    sweep_rows<CK, 1>([&](int i) { return PlainCol(M + (size_t)i * ld); }, {PlainCol(vec)}, m, wave, nwaves, ld, svec, ck2, lane,
                      [&](int i, const double (&dot)[1]) { if (lane == 0) out[i] = dot[0]; });
}

// y[j] = sum_i cost[basic[i]] * Binv[i,j]   (y = B^-T c_B, simplex.go:236) — column-parallel, row-chunked;
// partial sums in chunk-major scratch, then reduced in fixed order (deterministic).
__global__ __launch_bounds__(kBlock) void k_y_partial(const double *__restrict__ binv, int ld, int m,
                                                      const double *__restrict__ cost, const int32_t *__restrict__ basic,
                                                      double *__restrict__ scratch, int rows_per_chunk) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    const int chunk = blockIdx.y;
    const int i0 = chunk * rows_per_chunk, i1 = min(m, i0 + rows_per_chunk);
    if (j >= ld) return;
    double acc = 0;
    for (int i = i0; i < i1; i++) {
        const double cb = cost[basic[i]];
        if (cb != 0) acc += cb * binv[(size_t)i * ld + j];
    }
    scratch[(size_t)chunk * ld + j] = acc;
}
__global__ void k_y_reduce(const double *__restrict__ scratch, int ld, int nchunks, double *__restrict__ y) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ld) return;
    double acc = 0;
    for (int c = 0; c < nchunks; c++) acc += scratch[(size_t)c * ld + j];
    y[j] = acc;
}

// ------------------------------------------------------------------------------------------------
// Final basis solve: LU with partial pivoting in gonum's operation order, so that x_B = ab^-1 b is
// bit-identical to the reference's last `xbVec.SolveVec(ab, bVec)` (simplex.go:288-292 ->
// lapack/gonum/dgetf2.go:30-69 / dgetrf.go:29-70):
//   pivot = first max |a_ik| over the remaining rows in LOGICAL row order (Idamax, level1double.go:121-165)
//   l_ik  = a_ik * (1/a_kk)                      (dgetf2.go:56: Dscal by the reciprocal)
//   a_ij  = (-l_ik) * a_kj + a_ij                (Dger/Dgemm: rounded multiply THEN rounded add, no FMA)
// Rows are never moved: lpos[R] is the logical position of physical row R (row interchanges of
// dlaswp.go become index updates), rowstep[R] >= 0 marks rows already used as pivot rows.
// One launch per column; the argmax for column k+1 is fused into step k.
// ------------------------------------------------------------------------------------------------

// W[i*ldw + pos] = At[basic[pos]*ld + i]   (ab of simplex.go:144: column pos = column basic[pos] of A)
__global__ void k_gather_w(const double *__restrict__ At, int ld, int m, const int32_t *__restrict__ basic,
                           double *__restrict__ W, int ldw) {
    __shared__ double tile[32][33];
    const int p0 = blockIdx.y * 32, i0 = blockIdx.x * 32;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int pos = p0 + r, i = i0 + threadIdx.x;
        if (pos < m && i < m) tile[r][threadIdx.x] = At[(size_t)basic[pos] * ld + i];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int i = i0 + r, pos = p0 + threadIdx.x;
        if (pos < m && i < m) W[(size_t)i * ldw + pos] = tile[threadIdx.x][r];
    }
}

__device__ __forceinline__ void lu_take(unsigned long long &k, unsigned int &l, unsigned int &r, unsigned long long k2,
                                        unsigned int l2, unsigned int r2) {
    if (k2 < k || (k2 == k && l2 < l)) { k = k2; l = l2; r = r2; }
}

__device__ __forceinline__ void lu_block_reduce(unsigned long long &k, unsigned int &l, unsigned int &r,
                                                unsigned long long *sk, unsigned int *sl, unsigned int *sr) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long k2 = __shfl_xor(k, o, 64);
        unsigned int l2 = __shfl_xor(l, o, 64), r2 = __shfl_xor(r, o, 64);
        lu_take(k, l, r, k2, l2, r2);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sk[w] = k; sl[w] = l; sr[w] = r; }
    __syncthreads();
    k = sk[0]; l = sl[0]; r = sr[0];
#pragma unroll
    for (int t = 1; t < kWavesPerBlock; t++) lu_take(k, l, r, sk[t], sl[t], sr[t]);
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void k_lu_init(LUArgs a) {
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int sl[kWavesPerBlock], sr[kWavesPerBlock];
    unsigned long long bk = ~0ull;
    unsigned int bl = 0xFFFFFFFFu, br = 0xFFFFFFFFu;
    for (int R = blockIdx.x * kBlock + threadIdx.x; R < a.m; R += gridDim.x * kBlock) {
        a.lpos[R] = R;
        a.rowstep[R] = -1;
        lu_take(bk, bl, br, ordkey(-fabs(a.W[(size_t)R * a.ldw])), (unsigned int)R, (unsigned int)R);
    }
    lu_block_reduce(bk, bl, br, sk, sl, sr);
    if (threadIdx.x == 0) { a.pk[0][blockIdx.x] = bk; a.pl[0][blockIdx.x] = bl; a.pr[0][blockIdx.x] = br; }
}

__global__ __launch_bounds__(kBlock) void k_lu_step(LUArgs a, int k, int nparts) {
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int sl[kWavesPerBlock], sr[kWavesPerBlock];
    const int par = k & 1;
    // pivot of column k from the partials written by the previous step
    unsigned long long bk = ~0ull;
    unsigned int bl = 0xFFFFFFFFu, br = 0xFFFFFFFFu;
    for (int t = threadIdx.x; t < nparts; t += kBlock) lu_take(bk, bl, br, a.pk[par][t], a.pl[par][t], a.pr[par][t]);
    lu_block_reduce(bk, bl, br, sk, sl, sr);
    const int P = (int)br;    // physical pivot row
    const int jp = (int)bl;   // its logical position before the interchange
    const double piv = a.W[(size_t)P * a.ldw + k];
    const bool singular = (piv == 0);  // dgetf2.go:48-49: ok = false, no scaling, the rank-1 update is a no-op
    if (singular && blockIdx.x == 0 && threadIdx.x == 0) a.st->lu_singular = 1;
    const double rinv = 1.0 / piv;
    const double *__restrict__ prow = a.W + (size_t)P * a.ldw;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlock;
    unsigned long long nk = ~0ull;
    unsigned int nl = 0xFFFFFFFFu, nr = 0xFFFFFFFFu;
    for (int R = wave; R < a.m; R += nwaves) {
        if (a.rowstep[R] >= 0) continue;
        if (R == P) {
            if (lane == 0) { a.rowstep[R] = k; a.lpos[R] = k; }
            continue;
        }
        int lp = a.lpos[R];
        if (lp == k) { lp = jp; if (lane == 0) a.lpos[R] = jp; }  // the row that sat at logical k moves to jp (dlaswp)
        double *row = a.W + (size_t)R * a.ldw;
        if (!singular) {
            const double l = __dmul_rn(row[k], rinv);
            const double nlv = -l;
            for (int j = k + 1 + lane; j < a.m; j += 64) row[j] = __dadd_rn(__dmul_rn(nlv, prow[j]), row[j]);
            if (lane == 0) row[k] = l;
        }
        if (k + 1 < a.m) {
            // lane 0 wrote row[k+1] in its first iteration above (j = k+1+0); re-read through the same lane
            double v = 0;
            if (lane == 0) v = row[k + 1];
            v = __shfl(v, 0, 64);
            lu_take(nk, nl, nr, ordkey(-fabs(v)), (unsigned int)lp, (unsigned int)R);
        }
    }
    lu_block_reduce(nk, nl, nr, sk, sl, sr);
    if (threadIdx.x == 0) { a.pk[par ^ 1][blockIdx.x] = nk; a.pl[par ^ 1][blockIdx.x] = nl; a.pr[par ^ 1][blockIdx.x] = nr; }
}

// ------------------------------------------------------------------------------------------------
// host-callable launch wrappers (the engine is plain C++; only this file is device code)
// ------------------------------------------------------------------------------------------------

// dynamic LDS of a kernel that stages one m-long vector: the chunk (row_chunk2 > 0: the CK = true instance), else the whole vector
static size_t staged_lds(int ld, int row_chunk2) { return row_chunk2 > 0 ? (size_t)row_chunk2 * sizeof(double2) : (size_t)ld * sizeof(double); }

// (LPArgs::guard > 0: the guard instances)
template <bool G>
static void launch_price_t(const LPArgs &a, int g, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    hipExtLaunchKernelGGL((a.row_chunk2 > 0 ? k_price<G, true> : k_price<G, false>), dim3(g), dim3(kBlock), staged_lds(a.ld, a.row_chunk2), s, e0, e1, 0, a,
                          a.row_chunk2);
}
int launch_price(const LPArgs &a, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    const int g = grid_for_rows(a.nn);
    if (a.guard > 0) launch_price_t<true>(a, g, s, e0, e1);
    else launch_price_t<false>(a, g, s, e0, e1);
    return g;
}
template <bool G>
static void launch_ftran_t(const LPArgs &a, int g, int nparts_price, int forced_pos, int forced_var, hipStream_t s, hipEvent_t e0,
                           hipEvent_t e1) {
    hipExtLaunchKernelGGL((a.row_chunk2 > 0 ? k_ftran<G, true> : k_ftran<G, false>), dim3(g), dim3(kBlock), staged_lds(a.ld, a.row_chunk2), s, e0, e1, 0, a,
                          nparts_price, forced_pos, forced_var, a.row_chunk2);
}
int launch_ftran(const LPArgs &a, int nparts_price, int forced_pos, int forced_var, hipStream_t s, hipEvent_t e0,
                 hipEvent_t e1) {
    const int g = grid_for_rows(a.m);
    if (a.guard > 0) launch_ftran_t<true>(a, g, nparts_price, forced_pos, forced_var, s, e0, e1);
    else launch_ftran_t<false>(a, g, nparts_price, forced_pos, forced_var, s, e0, e1);
    return g;
}
template <bool G>
static void launch_update_t(const LPArgs &a, int g, int nparts_ratio, int forced_p, int no_swap, int bland, hipStream_t s, hipEvent_t e0,
                            hipEvent_t e1) {
    hipExtLaunchKernelGGL((a.row_chunk2 > 0 ? k_update<G, true> : k_update<G, false>), dim3(g), dim3(kBlock), staged_lds(a.ld, a.row_chunk2), s, e0, e1, 0, a,
                          nparts_ratio, forced_p, no_swap, bland, a.row_chunk2);
}
void launch_update(const LPArgs &a, int nparts_ratio, int forced_p, int no_swap, int bland, hipStream_t s, hipEvent_t e0,
                   hipEvent_t e1) {
    const int g = grid_for_rows(a.m);
    if (a.guard > 0) launch_update_t<true>(a, g, nparts_ratio, forced_p, no_swap, bland, s, e0, e1);
    else launch_update_t<false>(a, g, nparts_ratio, forced_p, no_swap, bland, s, e0, e1);
}
void launch_transpose_in(const double *A, int64_t lda, int m, int n, double *At, int ld, hipStream_t s) {
    dim3 grid((n + 31) / 32, (m + 31) / 32), block(32, 8);
    hipLaunchKernelGGL(k_transpose_in, grid, block, 0, s, A, lda, m, n, At, ld);
}
void launch_col_stats(const double *At, int ld, int m, int n, int32_t *nnz, int32_t *lastrow, int32_t *allone,
                      int32_t *rowflag, unsigned long long *range, hipStream_t s) {
    hipLaunchKernelGGL(k_col_stats, dim3(grid_for_rows(n)), dim3(kBlock), 0, s, At, ld, m, n, nnz, lastrow, allone, rowflag, range);
}
void launch_child_assemble(const double *At0, int ld0, int m0, int n0, double *At1, int ld1, int K, const int32_t *var,
                           const double *sign, hipStream_t s) {
    hipLaunchKernelGGL(k_child_assemble, dim3(n0 + K + 1), dim3(kBlock), 0, s, At0, ld0, m0, n0, At1, ld1, K, var, sign);
}
void launch_set_binv_perm(double *binv, int ld, int m, const int32_t *rho, hipStream_t s) {
    hipLaunchKernelGGL(k_set_binv_perm, dim3((m + 255) / 256), dim3(256), 0, s, binv, ld, m, rho);
}
void launch_matvec_rows(const double *M, int ld, int m, const double *vec, double *out, hipStream_t s, int row_chunk2) {
    hipLaunchKernelGGL((row_chunk2 > 0 ? k_matvec_rows<true> : k_matvec_rows<false>), dim3(grid_for_rows(m)), dim3(kBlock), staged_lds(ld, row_chunk2), s, M,
                       ld, m, vec, out, row_chunk2);
}
// scratch must hold y_chunks(m) * ld doubles
int y_chunks(int m) { int c = (m + 63) / 64; return c > 64 ? 64 : c; }
void launch_y_from_binv(const double *binv, int ld, int m, const double *cost, const int32_t *basic, double *scratch,
                        double *y, hipStream_t s) {
    const int nchunks = y_chunks(m);
    const int rpc = (m + nchunks - 1) / nchunks;
    dim3 grid((ld + kBlock - 1) / kBlock, nchunks);
    hipLaunchKernelGGL(k_y_partial, grid, dim3(kBlock), 0, s, binv, ld, m, cost, basic, scratch, rpc);
    hipLaunchKernelGGL(k_y_reduce, dim3((ld + 255) / 256), dim3(256), 0, s, scratch, ld, nchunks, y);
}
void launch_gather_w(const double *At, int ld, int m, const int32_t *basic, double *W, int ldw, hipStream_t s) {
    dim3 grid((m + 31) / 32, (m + 31) / 32), block(32, 8);
    hipLaunchKernelGGL(k_gather_w, grid, block, 0, s, At, ld, m, basic, W, ldw);
}
int lu_grid(int m) { return grid_for_rows(m); }
void launch_lu(const LUArgs &a, hipStream_t s) {
    const int g = lu_grid(a.m);
    hipLaunchKernelGGL(k_lu_init, dim3(g), dim3(kBlock), 0, s, a);
    for (int k = 0; k < a.m; k++) hipLaunchKernelGGL(k_lu_step, dim3(g), dim3(kBlock), 0, s, a, k, g);
}

}  // namespace gomilp
