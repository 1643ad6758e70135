// gfx950 kernels of the single-context warm start (engine_warm.cpp): a dual simplex on the revised-simplex
// kernels, and the two set-up kernels that build a child's B^-1 from its parent's kept state.
//
// One dual pivot = k_dual_leave (leaving row p: first index of min x_B, stop when >= -tol) -> k_dual_price (per nonbasic column
// a_j.y and a_j.rho with rho = B^-1[p,:], the dual ratio test r_j / -alpha_pj over alpha_pj < -1e-13 as a first-index argmin)
// -> k_ftran with the entering position taken from those partials (kDualPick) -> k_update with the leaving row taken from the
// state (kDualPick).  The decision rules are those of the pool's dual block kernel (bt_kernels.hip bt_inner2_dual_body).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "device_types.h"
#include "kernels_common.h"

namespace gomilp {

// the pricing kernel stages TWO m-long vectors: one pass fits the 64 KB LDS window up to ld = 4096, the chunked form streams
// them at most 2048 double2 each (64 KB) at a time
constexpr int kDualOnePassLd = 4096;

// ------------------------------------------------------------------------------------------------
// leaving row: one workgroup over x_B (m doubles).  The dual-pivot budget is DevState::max_pivots.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_dual_leave(const double *__restrict__ xb, int m, double tol, DevState *st) {
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int si[kWavesPerBlock];
    if (st->done) return;
    unsigned long long bk = ~0ull;
    unsigned int bi = 0xFFFFFFFFu;
    for (int i = threadIdx.x; i < m; i += kBlock) amin_take(bk, bi, ordkey(xb[i]), (unsigned int)i);
    block_argmin(bk, bi, sk, si);
    if (threadIdx.x == 0) {
        const double xmin = orddecode(bk);
        if (!(xmin < -tol) || bi >= (unsigned int)m) { st->done = 1; st->status = ST_OPTIMAL; }
        else if (st->max_pivots > 0 && st->pivots >= st->max_pivots) { st->done = 1; st->status = ST_MAX_PIVOTS; }
        else st->p = (int)bi;
    }
}

// ------------------------------------------------------------------------------------------------
// dual pricing: per nonbasic column a_j.y and a_j.rho, the row of At read once for both (kernels_common.h: sweep_rows with two
// vectors).  CK = false: y and rho staged whole (2 * ld doubles of LDS: ld <= 4096); CK = true: streamed through LDS ck2 double2
// each at a time.  The two forms agree bit for bit.
// ------------------------------------------------------------------------------------------------

// r_pos = cost[j] - a_j.y (kept in rvec for k_ftran / k_update), the ratio key of column pos
__device__ __forceinline__ unsigned long long dual_key(const LPArgs &a, int pos, double dy, double da, int lane) {
    const double r = a.cost[a.nonbasic[pos]] - dy;
    if (lane == 0) a.rvec[pos] = r;
    return ordkey(da < -1e-13 ? r / (-da) : __builtin_inf());
}

template <bool CK>
__global__ __launch_bounds__(kBlock) void k_dual_price(LPArgs a, int ck2) {
    extern __shared__ __attribute__((aligned(16))) double2 svec[];
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int si[kWavesPerBlock];
    DevState *st = a.st;
    if (st->done) return;
    const double *rho = a.binv_cur + (size_t)st->p * a.ld;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlock;
    unsigned long long bk = ~0ull;
    unsigned int bi = 0xFFFFFFFFu;
    sweep_rows<CK, 2>([&](int pos) { return PlainCol(a.At + (size_t)a.nonbasic[pos] * a.ld); }, {PlainCol(a.y), PlainCol(rho)}, a.nn, wave, nwaves, a.ld, svec,
                      ck2, lane, [&](int pos, const double (&dot)[2]) { amin_take(bk, bi, dual_key(a, pos, dot[0], dot[1], lane), (unsigned int)pos); });
    publish_partials(bk, bi, sk, si, a.pk_price, a.pi_price);
}

// ------------------------------------------------------------------------------------------------
// child B^-1 from the parent's kept B_p^-1 (mp x ldp) and J new branch rows (var_k, sign_k):
//   B^-1 = [[B_p^-1, 0], [R, I_J]],  R[k, :] = -sign_k * B_p^-1[kpos_k, :] where var_k is basic at parent position kpos_k, else 0.
// One workgroup per row of the child's m x ld buffer (padding columns written as zero).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_warm_binv(const double *__restrict__ Bp, int ldp, int mp, double *__restrict__ B, int ld,
                                                      const int32_t *__restrict__ kpos, const double *__restrict__ ksign) {
    const int i = blockIdx.x;
    double *dst = B + (size_t)i * ld;
    if (i < mp) {
        const double *src = Bp + (size_t)i * ldp;
        for (int c = threadIdx.x; c < ld; c += kBlock) dst[c] = c < mp ? src[c] : 0.0;
        return;
    }
    const int k = i - mp, pos = kpos[k];
    const double s = -ksign[k];
    const double *src = pos >= 0 ? Bp + (size_t)pos * ldp : nullptr;
    for (int c = threadIdx.x; c < ld; c += kBlock) dst[c] = c < mp ? (src ? s * src[c] : 0.0) : (c == i ? 1.0 : 0.0);
}

// ------------------------------------------------------------------------------------------------
// B^-1 gathered from a tableau T = B^-1 A_N (row-major or 4x4 tiles, tab_idx): column r of B^-1 is B^-1 e_r = B^-1 a_s for the
// unit column s of row r — T's column src[r] >= 0 when s is nonbasic there, e_p when s is basic at position p (src[r] = -1 - p).
// One workgroup per row of the m x ld output (padding columns zero).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_tab_to_binv(const double *__restrict__ T, int ldt, int tiled, int m,
                                                        const int32_t *__restrict__ src, double *__restrict__ B, int ld) {
    const int i = blockIdx.x;
    double *dst = B + (size_t)i * ld;
    for (int c = threadIdx.x; c < ld; c += kBlock) {
        double v = 0.0;
        if (c < m) {
            const int s = src[c];
            v = s >= 0 ? T[tab_idx(i, s, ldt, tiled)] : ((-1 - s) == i ? 1.0 : 0.0);
        }
        dst[c] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------------
void launch_dual_leave(const double *xb, int m, double tol, DevState *st, hipStream_t s) {
    hipLaunchKernelGGL(k_dual_leave, dim3(1), dim3(kBlock), 0, s, xb, m, tol, st);
}

int launch_dual_price(const LPArgs &a, hipStream_t s) {
    const int g = grid_for_rows(a.nn);
    // one pass while both vectors fit the 64 KB window; else (and whenever the row_chunk knob forces it) the chunked form
    if (a.row_chunk2 == 0 && a.ld <= kDualOnePassLd) {
        hipLaunchKernelGGL(k_dual_price<false>, dim3(g), dim3(kBlock), (size_t)2 * a.ld * sizeof(double), s, a, 0);
    } else {
        const int ck2 = (a.row_chunk2 > 0 && a.row_chunk2 < kDualOnePassLd / 2) ? a.row_chunk2 : kDualOnePassLd / 2;
        hipLaunchKernelGGL(k_dual_price<true>, dim3(g), dim3(kBlock), (size_t)2 * ck2 * sizeof(double2), s, a, ck2);
    }
    return g;
}

void launch_warm_binv(const double *Bp, int ldp, int mp, double *B, int ld, int m, const int32_t *kpos, const double *ksign, hipStream_t s) {
    hipLaunchKernelGGL(k_warm_binv, dim3(m), dim3(kBlock), 0, s, Bp, ldp, mp, B, ld, kpos, ksign);
}

void launch_tab_to_binv(const double *T, int ldt, bool tiled, int m, const int32_t *src, double *B, int ld, hipStream_t s) {
    hipLaunchKernelGGL(k_tab_to_binv, dim3(m), dim3(kBlock), 0, s, T, ldt, tiled ? 1 : 0, m, src, B, ld);
}

}  // namespace gomilp
