// gfx950 (CDNA4, wave64) kernels of the device-batched revised simplex: K1-K3 of simplex_kernels.hip with the relaxation as
// blockIdx.y, and the small kernels that run a relaxation's stages on the device (assembly of the children, slack start, Phase-I set-up, list rebuilds,
// refreshes, the Bland rule, the zero-level artificial exchange, the verdicts) so that a wave costs a constant number of host round trips per superstep.
//
// The pivot rules, the per-element work and the commit are the helpers of simplex_helpers.h, the code the single-relaxation
// kernels run: every dot product is one wave over one row (wave_dot_chunk), the argmins are first-index over per-workgroup
// partials, so a relaxation's values do not depend on the grid it gets or on the relaxations beside it.  Nothing is reduced
// across relaxations and no kernel waits for another workgroup: kernels communicate across launch boundaries only.
// Every field of a RevLP that a kernel reads was written by an earlier launch of the stream (RevLP::flips / flips_k2); the one
// exception, RevLP::x_best in k_rv_exch, only saves work.
//
// Every kernel that stages an m-long vector in LDS is a template on CK, as in simplex_kernels.hip: CK = false is one pass (the vector
// staged whole: rows up to the 64 KB window), CK = true the chunked form (the vector streamed through LDS ck2 double2 at a time; pool knob
// large_rows, or wherever the pool's row_chunk forces it).  The two forms differ in their staging and row loops only, and those are
// sweep_rows of kernels_common.h (update_rows of simplex_helpers.h for K3), so a relaxation's values do not depend on the chunk size
// either.  The chunked loops run to workgroup-uniform bounds (the relaxation's own m, nn and ld): every thread of a workgroup reaches
// every barrier.
//
// Every kernel that reads a child's column is a template on IP (pool knob rev_inplace), and IP only picks the loader (child_col):
// IP = false reads the At that k_rv_assemble wrote (PlainCol), IP = true reads the column from the relaxation's root in place (ChildCol,
// rev_child_col.h) — the same arithmetic on synthesised values, so a relaxation's values do not depend on the mode either.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_revised.h"
#include "device_types.h"
#include "gomilp_lp.h"
#include "kernels_common.h"
#include "rev_child_col.h"
#include "simplex_helpers.h"

namespace gomilp {

namespace {

__device__ __forceinline__ unsigned int block_min_u32(unsigned int v, unsigned int *sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned int)__shfl_xor((int)v, o, 64));
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sm[w] = v;
    __syncthreads();
    v = sm[0];
#pragma unroll
    for (int t = 1; t < kWavesPerBlock; t++) v = min(v, sm[t]);
    __syncthreads();
    return v;
}

// row of the 1 in the child's column n - 1 - pos: the K branch slacks first (descending scan, simplex.go:618-635), then the root's
__device__ __forceinline__ int child_rho(int pos, int K, int m0, const int32_t *rho0) {
    return pos < K ? m0 + K - 1 - pos : rho0[pos - K];
}

__device__ __forceinline__ void start_loop_state(DevState *st, int64_t max_pivots) {
    st->done = 0; st->status = ST_RUNNING; st->pivots = 0; st->q = -1; st->p = -1; st->rq = 0; st->dp = 0; st->mv = 0;
    st->max_pivots = max_pivots; st->lu_singular = 0;
}

__device__ __forceinline__ void clear_orders(RevLP *d) {
    d->do_lists = 0; d->do_refresh = 0; d->after = RA_NONE;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// At of every relaxation of the wave in one launch (k_child_assemble of simplex_kernels.hip with the relaxation as blockIdx.y;
// subproblem.go:81-139, :245-255): child A = [[A0, 0], [G#, I_K]], G# row k = sign_k * e_{var_k}, of the relaxation's own root.  In
// the transposed layout root column j keeps its m0 entries and gains sign_k at the branch rows on it; the K unit columns follow; row n
// is the zeroed artificial slot.  blockIdx.x = child column, up to the widest relaxation's n: a workgroup past its relaxation's width
// has nothing to write.  Plain loads and stores, no LDS, no workgroup depends on another.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rv_assemble(const RevLP *__restrict__ lps) {
    const RevLP *d = lps + blockIdx.y;
    const int j = blockIdx.x, n = d->n;
    if (j > n) return;
    const int m0 = d->m0, n0 = d->n0, K = d->K, ld = d->ld;
    double *dst = d->At + (size_t)j * ld;
    if (j < n0) {
        const double *src = d->At0 + (size_t)j * d->ld0;
        const int32_t *var = d->avar;
        const double *sign = d->asign;
        for (int i = threadIdx.x; i < ld; i += kBlock) {
            double v = 0.0;
            if (i < m0) v = src[i];
            else if (i < m0 + K && var[i - m0] == j) v = sign[i - m0];
            dst[i] = v;
        }
    } else {
        const int unit = (j < n0 + K) ? m0 + (j - n0) : -1;
        for (int i = threadIdx.x; i < ld; i += kBlock) dst[i] = (i == unit) ? 1.0 : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------
// start of a relaxation from its slack basis (Engine::solve_locked, unit-basis branch): b' = [b0; h], x_B = b'[rho], B^-1 = the
// permutation, and either the orders of the Phase-II start or the Phase-I set-up (simplex.go:529-546): the artificial column
// a_{n+1} = b - sum_{i != minidx} e_{rho_i} (one exact "- 1" per row) into row n of At and the forced no-swap pivot that brings it
// into position minidx.  (The buffers arrive zeroed.)  One workgroup per relaxation.
// IP (here and below): the form of a wave that reads its roots in place (pool knob rev_inplace, rev_child_col.h) — the artificial column
// goes into the relaxation's own row RevLP::art, a child's column comes through ChildCol; IP = false is the kernel on the assembled At.
// ------------------------------------------------------------------------------------------------
template <bool IP>
__global__ __launch_bounds__(kBlock) void k_rv_init(RevLP *lps) {
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int si[kWavesPerBlock];
    RevLP *d = lps + blockIdx.x;
    if (d->warm || d->gen) return;   // k_rv_warm_binv / k_rv_gen_start starts it
    const int m = d->m, n = d->n, ld = d->ld, m0 = d->m0, K = d->K;
    const int32_t *rho0 = d->rho0;
    double *b = d->b, *xb = d->xb, *binv0 = d->binv[0], *c1 = d->c1;
    int32_t *basic = d->basic;
    for (int i = threadIdx.x; i < ld; i += kBlock) b[i] = i < m0 ? d->b0[i] : (i < m ? d->rhs[i - m0] : 0.0);
    for (int j = threadIdx.x; j <= n; j += kBlock) c1[j] = j == n ? 1.0 : 0.0;
    __syncthreads();
    int infeasible = 0;
    unsigned long long bk = ~0ull;
    unsigned int bi = 0xFFFFFFFFu;
    for (int pos = threadIdx.x; pos < m; pos += kBlock) {
        const int r = child_rho(pos, K, m0, rho0);
        const double v = b[r];
        xb[pos] = v;
        basic[pos] = n - 1 - pos;
        binv0[(size_t)pos * ld + r] = 1.0;
        if (v < -1e-13) infeasible = 1;
        amin_take(bk, bi, ordkey(v), (unsigned int)pos);
    }
    infeasible = __syncthreads_or(infeasible);
    if (!infeasible) {
        if (threadIdx.x == 0) {
            d->run = RR_NONE; d->do_lists = 2; d->do_refresh = 2; d->after = RA_P2_LOOP;
        }
        return;
    }
    block_argmin(bk, bi, sk, si);
    const int minidx = (int)bi;   // floats.MinIdx(xb), simplex.go:531
    const int rmin = child_rho(minidx, K, m0, rho0);
    double *art = IP ? d->art : d->At + (size_t)n * ld;
    int nonzero = 0;
    for (int r = threadIdx.x; r < ld; r += kBlock) {
        double v = 0.0;
        if (r < m) v = (r == rmin) ? b[r] : -1 * 1.0 + b[r];
        art[r] = v;
        if (v != 0) nonzero = 1;
    }
    nonzero = __syncthreads_or(nonzero);
    if (threadIdx.x == 0) {
        d->phase1_used = 1;
        if (!nonzero) {   // verifyInputs of the recursive call: an empty column
            d->status = GOMILP_ERR_PHASE1_WRAPPED; d->wrapped = GOMILP_ERR_ZERO_COLUMN; d->stage = RS_DONE; d->run = RR_NONE;
        } else {
            d->f_var = n; d->f_pos = -1; d->f_p = minidx; d->f_noswap = 1;
            d->run = RR_FORCED; d->do_lists = 1; d->do_refresh = 1; d->after = RA_P1_LOOP;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// start of a warm relaxation from its parent's kept state (k_warm_binv of dual_kernels.hip per relaxation, Engine::warm_locked):
//   B^-1 = [[B_p^-1, 0], [R, I_J]],  R[k, :] = -sign_k * B_p^-1[kpos_k, :] where var_k is basic at parent position kpos_k, else 0,
// padding columns zero (the parent's ldp may differ from ld); the basis list is the parent's positions, then the slacks of the J new
// rows (the last J columns); b' as k_rv_init; the orders: ascending nonbasic list of the n columns, x_B = B^-1 b and y = B^-T c_B
// (the parent's y, zeros appended: dual feasible), then the dual loop.  grid: (rows of the tallest relaxation, relaxations).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rv_warm_binv(RevLP *lps) {
    RevLP *d = lps + blockIdx.y;
    if (!d->warm) return;
    const int i = blockIdx.x, m = d->m, n = d->n, ld = d->ld, mp = d->wmp, ldp = d->wldp, J = d->wJ;
    if (i >= m) return;
    const double *Bp = d->wbinv;
    double *dst = d->binv[0] + (size_t)i * ld;
    if (i < mp) {
        const double *src = Bp + (size_t)i * ldp;
        for (int c = threadIdx.x; c < ld; c += kBlock) dst[c] = c < mp ? src[c] : 0.0;
    } else {
        const int k = i - mp, pos = d->wkpos[k];
        const double s = -d->wsign[k];
        const double *src = pos >= 0 ? Bp + (size_t)pos * ldp : nullptr;
        for (int c = threadIdx.x; c < ld; c += kBlock) dst[c] = c < mp ? (src ? s * src[c] : 0.0) : (c == i ? 1.0 : 0.0);
    }
    if (i != 0) return;
    const int m0 = d->m0;
    double *b = d->b;
    int32_t *basic = d->basic;
    const int32_t *wbasic = d->wbasic;
    for (int r = threadIdx.x; r < ld; r += kBlock) b[r] = r < m0 ? d->b0[r] : (r < m ? d->rhs[r - m0] : 0.0);
    for (int pos = threadIdx.x; pos < m; pos += kBlock) basic[pos] = pos < mp ? wbasic[pos] : n - J + (pos - mp);
    if (threadIdx.x == 0) {
        d->run = RR_NONE; d->do_lists = 2; d->do_refresh = 1; d->after = RA_DUAL_LOOP;
    }
}

// ------------------------------------------------------------------------------------------------
// start of a relaxation whose root has no slack basis, from the root's searched basis (RevLP::gen; k_b_setup's general branch on B^-1
// instead of the tableau): the child's basis is its K branch slacks — position pos < K: the slack of branch row kk = K - 1 - pos, the
// descending scan of findLinearlyIndependent meets them first — then the root's basis, and by block elimination, copies and sign flips only,
//   B^-1 row pos < K:   [-sign_kk * B0^-1[p0(var_kk), :] | e_{m0 + kk}]  (zeros where var_kk is nonbasic at the root),   row K + i: [B0^-1 row i | 0],
//   x_B = [rhs_kk - sign_kk * x0[var_kk] ; x_B0].
// A worker computes this x_B by a fresh gonum-order solve of the child's basis, whose last bits may differ: where the start's decisions
// (feasible at -1e-13; the position of the minimum) could turn on them — an entry within 1e-9 of the threshold, the minimum and its
// runner-up within 1e-9 max(1, |min|) — the relaxation goes to a worker's whole solve (RS_HOST).  Else the orders of the Phase-II start, or
// of the Phase-I set-up with gminidx for k_rv_gen_art.  grid: (rows of the tallest relaxation, relaxations); workgroup 0 of a relaxation
// does everything but the rows of B^-1.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rv_gen_start(RevLP *lps) {
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int si[kWavesPerBlock];
    __shared__ unsigned long long ss[kWavesPerBlock];
    RevLP *d = lps + blockIdx.y;
    if (!d->gen) return;
    const int i = blockIdx.x, m = d->m, n = d->n, ld = d->ld, m0 = d->m0, n0 = d->n0, K = d->K, ldg = d->ldg;
    if (i >= m) return;
    const double *B0 = d->gB0inv;
    const int32_t *posvar = d->gposvar0;
    double *dst = d->binv[0] + (size_t)i * ld;
    if (i >= K) {
        const double *src = B0 + (size_t)(i - K) * ldg;
        for (int c = threadIdx.x; c < ld; c += kBlock) dst[c] = c < m0 ? src[c] : 0.0;
    } else {
        const int kk = K - 1 - i, pos = posvar[d->avar[kk]];
        const double s = -d->asign[kk];
        const double *src = pos >= 0 ? B0 + (size_t)pos * ldg : nullptr;
        for (int c = threadIdx.x; c < ld; c += kBlock) dst[c] = c < m0 ? (src ? s * src[c] : 0.0) : (c == m0 + kk ? 1.0 : 0.0);
    }
    if (i != 0) return;
    double *b = d->b, *xb = d->xb, *c1 = d->c1;
    int32_t *basic = d->basic;
    const double *xb0 = d->gxb0;
    const int32_t *basic0 = d->gbasic0;
    for (int r = threadIdx.x; r < ld; r += kBlock) b[r] = r < m0 ? d->b0[r] : (r < m ? d->rhs[r - m0] : 0.0);
    for (int j = threadIdx.x; j <= n; j += kBlock) c1[j] = j == n ? 1.0 : 0.0;
    int infeasible = 0, close = 0;
    unsigned long long bk = ~0ull, b2 = ~0ull;
    unsigned int bi = 0xFFFFFFFFu;
    for (int pos = threadIdx.x; pos < m; pos += kBlock) {
        double v;
        if (pos < K) {
            const int kk = K - 1 - pos, pv = posvar[d->avar[kk]];
            v = d->rhs[kk] - d->asign[kk] * (pv >= 0 ? xb0[pv] : 0.0);
            basic[pos] = n0 + kk;
        } else {
            v = xb0[pos - K];
            basic[pos] = basic0[pos - K];
        }
        xb[pos] = v;
        if (v < -1e-13) infeasible = 1;
        if (fabs(v + 1e-13) <= 1e-9) close = 1;
        amin2_take(bk, bi, b2, ordkey(v), (unsigned int)pos, ~0ull);
    }
    infeasible = __syncthreads_or(infeasible);
    close = __syncthreads_or(close);
    block_argmin2(bk, bi, b2, sk, si, ss);
    if (threadIdx.x != 0) return;
    const double vmin = orddecode(bk), v2 = orddecode(b2);
    if (close || (b2 != ~0ull && v2 - vmin <= 1e-9 * fmax(1.0, fabs(vmin)))) {
        d->stage = RS_HOST; d->run = RR_NONE;
        return;
    }
    if (!infeasible) {
        d->run = RR_NONE; d->do_lists = 2; d->do_refresh = 2; d->after = RA_P2_LOOP;
    } else {
        d->phase1_used = 1; d->gminidx = (int)bi;   // floats.MinIdx(xb), simplex.go:531
        d->f_var = n; d->f_pos = -1; d->f_p = (int)bi; d->f_noswap = 1;
        d->run = RR_FORCED; d->do_lists = 1; d->do_refresh = 1; d->after = RA_P1_LOOP;
    }
}

// ------------------------------------------------------------------------------------------------
// Phase-I artificial column of a searched start (k_gs_art of general_kernels.hip per relaxation; simplex.go:536-542): a_{n+1} = b minus
// every basic column but the one at position gminidx, by ascending position, element by element as `-1 * a + art` (floats.Sub per column),
// into row n of At (IP: the relaxation's row `art`).  One thread per row — consecutive threads read consecutive elements of a column —
// and one workgroup per relaxation, which therefore sees whether the column is empty (verifyInputs of the recursive call).
// ------------------------------------------------------------------------------------------------
template <bool IP>
__global__ __launch_bounds__(kBlock) void k_rv_gen_art(RevLP *lps) {
    RevLP *d = lps + blockIdx.x;
    if (!d->gen || d->stage != RS_RUN || d->run != RR_FORCED || d->gminidx < 0) return;
    const int m = d->m, n = d->n, ld = d->ld, minidx = d->gminidx;
    const double *At = d->At, *b = d->b;
    const int32_t *basic = d->basic;
    double *art = IP ? d->art : d->At + (size_t)n * ld;
    int nonzero = 0;
    for (int r = threadIdx.x; r < ld; r += kBlock) {
        double acc = 0.0;
        if (r < m) {
            acc = b[r];
            for (int pos = 0; pos < m; pos++) {
                if (pos == minidx) continue;
                const int j = basic[pos];
                double a;
                if constexpr (IP) a = ChildCol(d, j).elem(r);
                else a = At[(size_t)j * ld + r];
                acc = __dadd_rn(__dmul_rn(-1.0, a), acc);
            }
        }
        art[r] = acc;
        if (acc != 0) nonzero = 1;
    }
    nonzero = __syncthreads_or(nonzero);
    if (threadIdx.x == 0) {
        d->gminidx = -1;
        if (!nonzero) {
            d->status = GOMILP_ERR_PHASE1_WRAPPED; d->wrapped = GOMILP_ERR_ZERO_COLUMN; d->stage = RS_DONE; d->run = RR_NONE; clear_orders(d);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K1-K3, relaxation = blockIdx.y.  MODE = RR_LOOP: a pivot of the loop; RR_FORCED: the forced pivot of the Phase-I set-up;
// RR_DUAL (K2 / K3 only): a dual pivot of a warm start — the entering position from the partials of k_rv_dual_price, the leaving
// row from the state (kDualPick).
// The fields of the RevLP go into locals once (simplex_helpers.h: why the helpers take pointers).
//
// The Bland rule (Engine::host_bland; replaceBland, simplex.go:347-383) runs inside the loop: k_rv_bland, one small workgroup per
// relaxation in front of every pivot, looks at a loop that stopped with ST_NEED_BLAND — r rounded at rRoundTol, the first position
// with r <= -blandNegTol is the candidate — and turns the pivot behind it into the Bland step: K1 is skipped (the reduced costs of the
// stopped pivot stand), K2 runs the FTRAN of the candidate's column, K3 takes the leaving row by replaceBland's rule and commits with
// bland = 1.  The candidate's own minimum row always passes the rule's test (bland_leaving), so the first candidate is the last: no
// cursor over candidates is needed, and a degenerate step costs one pivot's launches and no host round trip.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rv_bland(RevLP *__restrict__ lps, const int *__restrict__ act) {
    __shared__ unsigned int sm[kWavesPerBlock];
    RevLP *d = lps + act[blockIdx.x];
    if (d->run != RR_LOOP) return;
    DevState *st = d->st;
    const bool need = st->done != 0 && st->status == ST_NEED_BLAND && d->bland_failed == 0;   // (uniform: written below behind the barriers)
    if (!need) {
        if (threadIdx.x == 0) d->bl = 0;
        return;
    }
    const int nn = d->nn;
    const double *rvec = d->rvec;
    unsigned int first = 0xFFFFFFFFu;
    for (int j = threadIdx.x; j < nn; j += kBlock) {
        double r = rvec[j];
        if (fabs(r) < 1e-13) r = 0;   // rRoundTol, :252-256
        if (r > -1e-14) continue;     // blandNegTol, :352
        first = (unsigned int)j;
        break;
    }
    first = block_min_u32(first, sm);
    if (threadIdx.x == 0) {
        if (first == 0xFFFFFFFFu) { d->bland_failed = 1; d->bl = 0; }   // lp.ErrBland: k_rv_ctrl ends the loop
        else { st->done = 0; st->status = ST_RUNNING; d->bl = 1; d->bl_pos = (int)first; }
    }
}

// column j of a relaxation's matrix as a loader: from its root in place (IP), or row j of the assembled At
template <bool IP>
__device__ __forceinline__ auto child_col(const RevLP *d, const double *At, int ld, int j) {
    if constexpr (IP) return ChildCol(d, j);
    else return PlainCol(At + (size_t)j * ld);
}

// G (K1-K3): the exact-step guard of simplex_helpers.h for the relaxations of a searched start (RevLP::gen, RevLP::guard): the runner-up keys
// beside the winners, ST_NEED_EXACT where a worker's loop takes an exact step (k_rv_ctrl: RS_HOST).  G = false is the kernel as it was.
template <bool IP, bool CK, bool G = false>
__global__ __launch_bounds__(kBlock) void k_rv_price(RevLP *__restrict__ lps, const int *__restrict__ act, int ck2) {
    extern __shared__ __attribute__((aligned(16))) double2 svec[];
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int si[kWavesPerBlock];
    __shared__ unsigned long long ss[G ? kWavesPerBlock : 1];
    const RevLP *d = lps + act[blockIdx.y];
    if (d->run != RR_LOOP || d->bl) return;
    DevState *st = d->st;
    if (!price_gate(st)) return;
    const int ld = d->ld, nn = d->nn;
    const double *At = d->At, *cost = d->cost, *y = d->y;
    double *rvec = d->rvec;
    const int32_t *nonbasic = d->nonbasic;
    unsigned long long *pk = d->pk_price;
    unsigned int *pi = d->pi_price;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlock;
    unsigned long long bk = ~0ull, b2 = ~0ull;
    unsigned int bi = 0xFFFFFFFFu;
    sweep_rows<CK, 1>([&](int pos) { return child_col<IP>(d, At, ld, nonbasic[pos]); }, {PlainCol(y)}, nn, wave, nwaves, ld, svec, ck2, lane,
                      [&](int pos, const double (&dot)[1]) { price_elem<G>(cost, rvec, pos, nonbasic[pos], dot[0], lane, bk, bi, b2); });
    publish<G>(bk, bi, b2, sk, si, ss, pk, pi);
}

template <int MODE, bool IP, bool CK, bool G = false>
__global__ __launch_bounds__(kBlock) void k_rv_ftran(RevLP *__restrict__ lps, const int *__restrict__ act, int nparts_price, int ck2) {
    extern __shared__ __attribute__((aligned(16))) double2 svec[];
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int si[kWavesPerBlock];
    __shared__ unsigned long long ss[G ? kWavesPerBlock : 1];
    RevLP *d = lps + act[blockIdx.y];
    if (d->run != MODE) return;
    DevState *st = d->st;
    const int m = d->m, ld = d->ld, flips = d->flips;
    int forced_pos, forced_var;
    if constexpr (MODE == RR_DUAL) { forced_pos = kDualPick; forced_var = -1; }
    else { forced_pos = MODE == RR_FORCED ? d->f_pos : (d->bl ? d->bl_pos : -1); forced_var = MODE == RR_FORCED ? d->f_var : -1; }
    const double tol = d->tol;
    const double *At = d->At, *binv_cur = d->binv[flips & 1], *xb = d->xb;
    double *rvec = d->rvec, *dvec = d->dvec, *move = d->move;
    const int32_t *nonbasic = d->nonbasic;
    const unsigned long long *pkp = d->pk_price;
    const unsigned int *pip = d->pi_price;
    unsigned long long *pk = d->pk_ratio;
    unsigned int *pi = d->pi_ratio;
    int var;
    double guard = 0.0;
    if constexpr (G) guard = d->guard;
    if (!pick_entering<G>(st, pkp, pip, nparts_price, rvec, nonbasic, tol, guard, forced_pos, forced_var, sk, si, ss, var)) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) d->flips_k2 = flips;   // K3 of this pivot reads the parity K2 worked on
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlock;
    unsigned long long bk = ~0ull, b2 = ~0ull;
    unsigned int bi = 0xFFFFFFFFu;
    sweep_rows<CK, 1>([&](int i) { return PlainCol(binv_cur + (size_t)i * ld); }, {child_col<IP>(d, At, ld, var)}, m, wave, nwaves, ld, svec, ck2, lane,
                      [&](int i, const double (&dot)[1]) { ratio_elem<G>(xb, dvec, move, i, dot[0], lane, bk, bi, b2); });
    publish<G>(bk, bi, b2, sk, si, ss, pk, pi);
}

// replaceBland's leaving row for the candidate whose FTRAN just ran (Engine::host_bland; simplex.go:357-380): the first-index
// minimum of move; all-infinite: unbounded (computeMove, :328); |move| <= blandZeroTol: the first row with move <= 1e-12 (the
// minimum's own row satisfies it, so the candidate is always taken).  false: the loop has stopped or stops here.
__device__ __forceinline__ bool bland_leaving(DevState *st, const unsigned long long *pk, const unsigned int *pi, int nparts_ratio,
                                              const double *move, int m, unsigned long long *sk, unsigned int *si, int &p) {
    if (st->done) return false;
    p = (int)reduce_partials(pk, pi, nparts_ratio, sk, si, nullptr);
    const double mv = move[p];
    if (mv == __builtin_inf()) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { st->done = 1; st->status = ST_UNBOUNDED; st->p = p; st->mv = mv; }
        return false;
    }
    if (!(fabs(mv) > 1e-12)) {
        unsigned int first = 0xFFFFFFFFu;
        for (int i = threadIdx.x; i < m; i += kBlock)
            if (!(move[i] > 1e-12)) { first = (unsigned int)i; break; }
        p = (int)block_min_u32(first, si);
    }
    return true;
}

template <int MODE, bool CK, bool G = false>
__global__ __launch_bounds__(kBlock) void k_rv_update(RevLP *__restrict__ lps, const int *__restrict__ act, int nparts_ratio, int ck2) {
    extern __shared__ __attribute__((aligned(16))) double2 svec[];
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int si[kWavesPerBlock];
    __shared__ unsigned long long ss[G ? kWavesPerBlock : 1];
    RevLP *d = lps + act[blockIdx.y];
    if (d->run != MODE) return;
    DevState *st = d->st;
    const int m = d->m, ld = d->ld, flips = d->flips_k2, phase = d->phase;
    int forced_p, no_swap, bland;
    if constexpr (MODE == RR_DUAL) { forced_p = kDualPick; no_swap = 0; bland = 0; }
    else { forced_p = MODE == RR_FORCED ? d->f_p : -1; no_swap = MODE == RR_FORCED ? d->f_noswap : 0; bland = MODE == RR_FORCED ? 0 : d->bl; }
    const double *binv_cur = d->binv[flips & 1];
    double *binv_next = d->binv[(flips + 1) & 1];
    double *xb = d->xb, *y = d->y, *dvec = d->dvec, *move = d->move;
    int32_t *basic = d->basic, *nonbasic = d->nonbasic;
    const unsigned long long *pk = d->pk_ratio;
    const unsigned int *pi = d->pi_ratio;
    int p;
    if (bland) {
        if (!bland_leaving(st, pk, pi, nparts_ratio, move, m, sk, si, p)) return;
    } else {
        double guard = 0.0;
        if constexpr (G) guard = d->guard;
        if (!pick_leaving<G>(st, pk, pi, nparts_ratio, move, dvec, guard, forced_p, sk, si, ss, p)) return;
    }
    const double dpv = dvec[p];
    const double *rowp_g = binv_cur + (size_t)p * ld;   // old row p
    update_rows<CK>(binv_cur, binv_next, ld, dvec, m, p, dpv, rowp_g, svec, ck2);
    if (blockIdx.x == 0) {
        commit_pivot(st, xb, y, dvec, move, basic, nonbasic, nullptr, 0, phase, m, ld, p, dpv, CK ? rowp_g : reinterpret_cast<const double *>(svec), no_swap,
                     bland);
        if (threadIdx.x == 0) {
            d->flips = flips + 1;
            if (bland) d->bland += 1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// the dual loop of a warm start: k_dual_leave / k_dual_price of dual_kernels.hip with the relaxation as a grid dimension, in front of
// k_rv_ftran<RR_DUAL> / k_rv_update<RR_DUAL>.  DevState::max_pivots holds the dual-pivot budget (k_rv_check).
// ------------------------------------------------------------------------------------------------

// leaving row: first index of min x_B, stop at >= -1e-13 (kDualFeasTol of engine_warm.cpp).  One workgroup per relaxation.
__global__ __launch_bounds__(kBlock) void k_rv_dual_leave(RevLP *__restrict__ lps, const int *__restrict__ act) {
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int si[kWavesPerBlock];
    const RevLP *d = lps + act[blockIdx.x];
    if (d->run != RR_DUAL) return;
    DevState *st = d->st;
    if (st->done) return;
    const int m = d->m;
    const double *xb = d->xb;
    unsigned long long bk = ~0ull;
    unsigned int bi = 0xFFFFFFFFu;
    for (int i = threadIdx.x; i < m; i += kBlock) amin_take(bk, bi, ordkey(xb[i]), (unsigned int)i);
    block_argmin(bk, bi, sk, si);
    if (threadIdx.x == 0) {
        const double xmin = orddecode(bk);
        if (!(xmin < -1e-13) || bi >= (unsigned int)m) { st->done = 1; st->status = ST_OPTIMAL; }
        else if (st->max_pivots > 0 && st->pivots >= st->max_pivots) { st->done = 1; st->status = ST_MAX_PIVOTS; }
        else st->p = (int)bi;
    }
}

// dual pricing: per nonbasic column a_j.y and a_j.rho (rho = row p of B^-1), the row of At read once for both; r_pos = cost[j] - a_j.y
// into rvec, the ratio r_j / -alpha_pj over alpha_pj < -1e-13 as a first-index argmin (k_dual_price's rule).  CK = false: y and rho staged
// whole, 2 * ld doubles of LDS, ld <= kRevDualLd; CK = true: streamed ck2 double2 each at a time, ck2 <= kRevDualLd / 2 (2 * ck2 double2 of
// LDS: 64 KB at most).
template <bool IP, bool CK>
__global__ __launch_bounds__(kBlock) void k_rv_dual_price(RevLP *__restrict__ lps, const int *__restrict__ act, int ck2) {
    extern __shared__ __attribute__((aligned(16))) double2 svec[];
    __shared__ unsigned long long sk[kWavesPerBlock];
    __shared__ unsigned int si[kWavesPerBlock];
    const RevLP *d = lps + act[blockIdx.y];
    if (d->run != RR_DUAL) return;
    const DevState *st = d->st;
    if (st->done) return;
    const int ld = d->ld, nn = d->nn;
    const double *At = d->At, *cost = d->cost, *y = d->y;
    double *rvec = d->rvec;
    const int32_t *nonbasic = d->nonbasic;
    unsigned long long *pk = d->pk_price;
    unsigned int *pi = d->pi_price;
    const double *rho = d->binv[d->flips & 1] + (size_t)st->p * ld;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlock;
    unsigned long long bk = ~0ull;
    unsigned int bi = 0xFFFFFFFFu;
    sweep_rows<CK, 2>([&](int pos) { return child_col<IP>(d, At, ld, nonbasic[pos]); }, {PlainCol(y), PlainCol(rho)}, nn, wave, nwaves, ld, svec, ck2, lane,
                      [&](int pos, const double (&dot)[2]) {
                          const double r = cost[nonbasic[pos]] - dot[0], da = dot[1];
                          if (lane == 0) rvec[pos] = r;
                          amin_take(bk, bi, ordkey(da < -1e-13 ? r / (-da) : __builtin_inf()), (unsigned int)pos);
                      });
    publish_partials(bk, bi, sk, si, pk, pi);
}

// ------------------------------------------------------------------------------------------------
// set-up launches behind the forced pivot: index lists, refreshes, the check that starts the loop
// ------------------------------------------------------------------------------------------------

// do_lists: the artificial (1) or the exchanged column f_var (3) into the basis list, and the nonbasic list as the ascending ids outside
// the basis (simplex.go:174-184)
__global__ __launch_bounds__(kBlock) void k_rv_lists(RevLP *__restrict__ lps, const int *__restrict__ act) {
    __shared__ int wtot[kWavesPerBlock];
    RevLP *d = lps + act[blockIdx.x];
    const int mode = d->do_lists;
    if (mode == 0 || d->stage != RS_RUN) return;
    const int m = d->m, n = d->n, ncols = mode == 1 ? n + 1 : n;
    int32_t *basic = d->basic, *nonbasic = d->nonbasic, *inb = d->inb;
    if (mode != 2 && threadIdx.x == 0) basic[d->f_p] = mode == 1 ? n : d->f_var;
    for (int j = threadIdx.x; j <= n; j += kBlock) inb[j] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += kBlock) inb[basic[i]] = 1;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int off = 0;
    for (int base = 0; base < ncols; base += kBlock) {
        const int j = base + threadIdx.x;
        const bool out = j < ncols && !inb[j];
        const unsigned long long bal = __ballot(out);
        if (lane == 0) wtot[w] = __popcll(bal);
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int t = 0; t < kWavesPerBlock; t++) { if (t < w) woff += wtot[t]; tot += wtot[t]; }
        if (out) nonbasic[off + woff + __popcll(bal & ((1ull << lane) - 1ull))] = j;
        off += tot;
        __syncthreads();
    }
}

// x_B = B^-1 b (k_matvec_rows)
template <bool CK>
__global__ __launch_bounds__(kBlock) void k_rv_matvec(RevLP *__restrict__ lps, const int *__restrict__ act, int ck2) {
    extern __shared__ __attribute__((aligned(16))) double2 svec[];
    const RevLP *d = lps + act[blockIdx.y];
    if (d->do_refresh != 1 || d->stage != RS_RUN) return;
    const int m = d->m, ld = d->ld;
    const double *M = d->binv[d->flips & 1], *vec = d->b;
    double *out = d->xb;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlock;
    sweep_rows<CK, 1>([&](int i) { return PlainCol(M + (size_t)i * ld); }, {PlainCol(vec)}, m, wave, nwaves, ld, svec, ck2, lane,
                      [&](int i, const double (&dot)[1]) { if (lane == 0) out[i] = dot[0]; });
}

// y = B^-T c_B in the arithmetic of k_y_partial / k_y_reduce (the chunking of launch_y_from_binv for this relaxation's m);
// blockIdx.y = chunk, blockIdx.z = list position
__global__ __launch_bounds__(kBlock) void k_rv_y_partial(RevLP *__restrict__ lps, const int *__restrict__ act) {
    const RevLP *d = lps + act[blockIdx.z];
    if (d->do_refresh == 0 || d->stage != RS_RUN) return;
    const int m = d->m, ld = d->ld;
    int nchunks = (m + 63) / 64;
    nchunks = nchunks > 64 ? 64 : nchunks;
    const int rows_per_chunk = (m + nchunks - 1) / nchunks;
    const int j = blockIdx.x * kBlock + threadIdx.x;
    const int chunk = blockIdx.y;
    if (chunk >= nchunks || j >= ld) return;
    const double *binv = d->binv[d->flips & 1], *cost = d->after == RA_P1_LOOP ? d->c1 : d->c2;
    const int32_t *basic = d->basic;
    const int i0 = chunk * rows_per_chunk, i1 = min(m, i0 + rows_per_chunk);
    double acc = 0;
    for (int i = i0; i < i1; i++) {
        const double cb = cost[basic[i]];
        if (cb != 0) acc += cb * binv[(size_t)i * ld + j];
    }
    d->yscratch[(size_t)chunk * ld + j] = acc;
}
__global__ __launch_bounds__(kBlock) void k_rv_y_reduce(RevLP *__restrict__ lps, const int *__restrict__ act) {
    const RevLP *d = lps + act[blockIdx.y];
    if (d->do_refresh == 0 || d->stage != RS_RUN) return;
    const int m = d->m, ld = d->ld;
    int nchunks = (m + 63) / 64;
    nchunks = nchunks > 64 ? 64 : nchunks;
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= ld) return;
    const double *scratch = d->yscratch;
    double acc = 0;
    for (int c = 0; c < nchunks; c++) acc += scratch[(size_t)c * ld + j];
    d->y[j] = acc;
}

// behind the set-up launches: the PANIC test of the Phase-I start (simplex.go:155-158 in the recursive call), the loop's state
__global__ __launch_bounds__(kBlock) void k_rv_check(RevLP *__restrict__ lps, const int *__restrict__ act) {
    RevLP *d = lps + act[blockIdx.x];
    const int after = d->after;
    if (after == RA_NONE || d->stage != RS_RUN) return;
    DevState *st = d->st;
    const int m = d->m, n = d->n;
    if (after == RA_P1_LOOP) {
        const double *xb = d->xb;
        int bad = 0;
        for (int i = threadIdx.x; i < m; i += kBlock) if (xb[i] < -1e-13) bad = 1;
        bad = __syncthreads_or(bad);
        if (bad) {
            if (threadIdx.x == 0) { d->status = GOMILP_ERR_PANIC; d->stage = RS_DONE; d->run = RR_NONE; clear_orders(d); }
            return;
        }
    }
    if (threadIdx.x == 0) {
        if (after == RA_P1_LOOP) {
            start_loop_state(st, d->max_pivots);
            d->phase = 1; d->nn = n + 1 - m; d->tol = 1e-10; d->cost = d->c1;
        } else if (after == RA_DUAL_LOOP) {
            start_loop_state(st, d->dual_budget);
            d->phase = 3; d->nn = n - m; d->tol = d->tol_user; d->cost = d->c2;
        } else {
            start_loop_state(st, d->max_pivots);
            d->phase = 2; d->nn = n - m; d->tol = d->tol_user; d->cost = d->c2;
        }
        d->run = after == RA_DUAL_LOOP ? RR_DUAL : RR_LOOP;
        clear_orders(d);
    }
}

// ------------------------------------------------------------------------------------------------
// control step behind a chunk of pivots: what a stopped loop means (Engine::run_loop's switch, the Phase-I verdict of
// Engine::solve_locked), the orders of the next superstep, the record the host reads.  One workgroup per active relaxation.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rv_ctrl(RevLP *__restrict__ lps, const int *__restrict__ act, RevOut *__restrict__ out) {
    __shared__ unsigned int sm[kWavesPerBlock];
    const int id = act[blockIdx.x];
    RevLP *d = lps + id;
    DevState *st = d->st;
    // (a loop that stopped for a Bland step goes on: k_rv_bland takes it in front of the next pivot)
    const bool stopped = d->stage == RS_RUN && d->run == RR_LOOP && st->done != 0 &&
                         !(st->status == ST_NEED_BLAND && d->bland_failed == 0);   // (uniform: nothing below writes these before the last barrier)
    if (stopped) {
        const int status = st->status, phase = d->phase, m = d->m, n = d->n;
        if (status == ST_NEED_BLAND) {   // replaceBland ran out of candidates: lp.ErrBland
            if (threadIdx.x == 0) {
                if (phase == 1) { d->piv1 = st->pivots; d->status = GOMILP_ERR_PHASE1_WRAPPED; d->wrapped = GOMILP_ERR_BLAND; }
                else { d->piv2 = st->pivots; d->status = GOMILP_ERR_BLAND; }
                d->stage = RS_DONE; d->run = RR_NONE;
            }
        } else if (status == ST_NEED_EXACT) {
            // a guarded loop (RevLP::gen) stopped where a worker's loop takes an exact step — a decision on a fresh gonum-order solve: a
            // worker solves the relaxation, whole
            if (threadIdx.x == 0) { d->stage = RS_HOST; d->run = RR_NONE; }
        } else {
            const int rc = status == ST_OPTIMAL ? GOMILP_OK : status == ST_UNBOUNDED ? GOMILP_ERR_UNBOUNDED
                         : status == ST_MAX_PIVOTS ? GOMILP_ERR_UNSUPPORTED : GOMILP_ERR_DEVICE;
            if (phase == 2) {
                if (threadIdx.x == 0) { d->piv2 = st->pivots; d->status = rc; d->stage = RS_DONE; d->run = RR_NONE; }
            } else if (rc != GOMILP_OK) {
                if (threadIdx.x == 0) {
                    d->piv1 = st->pivots; d->stage = RS_DONE; d->run = RR_NONE;
                    if (rc == GOMILP_ERR_DEVICE) d->status = rc;
                    else { d->status = GOMILP_ERR_PHASE1_WRAPPED; d->wrapped = rc; }   // simplex.go:557-559
                }
            } else {
                // Phase I ended at its optimum: where is the artificial, and at what level (simplex.go:561-565)
                const int32_t *basic = d->basic;
                unsigned int added = 0xFFFFFFFFu;
                for (int i = threadIdx.x; i < m; i += kBlock) if (basic[i] == n) added = (unsigned int)i;
                added = block_min_u32(added, sm);
                if (threadIdx.x == 0) {
                    d->piv1 = st->pivots;
                    const double xart = added != 0xFFFFFFFFu ? d->xb[added] : 0.0;
                    if (added != 0xFFFFFFFFu && fabs(xart) > 1e-13 && fabs(xart) < 1e-11) {
                        d->stage = RS_HOST; d->run = RR_NONE;   // too close to phaseIZeroTol: the verdict needs a fresh gonum-order solve
                    } else if (fabs(xart) > 1e-12) {
                        d->status = GOMILP_ERR_INFEASIBLE; d->stage = RS_DONE; d->run = RR_NONE;
                    } else if (added != 0xFFFFFFFFu) {
                        // the artificial stayed basic at level zero: the exchange of simplex.go:581-606 — the candidate scan in front of
                        // the next superstep's set-up launches, or (rev_exchange = 0) a worker's whole solve
                        if (d->exch_on) { d->run = RR_EXCH; d->x_added = (int)added; d->x_best = 0xFFFFFFFFu; }
                        else { d->stage = RS_HOST; d->run = RR_NONE; }
                    } else {
                        d->run = RR_NONE; d->do_lists = 2; d->do_refresh = 1; d->after = RA_P2_LOOP;
                    }
                }
            }
        }
    }
    // a dual loop that stopped (Engine::run_dual_loop's verdicts): primal feasible — the orders of a Phase-II start (ascending list,
    // fresh x_B / y: the "finish" of Engine::warm_locked); no ratio in the leaving row — the LP is infeasible, no x; the budget spent —
    // RS_COLD: the host re-initialises the slot and this run solves it cold
    if (d->stage == RS_RUN && d->run == RR_DUAL && st->done != 0 && threadIdx.x == 0) {
        const int status = st->status;
        d->pivd = st->pivots; d->run = RR_NONE;
        if (status == ST_OPTIMAL) { d->do_lists = 2; d->do_refresh = 1; d->after = RA_P2_LOOP; }
        else if (status == ST_DUAL_INFEASIBLE) { d->status = GOMILP_ERR_INFEASIBLE; d->stage = RS_DONE; }
        else if (status == ST_MAX_PIVOTS) d->stage = RS_COLD;
        else { d->status = GOMILP_ERR_DEVICE; d->stage = RS_DONE; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        RevOut o;
        o.stage = d->stage; o.status = d->status; o.wrapped = d->wrapped; o.phase1_used = d->phase1_used;
        o.piv1 = d->piv1; o.piv2 = d->piv2; o.bland = d->bland; o.pivd = d->pivd;
        o.flips = d->flips; o.dual = (d->run == RR_DUAL || d->after == RA_DUAL_LOOP) ? 1 : 0;
        o.scan = d->run == RR_EXCH ? 1 : 0; o.exch = d->exch;
        out[id] = o;
    }
}

// ------------------------------------------------------------------------------------------------
// The zero-level artificial exchange (Engine::solve_locked behind the Phase-I verdict; simplex.go:581-606): the artificial stayed basic
// at position `added` with x_B[added] = 0, and the first column j < n outside the basis, in ascending id, takes its place for which
//   d = B^-1 a_j,  |d_added| > 1e-9 max(1, max_i |d_i|)   and no   v_i < -1e-13,  v_added = theta = x_B[added] / d_added, v_i = x_B[i] - theta d_i.
// A worker tries the columns one after the other, one FTRAN and one round trip each; here every candidate is tried at once, one
// workgroup each, and the smallest id that passes wins an atomic min: the same column.  The candidates are the entries of the Phase-I
// loop's nonbasic list (n + 1 - m ids, every column outside the basis; the artificial is basic and not among them), in whatever order
// the loop's swaps left them: the minimum does not depend on it.  Every d_i is the dot product k_rv_ftran<RR_FORCED> computes for that
// column — a_j staged in LDS, one wave per row of the current B^-1 — so the verdicts at the two thresholds are the worker's, and the
// comparisons are written as the worker writes them (a NaN rejects through d_added only; its std::max skips a NaN in max_i |d_i|).
// d_added comes first: |d_added| <= 1e-9 fails whatever the maximum is, and such a candidate costs one row, not m.
// x_best is the one word a kernel of this file reads while its own launch writes it: a workgroup whose id is above a passing id it
// happens to see ends early.  That changes the work done, never the minimum.
// Dynamic LDS: ld doubles, as K2.  grid: (nonbasic positions of the widest relaxation, list positions).
// ------------------------------------------------------------------------------------------------
template <bool IP, bool CK>
__global__ __launch_bounds__(kBlock) void k_rv_exch(RevLP *__restrict__ lps, const int *__restrict__ act, int ck2) {
    extern __shared__ __attribute__((aligned(16))) double2 svec[];
    __shared__ double smax[kWavesPerBlock];
    RevLP *d = lps + act[blockIdx.y];
    if (d->run != RR_EXCH) return;
    const int m = d->m, n = d->n, ld = d->ld, added = d->x_added, pos = blockIdx.x;
    if (pos >= d->nn) return;
    const int j = d->nonbasic[pos];
    if (j < 0 || j >= n) return;   // (row n of At is the artificial: never a candidate)
    __shared__ unsigned int seen;
    if (threadIdx.x == 0) seen = __atomic_load_n(&d->x_best, __ATOMIC_RELAXED);
    __syncthreads();
    if (seen < (unsigned int)j) return;   // (workgroup-uniform)
    const double *binv_cur = d->binv[d->flips & 1], *xb = d->xb;
    const auto col = child_col<IP>(d, d->At, ld, j);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // d_added first, as one row's chunked dot by every wave (the same bits in each, workgroup-uniform; CK = false: the one chunk [0, ld2))
    const int ld2 = ld >> 1, cb = CK ? ck2 : ld2;
    DotAcc acc[1] = {{0, 0, 0, 0}};
    for (int c0 = 0; c0 < ld2; c0 += cb) {
        const int c1 = min(c0 + cb, ld2);
        stage_chunk<1>(svec, cb, {col}, c0, c1);
        wave_dot_chunk<1>(PlainCol(binv_cur + (size_t)added * ld), svec, cb, c0, c1, ld2, lane, acc);
    }
    const double dpv = wave_dot_finish(acc[0]);
    if (!(fabs(dpv) > 1e-9)) return;
    const double theta = xb[added] / dpv;
    double dmax = 0;
    int bad = 0;
    if constexpr (!CK) __syncthreads();   // (the sweep stages a_j again: no wave reads svec any more)
    // the rows by the workgroup's own kWavesPerBlock waves: row i = w, w + 4, ...
    sweep_rows<CK, 1>([&](int i) { return PlainCol(binv_cur + (size_t)i * ld); }, {col}, m, w, kWavesPerBlock, ld, svec, ck2, lane,
                      [&](int i, const double (&dot)[1]) {
                          const double di = dot[0];
                          const double a = fabs(di);
                          if (dmax < a) dmax = a;
                          const double v = (i == added) ? theta : xb[i] - theta * di;
                          if (v < -1e-13) bad = 1;
                      });
    if (lane == 0) smax[w] = dmax;
    bad = __syncthreads_or(bad);
    if (threadIdx.x != 0 || bad) return;
#pragma unroll
    for (int t = 0; t < kWavesPerBlock; t++) if (dmax < smax[t]) dmax = smax[t];
    if (!(fabs(dpv) > 1e-9 * (1.0 < dmax ? dmax : 1.0))) return;
    atomicMin(&d->x_best, (unsigned int)j);
}

// the scan's verdict: the forced pivot of the exchange — the worker's launch_ftran(column j) / launch_update(row added, no swap) on a
// loop state that runs again — with j into the basis list (do_lists = 3), then the orders of the Phase-II start; no candidate passed:
// infeasible, no x (simplex.go:606).  The exchange is a pivot of neither phase: piv1 stands as k_rv_ctrl took it.
__global__ void k_rv_exch_pick(RevLP *__restrict__ lps, const int *__restrict__ act) {
    RevLP *d = lps + act[blockIdx.x];
    if (threadIdx.x != 0 || d->run != RR_EXCH) return;
    const unsigned int best = d->x_best;
    if (best == 0xFFFFFFFFu) {
        d->status = GOMILP_ERR_INFEASIBLE; d->stage = RS_DONE; d->run = RR_NONE;
        return;
    }
    DevState *st = d->st;
    st->done = 0; st->status = ST_RUNNING; st->rq = 0;
    d->f_var = (int)best; d->f_pos = -1; d->f_p = d->x_added; d->f_noswap = 1;
    d->run = RR_FORCED; d->do_lists = 3; d->do_refresh = 1; d->after = RA_P2_LOOP;
    d->exch += 1;
}

// ------------------------------------------------------------------------------------------------
// host-callable launch wrappers: each takes the run's RevGeom and returns how many kernels it launched (rv_launch: one, counted)
// ------------------------------------------------------------------------------------------------
template <class... P, class... A>
static int rv_launch(void (*k)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A... a) {
    hipLaunchKernelGGL(k, grid, block, lds, s, a...);
    return 1;
}

int launch_rv_assemble(const RevLP *lps, int count, const RevGeom &g) {
    return rv_launch(k_rv_assemble, dim3(g.n_max + 1, count), dim3(kBlock), 0, g.stream, lps);
}
// (inplace: the IP = true instantiation of every kernel that reads a child's column; 0: the IP = false ones, the kernels as they were)
int launch_rv_init(RevLP *lps, int count, const RevGeom &g) {
    return rv_launch(g.inplace ? k_rv_init<true> : k_rv_init<false>, dim3(count), dim3(kBlock), 0, g.stream, lps);
}
// (ck2 > 0: the CK = true instances, ck2 double2 of dynamic LDS; 0: the one-pass instances with `lds` bytes)
static size_t rv_lds(size_t lds, int ck2) { return ck2 > 0 ? (size_t)ck2 * sizeof(double2) : lds; }

// K2 and K3 of one pivot of MODE (nparts_price: the workgroups of the pricing launch in front, 0: none)
template <int MODE>
static int launch_rv_k23(RevLP *lps, const int *act, int nact, int nparts_price, const RevGeom &g) {
    const auto k2 = g.ck2 > 0 ? (g.inplace ? k_rv_ftran<MODE, true, true> : k_rv_ftran<MODE, false, true>)
                              : (g.inplace ? k_rv_ftran<MODE, true, false> : k_rv_ftran<MODE, false, false>);
    const int n = rv_launch(k2, dim3(g.gr, nact), dim3(kBlock), rv_lds(g.lds, g.ck2), g.stream, lps, act, nparts_price, g.ck2);
    return n + rv_launch((g.ck2 > 0 ? k_rv_update<MODE, true> : k_rv_update<MODE, false>), dim3(g.gr, nact), dim3(kBlock), rv_lds(g.lds, g.ck2), g.stream, lps, act, g.gr, g.ck2);
}
int launch_rv_setup(RevLP *lps, const int *act, int nact, const RevGeom &g) {
    int n = launch_rv_k23<RR_FORCED>(lps, act, nact, 0, g);
    const int gy = (g.ld_max + kBlock - 1) / kBlock;
    n += rv_launch(k_rv_lists, dim3(nact), dim3(kBlock), 0, g.stream, lps, act);
    n += rv_launch((g.ck2 > 0 ? k_rv_matvec<true> : k_rv_matvec<false>), dim3(g.gr, nact), dim3(kBlock), rv_lds(g.lds, g.ck2), g.stream, lps, act, g.ck2);
    n += rv_launch(k_rv_y_partial, dim3(gy, 64, nact), dim3(kBlock), 0, g.stream, lps, act);
    n += rv_launch(k_rv_y_reduce, dim3(gy, nact), dim3(kBlock), 0, g.stream, lps, act);
    return n + rv_launch(k_rv_check, dim3(nact), dim3(kBlock), 0, g.stream, lps, act);
}
int launch_rv_pivot(RevLP *lps, const int *act, int nact, const RevGeom &g) {
    int n = rv_launch(k_rv_bland, dim3(nact), dim3(kBlock), 0, g.stream, lps, act);
    const auto k1 = g.ck2 > 0 ? (g.inplace ? k_rv_price<true, true> : k_rv_price<false, true>) : (g.inplace ? k_rv_price<true, false> : k_rv_price<false, false>);
    n += rv_launch(k1, dim3(g.gp, nact), dim3(kBlock), rv_lds(g.lds, g.ck2), g.stream, lps, act, g.ck2);
    return n + launch_rv_k23<RR_LOOP>(lps, act, nact, g.gp, g);
}
int launch_rv_ctrl(RevLP *lps, const int *act, int nact, RevOut *out, const RevGeom &g) {
    return rv_launch(k_rv_ctrl, dim3(nact), dim3(kBlock), 0, g.stream, lps, act, out);
}
int launch_rv_exchange(RevLP *lps, const int *act, int nact, const RevGeom &g) {
    const auto kx = g.ck2 > 0 ? (g.inplace ? k_rv_exch<true, true> : k_rv_exch<false, true>) : (g.inplace ? k_rv_exch<true, false> : k_rv_exch<false, false>);
    const int n = rv_launch(kx, dim3(g.nn_max, nact), dim3(kBlock), rv_lds(g.lds, g.ck2), g.stream, lps, act, g.ck2);
    return n + rv_launch(k_rv_exch_pick, dim3(nact), dim3(64), 0, g.stream, lps, act);
}
int launch_rv_gen_start(RevLP *lps, int count, const RevGeom &g) {
    return rv_launch(k_rv_gen_start, dim3(g.m_max, count), dim3(kBlock), 0, g.stream, lps);
}
int launch_rv_gen_art(RevLP *lps, int count, const RevGeom &g) {
    return rv_launch(g.inplace ? k_rv_gen_art<true> : k_rv_gen_art<false>, dim3(count), dim3(kBlock), 0, g.stream, lps);
}
// (one-pass forms only: a wave with a searched start does not stage in chunks)
int launch_rv_pivot_g(RevLP *lps, const int *act, int nact, const RevGeom &g) {
    int n = rv_launch((g.inplace ? k_rv_price<true, false, true> : k_rv_price<false, false, true>), dim3(g.gp, nact), dim3(kBlock), g.lds, g.stream, lps, act, 0);
    n += rv_launch((g.inplace ? k_rv_ftran<RR_LOOP, true, false, true> : k_rv_ftran<RR_LOOP, false, false, true>), dim3(g.gr, nact), dim3(kBlock), g.lds, g.stream, lps, act, g.gp, 0);
    return n + rv_launch((k_rv_update<RR_LOOP, false, true>), dim3(g.gr, nact), dim3(kBlock), g.lds, g.stream, lps, act, g.gr, 0);
}
int launch_rv_warm_binv(RevLP *lps, int count, const RevGeom &g) {
    return rv_launch(k_rv_warm_binv, dim3(g.m_max, count), dim3(kBlock), 0, g.stream, lps);
}
// (ck2d > 0: the CK = true pricing kernel, its TWO vectors ck2d double2 each, else the one-pass one with its two vectors' 2 * lds bytes;
// ck2: K2 / K3 as in launch_rv_pivot)
int launch_rv_dual_pivot(RevLP *lps, const int *act, int nact, const RevGeom &g) {
    int n = rv_launch(k_rv_dual_leave, dim3(nact), dim3(kBlock), 0, g.stream, lps, act);
    const auto k1 = g.ck2d > 0 ? (g.inplace ? k_rv_dual_price<true, true> : k_rv_dual_price<false, true>)
                               : (g.inplace ? k_rv_dual_price<true, false> : k_rv_dual_price<false, false>);
    n += rv_launch(k1, dim3(g.gp, nact), dim3(kBlock), rv_lds(2 * g.lds, 2 * g.ck2d), g.stream, lps, act, g.ck2d);
    return n + launch_rv_k23<RR_DUAL>(lps, act, nact, g.gp, g);
}

}  // namespace gomilp
