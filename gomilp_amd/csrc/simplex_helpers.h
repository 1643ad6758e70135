// Pivot rules, per-element work and commit of the revised-simplex kernels K1-K3 (simplex_kernels.hip) as __device__ helpers: the
// one-pass and chunked kernels of one LP and the batched kernels of a wave of LPs (batch_revised.hip: the relaxation is
// blockIdx.y) run this one code, so every form takes the same decisions from bit-identical values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "kernels_common.h"

namespace gomilp {

// ------------------------------------------------------------------------------------------------
// K1-K3 come in two forms each, one kernel template on CK: one pass (the m-long vector staged whole in LDS) and the chunked form
// (the vector streamed through LDS in chunks; for vectors longer than the LDS window, ld > 8192, or wherever the context knob
// row_chunk forces it).  The two forms differ only in their staging and row loops (kernels_common.h: sweep_rows; update_rows
// below): the pivot rules, the per-element work and the commit are the helpers below, so both forms take the same decisions from
// bit-identical values.
// The helpers take the pointers they use, not the LPArgs: a reference to the kernel's argument hides from the compiler that those
// pointers are kernel arguments that nothing in the kernel overwrites, and the kernel loses its scalar loads (rvec[q], nonbasic[q]).
// Template parameter G (every K1-K3 kernel and helper): the exact-step guard (LPArgs::guard > 0).  G = false is the code of every
// solve but the non-slack starts of the three-kernel loop; G = true carries each workgroup's runner-up key beside its winner (pk2 =
// pk + kMaxPartials) and stops with ST_NEED_EXACT where the block kernel of the blocked tableau does (bt_kernels.hip: reduced costs at
// the stop threshold or tied, a winning ratio at zero or tied, a pivot element of rounding-noise size; every decision when strict).
// ------------------------------------------------------------------------------------------------

// K1's gate: false once the loop has stopped, and when the pivot budget is spent (ST_MAX_PIVOTS)
__device__ __forceinline__ bool price_gate(DevState *st) {
    if (st->done) return false;
    if (st->max_pivots > 0 && st->pivots >= st->max_pivots) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { st->done = 1; st->status = ST_MAX_PIVOTS; }
        return false;
    }
    return true;
}

// reduced cost of nonbasic position pos (variable j, dot = At[j,:].y): r = cost[j] - dot (simplex.go:242-243) into rvec and the
// running first-index argmin (:247)
// (b2: the running runner-up key, G only)
template <bool G>
__device__ __forceinline__ void price_elem(const double *cost, double *rvec, int pos, int j, double dot, int lane, unsigned long long &bk,
                                           unsigned int &bi, unsigned long long &b2) {
    const double r = cost[j] - dot;
    if (lane == 0) rvec[pos] = r;
    if constexpr (G) amin2_take(bk, bi, b2, ordkey(r), (unsigned int)pos, ~0ull);
    else amin_take(bk, bi, ordkey(r), (unsigned int)pos);
}

// K2's entering variable, into var (wave-uniform).  forced_var >= 0: the variable given; forced_pos = kDualPick: the dual pivot's
// entering position, from the partials of k_dual_price (dual_kernels.hip); forced_pos >= 0: the position given (Bland / setup);
// else the first-index argmin of the reduced costs and the optimality test.  false: the loop has stopped or stops here.
// (pk / pi: the pricing partials; rvec, nonbasic, tol, guard as in LPArgs; ss: block scratch of the runner-up keys, G only)
template <bool G>
__device__ __forceinline__ bool pick_entering(DevState *st, const unsigned long long *pk, const unsigned int *pi, int nparts_price,
                                              const double *rvec, const int32_t *nonbasic, double tol, double guard, int forced_pos,
                                              int forced_var, unsigned long long *sk, unsigned int *si, unsigned long long *ss, int &var) {
    if (st->done) return false;
    int q = forced_pos;
    if (forced_var >= 0) {
        var = forced_var;
    } else if (q == kDualPick) {
        unsigned long long key;
        q = (int)reduce_partials(pk, pi, nparts_price, sk, si, &key);
        if (key >= ordkey(__builtin_inf())) {   // no alpha_pj < -1e-13 in row p: x_B[p] < 0 cannot be repaired, the LP is infeasible
            if (blockIdx.x == 0 && threadIdx.x == 0) { st->done = 1; st->status = ST_DUAL_INFEASIBLE; }
            return false;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) { st->q = q; st->rq = rvec[q]; }
        var = nonbasic[q];
    } else {
        if (q < 0) {
            unsigned long long key, key2;
            q = G ? (int)reduce_partials2(pk, pi, pk + kMaxPartials, nparts_price, sk, si, ss, &key, &key2)
                  : (int)reduce_partials(pk, pi, nparts_price, sk, si, nullptr);
            const double rq = rvec[q];
            if constexpr (G) {
                // bt_kernels.hip's test: at the stop threshold only the drift of the updated reduced costs matters (1e-12); a tie
                // matters only when the loop goes on; an infinite guard (strict) stops in front of every decision, the stop test too
                const double r2 = orddecode(key2);
                if (guard == __builtin_inf() || fabs(rq + tol) <= 1e-12 || (!(rq >= -tol) && r2 - rq <= guard * fmax(1.0, fabs(rq)))) {
                    if (blockIdx.x == 0 && threadIdx.x == 0) { st->done = 1; st->status = ST_NEED_EXACT; st->q = q; st->rq = rq; }
                    return false;
                }
            }
            if (rq >= -tol) {  // simplex.go:248 — optimal
                if (blockIdx.x == 0 && threadIdx.x == 0) { st->done = 1; st->status = ST_OPTIMAL; st->q = q; st->rq = rq; }
                return false;
            }
            if (blockIdx.x == 0 && threadIdx.x == 0) { st->q = q; st->rq = rq; }
        } else if (blockIdx.x == 0 && threadIdx.x == 0) {
            st->q = q; st->rq = rvec[q];
        }
        var = nonbasic[q];
    }
    return true;
}

// row i of the FTRAN (dp = B^-1[i,:].a_q): d = -d'_i, the ratio move_i = x_B[i]/|d_i| for d_i < 0 (simplex.go:306-342) into dvec /
// move and the running first-index argmin of move (:268)
template <bool G>
__device__ __forceinline__ void ratio_elem(const double *xb, double *dvec, double *move, int i, double dp, int lane, unsigned long long &bk,
                                           unsigned int &bi, unsigned long long &b2) {
    double d = -dp;                       // simplex.go:319
    if (fabs(d) < 1e-13) d = 0;           // dRoundTol, :321-325
    const double mv = (d >= 0) ? __builtin_inf() : xb[i] / fabs(d);  // :334-340
    if (lane == 0) { dvec[i] = dp; move[i] = mv; }
    if constexpr (G) amin2_take(bk, bi, b2, ordkey(mv), (unsigned int)i, ~0ull);
    else amin_take(bk, bi, ordkey(mv), (unsigned int)i);
}

// K3's leaving row, into p (wave-uniform).  forced_p >= 0: the row given; kDualPick: the one k_dual_leave chose (DevState::p); else
// the first-index argmin of the ratios.  false: the loop has stopped or stops here (unbounded, or a degenerate step for Bland).
// (pk / pi: the ratio partials; dvec, guard as in LPArgs; ss as in pick_entering)
template <bool G>
__device__ __forceinline__ bool pick_leaving(DevState *st, const unsigned long long *pk, const unsigned int *pi, int nparts_ratio,
                                             const double *move, const double *dvec, double guard, int forced_p, unsigned long long *sk,
                                             unsigned int *si, unsigned long long *ss, int &p) {
    if (st->done) return false;
    p = forced_p == kDualPick ? st->p : forced_p;
    if (p < 0) {
        unsigned long long key, key2;
        p = G ? (int)reduce_partials2(pk, pi, pk + kMaxPartials, nparts_ratio, sk, si, ss, &key, &key2)
              : (int)reduce_partials(pk, pi, nparts_ratio, sk, si, nullptr);
        const double mv = move[p];
        if (mv == __builtin_inf()) {  // no d_i < 0: unbounded (simplex.go:328-330)
            if (blockIdx.x == 0 && threadIdx.x == 0) { st->done = 1; st->status = ST_UNBOUNDED; st->p = p; st->mv = mv; }
            return false;
        }
        if constexpr (G) {
            // bt_kernels.hip's test, in front of the Bland stop: a winning ratio at zero, two rows within the guard of each other, or a
            // pivot element of rounding-noise size — decided on a fresh gonum-order x_B, never by the host Bland branch on updated values
            const double mv2 = orddecode(key2);
            if (mv <= guard || mv2 - mv <= guard * fmax(1.0, fabs(mv)) || fabs(dvec[p]) <= guard) {
                if (blockIdx.x == 0 && threadIdx.x == 0) { st->done = 1; st->status = ST_NEED_EXACT; st->p = p; st->mv = mv; }
                return false;
            }
        }
        if (mv <= 0) {  // degenerate step -> Bland rule (simplex.go:269)
            if (blockIdx.x == 0 && threadIdx.x == 0) { st->done = 1; st->status = ST_NEED_BLAND; st->p = p; st->mv = mv; }
            return false;
        }
    }
    return true;
}

// columns [c0, c1) of row i of the next B^-1 (rank-1 update with pivot row p, d'_p = dpv); rowp: old row p over the same columns
// in LDS, element c0 at 0
__device__ __forceinline__ void update_row(const double *binv_cur, double *binv_next, int ld, const double *dvec, int i, int p, double dpv,
                                           const double2 *rowp, int c0, int c1, int lane) {
    const double2 *src = reinterpret_cast<const double2 *>(binv_cur + (size_t)i * ld);
    double2 *dst = reinterpret_cast<double2 *>(binv_next + (size_t)i * ld);
    if (i == p) {
        for (int c = c0 + lane; c < c1; c += 64) {
            double2 v = rowp[c - c0];
            v.x = v.x / dpv; v.y = v.y / dpv;
            dst[c] = v;
        }
    } else {
        const double f = dvec[i] / dpv;
        for (int c = c0 + lane; c < c1; c += 64) {
            double2 v = src[c];
            const double2 rp = rowp[c - c0];
            v.x = v.x - f * rp.x; v.y = v.y - f * rp.y;
            dst[c] = v;
        }
    }
}

// K3's rows: every row of the next B^-1 by the waves of the grid, old row p (rowp_g, in B^-1) staged in LDS.  Elementwise, so the
// chunks of CK are only bounds: CK = false stages row p whole and takes a row at a time, CK = true takes a wave's rows kCkRows at a
// time and streams row p ck2 double2 at a time per group, to a workgroup-uniform bound (every thread reaches stage_chunk's barriers).
template <bool CK>
__device__ __forceinline__ void update_rows(const double *binv_cur, double *binv_next, int ld, const double *dvec, int m, int p, double dpv,
                                            const double *rowp_g, double2 *svec, int ck2) {
    const int ld2 = ld >> 1;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * kWavesPerBlock;
    if constexpr (CK) {
        const int kmax = (m + nwaves - 1) / nwaves;
        for (int k0 = 0; k0 < kmax; k0 += kCkRows) {
            for (int c0 = 0; c0 < ld2; c0 += ck2) {
                const int c1 = min(c0 + ck2, ld2);
                stage_chunk<1>(svec, ck2, {PlainCol(rowp_g)}, c0, c1);
#pragma unroll
                for (int r = 0; r < kCkRows; r++) {
                    const int i = wave + (k0 + r) * nwaves;
                    if (i < m) update_row(binv_cur, binv_next, ld, dvec, i, p, dpv, svec, c0, c1, lane);
                }
            }
        }
    } else {
        stage_vec<1>(svec, {PlainCol(rowp_g)}, ld2);
        for (int i = wave; i < m; i += nwaves) update_row(binv_cur, binv_next, ld, dvec, i, p, dpv, svec, 0, ld2, lane);
    }
}

// the rest of K3, by workgroup 0 after its rows: x_B and y (O(m); nobody else touches them in this kernel), the index swap
// (simplex.go:280), the trace record and the counters.  rowp: old row p of B^-1 (where update_rows left it whole: LDS for CK = false,
// B^-1 itself for CK = true: the same values).  (The other pointers and m, ld, trace_cap, phase as in LPArgs.)
__device__ __forceinline__ void commit_pivot(DevState *st, double *xb, double *y, const double *dvec, const double *move, int32_t *basic,
                                             int32_t *nonbasic, DevPivot *trace, int64_t trace_cap, int phase, int m, int ld, int p, double dpv,
                                             const double *rowp, int no_swap, int bland) {
    const double theta = xb[p] / dpv;
    const double rq = no_swap ? 0.0 : st->rq;
    const double alpha = rq / dpv;
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += kBlock) xb[i] = (i == p) ? theta : xb[i] - theta * dvec[i];
    for (int j = threadIdx.x; j < ld; j += kBlock) y[j] = y[j] + alpha * rowp[j];
    if (threadIdx.x == 0) {
        const int q = st->q;
        st->p = p; st->dp = dpv; st->mv = move[p];
        if (!no_swap) {
            const int ent = nonbasic[q], lea = basic[p];
            basic[p] = ent; nonbasic[q] = lea;  // simplex.go:280
            if (trace && st->trace_len < trace_cap) {
                DevPivot &t = trace[st->trace_len];
                t.phase = phase; t.bland = bland; t.min_idx = q; t.replace = p; t.entering = ent; t.leaving = lea;
            }
            st->trace_len += 1;
            st->pivots += 1;
        }
    }
}

// the workgroup's winner (and, G, its runner-up) into the partials
template <bool G>
__device__ __forceinline__ void publish(unsigned long long &bk, unsigned int &bi, unsigned long long &b2, unsigned long long *sk,
                                        unsigned int *si, unsigned long long *ss, unsigned long long *pk, unsigned int *pi) {
    if constexpr (G) publish_partials2(bk, bi, b2, sk, si, ss, pk, pi, pk + kMaxPartials);
    else publish_partials(bk, bi, sk, si, pk, pi);
}

}  // namespace gomilp
