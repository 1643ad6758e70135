// A child's column read from its root in place (pool knob rev_inplace; batch_revised.hip, DESIGN.md section 2.5e "Root in place"):
// ChildCol synthesises row j of the transposed child matrix that k_rv_assemble would write — the root's resident At0 row, the branch
// rows' signs, the unit columns of the branch slacks, the relaxation's own Phase-I artificial row — double2 by double2.  It is a loader of
// the dot and staging helpers of kernels_common.h, as PlainCol is for a row in memory: they add the same terms in the same lane, accumulator
// and order, zero terms included, so a relaxation's values are the bits of the materialised copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_revised.h"
#include "kernels_common.h"

namespace gomilp {

// Column j (0 <= j <= n) of the child of RevLP d, ld doubles, as k_rv_assemble defines it:
//   j < n0:        the root's row At0 + j * ld0 for indices < m0, then asign[k] at index m0 + k wherever avar[k] == j (every branch row on the
//                  variable counts), zero up to ld;
//   n0 <= j < n:   the unit column e_{m0 + j - n0};
//   j == n:        the relaxation's artificial row d->art (k_rv_init).
// The first `full` double2 come from memory as they lie there; behind them every element is looked at on its own (elem) — the root's
// padding at index m0 (odd m0) is NOT the child's value there: the double2 that straddles m0 takes its second half from the branch rows.
// ld and ld0 differ; nothing is read beyond index m0 - 1 of a root row, K - 1 of avar / asign, ld - 1 of the artificial row.
struct ChildCol {
    const double *base;      // the root's row, or the artificial row
    const double *asign;
    const int32_t *avar;
    int j, m0, K;            // (K = 0 for a unit column and for the artificial row: no branch-row look-up)
    int mem;                 // elements taken from `base`: m0 (root column), 0 (unit column), ld (artificial row)
    int full;                // double2 taken from `base` whole: mem / 2
    int unit;                // index of the 1 of a unit column, else -1

    // (an empty column: the slot of a row a group does not have)
    __host__ __device__ __forceinline__ ChildCol() : base(nullptr), asign(nullptr), avar(nullptr), j(0), m0(0), K(0), mem(0), full(0), unit(-1) {}
    __host__ __device__ __forceinline__ ChildCol(const RevLP *d, int col) {
        const int n0 = d->n0, n = d->n;
        j = col; m0 = d->m0; asign = d->asign; avar = d->avar;
        if (col < n0) { base = d->At0 + (size_t)col * d->ld0; mem = m0; K = d->K; unit = -1; }
        else if (col < n) { base = nullptr; mem = 0; K = 0; unit = m0 + (col - n0); }
        else { base = d->art; mem = d->ld; K = 0; unit = -1; }
        full = mem >> 1;
    }
    __host__ __device__ __forceinline__ double elem(int i) const {
        if (i < mem) return base[i];
        if (i == unit) return 1.0;
        const int k = i - m0;
        return (k >= 0 && k < K && avar[k] == j) ? asign[k] : 0.0;
    }
    __host__ __device__ __forceinline__ double2 load2(int c) const {
        if (c < full) return reinterpret_cast<const double2 *>(base)[c];
        return make_double2(elem(2 * c), elem(2 * c + 1));
    }
};

}  // namespace gomilp
