// A child's column read from its root in place (pool knob rev_inplace; batch_revised.hip, DESIGN.md section 2.5e "Root in place"):
// ChildCol synthesises row j of the transposed child matrix that k_rv_assemble would write — the root's resident At0 row, the branch
// rows' signs, the unit columns of the branch slacks, the relaxation's own Phase-I artificial row — double2 by double2, and the
// loader-templated forms of the dot and staging helpers of kernels_common.h run the arithmetic of those helpers on what it loads: the same
// terms in the same lane, accumulator and order, zero terms included, so a relaxation's values are the bits of the materialised copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_revised.h"
#include "kernels_common.h"

namespace gomilp {

// a padded row that lies in memory (rows of B^-1, the vectors y / rho): the loader the helpers below take where nothing is synthesised
struct PlainCol {
    const double2 *p;
    __host__ __device__ __forceinline__ double2 load2(int c) const { return p[c]; }
};

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

// wave_dot_chunk with the row behind a loader
template <int NV, class Row>
__device__ __forceinline__ void wave_dot_chunk_t(const Row &row, const double2 *__restrict__ svec, int sstride, int c0, int c1, int ld2, int lane,
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

// wave_dot_row
template <class Row>
__device__ __forceinline__ double wave_dot_row_t(const Row &row, const double2 *__restrict__ svec, int ld2, int lane) {
    DotAcc acc[1] = {{0, 0, 0, 0}};
    wave_dot_chunk_t<1>(row, svec, 0, 0, ld2, ld2, lane, acc);
    return wave_dot_finish(acc[0]);
}

// stage_vec
template <class Vec>
__device__ __forceinline__ void stage_vec_t(double2 *__restrict__ svec, const Vec &src, int ld2) {
    for (int c = threadIdx.x; c < ld2; c += kBlock) svec[c] = src.load2(c);
    __syncthreads();
}

// stage_chunk
template <int NV, class Vec>
__device__ __forceinline__ void stage_chunk_t(double2 *__restrict__ svec, int sstride, const Vec (&src)[NV], int c0, int c1) {
    __syncthreads();
    for (int c = threadIdx.x; c < c1 - c0; c += kBlock) {
#pragma unroll
        for (int v = 0; v < NV; v++) svec[v * sstride + c] = src[v].load2(c0 + c);
    }
    __syncthreads();
}

// dot_group: row r of the group (valid where has[r]) behind rows[r], the NV vectors behind vec[v]
template <int NV, class Row, class Vec>
__device__ __forceinline__ void dot_group_t(const Row (&rows)[kCkRows], const bool (&has)[kCkRows], int ld, const Vec (&vec)[NV], double2 *svec,
                                            int ck2, int lane, double (&dot)[kCkRows][NV]) {
    const int ld2 = ld >> 1;
    DotAcc acc[kCkRows][NV];
#pragma unroll
    for (int r = 0; r < kCkRows; r++)
#pragma unroll
        for (int v = 0; v < NV; v++) acc[r][v].a0 = acc[r][v].a1 = acc[r][v].a2 = acc[r][v].a3 = 0;
    for (int c0 = 0; c0 < ld2; c0 += ck2) {
        const int c1 = min(c0 + ck2, ld2);
        stage_chunk_t<NV>(svec, ck2, vec, c0, c1);
#pragma unroll
        for (int r = 0; r < kCkRows; r++)
            if (has[r]) wave_dot_chunk_t<NV>(rows[r], svec, ck2, c0, c1, ld2, lane, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kCkRows; r++)
#pragma unroll
        for (int v = 0; v < NV; v++) dot[r][v] = has[r] ? wave_dot_finish(acc[r][v]) : 0.0;
}

}  // namespace gomilp
