// The host half of the bit-exact final solve: the two triangular solves of Dgetrs and LU.Det() == 0, in gonum's rounding order, on
// the packed factors the device leaves (engine_final.cpp).  Plain host arithmetic: no HIP, nothing of the engine — tests pin it to
// the reference without a device (gomilp_debug_lu_host_solve, tests/test_lu_host_solve.py).
//
// The packed factors of an m x m basis: `dl` lists, ascending, the nd logical positions whose elimination step did arithmetic (the
// "dense" positions: only their columns of the in-place L\U carry off-diagonal entries); phys[i] is the physical row at logical
// position i; diag[R] is u_ii of physical row R.
#pragma once
#include <stdint.h>

namespace gomilp {

// LU.Det() == 0 (mat/lu.go:301, :118-135): exp(sum log|u_ii|) == 0, the sum taken in logical order
bool lu_det_is_zero(const double *diag, const int32_t *phys, int m);

// Dlaswp + Dtrsm(Lower, Unit) + Dtrsm(Upper, NonUnit) of Dgetrs (lapack/gonum/dgetrs.go:37-45).  W: m x nd, row R = the dense columns
// of physical row R.  rhs: m entries by physical row.  x: m entries by logical (basis) position.
void lu_host_solve(int m, int nd, const int32_t *dl, const int32_t *phys, const double *diag, const double *W, const double *rhs, double *x);

// The same for the dense positions alone (they depend on nothing else).  W: nd x nd, row s = logical position dl[s] restricted to the
// dense columns.  xdl / xdu: the solution at the dense positions after the lower / after both solves — all that the remaining rows
// need (lu_compressed.hip k_luc_solve_rows).
void lu_host_solve_coupled(int nd, const int32_t *dl, const int32_t *phys, const double *diag, const double *W, const double *rhs,
                           double *xdl, double *xdu);

}  // namespace gomilp
