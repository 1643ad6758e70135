// Host half of the bit-exact final solve (lu_host.h).  Built with -ffp-contract=off like everything else: every multiply and every
// add below is rounded on its own, as in the reference's kernels.
#include "lu_host.h"

#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace gomilp {

bool lu_det_is_zero(const double *diag, const int32_t *phys, int m) {
    // The sum of the binary exponents brackets sum log|u_ii| ( |u| in [2^(e-1), 2^e) ): only a product that could underflow (or a
    // zero / NaN on the diagonal) pays for the m logarithms in gonum's order.
    long long esum = 0;
    bool plain = true;
    for (int i = 0; i < m; i++) {
        int e = 0;
        const double d = diag[i];
        if (!(fabs(d) > 0) || !std::isfinite(d)) { plain = false; break; }
        (void)frexp(d, &e);
        esum += e;
    }
    // sum log|u_ii| >= (esum - m) ln 2, minus rounding of m additions; exp() is zero below -745.14
    if (plain && (double)(esum - m) * 0.6931471805599453 > -700.0) return false;   // (exp(logdet) != 0 for sure)
    double logdet = 0;
    for (int i = 0; i < m; i++) logdet += log(fabs(diag[phys[i]]));
    return exp(logdet) == 0;
}

namespace {

// The two Dtrsm of Dgetrs, per row in gonum's order: ascending k, zero multipliers skipped, b_i = (-a_ik)*b_k + b_i as a rounded
// multiply and a rounded add (blas/gonum/level3double.go:75-118).
inline double term(double bi, double va, double xk) { return va != 0 ? (-va) * xk + bi : bi; }

// the terms lo <= t < hi of one row
inline double chain(double bi, const double *row, const double *x, int lo, int hi) {
    for (int t = lo; t < hi; t++) bi = term(bi, row[t], x[t]);
    return bi;
}

// ... of four rows side by side (each row is one chain of dependent rounded additions: a single chain leaves the FPU idle)
inline void chain4(double acc[4], const double *const row[4], const double *x, int lo, int hi) {
    double b0 = acc[0], b1 = acc[1], b2 = acc[2], b3 = acc[3];
    const double *r0 = row[0], *r1 = row[1], *r2 = row[2], *r3 = row[3];
    for (int t = lo; t < hi; t++) {
        const double xk = x[t];
        b0 = term(b0, r0[t], xk); b1 = term(b1, r1[t], xk); b2 = term(b2, r2[t], xk); b3 = term(b3, r3[t], xk);
    }
    acc[0] = b0; acc[1] = b1; acc[2] = b2; acc[3] = b3;
}

}  // namespace

void lu_host_solve(int m, int nd, const int32_t *dl, const int32_t *phys, const double *diag, const double *W, const double *rhs, double *x) {
    // Dlaswp: b in logical row order
    for (int i = 0; i < m; i++) x[i] = rhs[phys[i]];
    // Only the nd columns whose elimination step did arithmetic carry off-diagonal entries, so a row depends on the solution at
    // those "dense" positions only: they are solved first, one after the other; every other row is then independent of the rest
    // and four of them run interleaved.
    std::vector<double> xdv(nd);
    double *xd = xdv.data();   // the solution at the dense positions
    struct Row { int i, below; };   // a logical position that is not dense, and the number of dense positions below it
    std::vector<Row> nl;            // ascending
    nl.reserve(m - nd);
    for (int i = 0, cnt = 0; i < m; i++) {
        if (cnt < nd && dl[cnt] == i) cnt++;
        else nl.push_back({i, cnt});
    }
    // up to four of those rows from nl[g] on: their packed rows, their running sums
    const double *row[4];
    double acc[4];
    auto load = [&](size_t g) {
        const int k = (int)std::min<size_t>(4, nl.size() - g);
        for (int r = 0; r < k; r++) { row[r] = W + (size_t)phys[nl[g + r].i] * nd; acc[r] = x[nl[g + r].i]; }
        return k;
    };
    // ---- Dtrsm(Left, Lower, NoTrans, Unit): row i takes the dense positions below it
    for (int s = 0; s < nd; s++) {
        const int i = dl[s];
        x[i] = xd[s] = chain(x[i], W + (size_t)phys[i] * nd, xd, 0, s);
    }
    for (size_t g = 0; g < nl.size(); g += 4) {
        const int k = load(g);
        const int c0 = k == 4 ? nl[g].below : 0;   // below is ascending: the four rows share the terms up to the first row's
        if (k == 4) chain4(acc, row, xd, 0, c0);
        for (int r = 0; r < k; r++) x[nl[g + r].i] = chain(acc[r], row[r], xd, c0, nl[g + r].below);
    }
    // ---- Dtrsm(Left, Upper, NoTrans, NonUnit): rows from the bottom, ascending k within a row (the dense positions above it), then * (1/u_ii)
    for (int s = nd - 1; s >= 0; s--) {
        const int i = dl[s];
        const double tinv = 1 / diag[phys[i]];
        x[i] = xd[s] = chain(x[i], W + (size_t)phys[i] * nd, xd, s + 1, nd) * tinv;
    }
    for (size_t g = 0; g < nl.size(); g += 4) {
        const int k = load(g);
        const int f3 = k == 4 ? nl[g + 3].below : nd;   // the leading terms of a row come first, in order; from the last row's on the four share them
        for (int r = 0; r < k; r++) acc[r] = chain(acc[r], row[r], xd, nl[g + r].below, f3);
        if (k == 4) chain4(acc, row, xd, f3, nd);
        for (int r = 0; r < k; r++) {
            const int i = nl[g + r].i;
            const double tinv = 1 / diag[phys[i]];
            x[i] = acc[r] * tinv;
        }
    }
}

void lu_host_solve_coupled(int nd, const int32_t *dl, const int32_t *phys, const double *diag, const double *W, const double *rhs,
                           double *xdl, double *xdu) {
    // Dtrsm(Left, Lower, NoTrans, Unit): four rows run side by side over the part of the solution that is known before the first of
    // them, then finish one after the other
    int s = 0;
    for (; s + 4 <= nd; s += 4) {
        const double *row[4];
        double acc[4];
        for (int r = 0; r < 4; r++) { row[r] = W + (size_t)(s + r) * nd; acc[r] = rhs[phys[dl[s + r]]]; }
        chain4(acc, row, xdl, 0, s);
        for (int r = 0; r < 4; r++) xdl[s + r] = chain(acc[r], row[r], xdl, s, s + r);
    }
    for (; s < nd; s++) xdl[s] = chain(rhs[phys[dl[s]]], W + (size_t)s * nd, xdl, 0, s);
    // Dtrsm(Left, Upper, NoTrans, NonUnit)
    for (s = nd - 1; s >= 0; s--) {
        const double tinv = 1 / diag[phys[dl[s]]];
        xdu[s] = chain(xdl[s], W + (size_t)s * nd, xdu, s + 1, nd) * tinv;
    }
}

}  // namespace gomilp
