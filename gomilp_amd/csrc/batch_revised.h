// Device-batched revised simplex (batch_revised.hip, engine_batch_revised.cpp): the three-kernel revised simplex of
// simplex_kernels.hip with the relaxation as blockIdx.y.  One RevLP per relaxation of a wave, resident in HBM: it plays the role
// of LPArgs (the pointers), carries the relaxation's stage and its ping-pong parity, and takes the work orders that the control
// kernels write for the set-up launches of the next superstep.  The relaxations of a wave may be children of several roots: every
// kernel reads its relaxation's shape and pointers from its RevLP, the grids are sized for the wave's largest shape.  The host enqueues a fixed list of launches per superstep and looks
// at one small record per relaxation afterwards.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"

namespace gomilp {

enum : int32_t {
    RS_RUN = 0,    // set-up launches or a pivot loop are running
    RS_DONE = 1,   // terminal: `status` holds the outcome (GOMILP_OK / ERR_BLAND / ERR_UNSUPPORTED after Phase II: basis + x_B ready for the final solve)
    RS_HOST = 2,   // terminal: a branch the schedule leaves to a worker's whole solve: the |x_art| band (1e-13 < |x_art| < 1e-11: the verdict
                   // needs a fresh gonum-order solve), the zero-level artificial exchange where the wave runs without it (rev_exchange = 0),
                   // and of a searched start (RevLP::gen) the start guard of k_rv_gen_start and every exact step (ST_NEED_EXACT)
    RS_COLD = 3    // a warm start that spent its dual-pivot budget: the host re-initialises the slot and the same run solves it cold
};
// RevLP::after: what k_rv_check does behind the set-up launches of a superstep
enum : int32_t {
    RA_NONE = 0,
    RA_P1_LOOP = 1,   // the PANIC test of the Phase-I start, then the Phase-I loop
    RA_P2_LOOP = 2,   // the Phase-II loop
    RA_DUAL_LOOP = 3  // the dual loop of a warm start (DevState::max_pivots = the dual-pivot budget)
};
// RevLP::run: which launches of a superstep work on the relaxation
// (RR_EXCH: Phase I ended with the artificial basic at level zero — the candidate scan k_rv_exch / k_rv_exch_pick in front of the set-up
// launches of the next superstep looks for the column that takes its place, simplex.go:581-606)
enum : int32_t { RR_NONE = 0, RR_LOOP = 1, RR_FORCED = 2, RR_DUAL = 3, RR_EXCH = 4 };

struct RevLP {
    // ---- fixed for the wave (written by the host) ----
    double *At;              // (n + 1) x ld: row j = column j of the child's A (k_rv_assemble), row n = the Phase-I artificial; null where the
                             // wave reads its roots in place (`inplace` at the tail)
    const double *c2;        // Phase-II cost [c0, 0, ...] (at least n + 1 entries)
    double *c1;              // Phase-I cost: e_n (n + 1 entries, written by k_rv_init)
    double *b;               // ld, zero padded
    double *binv[2];         // m x ld each: flip counter & 1 is the current one
    double *xb, *y, *dvec, *move, *rvec, *yscratch;
    int32_t *basic, *nonbasic, *inb;
    unsigned long long *pk_price, *pk_ratio;
    unsigned int *pi_price, *pi_ratio;
    DevState *st;
    const double *b0, *rhs;  // root right-hand side (m0), the child's branch right-hand sides (K)
    const int32_t *rho0;     // m0: row of the 1 in root column n0 - 1 - pos
    int32_t m0, n0, K, m, n, ld;   // (m0 / n0, b0 / c2 / rho0: of the relaxation's OWN root — a wave may hold children of several roots)
    int64_t max_pivots;      // pool knob max_pivots (0: none)
    double tol_user;         // Phase-II tolerance of the call
    // ---- state (device) ----
    int32_t stage, run;      // RS_*, RR_*
    int32_t flips;           // rank-1 updates committed so far (no-swap set-up pivots included): written by K3's committing thread,
    int32_t flips_k2;        // read by K2 and the refresh kernels; K2's copy for the K3 of the same pivot (no kernel reads what its own launch writes)
    int32_t phase, nn;
    double tol;
    const double *cost;
    // the Bland rule inside the loop (k_rv_bland in front of every pivot): bl = 1: this pivot is a Bland step on candidate position bl_pos
    // (K1 is skipped, K2 takes the position, K3 the leaving row by replaceBland's rule); bland_failed: no candidate was left (lp.ErrBland)
    int32_t bl, bl_pos, bland_failed, pad1;
    // ---- work orders for the set-up launches of the next superstep (written by k_rv_init / k_rv_ctrl, cleared by k_rv_check) ----
    int32_t f_var, f_pos, f_p, f_noswap, pad2;      // the forced pivot (run == RR_FORCED)
    int32_t do_lists;        // 1: basic[f_p] = n, nonbasic = ascending ids of n + 1 columns outside the basis; 2: of n columns;
                             // 3: basic[f_p] = f_var (the exchange), then as 2
    int32_t do_refresh;      // 1: x_B = B^-1 b and y = B^-T c_B; 2: y only
    int32_t after;           // RA_*
    // ---- outcome ----
    int32_t status, wrapped, phase1_used, pad0;
    int64_t piv1, piv2, bland;
    // ---- warm start (written by the host; behind the fields above, whose offsets the cold kernels' code keeps) ----
    // warm != 0: the parent's kept state (mp x ldp B^-1, mp basis positions), the parent position of each of the J new rows' variables
    // (-1: nonbasic there) and the rows' signs; k_rv_warm_binv builds the start, k_rv_init leaves the relaxation alone
    const double *wbinv, *wsign;
    const int32_t *wbasic, *wkpos;
    int32_t warm, wJ, wmp, wldp;
    int64_t dual_budget;
    int64_t pivd;            // outcome: dual pivots
    // ---- the zero-level artificial exchange (behind the warm fields, for the same reason) ----
    // exch_on: the wave runs with it (written by the host); x_added: the artificial's basis position (k_rv_ctrl); x_best: the smallest
    // candidate id that passed the scan so far (atomic min of k_rv_exch, 0xFFFFFFFF: none); exch: outcome, exchanges done
    int32_t exch_on, x_added;
    unsigned int x_best;
    int32_t exch;
    // ---- what k_rv_assemble builds At from (written by the host; at the tail, for the same reason): the relaxation's own root — its
    // resident At0 with row stride ld0 (m0 / n0 above) — and its K branch rows' variables and signs
    const double *At0;
    const double *asign;
    const int32_t *avar;
    int32_t ld0, pad3;
    // ---- the root in place (pool knob rev_inplace; written by the host, at the tail, for the same reason): inplace != 0: At is null, the
    // kernels read column j of the child through ChildCol (rev_child_col.h) from At0 / asign / avar, and the Phase-I artificial column
    // is the relaxation's own row `art` (ld doubles of the zeroed work arena, written by k_rv_init<true>)
    int32_t inplace, pad4;
    double *art;
    // ---- a root without a slack basis (pool knob rev_general; written by the host, at the tail, for the same reason): gen != 0: the
    // relaxation's root carries its searched basis (RootView::GeneralRev) — B0^-1 (m0 x ldg, padding column zero), x_B0, the basis list
    // and the position of every root variable (-1: nonbasic).  k_rv_gen_start builds the start (k_rv_init leaves the relaxation alone),
    // k_rv_gen_art the Phase-I artificial column of the start with gminidx >= 0 (the position the artificial is forced into), and the
    // pivots of its loops are the G = true instances of K1-K3 with this guard; pk_price / pk_ratio then hold 2 * kMaxPartials keys
    const double *gB0inv, *gxb0;
    const int32_t *gbasic0, *gposvar0;
    int32_t ldg, gen;
    int32_t gminidx, pad5;
    double guard;
};

// what the host reads of every active relaxation after a superstep
struct RevOut {
    int32_t stage, status, wrapped, phase1_used;
    int64_t piv1, piv2, bland, pivd;
    int32_t flips, dual;   // parity of the current B^-1 (the host keeps it for the children); 1: the dual loop runs or is ordered
    int32_t scan, exch;    // 1: the candidate scan of the exchange is ordered (run == RR_EXCH); exchanges done
};

// the launch geometry of a run: fixed from its first launch to its last, handed to every wrapper below
struct RevGeom {
    int gp, gr;                      // workgroups per relaxation of the pricing kernel and of the row kernels (grid_for_rows of the wave's largest nn / m)
    int ld_max, nn_max, m_max, n_max;   // the wave's largest ld, n + 1 - m, m and n: they size the grids (a relaxation's values do not depend on them)
    size_t lds;                      // bytes of the largest staged vector of the one-pass kernels (ck2 == 0)
    // ck2: 0: the one-pass kernels with `lds` bytes, exactly the launches of a wave within the LDS window; > 0: the chunked forms (CK = true), the
    // staged vector streamed through LDS ck2 double2 at a time (a multiple of 256, at most 4096: ck2 * sizeof(double2) bytes of dynamic LDS,
    // never more than 64 KB) — the same values, whatever the chunk.  ck2d: the same for the dual pricing kernel, which stages TWO vectors:
    // 0: one pass with 2 * lds bytes (ld_max <= kRevDualLd); > 0: each vector ck2d <= kRevDualLd / 2 double2 at a time
    int ck2, ck2d;
    // 0: the kernels on the assembled At; 1: the wave was not assembled (pool knob rev_inplace) — the IP = true instantiations of the kernels
    // that read a child's column, which take it from the relaxation's root through ChildCol; the other kernels of a list are the same either way
    int inplace;
    hipStream_t stream;
};
constexpr int kRevDualLd = 4096;

// launches (batch_revised.hip).  lps, count: the whole wave; act, nact: list positions -> relaxation.  Each returns the number of kernels it
// launched: the host sums them (RevBatchEngine::Stats::launches).
// the whole wave's At in one launch, in front of launch_rv_init: grid (n_max + 1 child columns, count relaxations); writes what
// k_child_assemble (simplex_kernels.hip) writes per child
int launch_rv_assemble(const RevLP *lps, int count, const RevGeom &g);
int launch_rv_init(RevLP *lps, int count, const RevGeom &g);
// warm starts: B^-1, basis list, b and the orders of every relaxation with warm != 0 (grid rows x count)
int launch_rv_warm_binv(RevLP *lps, int count, const RevGeom &g);
// searched starts (RevLP::gen; one-pass staging only): launch_rv_gen_start behind launch_rv_init — B^-1, x_B, the lists, b, c1, the start
// guard and the orders of every relaxation with gen != 0 (grid rows x count); launch_rv_gen_art behind it — the Phase-I artificial column of
// those that start infeasible (one workgroup per relaxation; reads the assembled At, or the root in place)
int launch_rv_gen_start(RevLP *lps, int count, const RevGeom &g);
int launch_rv_gen_art(RevLP *lps, int count, const RevGeom &g);
// the candidate scan of the relaxations with run == RR_EXCH, in front of launch_rv_setup: one workgroup per nonbasic position, then the
// verdict and the orders of the forced pivot
int launch_rv_exchange(RevLP *lps, const int *act, int nact, const RevGeom &g);
int launch_rv_setup(RevLP *lps, const int *act, int nact, const RevGeom &g);        // forced pivot, lists, refresh, check
int launch_rv_pivot(RevLP *lps, const int *act, int nact, const RevGeom &g);        // a loop pivot: Bland step?, K1, K2, K3
// a dual pivot of the relaxations in the dual loop: leaving row, dual pricing, K2 / K3 in their kDualPick form
int launch_rv_dual_pivot(RevLP *lps, const int *act, int nact, const RevGeom &g);
// K1-K3 of a loop pivot in their G = true instances over a list of relaxations of searched starts (no Bland step)
int launch_rv_pivot_g(RevLP *lps, const int *act, int nact, const RevGeom &g);
int launch_rv_ctrl(RevLP *lps, const int *act, int nact, RevOut *out, const RevGeom &g);

}  // namespace gomilp
