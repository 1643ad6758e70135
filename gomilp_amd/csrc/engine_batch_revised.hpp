// Device-batched wave of WIDE relaxations (n - m >= 2m): the three-kernel revised simplex with the relaxation as a grid dimension
// (batch_revised.hip).  The counterpart of BatchEngine (engine_batch.hpp), which only knows the tableau formulation: one stream, a
// fixed list of launches per superstep for the whole wave, one host round trip per superstep.  It takes exactly the waves whose
// relaxations a worker's Engine::solve would run on the revised pipelines without the exact-step guard, and computes what that
// solve computes: the kernels run the helpers of simplex_helpers.h, the stages follow Engine::solve_locked / run_loop / host_bland.
// With pool knob rev_general it also takes the children of wide roots WITHOUT a slack basis, from the root's searched basis: those run
// the guarded loop and leave the schedule (BS_HOST) wherever a worker's solve would decide on a fresh gonum-order solve.
#pragma once
#include <stdint.h>

#include "engine.hpp"
#include "engine_batch.hpp"

namespace gomilp {

class RevBatchEngine {
   public:
    struct Stats {
        int64_t launches = 0, supersteps = 0, warm_kept = 0;
        double seconds_total = 0;
    };
    explicit RevBatchEngine(int device);
    ~RevBatchEngine();
    // do children of this root with K_min..K_max branch rows run on the revised pipelines, unguarded, on a worker with these knobs?
    // (what SolvePlan::make decides per solve — use_tab, SolvePlan::exact_wanted, replay_if_feasible — for the whole range of children)
    // large_rows (the pool knob): the row limit of one-pass LDS staging (ld <= kLdsWindowLd) is dropped, every other condition stays
    // A wide root WITHOUT a slack basis passes where it carries RootView::genrev (pool knob rev_general, DESIGN.md section 2.5e "Equality-form
    // roots"): its children run the guarded loop (guard = 1e-9, exact_degenerate 1 or 2) and leave the schedule where a worker would take
    // an exact step; children of up to kRevGeneralMaxRows rows (the range the route is tested and timed over), one-pass staging only.
    // kRevGeneralAutoRows: what WavePlan routes at rev_general = 1 — at 81 rows the schedule runs a 24-child wave as fast as eight workers,
    // at 161 rows 11 % and at 300 rows 43 % slower (the workers solve such children on the blocked tableau, eight pivots per launch)
    static constexpr int kRevGeneralMaxRows = 300, kRevGeneralAutoRows = 96;
    static bool eligible(const Engine::RootView &R, int K_min, int K_max, int exact_degenerate, int cond_guard, int large_rows = 0);
    // The wave (relaxation i is a child of roots[root_of[i]] — root_of null: of roots[0] — with rows koff[i]..koff[i+1] of var / sign /
    // rhs; every root the wave uses must pass `eligible` with its own children's K range).  One schedule for the whole wave: each
    // relaxation carries its own root's shape and data, the grids and staged vectors are sized for the wave's largest relaxation, and a
    // relaxation's values depend neither on them nor on its neighbours.  on_done as BatchEngine::run_roots: stage
    // BS_DONE with the final status (basic / xb non-null where the status wants the final solve) or BS_HOST.  *fits = false: the wave's
    // buffers do not fit the free device memory — nothing ran, the caller solves the wave on the workers.
    // warm (pool knob warm_revised; nullptr: a cold wave): relaxation i starts from the kept WK_REVISED state that
    // parent[i] names when its branch rows extend that state's rows (a bitwise prefix) by J >= 1 — B^-1 = [[B_p^-1, 0], [R, I_J]], the
    // dual loop, then Phase II — and cold otherwise, in the same run; a relaxation with keep[i] that ends BS_DONE with GOMILP_OK leaves
    // its B^-1 and basis list in the store under tag[i].  A warm start that spends its dual budget is reported once with stage BS_COLD
    // (warm = 1, pivd), re-initialised in place and solved cold by the same run: its second report has warm = 0.  Without large_rows,
    // waves with ld_max > kRevDualLd run cold, with keeping; with it they start warm and price through the chunked dual kernel.
    // A kept state serves children of the root it was kept under only (root_serial).
    int run(const Engine::RootView *const *roots, int nroots, const int32_t *root_of, int64_t count, const int64_t *koff, const int32_t *var,
            const double *sign, const double *rhs, double tol, int64_t max_pivots, const BatchEngine::DoneFn &on_done, Stats *stats, bool *fits,
            const WarmSpec *warm = nullptr);

    // pool knob rev_exchange: a relaxation whose Phase I ends with the artificial basic at level zero exchanges it on the device (the
    // candidate scan of batch_revised.hip: launch_rv_exchange in front of the set-up launches of the supersteps that have such a
    // relaxation, nowhere else; Outcome::art_exchanges) and goes on to Phase II; off: it is handed over as BS_HOST.  The |x_art| band
    // (1e-13 < |x_art| < 1e-11) is BS_HOST either way: its verdict needs a fresh gonum-order solve.
    void set_exchange(bool on) { exchange_ = on; }

    // pool knobs large_rows / row_chunk: with large_rows the kernels that stage an m-long vector run in their chunked forms (CK = true of
    // batch_revised.hip) — row_chunk doubles at a time where the pool set it (any row count), else kAutoRowChunk beyond the LDS window —
    // and warm starts are not limited to kRevDualLd.  Bit-identical to the one-pass forms.  Off (default): row_chunk is not looked at.
    void set_large_rows(bool on, int64_t row_chunk) { large_rows_ = on; row_chunk_ = row_chunk; }

    // pool knob rev_inplace: the run assembles no At — no At arena, no k_rv_assemble launch; every kernel that reads a child's column takes
    // it from the relaxation's root where it lies (ChildCol, rev_child_col.h), and the Phase-I artificial column is one ld-long row per
    // relaxation in the work arena.  Bit-identical to the assembled run.  Off (default): today's launches.
    void set_inplace(bool on) { inplace_ = on; }
    // pool knob rev_mem_limit (MiB; 0: none): where it is below the free device memory it takes its place in the test behind *fits
    void set_mem_limit(int64_t mib) { mem_limit_mib_ = mib > 0 ? mib : 0; }

    // The layout of a wave's two arenas, in doubles, per relaxation: offsets into the work arena (cleared per wave; [wk0, wk1) is the
    // relaxation's own part) and `at` into the At arena.  inplace: no At (at = 0 everywhere, *at_tot = 0) and `art`, the ld-long row of
    // the artificial column, in the work arena (unused otherwise).
    struct Lay { size_t wk0, wk1; size_t at, binv0, binv1, xb, y, dvec, move, bb, rvec, c1, ysc, basic, nonbasic, inb, pkp, pkr, pip, pir, st, art, gpkp, gpkr; };
    // A pure function of the shapes (no HIP call): relaxation i is a child of root root_of[i] (null: of root 0; the caller has checked the
    // range) with koff[i + 1] - koff[i] branch rows.  lay: null, or room for count entries.  run sizes its buffers from it, and
    // gomilp_debug_rev_footprint reports it.  root_gen: null, or per root whether it has no slack basis but a searched one (RootView::genrev):
    // its relaxations take 4 * kMaxPartials doubles more, at the tail (gpkp / gpkr: the price and ratio keys with their runner-ups).
    static void layout(const int64_t *root_m, const int64_t *root_n, int64_t count, const int32_t *root_of, const int64_t *koff, bool inplace,
                       Lay *lay, size_t *at_tot, size_t *wk_tot, const char *root_gen = nullptr);

    // gives the wave buffers back (they grow with the largest wave seen: 5 MB per 300 x 1500 relaxation); the pool calls it when the
    // root changes
    void release();

   private:
    struct Buf;
    struct Wave;   // one call of run: its arguments, what the steps derive from them, the steps (engine_batch_revised.cpp)
    int device_;
    bool exchange_ = true;
    bool large_rows_ = false;
    int64_t row_chunk_ = 0;
    bool inplace_ = false;
    int64_t mem_limit_mib_ = 0;
    hipStream_t stream_ = nullptr;
    Buf *b_;
};

}  // namespace gomilp
