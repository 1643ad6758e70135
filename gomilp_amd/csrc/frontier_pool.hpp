// The frontier pool behind gomilp_pool_* / gomilp_frontier_solve*: its knobs (PoolKnobs), the routing of one wave as a pure function
// (WavePlan; DESIGN.md section 2.5f, probe: gomilp_debug_wave_plan) and the pool itself.  The wave runs in frontier_pool.cpp.
#pragma once
#include <stdint.h>

#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "engine.hpp"
#include "engine_batch.hpp"
#include "engine_batch_revised.hpp"

namespace gomilp {

// The pool's own knobs (gomilp_pool_set).  The first group routes a wave (WavePlan), the second is only kept here and handed on.
struct PoolKnobs {
    int batched = 1;            // 0 = every relaxation through a worker's single-relaxation engine (round-1 path)
    int batch_revised = 1;      // wide waves (n - m >= 2m) that the workers would run on the unguarded revised pipelines take the
                                // device-batched revised simplex (engine_batch_revised.hpp); 0: every such wave on the workers
    int warm_revised = 0;       // (opt-in) a gomilp_frontier_solve_warm call whose wave passes the wide routing test runs on the batched
                                // revised simplex too, with warm starts and keeping; 0: such a call goes to the workers, cold
    int rev_roots = 1;          // a wide wave that uses several roots, or a root other than the set_root problem (gomilp_frontier_solve_roots),
                                // runs on the batched revised simplex when every root it uses passes that schedule's test — one schedule for the
                                // wave, bit-identical results; 0: such a wave on the workers, whole
    int split_large = 1;        // waves of >= 4 large relaxations run as two interleaved schedules
    int split_phase = 1;        // relaxations that start feasible (Phase II from the slack basis: the long pivot chains of a wave) and
                                // relaxations that need Phase I (on a B&B frontier mostly proved infeasible within a few pivots) run as two
                                // schedules side by side: a block step of the wide group (hundreds of tableaus gathered / updated) no longer
                                // sits between two blocks of a long chain
    int large_loop = 0;         // relaxations of 1025..2048 rows / columns run on the workers' persistent loop kernels (four at a
                                // time, each with its pivot workgroups on an XCD of its own) instead of the batched launch pairs.  Off:
                                // measured 342 k pivots/s for 4 metric LPs against 391 k batched — four updates streaming at once
                                // raise the latency of every chain's agent-scope reads and polls
    int cond_guard = 1, exact_degenerate = 1;   // the workers' knobs of these names: every schedule of the pool decides as they do
                                                // (WavePlan reads cond_guard here, BatchEngine::run_roots its own copy: the defaults are equal and
                                                // gomilp_pool::apply_knobs is the only writer of the copy — keep the two in step)
    int64_t refresh = 0;        // the workers' knob of this name: a periodic refresh stays on the workers
    int large_rows = 0;         // (opt-in) roots and children beyond the 64 KB LDS window (ld > 8192): the workers accept what a context accepts
                                // there (slack-basis roots that fit the device memory), and wide waves of such relaxations run on the batched
                                // revised simplex in its chunked kernels (batch_revised.hip: the CK = true instances); warm starts of that schedule are no longer
                                // limited to 4096 rows.  0: pools keep the row limit of one-pass LDS staging
    // ---- kept and handed on (BatchEngine: gomilp_pool::apply_knobs; RevBatchEngine: per run)
    int rev_exchange = 1;       // on the batched revised simplex a relaxation whose Phase I ends with the artificial basic at level zero
                                // exchanges it on the device (batch_revised.hip: k_rv_exch) instead of going to a worker's whole solve — the same
                                // column, bit-identical results; 0: the hand-over (host_fallbacks)
    int rev_inplace = 0;        // (opt-in) a run of the batched revised simplex assembles no per-child A^T: its kernels read the root's resident
                                // A^T in place and synthesise the K branch entries and unit columns (rev_child_col.h) — no At arena ((n + 1) x ld
                                // doubles per relaxation), no k_rv_assemble launch, bit-identical results; 0: today's launches.  Routing does not
                                // depend on it
    int rev_general = 1;        // wide waves of roots WITHOUT a slack basis (equality rows; RootView::genrev) run on the batched revised simplex too:
                                // a child starts from its root's searched basis + its branch slacks (k_rv_gen_start), runs the guarded loop, and
                                // goes to a worker's whole solve where that would take an exact step (host_fallbacks); cold calls, one-pass
                                // staging, exact_degenerate 1 or 2.  1: children of up to RevBatchEngine::kRevGeneralAutoRows rows (beyond, the
                                // workers' blocked tableau is faster: DESIGN.md section 2.5e); 2: up to kRevGeneralMaxRows rows; 0: such waves on
                                // the workers, whole
    int64_t rev_mem_limit = 0;  // MiB, 0: none.  Where it is below the free device memory it takes its place in RevBatchEngine::run's test of
                                // whether a wave's buffers fit (a wave that does not fit runs on the workers, whole): a cap for a shared card
    int64_t max_pivots = 0;     // the workers' knob of this name, as the batched revised simplex needs it (negative: 0)
    int64_t row_chunk = 0;      // the workers' knob of this name (doubles per LDS chunk, a multiple of 512 up to 8192; 0: automatic): with
                                // large_rows = 1 the batched revised simplex stages in chunks of it too, at any row count; with large_rows = 0 that
                                // schedule never looks at it
    int batch_virt = 1;         // wide waves on virtual tableaus for their first block
    int batch_res = 0;          // block steps of narrow waves in the register-resident kernel (opt-in: k_b_loop / launch pairs otherwise)
    int batch_loop = 1;         // block steps of narrow waves in the persistent loop kernel
    int sample_batch = 0;       // HIP-event times of sampled block launches (BatchEngine::set_sampling)
    int bt_fault = 0;           // diagnostic flavour only: BatchEngine::set_fault

    // where gomilp_pool_set sends a key: Pool: recorded here, done; PoolAndWorkers: recorded here, and to the workers' engines;
    // WorkersFirst: recorded here only when every worker's engine accepted it; Workers: no knob of the pool's
    enum class Scope { Pool, PoolAndWorkers, WorkersFirst, Workers };
    static Scope scope(const char *key);
    // records `value` under `key`; false: not a key this struct holds ("lu_large": accepted and ignored — gomilp_pool_create leaves it 0)
    bool set(const char *key, int64_t value);
};

// The wave as the caller passed it: relaxation i is a child of root root_of[i] (nullptr: all of root 0) with the branch rows
// koff[i] .. koff[i + 1] - 1 of var / sign / rhs.
struct WaveArgs {
    int64_t count = 0;
    const int32_t *root_of = nullptr;
    const int64_t *koff = nullptr;
    const int32_t *var = nullptr;
    const double *sign = nullptr, *rhs = nullptr;
    int root(int64_t i) const { return root_of ? root_of[i] : 0; }
    int64_t K(int64_t i) const { return koff[i + 1] - koff[i]; }
};

// Which schedule takes a wave and how the tableau schedule cuts it: decided here and nowhere else, from the root views the pool holds
// (m, n, unit_basis, gen, verify_status, scale_span, hb), the wave and the knobs.  No HIP call, no allocation on the device, no lock.
// The routing table: DESIGN.md section 2.5f; tests/test_wave_plan.py asserts it through gomilp_debug_wave_plan.
struct WavePlan {
    enum Route : int { WORKERS = 0, REVISED = 1, TABLEAU = 2 };
    enum Cut : int { NONE = 0, ONE = 1, ONE_GATHERED = 2, PHASE_SPLIT = 3, HALVES = 4 };
    Route route = WORKERS;
    bool warm_call = false;   // gomilp_frontier_solve_warm: the tableau schedule takes gathered lists, with or without a warm start among them
    bool halves = false;      // TABLEAU: a cold wave of >= 4 large relaxations (rank-16 block kernel) under split_large

    static WavePlan make(const Engine::RootView *const *views, int nroots, const WaveArgs &w, bool warm_call, const PoolKnobs &knobs);
    // TABLEAU in a warm call: the relaxations that start from their parent's kept state (parent >= 0, at least one branch row,
    // resident[i]: the state is in the store as WK_TABLEAU) and the rest, both ascending.  `resident` is read where the first two hold.
    void warm_groups(const WaveArgs &w, const int64_t *parent, const char *resident, std::vector<int64_t> *warm_idx, std::vector<int64_t> *cold_idx) const;
    // TABLEAU, after the warm run: `cold_idx` is the cold list with the relaxations that spent their dual budget back in it, sorted
    // (read in a warm call only: a cold call's cold part is the whole wave).  PHASE_SPLIT: the lists of the feasible starts and of
    // the Phase-I starts; HALVES: relaxations [0, half) and [half, count).
    struct ColdCut { Cut cut = NONE; std::vector<int64_t> feasible, phase1; int64_t half = 0; };
    ColdCut cut_cold(const Engine::RootView *const *views, int nroots, const WaveArgs &w, const std::vector<int64_t> &cold_idx, const PoolKnobs &knobs) const;
};

// warm: parent / tag / keep per relaxation (each nullable), budget; null: a cold wave
struct WarmArgs { const int64_t *parent, *tag; const int32_t *keep; int32_t budget; };

}  // namespace gomilp

// One worker = one Engine (stream + work buffers) with its own resident copy of the root and a persistent host thread;
// the pivot loops of a wave run device-batched on the pool's BatchEngine (engine_batch.hpp), the workers take what is
// left per relaxation: the final gonum-order solve of a finished basis, or a whole solve where the batched schedule
// hands a relaxation back.
struct gomilp_pool {
    int device = 0;
    std::vector<std::unique_ptr<gomilp::Engine>> eng;
    std::vector<int64_t> root;  // root problem id inside each engine
    int64_t m0 = 0, n0 = 0;
    gomilp::PoolKnobs knobs;
    std::unique_ptr<gomilp::BatchEngine> batch;
    std::unique_ptr<gomilp::BatchEngine> batch2;   // second schedule (split waves, waves of large relaxations; created on first use)
    std::unique_ptr<gomilp::RevBatchEngine> rev;   // created on first use
    gomilp::WarmStore warm;     // final states kept for warm starts (gomilp_frontier_solve_warm), shared by both schedules
    gomilp::Engine::RootView view;      // of eng[0]'s root (all workers hold the same data)
    // further roots (gomilp_pool_add_root): resident in worker 0's engine only, read in place by the others
    std::vector<int64_t> extra_root;
    std::vector<std::unique_ptr<gomilp::Engine::RootView>> extra_view;
    std::mutex call_mu;         // one wave at a time per pool
    // A schedule that runs beside the calling thread's (the wide half of a split wave, the second half of a wave of large LPs) gets a
    // thread that LIVES with the pool: a std::thread per wave cost, once in ~50 waves, milliseconds (stack mapped and unmapped in a
    // process full of pinned and device-mapped memory: 6-10 ms waves among 4.0 ms ones in tools/wave_outliers.py).
    struct Aux {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        std::function<void()> task;
        bool has = false, done = true, stop = false;
        void loop();
        void run(std::function<void()> f);
        void wait();
        ~Aux();
    };
    Aux aux;
    // persistent workers
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv, cv_idle;
    std::deque<std::function<void(int)>> queue;
    int busy = 0;
    bool stop = false;

    void worker(int w);
    void submit(std::function<void(int)> f);
    void drain();
    ~gomilp_pool();

    // the knob values a tableau schedule decides on: both schedules of a split wave decide alike
    void apply_knobs(gomilp::BatchEngine &be) const;
    gomilp::BatchEngine &second_schedule();
};

namespace gomilp {
// gomilp_frontier_solve_roots (wa == nullptr) / gomilp_frontier_solve_warm
int frontier_solve(gomilp_pool *pool, const WaveArgs &w, double tol, double *z_out, double *x_out, int64_t ldx, int32_t *status_out,
                   int32_t *has_x_out, gomilp_frontier_stats *stats, const WarmArgs *wa);
}  // namespace gomilp
