// One wave of the frontier pool: WavePlan says where it goes (a pure function, below), the Wave runs it.
#include "frontier_pool.hpp"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>

using gomilp::BatchEngine;
using gomilp::Engine;
using gomilp::RevBatchEngine;

namespace gomilp {

// ---- PoolKnobs

PoolKnobs::Scope PoolKnobs::scope(const char *key) {
    const std::string k(key);
    for (const char *p : {"batched", "batch_revised", "warm_revised", "rev_exchange", "rev_roots", "split_large", "split_phase", "large_loop",
                          "batch_virt", "batch_res", "batch_loop", "sample_batch", "lu_large", "large_rows", "rev_inplace", "rev_mem_limit", "rev_general"})
        if (k == p) return Scope::Pool;
#ifdef GOMILP_DEBUG
    if (k == "bt_fault") return Scope::PoolAndWorkers;
#endif
    if (k == "cond_guard" || k == "exact_degenerate") return Scope::PoolAndWorkers;
    if (k == "refresh" || k == "max_pivots" || k == "row_chunk") return Scope::WorkersFirst;
    return Scope::Workers;
}

bool PoolKnobs::set(const char *key, int64_t value) {
    const std::string k(key);
    struct { const char *name; int *at; } flags[] = {
        {"batched", &batched}, {"batch_revised", &batch_revised}, {"warm_revised", &warm_revised}, {"rev_exchange", &rev_exchange},
        {"rev_roots", &rev_roots}, {"split_large", &split_large}, {"split_phase", &split_phase}, {"large_loop", &large_loop},
        {"batch_virt", &batch_virt}, {"batch_res", &batch_res}, {"batch_loop", &batch_loop}, {"sample_batch", &sample_batch},
        {"large_rows", &large_rows}, {"rev_inplace", &rev_inplace}};
    for (auto &f : flags) if (k == f.name) { *f.at = value ? 1 : 0; return true; }
    if (k == "lu_large") return true;
    if (k == "rev_general") {   // 0 off, 1 up to kRevGeneralAutoRows rows, 2 up to kRevGeneralMaxRows
        if (value < 0 || value > 2) return false;
        rev_general = (int)value;
        return true;
    }
    if (k == "rev_mem_limit") {   // MiB; 0: none
        if (value < 0) return false;
        rev_mem_limit = value;
        return true;
    }
    if (k == "cond_guard") { cond_guard = (int)value; return true; }
    if (k == "exact_degenerate") { exact_degenerate = (int)value; return true; }
#ifdef GOMILP_DEBUG
    if (k == "bt_fault") { bt_fault = (int)value; return true; }
#endif
    if (k == "refresh") { refresh = value; return true; }
    if (k == "max_pivots") { max_pivots = value < 0 ? 0 : value; return true; }
    if (k == "row_chunk") {   // (the value checks of gomilp_ctx_set)
        if (value < 0 || value % 512 != 0 || value > kLdsWindowLd) return false;
        row_chunk = value;
        return true;
    }
    return false;
}

// ---- WavePlan

namespace {
bool some_b_negative(const Engine::RootView &V) {
    for (double v : V.hb) if (v < -1e-13) return true;
    return false;
}
}  // namespace

WavePlan WavePlan::make(const Engine::RootView *const *views, int nroots, const WaveArgs &w, bool warm_call, const PoolKnobs &knobs) {
    WavePlan p;
    p.warm_call = warm_call;
    const int64_t count = w.count;
    if (!knobs.batched || count <= 0) return p;
    int K_max = 0;
    for (int64_t i = 0; i < count; i++) K_max = std::max<int>(K_max, (int)w.K(i));
    // some relaxation starts in Phase I: over every root the pool HOLDS (used by the wave or not) and every branch row of the wave
    bool any_p1 = false;
    for (int r = 0; r < nroots && !any_p1; r++) any_p1 = (views[r]->gen && !views[r]->unit_basis) || some_b_negative(*views[r]);
    for (int64_t k = w.koff[0]; k < w.koff[count] && !any_p1; k++) if (w.rhs[k] < -1e-13) any_p1 = true;
    // ---- the tableau schedule: every root the pool holds must pass
    bool use_batch = true;
    for (int r = 0; r < nroots && use_batch; r++) use_batch = BatchEngine::eligible(*views[r], K_max, any_p1, knobs.cond_guard);
    int m_big = 0, nn_big = 0;
    for (int r = 0; r < nroots; r++) { m_big = std::max(m_big, views[r]->m + K_max); nn_big = std::max(nn_big, views[r]->n - views[r]->m + (any_p1 ? 1 : 0)); }
    const int ldt_big = batch_ldt(nn_big), need = std::max(m_big, ldt_big);
    // 1025..2048 rows / columns, knob "large_loop": the workers' persistent loop kernels instead (four share the device,
    // Engine::loop_acquire)
    if (use_batch && knobs.large_loop && need > 1024 && need <= 2048) use_batch = false;
    if (use_batch) {
        p.route = TABLEAU;
        // Large relaxations (8-workgroup block kernel, rank-16 update): a block step of one schedule is [block kernels of all its
        // relaxations side by side] then [their updates one after the other]; two schedules of half the wave each, on two
        // streams, put one half's updates under the other half's block kernels.
        // (four schedules — one per LP of a wave of four — measured 363 k pivots / s against 408-440 k for one or two: the chains slow
        // each other through the memory system)
        p.halves = knobs.split_large && count >= 4 && bt_batch_k(m_big, ldt_big) == 16 && !warm_call;
        return p;
    }
    // ---- Wide waves: the device-batched revised simplex, where every relaxation of the wave is one that a worker's Engine::solve runs on the
    // revised pipelines without the exact-step guard (slack starts; a periodic refresh stays on the workers).  Cold calls, and with the
    // knob warm_revised the warm call: relaxations whose parent's kept state is of this schedule start from it (section 2.6b).
    // Rows beyond the LDS window (ld > 8192) only with the knob large_rows: the chunked kernels of batch_revised.hip.
    // The test runs over the roots the WAVE uses, each with the K range of its own children; roots the pool merely holds do not count.
    // One used root that fails (narrow, no basis to start from, a guarded size, a verify verdict) sends the wave where it went before, whole.
    // A used root without a slack basis passes with its searched basis (RootView::genrev, knob rev_general): the guarded loop, per relaxation.
    if (!knobs.batch_revised || (warm_call && !knobs.warm_revised) || knobs.refresh != 0) return p;
    std::vector<int> k_lo((size_t)nroots, INT32_MAX), k_hi((size_t)nroots, -1);
    bool other_root = false;   // the wave uses more than one root, or a root other than the set_root problem
    for (int64_t i = 0; i < count; i++) {
        const int ri = w.root(i), K = (int)w.K(i);
        k_lo[(size_t)ri] = std::min(k_lo[(size_t)ri], K); k_hi[(size_t)ri] = std::max(k_hi[(size_t)ri], K);
        if (ri != 0) other_root = true;
    }
    bool use_rev = knobs.rev_roots || !other_root;
    // a used root without a slack basis (RootView::genrev): knob rev_general, cold calls, one-pass staging (no CK x G kernel instances),
    // and children of up to kRevGeneralAutoRows rows (measured no slower than the workers) unless the knob is 2
    const int gen_rows = knobs.rev_general >= 2 ? RevBatchEngine::kRevGeneralMaxRows : RevBatchEngine::kRevGeneralAutoRows;
    for (int r = 0; r < nroots && use_rev; r++)
        if (k_hi[(size_t)r] >= 0 && !views[r]->unit_basis &&
            (!knobs.rev_general || warm_call || (knobs.large_rows && knobs.row_chunk > 0) || views[r]->m + k_hi[(size_t)r] > gen_rows)) use_rev = false;
    for (int r = 0; r < nroots && use_rev; r++)
        if (k_hi[(size_t)r] >= 0) use_rev = RevBatchEngine::eligible(*views[r], k_lo[(size_t)r], k_hi[(size_t)r], knobs.exact_degenerate, knobs.cond_guard, knobs.large_rows);
    // (a branch row on one of its root's slack columns: the child has no slack basis)
    for (int64_t i = 0; i < count && use_rev; i++) {
        const Engine::RootView &V = *views[w.root(i)];
        const int64_t first_slack = (int64_t)V.n - V.m;
        for (int64_t k = w.koff[i]; k < w.koff[i + 1] && use_rev; k++) if (w.var[k] < 0 || w.var[k] >= first_slack) use_rev = false;
    }
    if (use_rev) p.route = REVISED;
    return p;
}

void WavePlan::warm_groups(const WaveArgs &w, const int64_t *parent, const char *resident, std::vector<int64_t> *warm_idx, std::vector<int64_t> *cold_idx) const {
    for (int64_t i = 0; i < w.count; i++) {
        const bool warm = parent && parent[i] >= 0 && w.K(i) >= 1 && resident[i];
        (warm ? warm_idx : cold_idx)->push_back(i);
    }
}

WavePlan::ColdCut WavePlan::cut_cold(const Engine::RootView *const *views, int nroots, const WaveArgs &w, const std::vector<int64_t> &cold_idx, const PoolKnobs &knobs) const {
    ColdCut c;
    const int64_t ncold = warm_call ? (int64_t)cold_idx.size() : w.count;
    // relaxations that start feasible (slack basis, b >= 0, every branch right-hand side >= 0: Phase II at once) against those that
    // need Phase I
    if (knobs.split_phase && !halves && ncold >= 16) {
        std::vector<char> root_ok((size_t)nroots, 0);
        for (int r = 0; r < nroots; r++) root_ok[(size_t)r] = views[r]->unit_basis && !some_b_negative(*views[r]);
        for (int64_t t = 0; t < ncold; t++) {
            const int64_t i = warm_call ? cold_idx[(size_t)t] : t;
            bool f = root_ok[(size_t)w.root(i)] != 0;
            for (int64_t k = w.koff[i]; k < w.koff[i + 1] && f; k++) if (w.rhs[k] < -1e-13) f = false;
            (f ? c.feasible : c.phase1).push_back(i);
        }
    }
    if (ncold == 0) c.cut = NONE;   // (every relaxation of the call was a warm start that stayed warm)
    else if (!c.feasible.empty() && !c.phase1.empty()) c.cut = PHASE_SPLIT;
    else if (warm_call) c.cut = ONE_GATHERED;   // (the cold part is a proper subset of the call, or carries keep flags)
    else if (halves) { c.cut = HALVES; c.half = w.count / 2; }
    else c.cut = ONE;
    if (c.cut != PHASE_SPLIT) { c.feasible.clear(); c.phase1.clear(); }
    return c;
}

}  // namespace gomilp

// ---- the pool's threads

void gomilp_pool::Aux::loop() {
    for (;;) {
        std::function<void()> f;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return stop || has; });
            if (stop && !has) return;
            f = std::move(task); has = false;
        }
        f();
        { std::lock_guard<std::mutex> lk(mu); done = true; }
        cv.notify_all();
    }
}
void gomilp_pool::Aux::run(std::function<void()> f) {
    { std::lock_guard<std::mutex> lk(mu); task = std::move(f); has = true; done = false; }
    if (!th.joinable()) th = std::thread([this] { loop(); });
    cv.notify_all();
}
void gomilp_pool::Aux::wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return done; }); }
gomilp_pool::Aux::~Aux() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    cv.notify_all();
    if (th.joinable()) th.join();
}

void gomilp_pool::worker(int w) {
    for (;;) {
        std::function<void(int)> task;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return stop || !queue.empty(); });
            if (stop && queue.empty()) return;
            task = std::move(queue.front());
            queue.pop_front();
            busy++;
        }
        task(w);
        {
            std::lock_guard<std::mutex> lk(mu);
            busy--;
            if (queue.empty() && busy == 0) cv_idle.notify_all();
        }
    }
}
void gomilp_pool::submit(std::function<void(int)> f) {
    { std::lock_guard<std::mutex> lk(mu); queue.push_back(std::move(f)); }
    cv.notify_one();
}
void gomilp_pool::drain() {
    std::unique_lock<std::mutex> lk(mu);
    cv_idle.wait(lk, [&] { return queue.empty() && busy == 0; });
}
gomilp_pool::~gomilp_pool() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    cv.notify_all();
    for (auto &t : threads) t.join();
}

void gomilp_pool::apply_knobs(BatchEngine &be) const {
    be.set_cond_guard(knobs.cond_guard);
    be.set_exact_degenerate(knobs.exact_degenerate);
    be.set_sampling(knobs.sample_batch != 0);
    be.set_loop(knobs.batch_loop != 0);
    be.set_res(knobs.batch_res != 0);
    be.set_virt(knobs.batch_virt != 0);
#ifdef GOMILP_DEBUG
    be.set_fault(knobs.bt_fault);
#endif
}
BatchEngine &gomilp_pool::second_schedule() {
    if (!batch2) {
        batch2.reset(new BatchEngine(device));
        apply_knobs(*batch2);
    }
    return *batch2;
}

// ---- one wave

namespace {

using Clock = std::chrono::steady_clock;
double busy_since(Clock::time_point s0) { return std::chrono::duration<double>(Clock::now() - s0).count(); }

// a subset of the wave as a schedule of its own (the schedules take contiguous lists)
struct Group { std::vector<int32_t> root_of, var, keep; std::vector<int64_t> koff, parent, tag; std::vector<double> sign, rhs; };

// Everything a wave's schedules, the auxiliary thread and the submitted worker tasks touch: lives on the stack of the call, which
// leaves only after the auxiliary thread has been waited for and the workers drained.
struct Wave {
    gomilp_pool *pool;
    const gomilp::WaveArgs &a;
    const gomilp::WarmArgs *wa;
    double tol;
    double *z_out, *x_out;
    int64_t ldx;
    int32_t *status_out, *has_x_out;
    std::vector<const Engine::RootView *> views;
    int nroots = 0;
    std::vector<gomilp_frontier_stats> ws;   // per worker
    gomilp_frontier_stats agg = gomilp_frontier_stats();
    BatchEngine::Stats bs;
    // the tableau schedules report from two threads in the split routes: agg and cold_again under agg_mu there (the revised schedule
    // reports on the calling thread only)
    bool tableau = false;
    std::mutex agg_mu;
    std::vector<int64_t> cold_again;   // warm starts that spent their dual-pivot budget: solved cold by this same call

    // One relaxation on worker w's engine.  basic == nullptr: a whole solve (the round-1 path; also the fall-back of the batched
    // schedules); else the epilogue of a relaxation whose pivot loops ran device-batched: the final gonum-order solve of its basis.
    // child i of root r on worker w: root 0 lives in every worker's engine, the others in worker 0's
    void worker_step(int w, int64_t i, const int32_t *basic, const double *xb, int loop_rc) {
        const auto s0 = Clock::now();
        Engine &E = *pool->eng[w];
        gomilp_frontier_stats &S = ws[w];
        const int ri = a.root(i);
        const int64_t k0 = a.koff[i], K = a.K(i), n0 = views[ri]->n;
        const int64_t id = ri == 0 ? E.upload_child(pool->root[w], (int)K, a.var + k0, a.sign + k0, a.rhs + k0)
                                   : E.upload_child_of(*pool->eng[0], pool->extra_root[ri - 1], (int)K, a.var + k0, a.sign + k0, a.rhs + k0);
        if (id < 0) { status_out[i] = (int32_t)-id; return; }
        std::vector<double> x((size_t)(n0 + K), 0.0);
        gomilp_lp_stats st;
        int32_t hx = 0;
        double z = NAN;
        int rc;
        if (!basic) {
            rc = E.solve(id, tol, nullptr, &z, x.data(), &hx, nullptr, &st);
            E.free_problem(id);
        } else {
            const double t_up = busy_since(s0);
            rc = E.finish_from_basis(id, basic, xb, loop_rc, &z, x.data(), &hx, nullptr, &st);
            E.free_problem(id);
            if (GOMILP_DBG_ENV("GOMILP_DEBUG_TASKS") && busy_since(s0) > 5e-3)
                fprintf(stderr, "slow finish: worker %d child %lld upload %.2f ms finish %.2f ms (device %.2f host %.2f) rounds %lld dense %lld\n", w, (long long)i, 1e3 * t_up,
                        1e3 * st.seconds_total, 1e3 * st.seconds_final_device, 1e3 * st.seconds_final_host, (long long)st.lu_rounds, (long long)st.lu_dense_steps);
        }
        status_out[i] = rc; z_out[i] = z; has_x_out[i] = hx;
        if (hx) for (int64_t j = 0; j < n0; j++) x_out[i * ldx + j] = x[j];  // subproblem.go:157-159
        if (!basic) {
            S.relaxations++; S.pivots_phase1 += st.pivots_phase1; S.pivots_phase2 += st.pivots_phase2;
            S.bland_steps += st.bland_steps; S.phase1_runs += st.phase1_used;
        }
        S.kernel_launches += st.kernel_launches;
        S.seconds_busy_sum += busy_since(s0);
    }
    void submit_whole(int64_t i) { pool->submit([this, i](int w) { worker_step(w, i, nullptr, nullptr, 0); }); }

    // a schedule reports relaxation i (an index of the caller's arrays) terminal; basic / xb: non-null where its status needs the final
    // solve (BatchEngine: GOMILP_OK / ERR_BLAND; RevBatchEngine: ERR_UNSUPPORTED too)
    void on_done(int64_t i, const BatchEngine::Outcome &o, const int32_t *basic, const double *xb) {
        std::unique_lock<std::mutex> lk(agg_mu, std::defer_lock);
        if (tableau) lk.lock();
        if (o.warm) { agg.warm_started++; agg.pivots_dual += o.pivd; }
        if (o.stage == gomilp::BS_COLD) {   // (the revised schedule solves it cold in the same run and reports it again)
            agg.warm_fallbacks++;
            if (tableau) cold_again.push_back(i);
            return;
        }
        if (o.stage != gomilp::BS_DONE) {   // a path the device schedule does not cover (revised: the |x_art| band; with rev_exchange = 0 the zero-level artificial exchange; a searched start's start guard and exact steps)
            agg.host_fallbacks++;
            submit_whole(i);
            return;
        }
        agg.relaxations++; agg.batched_relaxations++;
        agg.pivots_phase1 += o.piv1; agg.pivots_phase2 += o.piv2; agg.bland_steps += o.bland; agg.phase1_runs += o.phase1_used;
        agg.art_exchanges += o.art_exchanges;
        if (basic) {
            const int rc0 = o.status;
            pool->submit([this, i, basic, xb, rc0](int w) { worker_step(w, i, basic, xb, rc0); });
        } else {
            status_out[i] = o.status;
            if (o.status == GOMILP_ERR_UNBOUNDED) z_out[i] = -INFINITY;   // simplex.go:261-263
        }
    }

    void run_workers() {
        for (int64_t i = 0; i < a.count; i++) submit_whole(i);
    }

    // *fits = false: the wave's buffers do not fit the free device memory: the workers take it, whole
    int run_revised(bool *fits) {
        if (!pool->rev) pool->rev.reset(new RevBatchEngine(pool->device));
        RevBatchEngine::Stats rs;
        pool->rev->set_exchange(pool->knobs.rev_exchange != 0);
        pool->rev->set_large_rows(pool->knobs.large_rows != 0, pool->knobs.row_chunk);
        pool->rev->set_inplace(pool->knobs.rev_inplace != 0);
        pool->rev->set_mem_limit(pool->knobs.rev_mem_limit);
        gomilp::WarmSpec wspec;
        if (wa) {
            wspec.store = &pool->warm; wspec.parent = wa->parent; wspec.tag = wa->tag; wspec.keep = wa->keep; wspec.dual_budget = wa->budget;
        }
        auto od = [this](int64_t i, const BatchEngine::Outcome &o, const int32_t *basic, const double *xb) { on_done(i, o, basic, xb); };   // (called on this thread)
        const int rc = pool->rev->run(views.data(), nroots, a.root_of, a.count, a.koff, a.var, a.sign, a.rhs, tol, pool->knobs.max_pivots, od, &rs, fits, wa ? &wspec : nullptr);
        if (rc == GOMILP_OK && *fits) { bs.launches = rs.launches; bs.supersteps = rs.supersteps; bs.seconds_total = rs.seconds_total; bs.warm_kept = rs.warm_kept; }
        return rc;
    }

    // ---- the tableau schedule

    // runs one after the other: sums; runs side by side: the longer one
    void merge_stats(const BatchEngine::Stats &bs2, bool serial) {
        bs.launches += bs2.launches; bs.blocks += bs2.blocks; bs.blocks_sampled += bs2.blocks_sampled;
        bs.supersteps = serial ? bs.supersteps + bs2.supersteps : std::max(bs.supersteps, bs2.supersteps);
        bs.seconds_inner += bs2.seconds_inner; bs.seconds_update += bs2.seconds_update;
        bs.seconds_total = serial ? bs.seconds_total + bs2.seconds_total : std::max(bs.seconds_total, bs2.seconds_total);
        bs.warm_kept += bs2.warm_kept;
    }
    // (sized once, rows copied in runs: an 8192-wide wave has 100 k branch rows — element-wise push_backs were 1.5 ms of it, in front of
    // the first kernel)
    void gather(const std::vector<int64_t> &idx, Group &g) const {
        const size_t ng = idx.size();
        size_t tot = 0;
        for (int64_t i : idx) tot += (size_t)a.K(i);
        g.koff.resize(ng + 1); g.root_of.resize(ng); g.parent.resize(ng); g.tag.resize(ng); g.keep.resize(ng);
        g.var.resize(std::max<size_t>(tot, 1)); g.sign.resize(std::max<size_t>(tot, 1)); g.rhs.resize(std::max<size_t>(tot, 1));   // (valid pointers for K = 0 everywhere)
        g.var[0] = 0; g.sign[0] = 0; g.rhs[0] = 0;
        size_t at = 0;
        g.koff[0] = 0;
        for (size_t t = 0; t < ng; t++) {
            const int64_t i = idx[t];
            const size_t K = (size_t)a.K(i);
            g.root_of[t] = a.root(i);
            if (K) {
                memcpy(&g.var[at], a.var + a.koff[i], K * sizeof(int32_t));
                memcpy(&g.sign[at], a.sign + a.koff[i], K * sizeof(double));
                memcpy(&g.rhs[at], a.rhs + a.koff[i], K * sizeof(double));
            }
            at += K;
            g.koff[t + 1] = (int64_t)at;
            g.parent[t] = wa && wa->parent ? wa->parent[i] : -1;
            g.tag[t] = wa && wa->tag ? wa->tag[i] : -1;
            g.keep[t] = wa && wa->keep && wa->tag && wa->tag[i] >= 0 ? wa->keep[i] : 0;
        }
    }
    int run_group(BatchEngine &be, const std::vector<int64_t> &idx, const Group &g, bool start_warm, BatchEngine::Stats *out) {
        gomilp::WarmSpec wspec;
        wspec.store = &pool->warm; wspec.parent = g.parent.data(); wspec.tag = g.tag.data(); wspec.keep = g.keep.data();
        wspec.dual_budget = wa ? wa->budget : 0; wspec.start_warm = start_warm;
        auto od = [this, &idx](int64_t i, const BatchEngine::Outcome &o, const int32_t *basic, const double *xb) { on_done(idx[(size_t)i], o, basic, xb); };
        return be.run_roots(views.data(), nroots, g.root_of.data(), (int64_t)idx.size(), g.koff.data(), g.var.data(), g.sign.data(), g.rhs.data(), tol, od, out,
                            wa ? &wspec : nullptr);
    }
    // relaxations [lo, hi) of the caller's arrays as they are
    int run_range(BatchEngine &be, int64_t lo, int64_t hi, BatchEngine::Stats *out) {
        auto od = [this, lo](int64_t i, const BatchEngine::Outcome &o, const int32_t *basic, const double *xb) { on_done(i + lo, o, basic, xb); };
        return be.run_roots(views.data(), nroots, a.root_of ? a.root_of + lo : nullptr, hi - lo, a.koff + lo, a.var, a.sign, a.rhs, tol, od, out);
    }

    int run_one_gathered(const std::vector<int64_t> &cold_idx) {
        Group gc;
        BatchEngine::Stats bsc;
        gather(cold_idx, gc);
        const int rc = run_group(*pool->batch, cold_idx, gc, false, &bsc);
        merge_stats(bsc, true);
        return rc;
    }
    // two schedules side by side: the feasible starts (the long chains: the critical path of the wave) on the calling thread, where they
    // start without waiting for a thread to come up; the Phase-I starts on the auxiliary thread, which puts their lists together itself
    int run_phase_split(const gomilp::WavePlan::ColdCut &cut) {
        Group gf, gp;
        gather(cut.feasible, gf);
        BatchEngine &long_chains = pool->second_schedule(), &wide = *pool->batch;
        BatchEngine::Stats bsc, bs2;
        int rc = GOMILP_OK;
        wide.set_low_priority(true);   // the wide group yields to the long chains
        wide.set_loop_share(2); long_chains.set_loop_share(2);   // two schedules with persistent launches: half the loop slots each
        pool->aux.run([&] {
            hipSetDevice(pool->device);
            gather(cut.phase1, gp);
            rc = run_group(wide, cut.phase1, gp, false, &bsc);
        });
        const int rc2 = run_group(long_chains, cut.feasible, gf, false, &bs2);
        pool->aux.wait();
        wide.set_low_priority(false);
        wide.set_loop_share(1); long_chains.set_loop_share(1);
        merge_stats(bsc, true); merge_stats(bs2, false);
        return rc == GOMILP_OK ? rc2 : rc;
    }
    // two schedules, each with a contiguous half of the wave, each on its own stream and host thread, their block kernels on XCDs of
    // their own (BatchEngine::set_xcd_offset): one schedule's updates and control steps run under the other schedule's blocks
    int run_halves(int64_t half) {
        BatchEngine *be[2] = {pool->batch.get(), &pool->second_schedule()};
        const int64_t lo[3] = {0, half, a.count};
        BatchEngine::Stats bsx[2];
        int rcx[2] = {GOMILP_OK, GOMILP_OK};
        auto run_part = [&](int t) {
            hipSetDevice(pool->device);
            be[t]->set_xcd_offset(2 * t);
            rcx[t] = run_range(*be[t], lo[t], lo[t + 1], &bsx[t]);
            be[t]->set_xcd_offset(0);
        };
        pool->aux.run([&run_part] { run_part(1); });
        run_part(0);
        pool->aux.wait();
        bs = bsx[0];
        merge_stats(bsx[1], false);
        return rcx[0] == GOMILP_OK ? rcx[1] : rcx[0];
    }

    // warm starts first (the relaxations whose parent's final state is resident), then the cold part as WavePlan::cut_cold cuts it.
    // The caller drains the workers, after an error too.
    int run_tableau(const gomilp::WavePlan &plan) {
        tableau = true;
        std::vector<int64_t> cold_idx;
        if (wa) {
            std::vector<int64_t> warm_idx;
            std::vector<char> resident((size_t)a.count, 0);
            for (int64_t i = 0; i < a.count && wa->parent; i++)
                if (wa->parent[i] >= 0 && a.K(i) >= 1) { auto e = pool->warm.find(wa->parent[i]); resident[(size_t)i] = e && e->kind == gomilp::WK_TABLEAU; }
            plan.warm_groups(a, wa->parent, resident.data(), &warm_idx, &cold_idx);
            if (!warm_idx.empty()) {
                Group gw;
                gather(warm_idx, gw);
                const int rc = run_group(*pool->batch, warm_idx, gw, true, &bs);
                if (rc != GOMILP_OK) return rc;
                std::lock_guard<std::mutex> lk(agg_mu);
                for (int64_t i : cold_again) cold_idx.push_back(i);
                cold_again.clear();
                std::sort(cold_idx.begin(), cold_idx.end());
            }
        }
        const gomilp::WavePlan::ColdCut cut = plan.cut_cold(views.data(), nroots, a, cold_idx, pool->knobs);
        switch (cut.cut) {
            case gomilp::WavePlan::NONE: return GOMILP_OK;
            case gomilp::WavePlan::ONE: return run_range(*pool->batch, 0, a.count, &bs);
            case gomilp::WavePlan::ONE_GATHERED: return run_one_gathered(cold_idx);
            case gomilp::WavePlan::PHASE_SPLIT: return run_phase_split(cut);
            case gomilp::WavePlan::HALVES: return run_halves(cut.half);
        }
        return GOMILP_ERR_BAD_SHAPE;
    }

    void fold_stats(gomilp_frontier_stats *stats, Clock::time_point t0) const {
        *stats = agg;
        for (auto &S : ws) {
            stats->relaxations += S.relaxations; stats->pivots_phase1 += S.pivots_phase1; stats->pivots_phase2 += S.pivots_phase2;
            stats->bland_steps += S.bland_steps; stats->phase1_runs += S.phase1_runs; stats->kernel_launches += S.kernel_launches;
            stats->seconds_busy_sum += S.seconds_busy_sum;
        }
        stats->kernel_launches += bs.launches;
        stats->supersteps = bs.supersteps; stats->seconds_batch = bs.seconds_total;
        stats->blocks = bs.blocks; stats->blocks_sampled = bs.blocks_sampled;
        stats->seconds_inner_kernels = bs.seconds_inner; stats->seconds_update_kernels = bs.seconds_update;
        stats->warm_kept = bs.warm_kept;
        stats->workers = (int)pool->eng.size(); stats->device_id = pool->device;
        stats->seconds_total = busy_since(t0);
    }
};

}  // namespace

int gomilp::frontier_solve(gomilp_pool *pool, const WaveArgs &a, double tol, double *z_out, double *x_out, int64_t ldx, int32_t *status_out,
                           int32_t *has_x_out, gomilp_frontier_stats *stats, const WarmArgs *wa) {
    const int64_t count = a.count;
    if (!pool || count < 0 || !a.koff || !z_out || !x_out || !status_out || !has_x_out) return GOMILP_ERR_BAD_SHAPE;
    for (auto r : pool->root) if (r < 0) return GOMILP_ERR_BAD_SHAPE;
    std::lock_guard<std::mutex> call_guard(pool->call_mu);
    const auto t0 = Clock::now();
    Wave wave{pool, a, wa, tol, z_out, x_out, ldx, status_out, has_x_out};
    wave.nroots = 1 + (int)pool->extra_root.size();
    wave.views.resize((size_t)wave.nroots);
    wave.views[0] = &pool->view;
    for (int r = 1; r < wave.nroots; r++) wave.views[(size_t)r] = pool->extra_view[(size_t)r - 1].get();
    for (int64_t i = 0; i < count; i++) {
        const int ri = a.root(i);
        if (ri < 0 || ri >= wave.nroots || wave.views[(size_t)ri]->n > ldx) return GOMILP_ERR_BAD_SHAPE;
    }
    wave.ws.assign(pool->eng.size(), gomilp_frontier_stats());
    for (int64_t i = 0; i < count; i++) { z_out[i] = NAN; has_x_out[i] = 0; status_out[i] = GOMILP_ERR_DEVICE; }

    const WavePlan plan = WavePlan::make(wave.views.data(), wave.nroots, a, wa != nullptr, pool->knobs);
    WavePlan::Route route = plan.route;
    if (route == WavePlan::REVISED) {
        bool fits = true;
        const int rc = wave.run_revised(&fits);
        pool->drain();
        if (rc != GOMILP_OK) return rc;
        if (!fits) route = WavePlan::WORKERS;
    }
    if (route == WavePlan::TABLEAU) {
        const int rc = wave.run_tableau(plan);
        pool->drain();
        if (rc != GOMILP_OK) return rc;
    } else if (route == WavePlan::WORKERS) {
        wave.run_workers();
        pool->drain();
    }
    if (stats) wave.fold_stats(stats, t0);
    return GOMILP_OK;
}
