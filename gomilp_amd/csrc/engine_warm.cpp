// Single-context warm start (gomilp_lp_solve_warm): a solved problem keeps its final basis and an explicit B^-1;
// a descendant starts from that basis + the slacks of its J new branch rows — dual feasible, primal infeasible at most in those rows —
// and a dual simplex on the revised-simplex kernels (dual_kernels.hip + k_ftran / k_update) repairs it.  The primal Phase-II loop
// and the epilogue of a cold solve finish the job (engine.cpp solve_tail).
#include "engine_work.hpp"

namespace gomilp {

namespace {
constexpr int kWarmBudgetSpent = -4;   // warm_locked: the dual-pivot budget ran out (the caller solves cold: fallback 4)
constexpr int kWarmNoPath = -5;        // warm_locked: this shape has no warm path here (fallback 5)
constexpr int kDefaultDualBudget = 64;
constexpr size_t kKeepPoolMax = 8;
// the dual loop stops when min x_B >= -kDualFeasTol: the primal feasibility tolerance of the reference's starting-basis test
// (simplex.go:459-469), as the pool's dual kernel (batch_kernels.hip) — with the caller's tol (GoMILP passes 0) a rounding-level
// negative x_B of a row without a negative alpha would be reported as an infeasible LP
constexpr double kDualFeasTol = 1e-13;
}  // namespace

void Engine::drop_kept(int64_t id) {
    auto it = kept_.find(id);
    if (it == kept_.end()) return;
    if (it->second.d) keep_pool_.emplace_back(it->second.d, it->second.cap);
    kept_.erase(it);
    while (keep_pool_.size() > kKeepPoolMax) {   // (rare: more released states than nodes alive at once)
        hipFree(keep_pool_.front().first);
        keep_pool_.erase(keep_pool_.begin());
    }
}

// At the end of a solve that keeps its state (loop status OK): B^-1 of the final basis into a buffer of its own.
//   revised pipelines (0, 1): the current ping-pong copy, device to device;
//   tableau pipelines (2, 3) on a slack-basis start: gathered from T = B^-1 A_N — column r of B^-1 is B^-1 a_s for the unit column s of
//   row r (the slack of the start): T's column of s when s is nonbasic, e_p when s is basic at position p.  T[tcur_] is fully updated
//   here: the blocked loop applies every block's rank-K terms before it returns (the same state cond_check reads).
//   A general start (no rho_slack) on the tableau or on the guarded revised loop keeps no B^-1: its children run cold (warm starts
//   from such parents: not built).  (A warm solve's own state comes without rho_slack too, and is kept from B^-1 as above.)
void Engine::keep_capture(const Problem &P, int64_t id, int pipeline, const std::vector<int32_t> &basic,
                          const std::vector<int32_t> &basic_start, const std::vector<int32_t> *rho_slack) {
    Work &w = *w_;
    const int m = P.m, n = P.n;
    Kept k;
    k.m = m; k.ld = P.ld; k.basic = basic;
    const bool tab = pipeline >= 2;
    if (!rho_slack && (tab || plan_.gen_revised)) { k.no_warm = true; kept_[id] = std::move(k); return; }
    const size_t need = (size_t)m * P.ld;
    for (size_t i = 0; i < keep_pool_.size(); i++)
        if (keep_pool_[i].second >= need) {
            k.d = keep_pool_[i].first; k.cap = keep_pool_[i].second;
            keep_pool_.erase(keep_pool_.begin() + i);
            break;
        }
    if (!k.d) {
        if (!device_fits(need * sizeof(double)) || dmalloc(&k.d, need) != hipSuccess) { k.d = nullptr; return; }   // not kept
        k.cap = need;
    }
    bool ok = true;
    if (!tab) {
        ok = hipMemcpyAsync(k.d, w.binv[cur_], need * sizeof(double), hipMemcpyDeviceToDevice, stream_) == hipSuccess;
    } else {
        const int nn = n - m;
        std::vector<int32_t> where(n, 0), src(m);
        ok = hipMemcpyAsync(w.h_idx, w.nonbasic, (size_t)nn * sizeof(int32_t), hipMemcpyDeviceToHost, stream_) == hipSuccess &&
             sync_stream() == hipSuccess;
        if (ok) {
            for (int p = 0; p < m; p++) where[basic[p]] = -1 - p;
            for (int jp = 0; jp < nn; jp++) where[w.h_idx[jp]] = jp;
            for (int pos = 0; pos < m; pos++) src[(*rho_slack)[pos]] = where[basic_start[pos]];
            ok = stage_upload(w.rho, src.data(), (size_t)m * sizeof(int32_t)) == GOMILP_OK;
        }
        if (ok) {
            launch_tab_to_binv(w.T[tcur_], ldt_, t_tiled_, m, w.rho, k.d, P.ld, stream_);
            launches_++;
        }
    }
    if (!ok) { keep_pool_.emplace_back(k.d, k.cap); return; }
    kept_[id] = std::move(k);
}

// J >= 1 new rows of P beyond the problem `parent` (see gomilp_lp_solve_warm)
bool Engine::descendant(const Problem &P, int64_t parent, int *J) const {
    const Problem &Q = *problems_[parent];
    *J = 0;
    if (!P.is_child || !P.root_ptr) return false;
    const int Kc = (int)P.kvar.size();
    if (P.root == parent && P.root_ptr == &Q) { *J = Kc; return Kc >= 1; }
    if (!Q.is_child || P.root < 0 || P.root != Q.root || P.root_ptr != Q.root_ptr) return false;
    const int Kp = (int)Q.kvar.size();
    if (Kc <= Kp) return false;
    const int m0 = P.m - Kc;
    for (int k = 0; k < Kp; k++)
        if (P.kvar[k] != Q.kvar[k] || memcmp(&P.ksign[k], &Q.ksign[k], sizeof(double)) != 0 ||
            memcmp(&P.hb[(size_t)m0 + k], &Q.hb[(size_t)m0 + k], sizeof(double)) != 0)
            return false;
    *J = Kc - Kp;
    return true;
}

int Engine::solve_warm(int64_t id, int64_t parent, int keep, int dual_budget, double tol, double *opt_f, double *opt_x, int32_t *has_x,
                       int64_t *basis_out, gomilp_lp_stats *stats, gomilp_warm_stats *wstats) {
    std::lock_guard<std::mutex> g(mu_);
    gomilp_warm_stats wlocal;
    gomilp_warm_stats *ws = wstats ? wstats : &wlocal;
    memset(ws, 0, sizeof(*ws));
    gomilp_lp_stats slocal;
    gomilp_lp_stats *st = stats ? stats : &slocal;
    const bool valid = id >= 0 && (size_t)id < problems_.size() && problems_[id];
    if (valid) drop_kept(id);
    keep_id_ = keep ? id : -1;
    int fb = 0, J = 0;
    const Kept *K = nullptr;
    if (!valid || !opt_f || !opt_x || !has_x) fb = 1;   // (the cold solve reports the bad call)
    else if (parent < 0) fb = 1;
    else if ((size_t)parent >= problems_.size() || !problems_[parent] || !kept_.count(parent)) fb = 2;
    else if (!descendant(*problems_[id], parent, &J)) fb = 3;
    else {
        K = &kept_.at(parent);
        const Problem &P = *problems_[id];
        if (K->no_warm || knobs_.exact_degenerate == 3 || P.verify_status != GOMILP_OK || P.m >= P.n) fb = 5;
        else if (!K->d) fb = 2;
    }
    ws->new_rows = J;
    int rc = GOMILP_OK;
    if (!fb) {
        rc = warm_locked(id, *K, J, dual_budget > 0 ? dual_budget : kDefaultDualBudget, tol, opt_f, opt_x, has_x, basis_out, st, ws);
        if (rc == kWarmBudgetSpent) fb = 4;
        else if (rc == kWarmNoPath) fb = 5;
        else ws->warm_started = 1;
    }
    if (fb) {
        if (valid) drop_kept(id);   // (a warm attempt that gave up kept nothing)
        rc = solve_cold_locked(id, tol, nullptr, opt_f, opt_x, has_x, basis_out, stats);
    }
    ws->fallback = fb;
    keep_id_ = -1;
    if (valid) {
        auto it = kept_.find(id);
        if (it != kept_.end() && rc != GOMILP_OK) { drop_kept(id); it = kept_.end(); }
        if (it != kept_.end() && it->second.d) { ws->kept = 1; ws->keep_bytes = (int64_t)((size_t)it->second.m * it->second.ld * sizeof(double)); }
    }
    return rc;
}

// The warm path proper.  Returns a status, kWarmBudgetSpent or kWarmNoPath (nothing returned to the caller yet in those two cases).
int Engine::warm_locked(int64_t id, const Kept &K, int J, int dual_budget, double tol, double *opt_f, double *opt_x, int32_t *has_x,
                        int64_t *basis_out, gomilp_lp_stats *st, gomilp_warm_stats *ws) {
    const double t0 = now_s();
    memset(st, 0, sizeof(*st));
    st->device_id = device_;
    *has_x = 0;
    *opt_f = std::numeric_limits<double>::quiet_NaN();
    const Problem &P = *problems_[id];
    st->seconds_upload = P.seconds_upload;
    auto finish = [&](int code) { return close_stats(st, t0, code); };
    open_stats();
    const int m = P.m, n = P.n, mp = K.m, Kc = (int)P.kvar.size();
    if (mp + J != m || (int)K.basic.size() != mp) return kWarmNoPath;
    if (P.ld > kLdsWindowLd && !large_solve_fits(P)) return kWarmNoPath;
    int rc = ensure_work(m, n + 1);
    if (rc != GOMILP_OK) return finish(rc);
    Work &w = *w_;
    w.st_host->trace_len = 0;
    plan_ = SolvePlan::warm(P.ld, P.scale_span, knobs_);
    gen_binv_dev_ = false; shadow_trace_ = false;
    // ---- start: the parent's positions, then the slacks of the J new rows (the last J columns of the problem)
    std::vector<int32_t> basic(K.basic), posof(n, -1);
    for (int p = 0; p < mp; p++) posof[K.basic[p]] = p;
    std::vector<int32_t> kpos(J);
    std::vector<double> ksg(J);
    for (int k = 0; k < J; k++) {
        basic.push_back(n - J + k);
        kpos[k] = posof[P.kvar[Kc - J + k]];
        ksg[k] = P.ksign[Kc - J + k];
    }
    std::vector<int32_t> nonbasic;
    build_nonbasic(basic, n, nonbasic);
    const int nn = (int)nonbasic.size();
    if ((rc = stage_upload(w.rho, kpos.data(), (size_t)J * sizeof(int32_t))) != GOMILP_OK) return finish(rc);
    if ((rc = stage_upload(w.move, ksg.data(), (size_t)J * sizeof(double))) != GOMILP_OK) return finish(rc);
    cur_ = 0; ycur_ = 0;
    launch_warm_binv(K.d, K.ld, mp, w.binv[0], P.ld, m, w.rho, w.move, stream_);
    HIP_TRY(hipMemsetAsync(w.yb[0], 0, (size_t)P.ld * sizeof(double), stream_));
    HIP_TRY(hipMemsetAsync(w.yb[1], 0, (size_t)P.ld * sizeof(double), stream_));
    launches_++;
    if ((rc = upload_index_lists(basic, nonbasic)) != GOMILP_OK) return finish(rc);
    refresh_xb_y(P, P.dc);   // x_B = B^-1 b, y = B^-T c_B (= the parent's y, zeros appended)
    HIP_TRY(sync_stream());
    ws->seconds_setup = now_s() - t0;
    // ---- dual loop
    st->pipeline = plan_.pipeline;
    rc = run_dual_loop(P, kDualFeasTol, nn, dual_budget, ws);
    if (rc == kWarmBudgetSpent) return rc;
    if (rc != GOMILP_OK) return finish(rc);   // GOMILP_ERR_INFEASIBLE (no x), or a device failure
    // ---- Phase II from the dual loop's basis (nonbasic list in ascending order again, fresh x_B / y), then the cold epilogue
    HIP_TRY(hipMemcpyAsync(w.h_idx, w.basic, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(sync_stream());
    for (int i = 0; i < m; i++) basic[i] = w.h_idx[i];
    build_nonbasic(basic, n, nonbasic);
    if ((rc = upload_index_lists(basic, nonbasic)) != GOMILP_OK) return finish(rc);
    refresh_xb_y(P, P.dc);
    const int loop_rc = run_loop(P, 2, tol, nn, P.dc, st);
    std::vector<double> xb(m, 0.0);
    rc = solve_tail(P, id, loop_rc, basic, xb, basic, nullptr, opt_f, opt_x, has_x, basis_out, st);
    return finish(rc);
}

// Dual simplex on the revised-simplex kernels, chunks of pivots enqueued with one state read per chunk (as run_loop).  Each pivot:
// k_dual_leave -> k_dual_price -> k_ftran (entering from the dual partials) -> k_update (leaving row from the state).
// Returns GOMILP_OK (primal feasible), GOMILP_ERR_INFEASIBLE, kWarmBudgetSpent or GOMILP_ERR_DEVICE.
int Engine::run_dual_loop(const Problem &P, double tol, int nn, int dual_budget, gomilp_warm_stats *ws) {
    Work &w = *w_;
    DevState &hs = *w.st_host;
    hs.done = 0; hs.status = ST_RUNNING; hs.pivots = 0; hs.q = hs.p = -1; hs.rq = hs.dp = hs.mv = 0;
    hs.max_pivots = dual_budget;
    hs.lu_singular = 0;
    sync_state_to_device();
    HIP_TRY(hipEventRecord(w.ev[0], stream_));
    int ret = GOMILP_OK;
    for (;;) {
        const int64_t before = hs.pivots;
        // children usually need a handful of dual pivots: a short first chunk (no-op launches behind the end cost a launch each);
        // never more than the budget + 1 (the launch that sees the budget spent)
        const int64_t nt = std::min<int64_t>(before == 0 ? 4 : bt_knobs_.chunk, dual_budget - before + 1);
        for (int64_t t = 0; t < nt; t++) {
            LPArgs a = make_args(P, 3, tol, nn, P.dc);
            a.binv_cur = w.binv[(cur_ + t) & 1];
            a.binv_next = w.binv[(cur_ + t + 1) & 1];
            launch_dual_leave(w.xb, P.m, tol, w.st, stream_);
            const int gp = launch_dual_price(a, stream_);
            const int gr = launch_ftran(a, gp, kDualPick, -1, stream_);
            launch_update(a, gr, kDualPick, 0, 0, stream_);
            launches_ += 4;
        }
        HIP_TRY(hipMemcpyAsync(w.st_host, w.st, sizeof(DevState), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(sync_stream());
        HIP_TRY(hipGetLastError());
        cur_ = (int)((cur_ + (hs.pivots - before)) & 1);
        if (!hs.done) continue;
        if (hs.status == ST_OPTIMAL) ret = GOMILP_OK;                    // x_B >= -tol: primal feasible
        else if (hs.status == ST_DUAL_INFEASIBLE) ret = GOMILP_ERR_INFEASIBLE;
        else if (hs.status == ST_MAX_PIVOTS) ret = kWarmBudgetSpent;
        else ret = GOMILP_ERR_DEVICE;
        break;
    }
    HIP_TRY(hipEventRecord(w.ev[1], stream_));
    HIP_TRY(hipEventSynchronize(w.ev[1]));
    float ms = 0;
    hipEventElapsedTime(&ms, w.ev[0], w.ev[1]);
    ws->seconds_dual = ms * 1e-3;
    ws->pivots_dual = hs.pivots;
    return ret;
}

}  // namespace gomilp
