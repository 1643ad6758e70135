// extern "C" surface declared in include/gomilp_lp.h.  Each entry point names the reference
// interface it replaces; see INTEGRATION.md for the cgo binding.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "engine.hpp"
#include "frontier_pool.hpp"
#include "lu_host.h"

using gomilp::BatchEngine;
using gomilp::Engine;

struct gomilp_ctx {
    std::unique_ptr<Engine> eng;
};

#ifdef GOMILP_DEBUG
namespace gomilp { void luc_stamps_read(unsigned long long *out); void res_stamps_read(unsigned long long *out); void lux_stamps_read(unsigned long long *out); }
#endif

extern "C" {

const char *gomilp_version(void) { return "gomilp_amd 0.1 (gfx950)"; }
int gomilp_device_count(void) { return gomilp::device_count(); }
const char *gomilp_compiled_arch(void) { return gomilp::compiled_arch(); }

gomilp_ctx *gomilp_ctx_create(int device, int *status) {
    int n = gomilp::device_count();
    if (n <= 0) { if (status) *status = GOMILP_ERR_DEVICE; return nullptr; }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    if (device >= n) { if (status) *status = GOMILP_ERR_DEVICE; return nullptr; }
    gomilp_ctx *c = new gomilp_ctx;
    c->eng.reset(new Engine(device));
    if (status) *status = GOMILP_OK;
    return c;
}
void gomilp_ctx_destroy(gomilp_ctx *ctx) { delete ctx; }
int gomilp_ctx_device(const gomilp_ctx *ctx) { return ctx ? ctx->eng->device() : -1; }
int gomilp_ctx_set(gomilp_ctx *ctx, const char *key, int64_t value) {
    if (!ctx || !key) return GOMILP_ERR_BAD_SHAPE;
    return ctx->eng->set(key, value);
}
int64_t gomilp_lp_upload(gomilp_ctx *ctx, const double *c, const double *A, int64_t lda, const double *b, int64_t m,
                         int64_t n) {
    if (!ctx) return -GOMILP_ERR_BAD_SHAPE;
    return ctx->eng->upload(c, A, lda, b, m, n);
}
int gomilp_lp_free(gomilp_ctx *ctx, int64_t problem) {
    if (!ctx) return GOMILP_ERR_BAD_SHAPE;
    return ctx->eng->free_problem(problem);
}
int gomilp_lp_solve_resident(gomilp_ctx *ctx, int64_t problem, double tol, const int64_t *initial_basic, double *opt_f,
                             double *opt_x, int32_t *has_x, int64_t *basis_out, gomilp_lp_stats *stats) {
    if (!ctx) return GOMILP_ERR_BAD_SHAPE;
    return ctx->eng->solve(problem, tol, initial_basic, opt_f, opt_x, has_x, basis_out, stats);
}
int gomilp_lp_solve_warm(gomilp_ctx *ctx, int64_t problem, int64_t parent, int32_t keep, int32_t dual_budget, double tol,
                         double *opt_f, double *opt_x, int32_t *has_x, int64_t *basis_out, gomilp_lp_stats *stats,
                         gomilp_warm_stats *wstats) {
    if (!ctx) return GOMILP_ERR_BAD_SHAPE;
    return ctx->eng->solve_warm(problem, parent, keep, dual_budget, tol, opt_f, opt_x, has_x, basis_out, stats, wstats);
}
int64_t gomilp_lp_upload_child(gomilp_ctx *ctx, int64_t root_problem, int32_t K, const int32_t *var, const double *sign,
                               const double *rhs) {
    if (!ctx) return -GOMILP_ERR_BAD_SHAPE;
    return ctx->eng->upload_child(root_problem, K, var, sign, rhs);
}

gomilp_pool *gomilp_pool_create(int device, int workers, int *status) {
    int n = gomilp::device_count();
    if (n <= 0) { if (status) *status = GOMILP_ERR_DEVICE; return nullptr; }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    if (device >= n || workers < 1 || workers > 64) { if (status) *status = device >= n ? GOMILP_ERR_DEVICE : GOMILP_ERR_BAD_SHAPE; return nullptr; }
    gomilp_pool *p = new gomilp_pool;
    p->device = device;
    for (int w = 0; w < workers; w++) {
        p->eng.emplace_back(new Engine(device));
        p->root.push_back(-1);
        // the workers finish the relaxations of a wave side by side, next to the batched schedule's own persistent launches: their final
        // solves keep the LU schedule that waits for nobody (lu_compressed.hip: look-ahead launches wait for their own workgroups)
        p->eng.back()->set("lu_look", 0);
        // ... and for the same reason never the eight-workgroup LU panel of the bases beyond 4096 rows (knob lu_large: every such panel wants
        // 8 CUs of one XCD with nearly all of their LDS; side by side they would hold each other off until the bounded polls give up)
        p->eng.back()->set("lu_large", 0);
        // pools (frontier waves, batched schedules, warm starts) keep the row limit of one-pass LDS staging: roots and children
        // beyond 8192 rows are refused as GOMILP_ERR_UNSUPPORTED — until the pool knob large_rows lifts it (gomilp_pool_set)
        p->eng.back()->limit_rows_to_lds_window();
    }
    p->batch.reset(new BatchEngine(device));
    for (int w = 0; w < workers; w++) p->threads.emplace_back([p, w] { p->worker(w); });
    if (status) *status = GOMILP_OK;
    return p;
}
void gomilp_pool_destroy(gomilp_pool *pool) { delete pool; }

int gomilp_pool_set(gomilp_pool *pool, const char *key, int64_t value) {
    if (!pool || !key) return GOMILP_ERR_BAD_SHAPE;
    std::lock_guard<std::mutex> g(pool->call_mu);
    using Scope = gomilp::PoolKnobs::Scope;
    const Scope sc = gomilp::PoolKnobs::scope(key);
    if (std::string(key) == "large_rows") {
        // the workers take what a context takes beyond the LDS window, or keep the window; a pool that holds a root beyond it keeps the knob
        if (!value) {
            bool beyond = pool->root[0] >= 0 && pool->view.ld > gomilp::kLdsWindowLd;
            for (auto &v : pool->extra_view) beyond = beyond || v->ld > gomilp::kLdsWindowLd;
            if (beyond) return GOMILP_ERR_BAD_SHAPE;
        }
        for (auto &e : pool->eng) e->limit_rows_to_lds_window(value == 0);
    }
    if (sc == Scope::Pool || sc == Scope::PoolAndWorkers) {
        if (!pool->knobs.set(key, value)) return GOMILP_ERR_BAD_SHAPE;   // (a value the knob refuses: a negative rev_mem_limit)
        pool->apply_knobs(*pool->batch);
        if (pool->batch2) pool->apply_knobs(*pool->batch2);
        if (sc == Scope::Pool) return GOMILP_OK;
    }
    int rc = GOMILP_OK;
    for (auto &e : pool->eng) { const int r = e->set(key, value); if (r != GOMILP_OK) rc = r; }
    if (rc == GOMILP_OK && sc == Scope::WorkersFirst) pool->knobs.set(key, value);
    return rc;
}

int gomilp_pool_set_root(gomilp_pool *pool, const double *c0, const double *A0, int64_t lda, const double *b0, int64_t m0,
                         int64_t n0) {
    if (!pool) return GOMILP_ERR_BAD_SHAPE;
    std::lock_guard<std::mutex> g(pool->call_mu);
    for (auto id : pool->extra_root) pool->eng[0]->free_problem(id);
    pool->extra_root.clear(); pool->extra_view.clear();
    pool->warm.clear();
    if (pool->rev) pool->rev->release();
    for (size_t w = 0; w < pool->eng.size(); w++) {
        if (pool->root[w] >= 0) pool->eng[w]->free_problem(pool->root[w]);
        int64_t id = pool->eng[w]->upload(c0, A0, lda, b0, m0, n0);
        if (id < 0) { pool->root[w] = -1; return (int)-id; }
        pool->root[w] = id;
    }
    pool->m0 = m0; pool->n0 = n0;
    if (!pool->eng[0]->root_view(pool->root[0], &pool->view)) return GOMILP_ERR_DEVICE;
    // (knob large_rows) beyond the LDS window only slack-basis roots, as on a context: the general start's search stages m-long rows
    if (pool->view.ld > gomilp::kLdsWindowLd && !pool->view.unit_basis && pool->view.verify_status == GOMILP_OK) {
        for (size_t w = 0; w < pool->eng.size(); w++) { pool->eng[w]->free_problem(pool->root[w]); pool->root[w] = -1; }
        return GOMILP_ERR_UNSUPPORTED;
    }
    if (!pool->view.unit_basis && pool->view.verify_status == GOMILP_OK) pool->eng[0]->root_general(pool->root[0], &pool->view);   // equality rows: one column search per root
    // first-touch allocations of every worker (work buffers, child slot, final-solve workspace) happen here, not inside the
    // first waves: each worker finishes one dummy child (8 slack rows x_0 <= 1e30) from its slack basis
    if (pool->view.unit_basis && pool->view.verify_status == GOMILP_OK) {
        const int W = (int)pool->eng.size(), K = 8;
        std::atomic<int> started(0);
        for (int t = 0; t < W; t++)
            pool->submit([pool, W, K, &started](int w) {
                started.fetch_add(1);
                while (started.load() < W) std::this_thread::yield();   // every worker takes exactly one of the W tasks
                Engine &E = *pool->eng[w];
                std::vector<int32_t> var(K, 0);
                std::vector<double> sign(K, 1.0), rhs(K, 1e30);
                const int64_t id = E.upload_child(pool->root[w], K, var.data(), sign.data(), rhs.data());
                if (id < 0) return;
                const int m = pool->view.m + K, n = pool->view.n + K;
                std::vector<int32_t> basic(m);
                for (int pos = 0; pos < m; pos++) basic[pos] = n - 1 - pos;
                std::vector<double> xb(m, 0.0), x(n, 0.0);
                double z = 0; int32_t hx = 0;
                E.finish_from_basis(id, basic.data(), xb.data(), GOMILP_OK, &z, x.data(), &hx, nullptr, nullptr);
                E.free_problem(id);
            });
        pool->drain();
    }
    return GOMILP_OK;
}

int gomilp_frontier_solve_roots(gomilp_pool *pool, int64_t count, const int32_t *root_of, const int64_t *koff, const int32_t *var,
                                const double *sign, const double *rhs, double tol, double *z_out, double *x_out, int64_t ldx,
                                int32_t *status_out, int32_t *has_x_out, gomilp_frontier_stats *stats) {
    return gomilp::frontier_solve(pool, gomilp::WaveArgs{count, root_of, koff, var, sign, rhs}, tol, z_out, x_out, ldx, status_out, has_x_out, stats, nullptr);
}

int gomilp_frontier_solve_warm(gomilp_pool *pool, int64_t count, const int64_t *koff, const int32_t *var, const double *sign,
                               const double *rhs, const int64_t *parent, const int64_t *tag, const int32_t *keep, int32_t dual_budget,
                               double tol, double *z_out, double *x_out, int32_t *status_out, int32_t *has_x_out,
                               gomilp_frontier_stats *stats) {
    if (!pool) return GOMILP_ERR_BAD_SHAPE;
    gomilp::WarmArgs wa{parent, tag, keep, dual_budget};
    return gomilp::frontier_solve(pool, gomilp::WaveArgs{count, nullptr, koff, var, sign, rhs}, tol, z_out, x_out, pool->n0, status_out, has_x_out, stats, &wa);
}

int gomilp_pool_release_warm(gomilp_pool *pool, int64_t tag) {
    if (!pool) return GOMILP_ERR_BAD_SHAPE;
    // (behind the pool's call lock like every other entry point: an entry released while a warm wave runs would go back to the free list and
    // could be recycled by that wave's own harvest — the copy of a kept child into it would overwrite a parent tableau the wave still reads)
    std::lock_guard<std::mutex> g(pool->call_mu);
    if (tag < 0) pool->warm.clear(); else pool->warm.release(tag);
    return GOMILP_OK;
}

int gomilp_frontier_solve(gomilp_pool *pool, int64_t count, const int64_t *koff, const int32_t *var, const double *sign,
                          const double *rhs, double tol, double *z_out, double *x_out, int32_t *status_out,
                          int32_t *has_x_out, gomilp_frontier_stats *stats) {
    if (!pool) return GOMILP_ERR_BAD_SHAPE;
    return gomilp_frontier_solve_roots(pool, count, nullptr, koff, var, sign, rhs, tol, z_out, x_out, pool->n0, status_out, has_x_out, stats);
}

// The root relaxation (subproblem.go:172) on the pool's first worker.
int gomilp_pool_solve_root(gomilp_pool *pool, double tol, double *opt_f, double *opt_x, int32_t *has_x, gomilp_lp_stats *stats) {
    if (!pool || pool->root[0] < 0) return GOMILP_ERR_BAD_SHAPE;
    std::lock_guard<std::mutex> g(pool->call_mu);
    return pool->eng[0]->solve(pool->root[0], tol, nullptr, opt_f, opt_x, has_x, nullptr, stats);
}

int gomilp_pool_add_root(gomilp_pool *pool, const double *c, const double *A, int64_t lda, const double *b, int64_t m, int64_t n) {
    if (!pool) return -GOMILP_ERR_BAD_SHAPE;
    std::lock_guard<std::mutex> g(pool->call_mu);
    if (pool->root[0] < 0) return -GOMILP_ERR_BAD_SHAPE;   // gomilp_pool_set_root first
    const int64_t id = pool->eng[0]->upload(c, A, lda, b, m, n);
    if (id < 0) return (int)id;
    std::unique_ptr<Engine::RootView> v(new Engine::RootView);
    if (!pool->eng[0]->root_view(id, v.get())) return -GOMILP_ERR_DEVICE;
    if (v->ld > gomilp::kLdsWindowLd && !v->unit_basis && v->verify_status == GOMILP_OK) {
        pool->eng[0]->free_problem(id);
        return -GOMILP_ERR_UNSUPPORTED;
    }
    if (!v->unit_basis && v->verify_status == GOMILP_OK) pool->eng[0]->root_general(id, v.get());
    pool->extra_root.push_back(id);
    pool->extra_view.push_back(std::move(v));
    return (int)pool->extra_root.size();
}

// diagnostic (host only, no device): the column search of findLinearlyIndependent as the engine performs it for non-slack
// starting bases; fast = 1: incremental QR (O(m^2 n)), 0: a fresh exact condition number per candidate (O(m^4))
int64_t gomilp_debug_find_independent(const double *A, int64_t lda, int64_t m, int64_t n, int64_t *idx_out, int fast) {
    if (!A || !idx_out || m <= 0 || n <= 0 || lda < n || m > 4096 || n > (1 << 20)) return -GOMILP_ERR_BAD_SHAPE;
    std::vector<double> a((size_t)m * n);
    for (int64_t i = 0; i < m; i++) for (int64_t j = 0; j < n; j++) a[(size_t)i * n + j] = A[i * lda + j];
    std::vector<int32_t> idx;
    if (fast) gomilp::general_find_linearly_independent(a, (int)m, (int)n, idx);
    else gomilp::general_find_linearly_independent_slow(a, (int)m, (int)n, idx);
    for (size_t k = 0; k < idx.size(); k++) idx_out[k] = idx[k];
    return (int64_t)idx.size();
}

// diagnostic (host only): the condition-number estimate the engine takes its mat.Condition verdict on beyond the exact screen
// (Engine::cond_check): |B|_1 times the Hager / Higham estimate of |B^-1|_1 (inf = 0; gonum: the duals' solve with ab^T), or
// |B|_inf times the estimate of |B^-1|_inf (inf = 1: the solves with ab).  -1: singular to working precision.
double gomilp_debug_cond_estimate(const double *B, int64_t n, int inf) {
    if (!B || n <= 0 || n > 4096) return -1.0;
    std::vector<double> b((size_t)n * n), inv;
    for (int64_t i = 0; i < n * n; i++) b[(size_t)i] = B[i];
    if (!gomilp::general_invert(b, (int)n, inv)) return -1.0;
    double norm = 0;
    if (!inf) { for (int64_t j = 0; j < n; j++) { double s2 = 0; for (int64_t i = 0; i < n; i++) s2 += fabs(b[(size_t)(i * n + j)]); norm = std::max(norm, s2); } }
    else { for (int64_t i = 0; i < n; i++) { double s2 = 0; for (int64_t j = 0; j < n; j++) s2 += fabs(b[(size_t)(i * n + j)]); norm = std::max(norm, s2); } }
    return norm * gomilp::inverse_norm1_estimate(inv, (int)n, inf != 0);
}

// diagnostic: the same search with the scan on the device (general_kernels.hip), on a problem resident in `ctx`
int gomilp_debug_gonum_lu_cond(const double *M, int64_t n, int transposed, double *cond) {
    if (!M || !cond || n < 1 || n > gomilp::kGonumCondMax) return -1;
    bool dz = false;
    if (!gomilp::gonum_lu_cond(M, (int)n, (int)n, transposed != 0, cond, &dz)) return -1;
    return dz ? 1 : 0;
}

int gomilp_debug_lu_host_solve(int64_t m, int64_t nd, const int32_t *dl, const int32_t *phys, const double *diag, const double *W, int coupled,
                               const double *rhs, double *x) {
    if (m < 1 || m > 16384 || nd < 0 || nd > m || !phys || !diag || !rhs || !x || (nd > 0 && (!dl || !W))) return -1;
    const int64_t nx = coupled ? nd : m;
    for (int64_t i = 0; i < nx; i++) x[i] = 0.0;
    if (gomilp::lu_det_is_zero(diag, phys, (int)m)) return 1;   // (Engine::lu_solve gives zeros as well)
    if (coupled) {
        std::vector<double> xdl((size_t)nd);
        gomilp::lu_host_solve_coupled((int)nd, dl, phys, diag, W, rhs, xdl.data(), x);
    } else gomilp::lu_host_solve((int)m, (int)nd, dl, phys, diag, W, rhs, x);
    return 0;
}

int gomilp_debug_bt_plan(int64_t m, int64_t ldt, int64_t nknobs, const char *const *keys, const int64_t *values, int64_t ncu, int64_t *out) {
    if (m < 1 || ldt < 1 || m > (1 << 20) || ldt > (1 << 22) || nknobs < 0 || (nknobs > 0 && (!keys || !values)) || !out) return -GOMILP_ERR_BAD_SHAPE;
    gomilp::BtKnobs knobs;
    for (int64_t i = 0; i < nknobs; i++) {
        const int rc = keys[i] ? knobs.set(keys[i], values[i]) : -1;
        if (rc != GOMILP_OK) return -GOMILP_ERR_BAD_SHAPE;   // (a key that is none of the plan's knobs included)
    }
    const gomilp::BtPlan p = gomilp::BtPlan::make((int)m, (int)ldt, knobs);
    const gomilp::BtLoopShape sh = gomilp::bt_loop_shape(p.loop), rep = gomilp::bt_loop_shape(p.rep);
    const int64_t f[GOMILP_BT_PLAN_FIELDS] = {
        p.pipeline, p.K, p.tiled, p.tiled_forced, p.cfg.groups, p.cfg.nt, p.cfg.ri, p.blocks_per_chunk,
        (int64_t)p.loop, sh.groups, sh.nt, sh.kb, sh.wave_rec, sh.stamped, sh.min_grid, p.is_loop() ? p.slot_weight : 0, p.upd_cap,
        p.is_loop() ? p.grid((int)ncu, p.loop) : 0,
        (int64_t)p.rep, rep.nt, rep.stamped, p.rep_upd_cap, p.rep != gomilp::BtLoop::None ? p.grid((int)ncu, p.rep) : 0};
    for (int i = 0; i < GOMILP_BT_PLAN_FIELDS; i++) out[i] = f[i];
    return GOMILP_BT_PLAN_FIELDS;
}

int gomilp_debug_solve_plan(int64_t m, int64_t n, int32_t start, double scale_span, int64_t nknobs, const char *const *keys, const int64_t *values, double *out) {
    if (m < 1 || n <= m || n > (1 << 24) || start < 0 || start > 2 || nknobs < 0 || (nknobs > 0 && (!keys || !values)) || !out) return -GOMILP_ERR_BAD_SHAPE;
    gomilp::SolveKnobs knobs;
    for (int64_t i = 0; i < nknobs; i++) {
        const int rc = keys[i] ? knobs.set(keys[i], values[i]) : -1;
        if (rc != GOMILP_OK) return -GOMILP_ERR_BAD_SHAPE;   // (a key that is none of the plan's knobs included)
    }
    const gomilp::SolvePlan p = gomilp::SolvePlan::make((int)m, (int)n, (int)((m + 1) & ~(int64_t)1), (gomilp::SolvePlan::StartKind)start, scale_span, knobs);
    const double f[GOMILP_SOLVE_PLAN_FIELDS] = {(double)p.status, (double)p.pipeline, (double)p.use_tab, (double)p.blocked, (double)p.gen_start, (double)p.gen_revised,
                                                (double)p.badly_scaled, p.guard, p.cguard, (double)p.replay_if_feasible, (double)p.search_on_device,
                                                (double)p.art_on_device, (double)p.needs_host_A};
    for (int i = 0; i < GOMILP_SOLVE_PLAN_FIELDS; i++) out[i] = f[i];
    return GOMILP_SOLVE_PLAN_FIELDS;
}

// diagnostic (host only, no device): the routing of one frontier wave.  The root views are made here from the fields WavePlan reads; a
// General / GeneralRev made on the host holds null pointers, which its destructor leaves alone.
int gomilp_debug_wave_plan(int64_t nroots, const int64_t *root_m, const int64_t *root_n, const int32_t *root_flags, const double *root_scale_span,
                           int64_t count, const int32_t *root_of, const int64_t *koff, const int32_t *var, const double *rhs, int32_t warm_call,
                           const int32_t *warm, int64_t nspent, const int64_t *spent, int64_t nknobs, const char *const *keys, const int64_t *values,
                           int32_t *route, int32_t *cut, int32_t *group, int32_t *pos) {
    if (nroots < 1 || nroots > 64 || !root_m || !root_n || !root_flags || !root_scale_span || count < 0 || count > (1 << 20) || !koff || !var || !rhs ||
        (warm_call && !warm) || nspent < 0 || (nspent > 0 && (!spent || !warm_call)) || nknobs < 0 || (nknobs > 0 && (!keys || !values)) || !route || !cut || !group || !pos)
        return -GOMILP_ERR_BAD_SHAPE;
    std::vector<Engine::RootView> roots((size_t)nroots);
    std::vector<const Engine::RootView *> views((size_t)nroots);
    for (int64_t r = 0; r < nroots; r++) {
        if (root_m[r] < 1 || root_n[r] < 1 || root_m[r] > (1 << 20) || root_n[r] > (1 << 20)) return -GOMILP_ERR_BAD_SHAPE;
        Engine::RootView &V = roots[(size_t)r];
        V.m = (int)root_m[r]; V.n = (int)root_n[r]; V.scale_span = root_scale_span[r];
        V.unit_basis = (root_flags[r] & GOMILP_WP_ROOT_UNIT_BASIS) != 0;
        // (as Engine::root_general: a narrow root keeps its tableau, a wide one within the limits its B0^-1)
        if ((root_flags[r] & GOMILP_WP_ROOT_GENERAL) && Engine::RootView::general_rev_shape(V.m, V.n)) V.genrev = std::make_shared<Engine::RootView::GeneralRev>();
        else if (root_flags[r] & GOMILP_WP_ROOT_GENERAL) V.gen = std::make_shared<Engine::RootView::General>();
        V.hb.assign((size_t)V.m, 1.0);
        if (root_flags[r] & GOMILP_WP_ROOT_B_NEGATIVE) V.hb[0] = -1.0;
        V.verify_status = (root_flags[r] & GOMILP_WP_ROOT_VERIFY_BAD) ? GOMILP_ERR_BAD_SHAPE : GOMILP_OK;
        views[(size_t)r] = &V;
    }
    if (koff[0] < 0) return -GOMILP_ERR_BAD_SHAPE;
    for (int64_t i = 0; i < count; i++)
        if (koff[i + 1] < koff[i] || (root_of && (root_of[i] < 0 || root_of[i] >= nroots))) return -GOMILP_ERR_BAD_SHAPE;
    gomilp::PoolKnobs knobs;
    for (int64_t i = 0; i < nknobs; i++) if (!keys[i] || !knobs.set(keys[i], values[i])) return -GOMILP_ERR_BAD_SHAPE;   // (a key that is none of the pool's knobs included)
    const gomilp::WaveArgs w{count, root_of, koff, var, nullptr, rhs};
    const gomilp::WavePlan plan = gomilp::WavePlan::make(views.data(), (int)nroots, w, warm_call != 0, knobs);
    *route = plan.route; *cut = gomilp::WavePlan::NONE;
    for (int64_t i = 0; i < count; i++) { group[i] = GOMILP_WP_GROUP_WHOLE; pos[i] = (int32_t)i; }
    if (plan.route != gomilp::WavePlan::TABLEAU) return GOMILP_OK;
    std::vector<int64_t> warm_idx, cold_idx;
    if (warm_call) {
        std::vector<int64_t> parent((size_t)count);
        std::vector<char> resident((size_t)count);
        for (int64_t i = 0; i < count; i++) { parent[(size_t)i] = warm[i] ? 0 : -1; resident[(size_t)i] = warm[i] != 0; }
        plan.warm_groups(w, parent.data(), resident.data(), &warm_idx, &cold_idx);
        for (size_t t = 0; t < warm_idx.size(); t++) { group[warm_idx[t]] = GOMILP_WP_GROUP_WARM; pos[warm_idx[t]] = (int32_t)t; }
        for (int64_t s = 0; s < nspent; s++) {   // as the wave does after the warm run
            if (spent[s] < 0 || spent[s] >= count || group[spent[s]] != GOMILP_WP_GROUP_WARM) return -GOMILP_ERR_BAD_SHAPE;
            group[spent[s]] = GOMILP_WP_GROUP_WHOLE;
            cold_idx.push_back(spent[s]);
        }
        if (!warm_idx.empty()) std::sort(cold_idx.begin(), cold_idx.end());
    }
    const gomilp::WavePlan::ColdCut c = plan.cut_cold(views.data(), (int)nroots, w, cold_idx, knobs);
    *cut = c.cut;
    if (c.cut == gomilp::WavePlan::ONE_GATHERED) for (size_t t = 0; t < cold_idx.size(); t++) pos[cold_idx[t]] = (int32_t)t;
    for (size_t t = 0; t < c.feasible.size(); t++) { group[c.feasible[t]] = GOMILP_WP_GROUP_FEASIBLE; pos[c.feasible[t]] = (int32_t)t; }
    for (size_t t = 0; t < c.phase1.size(); t++) { group[c.phase1[t]] = GOMILP_WP_GROUP_PHASE1; pos[c.phase1[t]] = (int32_t)t; }
    if (c.cut == gomilp::WavePlan::HALVES)
        for (int64_t i = 0; i < count; i++) { group[i] = i < c.half ? GOMILP_WP_GROUP_HALF0 : GOMILP_WP_GROUP_HALF1; pos[i] = (int32_t)(i < c.half ? i : i - c.half); }
    return GOMILP_OK;
}

// diagnostic (host only, no device): the two arenas of a wave of the batched revised simplex, in doubles — RevBatchEngine::layout, the
// function RevBatchEngine::run sizes its buffers from
int gomilp_debug_rev_footprint(int64_t nroots, const int64_t *root_m, const int64_t *root_n, int64_t count, const int32_t *root_of, const int64_t *koff,
                               int32_t inplace, int64_t *out) {
    if (nroots < 1 || nroots > 64 || !root_m || !root_n || count < 0 || count > (1 << 20) || !koff || !out || koff[0] < 0) return -GOMILP_ERR_BAD_SHAPE;
    for (int64_t r = 0; r < nroots; r++)
        if (root_m[r] < 1 || root_n[r] < 1 || root_m[r] > (1 << 20) || root_n[r] > (1 << 20)) return -GOMILP_ERR_BAD_SHAPE;
    for (int64_t i = 0; i < count; i++)
        if (koff[i + 1] < koff[i] || koff[i + 1] - koff[i] > (1 << 20) || (root_of && (root_of[i] < 0 || root_of[i] >= nroots))) return -GOMILP_ERR_BAD_SHAPE;
    size_t at_tot = 0, wk_tot = 0;
    gomilp::RevBatchEngine::layout(root_m, root_n, count, root_of, koff, inplace != 0, nullptr, &at_tot, &wk_tot);
    out[0] = (int64_t)at_tot; out[1] = (int64_t)wk_tot;
    return GOMILP_OK;
}

int64_t gomilp_debug_find_independent_device(gomilp_ctx *ctx, int64_t problem, int64_t *idx_out, int64_t cap) {
    if (!ctx || !idx_out) return -GOMILP_ERR_BAD_SHAPE;
    std::vector<int32_t> idx;
    const int rc = ctx->eng->debug_find_independent(problem, idx);
    if (rc != GOMILP_OK && rc != GOMILP_ERR_SINGULAR) return -rc;
    for (size_t k = 0; k < idx.size() && (int64_t)k < cap; k++) idx_out[k] = idx[k];
    return (int64_t)idx.size();
}

// launches of the loop kernel's pivot role with replicated reduced costs so far (tests: the kernel under test really ran)
long long gomilp_debug_loop_rep_launches(void) { return gomilp::bt_loop_rep_launches(); }
// launches of the 16 x 128 loop kernel with one exchange record per wave so far (tests: the kernel under test really ran)
long long gomilp_debug_loop_wave_rec_launches(void) { return gomilp::bt_loop_wave_rec_launches(); }
#ifdef GOMILP_DEBUG
// diagnostic flavour only: cycle sums of the final-solve panel kernel (lu_compressed.hip), 4 waves x 16 segments
void gomilp_debug_luc_stamps(unsigned long long *out) { gomilp::luc_stamps_read(out); }
void gomilp_debug_lux_stamps(unsigned long long *out) { gomilp::lux_stamps_read(out); }
void gomilp_debug_res_stamps(unsigned long long *out) { gomilp::res_stamps_read(out); }
#endif

int64_t gomilp_lp_last_trace(gomilp_ctx *ctx, gomilp_pivot *out, int64_t cap) {
    if (!ctx) return -1;
    return ctx->eng->last_trace(out, cap);
}

// lp.Simplex drop-in (simplex.go:88).  The reference's solveWorker goroutines (tree.go:98-100,196-205) call it concurrently:
// every call checks a context (engine + stream + recycled buffers) out of a per-device free list and puts it back, so N
// callers run on N streams; a context is created when the list is empty (at most kFlatMaxCtx per device, then callers
// wait).  The call uploads, solves and releases: nothing of the caller's memory is retained (cgo rules).
namespace {
constexpr int kFlatMaxCtx = 32;
struct FlatPool {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<gomilp_ctx *> free_list;
    int created = 0;
};
FlatPool &flat_pool(int dev) {
    static std::mutex mu;
    static std::map<int, FlatPool *> pools;   // never destroyed: contexts live as long as the process (HIP tears down at exit)
    std::lock_guard<std::mutex> g(mu);
    auto it = pools.find(dev);
    if (it == pools.end()) it = pools.emplace(dev, new FlatPool).first;
    return *it->second;
}
}  // namespace

int gomilp_lp_simplex(const double *c, const double *A, int64_t lda, const double *b, int64_t m, int64_t n, double tol,
                      const int64_t *initial_basic, double *opt_f, double *opt_x, int32_t *has_x, int64_t *basis_out,
                      gomilp_lp_stats *stats) {
    if (has_x) *has_x = 0;
    if (opt_f) *opt_f = NAN;
    if (!c || !A || !b || !opt_f || !opt_x || !has_x || m <= 0 || n <= 0 || lda < n) return GOMILP_ERR_BAD_SHAPE;
    int dev = 0;
    if (gomilp::device_count() <= 0 || hipGetDevice(&dev) != hipSuccess) return GOMILP_ERR_DEVICE;
    FlatPool &fp = flat_pool(dev);
    gomilp_ctx *ctx = nullptr;
    {
        std::unique_lock<std::mutex> lk(fp.mu);
        for (;;) {
            if (!fp.free_list.empty()) { ctx = fp.free_list.back(); fp.free_list.pop_back(); break; }
            if (fp.created < kFlatMaxCtx) { fp.created++; break; }   // create outside the lock
            fp.cv.wait(lk);
        }
    }
    if (!ctx) {
        int st = 0;
        ctx = gomilp_ctx_create(dev, &st);
        if (!ctx) {
            { std::lock_guard<std::mutex> lk(fp.mu); fp.created--; }
            fp.cv.notify_one();
            return st;
        }
    }
    int rc;
    int64_t id = ctx->eng->upload(c, A, lda, b, m, n, true);   // (lazy host copy: Engine::upload)
    if (id < 0) rc = (int)-id;
    else {
        rc = gomilp_lp_solve_resident(ctx, id, tol, initial_basic, opt_f, opt_x, has_x, basis_out, stats);
        gomilp_lp_free(ctx, id);
    }
    { std::lock_guard<std::mutex> lk(fp.mu); fp.free_list.push_back(ctx); }
    fp.cv.notify_one();
    return rc;
}

}  // extern "C"
