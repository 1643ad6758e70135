// Host side of the device-batched revised simplex (engine_batch_revised.hpp).  Buf: the device and pinned buffers, which grow with the
// largest wave seen.  Wave: one call of run — its arguments, what each step derives from them, and the steps in the order run calls
// them: four of pure host code (measure, match_warm, lay_out, geometry), then Buf::ensure, stage, start and, until no relaxation is
// active, superstep (the fixed launch list, one read-back) and harvest (the hand-over of finished relaxations).  DESIGN.md §2.5e "Host
// side of a run" says which step synchronises and which host buffer has to outlive which of them.
#include "engine_batch_revised.hpp"

#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <vector>

#include "batch_revised.h"
#include "kernels_common.h"

namespace gomilp {

#define RV_TRY(expr) do { if ((expr) != hipSuccess) return GOMILP_ERR_DEVICE; } while (0)
#define RV_STEP(expr) do { const int rc_ = (expr); if (rc_ != GOMILP_OK) return rc_; } while (0)

namespace {
constexpr int kFirstChunk = 8, kChunk = 32;   // pivots per superstep: most children of a frontier leave Phase I within a few pivots
size_t even(size_t v) { return (v + 1) & ~(size_t)1; }

// does this outcome carry the basis list and x_B, for the final solve?  (harvest copies them exactly where it reports them)
bool carries_basis(const RevOut &o) {
    return o.stage == RS_DONE && (o.status == GOMILP_OK || o.status == GOMILP_ERR_BLAND || o.status == GOMILP_ERR_UNSUPPORTED);
}
// what on_done hears of a relaxation that left the run state (RS_COLD: only that its dual budget is spent, and the dual pivots)
BatchEngine::Outcome outcome_of(const RevOut &o, int warm) {
    BatchEngine::Outcome oc;
    oc.warm = warm; oc.pivd = o.pivd;
    if (o.stage == RS_COLD) { oc.stage = BS_COLD; return oc; }
    oc.stage = o.stage == RS_DONE ? BS_DONE : BS_HOST;
    oc.status = o.status; oc.wrapped = o.wrapped; oc.phase1_used = o.phase1_used;
    oc.piv1 = o.piv1; oc.piv2 = o.piv2; oc.bland = o.bland;
    oc.art_exchanges = o.exch;
    return oc;
}
hipError_t regrow(double **p, size_t *cap, size_t need) {
    if (need <= *cap) return hipSuccess;
    if (*p) hipFree(*p);
    *p = nullptr; *cap = 0;
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(p), need * sizeof(double));
    if (e == hipSuccess) *cap = need;
    return e;
}
}  // namespace

struct RevBatchEngine::Buf {
    double *d_at = nullptr, *d_work = nullptr;       // the children's At (assembled, never cleared) / everything else (cleared per wave)
    size_t cap_at = 0, cap_work = 0;                 // in doubles
    RevLP *d_lps = nullptr;
    RevOut *d_out = nullptr;
    int *d_act = nullptr;
    size_t cap_lp = 0;
    double *d_k = nullptr;                           // sign | rhs | b0 | c2 (doubles), then var | rho0 (ints)
    size_t cap_k = 0;
    RevOut *h_out = nullptr;
    int *h_act = nullptr;
    int32_t *h_basic = nullptr;
    double *h_xb = nullptr;
    size_t cap_h = 0;
    void free_all() {
        for (void *p : {(void *)d_at, (void *)d_work, (void *)d_lps, (void *)d_out, (void *)d_act, (void *)d_k}) if (p) hipFree(p);
        for (void *p : {(void *)h_out, (void *)h_act, (void *)h_basic, (void *)h_xb}) if (p) hipHostFree(p);
        d_at = d_work = d_k = nullptr; d_lps = nullptr; d_out = nullptr; d_act = nullptr;
        h_out = nullptr; h_act = nullptr; h_basic = nullptr; h_xb = nullptr;
        cap_at = cap_work = cap_lp = cap_k = cap_h = 0;
    }
    // room for a wave of `count` relaxations: the three arenas (in doubles), the per-relaxation arrays, the pinned result arenas
    // (count * ld_max).  What has to grow must fit the free device memory (with the head-room of Engine::device_fits; mem_limit_mib: pool
    // knob rev_mem_limit, a cap below the free memory takes its place): else *fits = false and nothing changed — the wave goes to the
    // workers.  Synchronises the stream before it frees anything.
    int ensure(size_t at_tot, size_t wk_tot, size_t k_tot, size_t count, size_t ld_max, int64_t mem_limit_mib, hipStream_t stream, bool *fits) {
        size_t grow = 0;
        if (at_tot > cap_at) grow += at_tot;
        if (wk_tot > cap_work) grow += wk_tot;
        if (k_tot > cap_k) grow += k_tot;
        grow *= sizeof(double);
        if (count > cap_lp) grow += count * (sizeof(RevLP) + sizeof(RevOut) + sizeof(int));
        if (grow) {
            size_t avail = 0, total = 0;
            RV_TRY(hipMemGetInfo(&avail, &total));
            if (mem_limit_mib > 0 && (uint64_t)mem_limit_mib < ((uint64_t)avail >> 20)) avail = (size_t)mem_limit_mib << 20;
            // (buffers that the re-allocation releases are not counted as free: conservative)
            if (grow + grow / 16 + ((size_t)256 << 20) > avail) { *fits = false; return GOMILP_OK; }
        }
        RV_TRY(hipStreamSynchronize(stream));
        RV_TRY(regrow(&d_at, &cap_at, at_tot));
        RV_TRY(regrow(&d_work, &cap_work, wk_tot));
        RV_TRY(regrow(&d_k, &cap_k, k_tot));
        if (count > cap_lp) {
            for (void *p : {(void *)d_lps, (void *)d_out, (void *)d_act}) if (p) hipFree(p);
            for (void *p : {(void *)h_out, (void *)h_act}) if (p) hipHostFree(p);
            d_lps = nullptr; d_out = nullptr; d_act = nullptr; h_out = nullptr; h_act = nullptr; cap_lp = 0;
            RV_TRY(hipMalloc(reinterpret_cast<void **>(&d_lps), count * sizeof(RevLP)));
            RV_TRY(hipMalloc(reinterpret_cast<void **>(&d_out), count * sizeof(RevOut)));
            RV_TRY(hipMalloc(reinterpret_cast<void **>(&d_act), count * sizeof(int)));
            RV_TRY(hipHostMalloc(reinterpret_cast<void **>(&h_out), count * sizeof(RevOut), hipHostMallocDefault));
            RV_TRY(hipHostMalloc(reinterpret_cast<void **>(&h_act), count * sizeof(int), hipHostMallocDefault));
            cap_lp = count;
        }
        if (count * ld_max > cap_h) {
            for (void *p : {(void *)h_basic, (void *)h_xb}) if (p) hipHostFree(p);
            h_basic = nullptr; h_xb = nullptr; cap_h = 0;
            RV_TRY(hipHostMalloc(reinterpret_cast<void **>(&h_basic), count * ld_max * sizeof(int32_t), hipHostMallocDefault));
            RV_TRY(hipHostMalloc(reinterpret_cast<void **>(&h_xb), count * ld_max * sizeof(double), hipHostMallocDefault));
            cap_h = count * ld_max;
        }
        return GOMILP_OK;
    }
};

RevBatchEngine::RevBatchEngine(int device) : device_(device), b_(new Buf) {}

RevBatchEngine::~RevBatchEngine() {
    hipSetDevice(device_);
    if (stream_) hipStreamSynchronize(stream_);
    b_->free_all();
    delete b_;
    if (stream_) hipStreamDestroy(stream_);
}

void RevBatchEngine::release() {
    hipSetDevice(device_);
    if (stream_) hipStreamSynchronize(stream_);
    b_->free_all();
}

bool RevBatchEngine::eligible(const Engine::RootView &R, int K_min, int K_max, int exact_degenerate, int cond_guard, int large_rows) {
    // a wide root without a slack basis counts where it carries its searched basis (RootView::GeneralRev: pool knob rev_general)
    const bool gen = !R.unit_basis && R.genrev;
    if (R.verify_status != GOMILP_OK || !(R.unit_basis || gen)) return false;
    const int m_lo = R.m + K_min, m_hi = R.m + K_max, n_hi = R.n + K_max;
    if (m_hi >= n_hi || (R.n - R.m) < 2 * m_hi) return false;   // the revised formulation (engine.cpp: use_tab's n - m < 2m rule)
    if (gen) {
        // the guarded loop (G = true of K1-K3) with the hand-over of exact steps: modes 1 and 2, where a worker's solve of such a start
        // runs with guard = 1e-9; mode 0 (no guard) and strict mode stay on the workers.  One-pass staging only, up to kRevGeneralMaxRows
        if (exact_degenerate != 1 && exact_degenerate != 2) return false;
        if (m_hi > kRevGeneralMaxRows || ((m_hi + 1) & ~1) > kLdsWindowLd) return false;
    } else if (SolvePlan::exact_wanted(exact_degenerate, m_lo, true, R.scale_span)) {
        // the exact-step guard is off for every shape: the blocked tableau with exact steps stays on the workers
        return false;
    }
    if (cond_guard && m_lo <= 64) return false;                  // the replay of gonum's condition guards runs in Engine::solve only
    // pools keep the row limit of one-pass LDS staging unless the knob large_rows lifts it (the chunked kernels of batch_revised.hip)
    if (!large_rows && ((m_hi + 1) & ~1) > kLdsWindowLd) return false;
    return true;
}

void RevBatchEngine::layout(const int64_t *root_m, const int64_t *root_n, int64_t count, const int32_t *root_of, const int64_t *koff, bool inplace,
                            Lay *lay, size_t *at_tot_out, size_t *wk_tot_out, const char *root_gen) {
    size_t at_tot = 0, wk_tot = 0;
    for (int64_t i = 0; i < count; i++) {
        const int r = root_of ? root_of[i] : 0;
        const int K = (int)(koff[i + 1] - koff[i]), m = (int)root_m[r] + K, n = (int)root_n[r] + K, ld = (m + 1) & ~1;
        Lay L;
        L.at = inplace ? 0 : at_tot;
        if (!inplace) at_tot += (size_t)(n + 1) * ld;
        auto take = [&](size_t doubles) { const size_t o = wk_tot; wk_tot += even(doubles); return o; };
        L.wk0 = wk_tot;
        L.binv0 = take((size_t)m * ld); L.binv1 = take((size_t)m * ld);
        L.xb = take(ld); L.y = take(ld); L.dvec = take(ld); L.move = take(ld); L.bb = take(ld);
        L.rvec = take((size_t)n + 1 - m); L.c1 = take((size_t)n + 1); L.ysc = take((size_t)64 * ld);
        L.basic = take(((size_t)ld + 1) / 2); L.nonbasic = take(((size_t)n + 2 - m + 1) / 2); L.inb = take(((size_t)n + 2 + 1) / 2);
        L.pkp = take(kMaxPartials); L.pkr = take(kMaxPartials); L.pip = take(kMaxPartials / 2); L.pir = take(kMaxPartials / 2);
        L.st = take((sizeof(DevState) + 7) / 8);
        L.art = inplace ? take(ld) : 0;   // (behind everything else: the other offsets of a relaxation are those of the assembled layout)
        // a searched start: the price / ratio keys with the workgroups' runner-up keys behind them (pk2 = pk + kMaxPartials of the G helpers);
        // behind everything else too — a relaxation of a slack root keeps its layout
        L.gpkp = L.gpkr = 0;
        if (root_gen && root_gen[r]) { L.gpkp = take(2 * kMaxPartials); L.gpkr = take(2 * kMaxPartials); }
        L.wk1 = wk_tot;
        if (lay) lay[i] = L;
    }
    *at_tot_out = at_tot; *wk_tot_out = wk_tot;
}

// One call of run.  The members are grouped by the step that writes them; a later step only reads what an earlier one wrote.
struct RevBatchEngine::Wave {
    // ---- the engine and the arguments of run ----
    RevBatchEngine &E;
    Buf &b;
    const Engine::RootView *const *roots; int nroots; const int32_t *root_of; int64_t count; const int64_t *koff;
    const int32_t *var; const double *sign, *rhs; double tol; int64_t max_pivots; const BatchEngine::DoneFn &on_done; const WarmSpec *warm;

    int root_index(int64_t i) const { return root_of ? root_of[i] : 0; }
    const Engine::RootView &root_at(int64_t i) const { return *roots[root_index(i)]; }
    int rows_of(int64_t i) const { return (int)(koff[i + 1] - koff[i]); }

    // ---- measure (pure host): the wave's largest shapes, over its relaxations (each has its own root's m0 / n0) — they size the grids, the
    // staged vectors and the host buffers; nn1_max: nonbasic positions of a Phase-I loop (n + 1 - m, the same for every K of a root).
    // root_gen / is_gen: roots without a slack basis (pool knob rev_general) and their relaxations, which start from the root's searched
    // basis and run the guarded loop
    int K_max = 0, m_max = 0, n_max = 0, nn1_max = 0, ld_max = 0;
    int64_t k_base = 0, ktot = 0, ngen = 0;
    std::vector<char> root_used, root_gen, is_gen;
    int measure() {
        for (int64_t i = 0; i < count && root_of; i++) if (root_of[i] < 0 || root_of[i] >= nroots) return GOMILP_ERR_BAD_SHAPE;
        k_base = koff[0]; ktot = koff[count] - koff[0];
        root_used.assign((size_t)nroots, 0);
        for (int64_t i = 0; i < count; i++) {
            const Engine::RootView &R = root_at(i);
            const int K = rows_of(i);
            K_max = std::max(K_max, K);
            m_max = std::max(m_max, R.m + K); n_max = std::max(n_max, R.n + K); nn1_max = std::max(nn1_max, R.n + 1 - R.m);
            root_used[(size_t)root_index(i)] = 1;
        }
        ld_max = (m_max + 1) & ~1;
        root_gen.assign((size_t)nroots, 0);
        for (int r = 0; r < nroots; r++) root_gen[(size_t)r] = root_used[(size_t)r] && !roots[r]->unit_basis && roots[r]->genrev ? 1 : 0;
        is_gen.resize((size_t)count);
        for (int64_t i = 0; i < count; i++) ngen += is_gen[(size_t)i] = root_gen[(size_t)root_index(i)];
        if (ngen && (ld_max > kLdsWindowLd || (E.large_rows_ && E.row_chunk_ > 0))) return GOMILP_ERR_BAD_SHAPE;   // (WavePlan: one-pass staging only)
        return GOMILP_OK;
    }

    // ---- match_warm (pure host): the kept WK_REVISED state that parent[i] names, where this relaxation's rows extend its rows (bitwise
    // prefix) by J >= 1; kp: where the parent positions of its J new rows' variables start among the wave's wj_tot
    struct Plan { std::shared_ptr<WarmEntry> e; int J = 0; size_t kp = 0; };
    std::vector<Plan> plan;
    size_t wj_tot = 0;
    int64_t nwarm = 0;
    void match_warm() {
        plan.resize((size_t)count);
        // (the one-pass dual pricing stages two vectors whole: without large_rows, waves beyond kRevDualLd run cold, with keeping)
        if (!(warm && warm->store && warm->start_warm && warm->parent && (ld_max <= kRevDualLd || E.large_rows_))) return;
        for (int64_t i = 0; i < count; i++) {
            const int K = rows_of(i);
            if (warm->parent[i] < 0 || K < 1) continue;
            std::shared_ptr<WarmEntry> e = warm->store->find(warm->parent[i]);
            const Engine::RootView &R = root_at(i);
            if (!R.unit_basis) continue;   // (a searched start runs cold)
            if (!e || e->kind != WK_REVISED || e->root_serial != R.serial || e->K >= K || e->m != R.m + e->K || e->n != R.n + e->K ||
                (int)e->hbasic.size() != e->m || (int)e->kvar.size() != e->K) continue;
            const int64_t k0 = koff[i];
            bool prefix = true;
            for (int k = 0; k < e->K && prefix; k++)
                prefix = var[k0 + k] == e->kvar[(size_t)k] && memcmp(&sign[k0 + k], &e->ksign[(size_t)k], sizeof(double)) == 0 &&
                         memcmp(&rhs[k0 + k], &e->krhs[(size_t)k], sizeof(double)) == 0;
            if (!prefix) continue;
            Plan &P = plan[(size_t)i];
            P.e = e; P.J = K - e->K; P.kp = wj_tot;
            wj_tot += (size_t)P.J;
            nwarm++;
        }
    }

    // ---- lay_out (pure host): per relaxation, offsets into the two arenas (RevBatchEngine::layout: doubles; every buffer 16-byte aligned);
    // the shared arena: sign | rhs (ktot each), then one block per used root — b0 (m_r) | c2 = [c, 0...] (n_r + K_max + 2) among the
    // doubles; var (ktot), rho0 (m_r + 1) per used root, then kpos (wj_tot) among the ints
    struct RootBlk { size_t b0 = 0, c2 = 0, rho = 0; };
    std::vector<Lay> lay;
    std::vector<RootBlk> blk;
    size_t at_tot = 0, wk_tot = 0, k_doubles = 0, k_ints = 0, k_tot = 0;
    void lay_out() {
        lay.resize((size_t)count);
        std::vector<int64_t> root_m((size_t)nroots), root_n((size_t)nroots);
        for (int r = 0; r < nroots; r++) if (root_used[(size_t)r]) { root_m[(size_t)r] = roots[r]->m; root_n[(size_t)r] = roots[r]->n; }
        layout(root_m.data(), root_n.data(), count, root_of, koff, E.inplace_, lay.data(), &at_tot, &wk_tot, root_gen.data());
        blk.resize((size_t)nroots);
        k_doubles = even((size_t)2 * ktot + 2); k_ints = (size_t)ktot + 1;
        for (int r = 0; r < nroots; r++) {
            if (!root_used[(size_t)r]) continue;
            RootBlk &B = blk[(size_t)r];
            B.b0 = k_doubles; k_doubles += even((size_t)roots[r]->m);
            B.c2 = k_doubles; k_doubles += even((size_t)roots[r]->n + K_max + 2);
            B.rho = k_ints; k_ints += (size_t)roots[r]->m + 1;
        }
        k_tot = k_doubles + (k_ints + wj_tot + 1) / 2 + 2;
    }

    // ---- geometry (pure host): what every launch of the run shares (RevGeom, batch_revised.h) ----
    RevGeom g{};
    void geometry() {
        // (the pricing grid: K_max positions more than the longest list, as the schedule has always sized it — a relaxation's values do
        // not depend on the grid it gets)
        g.gp = grid_for_rows(nn1_max + K_max); g.gr = grid_for_rows(m_max);
        g.ld_max = ld_max; g.nn_max = nn1_max; g.m_max = m_max; g.n_max = n_max;
        // the chunk of the staged vectors, in double2 (0: the one-pass kernels, exactly the launches of a pool without large_rows): the
        // pool's row_chunk where large_rows is on and it is set, else kAutoRowChunk beyond the LDS window; the dual pricing kernel stages
        // two vectors, so it goes chunked beyond kRevDualLd, or wherever the primal chunk is forced, with at most kRevDualLd / 2 per vector
        g.ck2 = 0;
        if (E.large_rows_ && E.row_chunk_ > 0) g.ck2 = (int)(E.row_chunk_ / 2);
        else if (ld_max > kLdsWindowLd) g.ck2 = kAutoRowChunk / 2;
        g.ck2d = g.ck2 > 0 ? std::min(g.ck2, kRevDualLd / 2) : (ld_max > kRevDualLd ? kRevDualLd / 2 : 0);
        g.lds = g.ck2 > 0 ? 0 : (size_t)ld_max * sizeof(double);
        g.inplace = E.inplace_ ? 1 : 0;   // (the knob is read here and by lay_out: the whole run is of one mode)
        g.stream = E.stream_;
    }

    // ---- stage: the shared arena and the RevLPs, filled on the host and uploaded; the work arena cleared ----
    std::vector<double> hk;    // the shared arena's host image: PAGEABLE, so it lives until the synchronisation that ends `start`
    std::vector<RevLP> lps;    // lives for the run: harvest reads the device pointers, and uploads a slot again where it restarts it cold
    int stage() {
        hk.assign(k_tot, 0.0);
        double *h_sign = hk.data(), *h_rhs = h_sign + ktot;
        int32_t *h_var = reinterpret_cast<int32_t *>(hk.data() + k_doubles), *h_kpos = h_var + k_ints;
        for (int64_t k = 0; k < ktot; k++) { h_sign[k] = sign[k_base + k]; h_rhs[k] = rhs[k_base + k]; h_var[k] = var[k_base + k]; }
        for (int r = 0; r < nroots; r++) {
            if (!root_used[(size_t)r]) continue;
            const Engine::RootView &R = *roots[r];
            double *h_b0 = hk.data() + blk[(size_t)r].b0, *h_c2 = hk.data() + blk[(size_t)r].c2;
            int32_t *h_rho = h_var + blk[(size_t)r].rho;
            for (int i = 0; i < R.m; i++) { h_b0[i] = R.hb[(size_t)i]; h_rho[i] = R.unit_basis ? R.rho0[(size_t)i] : 0; }
            for (int j = 0; j < R.n; j++) h_c2[j] = R.hc[(size_t)j];   // c' = [c, 0] (subproblem.go:110-114)
        }
        // (kpos: the parent position of each new row's variable, -1: nonbasic there)
        for (int64_t i = 0; i < count && nwarm; i++) {
            const Plan &P = plan[(size_t)i];
            if (!P.e) continue;
            const int K = rows_of(i);
            for (int k = 0; k < P.J; k++) {
                const int32_t v = var[koff[i] + K - P.J + k];
                int32_t pos = -1;
                for (int q = 0; q < P.e->m; q++) if (P.e->hbasic[(size_t)q] == v) { pos = q; break; }
                h_kpos[P.kp + (size_t)k] = pos;
            }
        }
        double *d_sign = b.d_k, *d_rhs = d_sign + ktot;
        int32_t *d_var = reinterpret_cast<int32_t *>(b.d_k + k_doubles), *d_kpos = d_var + k_ints;
        RV_TRY(hipMemcpyAsync(b.d_k, hk.data(), k_tot * sizeof(double), hipMemcpyHostToDevice, g.stream));

        lps.resize((size_t)count);
        for (int64_t i = 0; i < count; i++) {
            const Engine::RootView &R = root_at(i);
            const RootBlk &B = blk[(size_t)root_index(i)];
            const int m0 = R.m, n0 = R.n;
            const int K = rows_of(i), m = m0 + K, n = n0 + K, ld = (m + 1) & ~1;
            const double *d_b0 = b.d_k + B.b0, *d_c2 = b.d_k + B.c2;
            const int32_t *d_rho = d_var + B.rho;
            const Lay &L = lay[(size_t)i];
            RevLP &d = lps[(size_t)i];
            memset(&d, 0, sizeof(d));
            double *w = b.d_work;
            d.At = g.inplace ? nullptr : b.d_at + L.at; d.c2 = d_c2; d.c1 = w + L.c1; d.b = w + L.bb;
            d.binv[0] = w + L.binv0; d.binv[1] = w + L.binv1;
            d.xb = w + L.xb; d.y = w + L.y; d.dvec = w + L.dvec; d.move = w + L.move; d.rvec = w + L.rvec; d.yscratch = w + L.ysc;
            d.basic = reinterpret_cast<int32_t *>(w + L.basic); d.nonbasic = reinterpret_cast<int32_t *>(w + L.nonbasic);
            d.inb = reinterpret_cast<int32_t *>(w + L.inb);
            d.pk_price = reinterpret_cast<unsigned long long *>(w + L.pkp); d.pk_ratio = reinterpret_cast<unsigned long long *>(w + L.pkr);
            d.pi_price = reinterpret_cast<unsigned int *>(w + L.pip); d.pi_ratio = reinterpret_cast<unsigned int *>(w + L.pir);
            d.st = reinterpret_cast<DevState *>(w + L.st);
            d.b0 = d_b0; d.rhs = d_rhs + (koff[i] - k_base); d.rho0 = d_rho;
            d.m0 = m0; d.n0 = n0; d.K = K; d.m = m; d.n = n; d.ld = ld;
            d.max_pivots = max_pivots; d.tol_user = tol;
            d.stage = RS_RUN; d.run = RR_NONE; d.cost = d_c2; d.f_var = d.f_pos = d.f_p = -1;
            d.exch_on = E.exchange_ ? 1 : 0; d.x_added = -1; d.x_best = 0xFFFFFFFFu;
            d.At0 = R.dAt; d.ld0 = R.ld; d.avar = d_var + (koff[i] - k_base); d.asign = d_sign + (koff[i] - k_base);
            d.inplace = g.inplace; d.art = g.inplace ? w + L.art : nullptr;
            d.gminidx = -1;
            if (is_gen[(size_t)i]) {
                const Engine::RootView::GeneralRev &G = *R.genrev;
                d.gen = 1; d.gB0inv = G.dB0inv; d.gxb0 = G.dxb0; d.gbasic0 = G.dbasic0; d.gposvar0 = G.dposvar0; d.ldg = G.ld;
                d.guard = 1e-9;   // (SolvePlan::guard of a searched start at exact_degenerate 1 / 2: RevBatchEngine::eligible)
                d.pk_price = reinterpret_cast<unsigned long long *>(w + L.gpkp); d.pk_ratio = reinterpret_cast<unsigned long long *>(w + L.gpkr);
            }
            const Plan &P = plan[(size_t)i];
            if (P.e) {
                d.warm = 1; d.wJ = P.J; d.wmp = P.e->m; d.wldp = P.e->ld;
                d.wbinv = P.e->T; d.wbasic = P.e->basic; d.wkpos = d_kpos + P.kp; d.wsign = d_sign + (koff[i] - k_base) + (K - P.J);
                d.dual_budget = warm->dual_budget > 0 ? warm->dual_budget : 64;
            }
        }
        RV_TRY(hipMemcpyAsync(b.d_lps, lps.data(), (size_t)count * sizeof(RevLP), hipMemcpyHostToDevice, g.stream));
        RV_TRY(hipMemsetAsync(b.d_work, 0, wk_tot * sizeof(double), g.stream));
        return GOMILP_OK;
    }

    // ---- start: every relaxation's start on the device, then the run state of the supersteps ----
    std::vector<int> act;                       // the active relaxations, in list order
    std::vector<char> is_warm, in_dual, in_scan;   // started warm (and still is) / the dual loop runs or is ordered / the candidate scan of
                                                   // the artificial exchange is ordered
    int64_t launches = 0, steps = 0, kept = 0;
    int start() {
        // (the roots' At0 are read where they lie: a root's upload, Engine::upload on its owner's stream, ends with a synchronisation of
        // that stream, so every root the pool holds is complete on the device before this stream reads it)
        // (rev_inplace: nothing is assembled — the kernels read those At0 through ChildCol for the whole run)
        if (!g.inplace) launches += launch_rv_assemble(b.d_lps, (int)count, g);
        launches += launch_rv_init(b.d_lps, (int)count, g);
        if (nwarm) launches += launch_rv_warm_binv(b.d_lps, (int)count, g);
        if (ngen) {
            launches += launch_rv_gen_start(b.d_lps, (int)count, g);
            launches += launch_rv_gen_art(b.d_lps, (int)count, g);
        }
        RV_TRY(hipStreamSynchronize(g.stream));   // (the pageable staging vectors go out of use here)
        RV_TRY(hipGetLastError());
        act.resize((size_t)count); is_warm.resize((size_t)count); in_dual.resize((size_t)count); in_scan.assign((size_t)count, 0);
        for (int64_t i = 0; i < count; i++) { act[(size_t)i] = (int)i; is_warm[(size_t)i] = in_dual[(size_t)i] = plan[(size_t)i].e ? 1 : 0; }
        return GOMILP_OK;
    }

    // ---- superstep: the launch list over the active relaxations, then their RevOut records on the host (b.h_out) ----
    int superstep() {
        const int nact = (int)act.size();
        // (the relaxations of searched starts behind the others: their loop pivots are launches of their own over that part of the list)
        if (ngen) std::stable_partition(act.begin(), act.end(), [&](int id) { return !is_gen[(size_t)id]; });
        int nslack = 0;
        for (int id : act) nslack += is_gen[(size_t)id] ? 0 : 1;
        memcpy(b.h_act, act.data(), (size_t)nact * sizeof(int));
        RV_TRY(hipMemcpyAsync(b.d_act, b.h_act, (size_t)nact * sizeof(int), hipMemcpyHostToDevice, g.stream));
        // (the dual launches only while some active relaxation is in the dual stage: a cold wave's list is setup, chunk x pivot, ctrl)
        bool any_dual = false, any_primal = false, any_scan = false;
        for (int id : act) {
            if (is_gen[(size_t)id]) continue;
            (in_dual[(size_t)id] ? any_dual : any_primal) = true;
        }
        for (int id : act) if (in_scan[(size_t)id]) any_scan = true;
        const int ng = nact - nslack;
        // (the scan's verdict orders the forced pivot that the set-up launches behind it run: an exchange costs no superstep of its own)
        if (any_scan) launches += launch_rv_exchange(b.d_lps, b.d_act, nact, g);
        launches += launch_rv_setup(b.d_lps, b.d_act, nact, g);
        const int chunk = steps < 2 ? kFirstChunk : kChunk;
        for (int t = 0; t < chunk; t++) {
            if (any_dual) launches += launch_rv_dual_pivot(b.d_lps, b.d_act, nslack, g);
            if (any_primal) launches += launch_rv_pivot(b.d_lps, b.d_act, nslack, g);
            if (ng) launches += launch_rv_pivot_g(b.d_lps, b.d_act + nslack, ng, g);
        }
        launches += launch_rv_ctrl(b.d_lps, b.d_act, nact, b.d_out, g);
        RV_TRY(hipMemcpyAsync(b.h_out, b.d_out, (size_t)count * sizeof(RevOut), hipMemcpyDeviceToHost, g.stream));
        RV_TRY(hipStreamSynchronize(g.stream));
        RV_TRY(hipGetLastError());
        steps++;
        return GOMILP_OK;
    }

    // ---- harvest: what the superstep's records say — who goes on, who starts again cold, who is reported ----
    int harvest() {
        struct Keep { int id; std::shared_ptr<WarmEntry> e; };
        std::vector<Keep> keeps;
        std::vector<int> next, done_now;
        bool copies = false;
        for (int id : act) {
            const RevOut &o = b.h_out[id];
            in_dual[(size_t)id] = o.dual ? 1 : 0;
            in_scan[(size_t)id] = o.scan ? 1 : 0;
            if (o.stage == RS_RUN) { next.push_back(id); continue; }
            if (o.stage == RS_COLD) {
                // the dual budget is spent: reported as a fallback, then the slot starts again from its slack basis — its work area zeroed, its
                // RevLP as the wave's first upload but cold, its assembled At as it is — and runs through the following supersteps
                on_done(id, outcome_of(o, 1), nullptr, nullptr);
                RevLP &d = lps[(size_t)id];
                const Lay &L = lay[(size_t)id];
                d.warm = 0;
                is_warm[(size_t)id] = 0; in_dual[(size_t)id] = 0; in_scan[(size_t)id] = 0;
                RV_TRY(hipMemsetAsync(b.d_work + L.wk0, 0, (L.wk1 - L.wk0) * sizeof(double), g.stream));
                RV_TRY(hipMemcpyAsync(b.d_lps + id, &d, sizeof(RevLP), hipMemcpyHostToDevice, g.stream));
                launches += launch_rv_init(b.d_lps + id, 1, g);
                next.push_back(id);
                continue;
            }
            done_now.push_back(id);
            if (!carries_basis(o)) continue;
            const RevLP &d = lps[(size_t)id];
            RV_TRY(hipMemcpyAsync(b.h_basic + (size_t)id * ld_max, d.basic, (size_t)d.m * sizeof(int32_t), hipMemcpyDeviceToHost, g.stream));
            RV_TRY(hipMemcpyAsync(b.h_xb + (size_t)id * ld_max, d.xb, (size_t)d.m * sizeof(double), hipMemcpyDeviceToHost, g.stream));
            copies = true;
            if (o.status == GOMILP_OK && warm && warm->store && warm->keep && warm->tag && warm->keep[id] && warm->tag[id] >= 0) {
                // kept for its children: the current B^-1 and the basis list, device to device on this stream (the slot is terminal:
                // nothing writes its buffers before the next run, which starts behind this stream)
                std::shared_ptr<WarmEntry> e = warm->store->acquire_revised(d.m, d.ld);
                if (e) {
                    RV_TRY(hipMemcpyAsync(e->T, d.binv[o.flips & 1], (size_t)d.m * d.ld * sizeof(double), hipMemcpyDeviceToDevice, g.stream));
                    RV_TRY(hipMemcpyAsync(e->basic, d.basic, (size_t)d.m * sizeof(int32_t), hipMemcpyDeviceToDevice, g.stream));
                    keeps.push_back({id, e});
                }
            }
        }
        if (copies) RV_TRY(hipStreamSynchronize(g.stream));
        for (const Keep &kp : keeps) {
            const RevLP &d = lps[(size_t)kp.id];
            WarmEntry &e = *kp.e;
            const int64_t k0 = koff[kp.id];
            e.kind = WK_REVISED; e.m = d.m; e.n = d.n; e.ld = d.ld; e.K = d.K; e.nn = 0; e.ldt = 0;
            e.root_serial = root_at(kp.id).serial;
            e.hbasic.assign(b.h_basic + (size_t)kp.id * ld_max, b.h_basic + (size_t)kp.id * ld_max + d.m);
            e.kvar.assign(var + k0, var + k0 + d.K); e.ksign.assign(sign + k0, sign + k0 + d.K); e.krhs.assign(rhs + k0, rhs + k0 + d.K);
            warm->store->put(warm->tag[kp.id], kp.e);
            kept++;
        }
        for (int id : done_now) {
            const RevOut &o = b.h_out[id];
            const bool fin = carries_basis(o);
            on_done(id, outcome_of(o, is_warm[(size_t)id]), fin ? b.h_basic + (size_t)id * ld_max : nullptr, fin ? b.h_xb + (size_t)id * ld_max : nullptr);
        }
        act.swap(next);
        return GOMILP_OK;
    }
};

int RevBatchEngine::run(const Engine::RootView *const *roots, int nroots, const int32_t *root_of, int64_t count, const int64_t *koff,
                        const int32_t *var, const double *sign, const double *rhs, double tol, int64_t max_pivots,
                        const BatchEngine::DoneFn &on_done, Stats *stats, bool *fits, const WarmSpec *warm) {
    const auto t0 = std::chrono::steady_clock::now();
    *fits = true;
    if (count <= 0) return GOMILP_OK;
    if (!roots || nroots < 1) return GOMILP_ERR_BAD_SHAPE;
    RV_TRY(hipSetDevice(device_));
    if (!stream_) RV_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    Wave w{*this, *b_, roots, nroots, root_of, count, koff, var, sign, rhs, tol, max_pivots, on_done, warm};
    RV_STEP(w.measure());
    w.match_warm();
    w.lay_out();
    w.geometry();
    RV_STEP(b_->ensure(w.at_tot, w.wk_tot, w.k_tot, (size_t)count, (size_t)w.ld_max, mem_limit_mib_, stream_, fits));
    if (!*fits) return GOMILP_OK;   // (nothing ran: the wave goes to the workers)
    RV_STEP(w.stage());
    RV_STEP(w.start());
    while (!w.act.empty()) {
        RV_STEP(w.superstep());
        RV_STEP(w.harvest());
    }
    if (stats) {
        stats->launches = w.launches; stats->supersteps = w.steps; stats->warm_kept = w.kept;
        stats->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return GOMILP_OK;
}

}  // namespace gomilp
