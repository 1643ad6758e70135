// Host-side engine: see engine.hpp.  Control flow mirrors gonum's simplex()
// (vendor/gonum.org/v1/gonum/optimize/convex/lp/simplex.go:93-302); all O(m^2)/O(m*n) work is
// enqueued as gfx950 kernels (simplex_kernels.hip).  No CPU fallback exists: any HIP failure
// surfaces as GOMILP_ERR_DEVICE.
#include "engine_work.hpp"

#include <condition_variable>
#include <atomic>

namespace gomilp {

int device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *compiled_arch() { return "gfx950"; }

Engine::Engine(int device) : device_(device), w_(new Work) {}

Engine::~Engine() {
    hipSetDevice(device_);
    if (up_dA_) hipFree(up_dA_);
    if (up_stats_) hipFree(up_stats_);
    for (auto *vec : {&problems_, &child_pool_, &root_pool_})
        for (auto &p : *vec) {
            if (!p) continue;
            hipFree(p->dAt); hipFree(p->db);
            if (!p->is_child) {   // a child's c / c1 / sign / var live inside its b block
                hipFree(p->dc); hipFree(p->dc1);
                if (p->dvar) hipFree(p->dvar);
                if (p->dsign) hipFree(p->dsign);
            }
        }
    for (auto &kv : kept_) if (kv.second.d) hipFree(kv.second.d);
    for (auto &b : keep_pool_) hipFree(b.first);
    w_->release_all();
    if (stream_) hipStreamDestroy(stream_);
}

// Persistent loop kernels wait for their own workgroups, so every workgroup of a launch must be resident.  The 128-thread shape
// (up to 2048 rows: 136 workgroups of two waves, four fit a CU) leaves room for four launches at once, each with its pivot
// workgroups on an XCD of its own; the 256- / 512-thread shapes fill the chip (one workgroup per CU) and run alone.
namespace {
struct LoopSlots { std::mutex mu; std::condition_variable cv; int used = 0, big_waiting = 0; bool busy[4] = {false, false, false, false}; };
LoopSlots &loop_slots(int dev) { static LoopSlots s[64]; return s[dev & 63]; }
}  // namespace
int Engine::loop_acquire(int dev, int weight) {
    LoopSlots &L = loop_slots(dev);
    std::unique_lock<std::mutex> lk(L.mu);
    if (weight >= 4) {
        L.big_waiting++;   // from here on no further small launch is admitted: a stream of them would never let `used` reach 0
        L.cv.wait(lk, [&] { return L.used == 0; });
        L.big_waiting--;
        L.used = 4;
        for (bool &b2 : L.busy) b2 = true;
        return 0;
    }
    L.cv.wait(lk, [&] { return L.used < 4 && L.big_waiting == 0; });
    L.used++;
    for (int i = 0; i < 4; i++) if (!L.busy[i]) { L.busy[i] = true; return i; }
    return 0;
}
bool Engine::loop_try_acquire_all(int dev) {
    LoopSlots &L = loop_slots(dev);
    std::lock_guard<std::mutex> lk(L.mu);
    if (L.used != 0 || L.big_waiting != 0) return false;
    L.used = 4;
    for (bool &b2 : L.busy) b2 = true;
    return true;
}
void Engine::loop_release(int dev, int weight, int slot) {
    LoopSlots &L = loop_slots(dev);
    {
        std::lock_guard<std::mutex> lk(L.mu);
        if (weight >= 4) { L.used = 0; for (bool &b2 : L.busy) b2 = false; }
        else { L.used--; L.busy[slot & 3] = false; }
    }
    L.cv.notify_all();
}

int BtKnobs::set(const std::string &key, int64_t v) {
    if (key == "chunk") { if (v < 1) return GOMILP_ERR_BAD_SHAPE; chunk = v; }
    else if (key == "max_pivots") max_pivots = v < 0 ? 0 : v;
    else if (key == "block_k") { if (v < 0 || v > bt_max_k()) return GOMILP_ERR_BAD_SHAPE; block_k = v; }
    else if (key == "bt_nt") { if (v != 0 && v != 256 && v != 512 && v != 1024) return GOMILP_ERR_BAD_SHAPE; bt_nt = v; }
    else if (key == "bt_old") bt_old = v ? 1 : 0;
    else if (key == "bt_stamps") bt_stamps = v < 0 ? 0 : (v > 2 ? 2 : v);
    else if (key == "bt_groups") { if (v != -1 && v != 0 && v != 2 && v != 4 && v != 8 && v != 16) return GOMILP_ERR_BAD_SHAPE; bt_groups = v; }
    else if (key == "bt_lag") bt_lag = v ? 1 : 0;
    else if (key == "loop_chunk") { if (v < 32) return GOMILP_ERR_BAD_SHAPE; loop_chunk = v; }
    else if (key == "loop_grid") { if (v < 0 || v > 4096) return GOMILP_ERR_BAD_SHAPE; loop_grid = v; }
    else if (key == "loop_upd") { if (v < 0) return GOMILP_ERR_BAD_SHAPE; loop_upd = v; }
    else if (key == "loop_rep") loop_rep = v ? 1 : 0;
    else if (key == "loop_g") { if (v != 0 && v != 8 && v != 16) return GOMILP_ERR_BAD_SHAPE; loop_g = v; }
    else if (key == "loop_wave_rec") loop_wave_rec = v ? 1 : 0;
    else if (key == "loop_k") { if (v != 0 && v != 8 && v != 12 && v != 16) return GOMILP_ERR_BAD_SHAPE; loop_k = v; }
    else return -1;
    return GOMILP_OK;
}

int SolveKnobs::set(const std::string &key, int64_t v) {
    if (key == "fused") fused = v ? 1 : 0;
    else if (key == "tableau") tableau = v ? 1 : 0;
    else if (key == "blocked") blocked = v ? 1 : 0;
    else if (key == "general_device") general_device = v ? 1 : 0;
    else if (key == "general_min_rows") general_min_rows = v < 2 ? 2 : v;
    else if (key == "exact_degenerate") { if (v < 0 || v > 3) return GOMILP_ERR_BAD_SHAPE; exact_degenerate = v; }   // 3: strict — EVERY pivot decided on fresh gonum-order solves (engine_tableau.cpp exact_step)
    else if (key == "cond_guard") cond_guard = v ? 1 : 0;
    else return -1;
    return GOMILP_OK;
}

// The one place that says where a single solve of m < n rows goes ("Where a solve goes"; tests/test_solve_plan.py).
SolvePlan SolvePlan::make(int m, int n, int ld, StartKind start, double scale_span, const SolveKnobs &k) {
    SolvePlan p;
    const bool slack = start == Slack, strict = k.exact_degenerate == 3;
    p.gen_start = p.needs_host_A = !slack;   // (the search, the set-up and the exact steps of a non-slack start read the host copy of A)
    p.badly_scaled = scale_span > 1e9;
    // beyond the LDS window (chunked staging) only the three-kernel revised simplex runs, from slack starts: the general
    // start's search and set-up stage m-long rows, and the single-kernel tableau returned a wrong ErrUnbounded on a 12288 x 18432 slack
    // start after a run of Bland steps
    const bool windowed = ld <= kLdsWindowLd;
    if (!windowed && !slack) { p.status = GOMILP_ERR_UNSUPPORTED; return p; }
    // A non-slack starting basis (equality rows, supplied basis) takes the tableau pipelines wherever their row fits: their set-up accepts
    // any B^-1; the n - m < 2m rule is only the bytes-per-pivot trade-off between the two formulations (the explicit tableau moves
    // 16*m*(n-m) bytes per pivot in one launch, the revised form 8*[m(n-m) + 2m^2] in two).  So does a wide LP that wants exact steps when
    // the BLOCKED tableau takes it: on slack starts only the block kernels stop in front of a degenerate pivot (ST_NEED_EXACT) for
    // Engine::exact_step — the single-kernel tableau and the revised pipelines decide every pivot on their updated quantities.
    // (tableau = 0 keeps the revised pipelines, blocked = 0 the n - m < 2m rule, both without the guard on slack starts: A/B knobs.)
    const int nn_max = n + 1 - m;
    const bool tab_fits = (size_t)tab_ld(nn_max) * sizeof(double) <= 64 * 1024;
    const bool bt_ok = k.blocked && bt_supported(m, nn_max);
    const bool exact = exact_wanted(k.exact_degenerate, m, slack, scale_span);
    p.use_tab = k.tableau && ((n - m) < 2 * m || !slack || (exact && bt_ok)) && tab_fits && windowed;
    p.blocked = p.use_tab && bt_ok;
    // A non-slack start the tableau does not take (its row beyond the LDS window: n - m > 8191, or knob tableau = 0) runs the three-kernel
    // revised loop with the exact-step guard (LPArgs::guard; the fused pipeline has none): the exact steps need the host copy of A, kept
    // up to m * n = 2^25
    p.gen_revised = !slack && !p.use_tab && (size_t)m * (size_t)n <= ((size_t)1 << 25);
    // strict mode IS the exact steps: where neither the blocked tableau nor that loop runs, the solve refuses instead of deciding the
    // default way; a non-slack start that neither the tableau nor that loop takes has nowhere to go
    if ((strict && !p.blocked && !p.gen_revised) || (!slack && !p.use_tab && !p.gen_revised)) { p.status = GOMILP_ERR_UNSUPPORTED; return p; }
    p.pipeline = p.use_tab ? (p.blocked ? 3 : 2) : ((k.fused && fused_supported(ld) && !p.gen_revised) ? 1 : 0);
    // degenerate vertices decided on a fresh gonum-order x_B where the pipeline has exact steps; strict: an infinite guard —
    // the kernels stop in front of EVERY decision, stop test included, and the host repeats the reference's iteration on fresh solves
    if (p.blocked || p.gen_revised) p.guard = strict ? std::numeric_limits<double>::infinity() : exact ? 1e-9 : 0.0;
    p.cguard = (k.cond_guard && slack && m > 64) ? 1e-9 : 0.0;   // (<= 64 rows: the per-pivot replay; non-slack starts: the guard above is on)
    p.replay_if_feasible = k.cond_guard && m <= 64 && start != Supplied;
    p.search_on_device = m >= k.general_min_rows && k.general_device;
    p.art_on_device = !slack && m >= k.general_min_rows;
    return p;
}

SolvePlan SolvePlan::warm(int ld, double scale_span, const SolveKnobs &k) {
    SolvePlan p;
    p.badly_scaled = scale_span > 1e9;
    p.pipeline = (k.fused && fused_supported(ld)) ? 1 : 0;
    return p;
}

int Engine::set(const std::string &key, int64_t v) {
    std::lock_guard<std::mutex> g(mu_);
    const int bt = bt_knobs_.set(key, v);
    if (bt >= 0) return bt;
    const int sk = knobs_.set(key, v);
    if (sk >= 0) return sk;
    if (key == "refresh") { if (v < 0) return GOMILP_ERR_BAD_SHAPE; refresh_ = v; }
    else if (key == "trace") trace_on_ = v ? 1 : 0;
    else if (key == "sample_events") sample_events_ = v < 0 ? 0 : v;
    else if (key == "lu_look") lu_look_ = v ? 1 : 0;
    else if (key == "lu_large") lu_large_ = v ? 1 : 0;
    else if (key == "lu_blocked") lu_blocked_ = v < 0 ? 0 : (v > 2 ? 3 : v);  // 0 per column, 1 blocked panels, 2 compressed rounds (slot panel), 3 the same with the look-ahead schedule (default; lu_compressed.hip)
    else if (key == "bt_upd_valu") bt_upd_valu_ = v ? 1 : 0;
#ifdef GOMILP_DEBUG
    else if (key == "bt_fault") bt_fault_ = v;   // fault injection, diagnostic flavour only: 1 a workgroup of the block / loop kernels, 2 the U-solve workgroup of the look-ahead LU
#endif
    else if (key == "lu_cross") lu_cross_ = v < 0 ? -1 : (v > 2 ? 2 : v);   // the panel's rows on the workgroups of one XCD (lu_cross.hip): 0 never, 1 sixteen slots in the plain schedule, 2 thirty-two slots in the schedule lu_blocked names, -1 (default) 2 for bases of 1281 .. 2048 rows
    else if (key == "general_block") general_block_ = v ? 1 : 0;
    else if (key == "poll_delay") { if (v < 0 || v > 64) return GOMILP_ERR_BAD_SHAPE; poll_delay_ = v; }
    else if (key == "row_chunk") { if (v < 0 || v % 512 != 0 || v > kLdsWindowLd) return GOMILP_ERR_BAD_SHAPE; row_chunk_ = v; }   // (whole 256-double2 steps of wave_dot_chunk)
    else return GOMILP_ERR_BAD_SHAPE;
    return GOMILP_OK;
}

int Engine::ensure_work(int m, int ncols) {
    HIP_TRY(hipSetDevice(device_));
    if (!stream_) HIP_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    Work &w = *w_;
    if (!w.st) {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device_) == hipSuccess && ncu > 0) ncu_ = ncu;
        // (the keys twice over: the runner-up keys of the guard instances of K1-K3 follow at + kMaxPartials, LPArgs::guard)
        HIP_TRY(dmalloc(&w.pk_price, 2 * kMaxPartials)); HIP_TRY(dmalloc(&w.pk_ratio, 2 * kMaxPartials));
        HIP_TRY(dmalloc(&w.pi_price, kMaxPartials)); HIP_TRY(dmalloc(&w.pi_ratio, kMaxPartials));
        HIP_TRY(dmalloc(&w.pv_price, kMaxPartials)); HIP_TRY(dmalloc(&w.pb_ratio, kMaxPartials)); HIP_TRY(dmalloc(&w.pd_ratio, kMaxPartials)); HIP_TRY(dmalloc(&w.px_ratio, kMaxPartials));
        for (int t = 0; t < 2; t++) {
            HIP_TRY(dmalloc(&w.lpk[t], kMaxPartials)); HIP_TRY(dmalloc(&w.lpl[t], kMaxPartials)); HIP_TRY(dmalloc(&w.lpr[t], kMaxPartials));
        }
        HIP_TRY(dmalloc(&w.st, 1));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w.st_host), sizeof(DevState), hipHostMallocDefault));
        HIP_TRY(dmalloc(&w.luctl, 2));   // (by round parity: lu_compressed.hip, look-ahead schedule)
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w.luctl_host), 2 * sizeof(LUCtl), hipHostMallocDefault));
        w.trace_cap = 1 << 18;
        HIP_TRY(dmalloc(&w.trace, (size_t)w.trace_cap));
        HIP_TRY(hipEventCreate(&w.ev[0])); HIP_TRY(hipEventCreate(&w.ev[1]));
    }
    const int ld = (m + 1) & ~1;
    if (m <= w.cap_m && ncols <= w.cap_cols) return GOMILP_OK;
    // head-room: B&B children grow by one row and one column per level; without it every level would release and
    // re-allocate the whole work set (hipFree synchronises the device, pinned allocations are slow)
    const int nm = std::max(m + 32 + m / 16, w.cap_m), nc = std::max(ncols + 64 + ncols / 16, w.cap_cols);
    const int nld = std::max((nm + 1) & ~1, w.cap_ld);
    w.release();
    for (auto &p : w.binv) HIP_TRY(dmalloc(&p, (size_t)nm * nld));
    HIP_TRY(dmalloc(&w.W, (size_t)nm * nld));
    HIP_TRY(dmalloc(&w.xb, (size_t)nld)); HIP_TRY(dmalloc(&w.yb[0], (size_t)nld)); HIP_TRY(dmalloc(&w.yb[1], (size_t)nld));
    HIP_TRY(dmalloc(&w.dvec, (size_t)nld));
    HIP_TRY(dmalloc(&w.move, (size_t)nld)); HIP_TRY(dmalloc(&w.rvec, (size_t)nc));
    HIP_TRY(dmalloc(&w.yscratch, (size_t)64 * nld));
    HIP_TRY(dmalloc(&w.basic, (size_t)nm + (size_t)nc)); w.nonbasic = w.basic + nm;   // one block: both lists go up in one copy
    // (rowstep: + two snapshots, by round parity, for the look-ahead schedule of the compressed LU)
    HIP_TRY(dmalloc(&w.lpos, (size_t)nm)); HIP_TRY(dmalloc(&w.rowstep, (size_t)3 * nm)); HIP_TRY(dmalloc(&w.rho, (size_t)nm));
    HIP_TRY(dmalloc(&w.unitrow, (size_t)nm)); HIP_TRY(dmalloc(&w.denseflag, (size_t)nm)); HIP_TRY(dmalloc(&w.dlist, (size_t)nm));
    HIP_TRY(dmalloc(&w.ludiag, (size_t)nm)); HIP_TRY(dmalloc(&w.Wd, (size_t)nm * nld + 512));   // (+ the tail of k_luc_pack_small: row positions, flags, two control blocks)
    HIP_TRY(dmalloc(&w.luLp, (size_t)64 * nld)); HIP_TRY(dmalloc(&w.luUp, (size_t)64 * nld));   // (2 x 32 rows: by round parity)
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w.h_W), ((size_t)nm * nld + 512) * sizeof(double), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w.h_vec), (size_t)std::max(nld, nc) * sizeof(double), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w.h_chk), (size_t)nld * sizeof(double), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w.h_idx), ((size_t)nm + (size_t)nc) * sizeof(int32_t), hipHostMallocDefault));   // mirrors the basic | nonbasic device block
    {
        const size_t cap = std::max<size_t>(4096, sizeof(double) * ((size_t)std::max(nld, nc) + 64));
        for (int t = 0; t < Work::kStageSlots; t++) {
            if (w.stage_cap[t] >= cap) continue;
            if (w.stage_inflight) { hipStreamSynchronize(stream_); w.stage_inflight = 0; }
            if (w.stage_buf[t]) hipHostFree(w.stage_buf[t]);
            w.stage_buf[t] = nullptr; w.stage_cap[t] = 0;
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w.stage_buf[t]), cap, hipHostMallocDefault));
            w.stage_cap[t] = cap;
        }
    }
    w.cap_m = nm; w.cap_ld = nld; w.cap_cols = nc;
    return GOMILP_OK;
}

// ------------------------------------------------------------------------------------------------
// upload: A (row-major m x n) -> At ((n+1) x ld) in HBM, column statistics for verifyInputs and for
// the unit-column fast path of findLinearlyIndependent (simplex.go:385-439, :611-637)
// ------------------------------------------------------------------------------------------------
int64_t Engine::upload(const double *c, const double *A, int64_t lda, const double *b, int64_t m64, int64_t n64, bool lazy_host) {
    std::lock_guard<std::mutex> g(mu_);
    if (!c || !A || !b || m64 <= 0 || n64 <= 0 || lda < n64 || m64 > (1 << 20) || n64 > (1 << 22)) return -GOMILP_ERR_BAD_SHAPE;
    const int m = (int)m64, n = (int)n64;
    const int ld = (m + 1) & ~1;
    if (ld > kLdsWindowLd && lds_window_only_) return -GOMILP_ERR_UNSUPPORTED;  // one-pass LDS staging of one row
    if (hipSetDevice(device_) != hipSuccess) return -GOMILP_ERR_DEVICE;
    if (!stream_ && hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess) return -GOMILP_ERR_DEVICE;
    const double t0 = now_s();
    const size_t need_at = (size_t)(n + 1) * ld, need_c = (size_t)n + 1, need_b = (size_t)ld;
    std::unique_ptr<Problem> P;
    for (size_t i = 0; i < root_pool_.size(); i++) {   // a released root whose buffers fit
        Problem &q = *root_pool_[i];
        if (q.cap_at >= need_at && q.cap_c >= need_c && q.cap_b >= need_b) {
            P = std::move(root_pool_[i]);
            root_pool_.erase(root_pool_.begin() + i);
            break;
        }
    }
    const bool recycled = (bool)P;
    if (ld > kLdsWindowLd) {   // beyond the LDS window: shapes whose buffers do not fit are refused before anything is allocated
        const size_t dbl = (up_dA_cap_ < (size_t)m * n ? (size_t)m * n : 0) + (recycled ? 0 : need_at + 2 * need_c + need_b);
        if (!device_fits(dbl * sizeof(double))) {
            if (recycled) root_pool_.push_back(std::move(P));
            return -GOMILP_ERR_UNSUPPORTED;
        }
    }
    if (!P) P.reset(new Problem);
    P->m = m; P->n = n; P->ld = ld;
    double *dA = nullptr;
    int32_t *dstats = nullptr;
    auto fail = [&](int code) -> int64_t {
        if (P->dAt) hipFree(P->dAt);
        if (P->dc) hipFree(P->dc);
        if (P->dc1) hipFree(P->dc1);
        if (P->db) hipFree(P->db);
        return -code;
    };
#define UP_TRY(expr) do { if ((expr) != hipSuccess) return fail(GOMILP_ERR_DEVICE); } while (0)
    if (up_dA_cap_ < (size_t)m * n) {
        if (up_dA_) hipFree(up_dA_);
        up_dA_ = nullptr; up_dA_cap_ = 0;
        UP_TRY(dmalloc(&up_dA_, (size_t)m * n));
        up_dA_cap_ = (size_t)m * n;
    }
    const size_t range_off = ((size_t)3 * n + m + 1) & ~(size_t)1;   // two 64-bit words behind the lists: max / min non-zero |a_ij|
    if (up_stats_cap_ < range_off + 4) {
        if (up_stats_) hipFree(up_stats_);
        up_stats_ = nullptr; up_stats_cap_ = 0;
        UP_TRY(dmalloc(&up_stats_, range_off + 4));
        up_stats_cap_ = range_off + 4;
    }
    dA = up_dA_; dstats = up_stats_;
    if (!recycled) {
        UP_TRY(dmalloc(&P->dAt, need_at));
        UP_TRY(dmalloc(&P->dc, need_c));
        UP_TRY(dmalloc(&P->dc1, need_c));
        UP_TRY(dmalloc(&P->db, need_b));
        P->cap_at = need_at; P->cap_c = need_c; P->cap_b = need_b;
    }
    UP_TRY(hipMemcpy2DAsync(dA, (size_t)n * sizeof(double), A, (size_t)lda * sizeof(double), (size_t)n * sizeof(double), m,
                            hipMemcpyHostToDevice, stream_));
    UP_TRY(hipMemsetAsync(P->dAt, 0, (size_t)(n + 1) * ld * sizeof(double), stream_));
    UP_TRY(hipMemsetAsync(P->dc, 0, ((size_t)n + 1) * sizeof(double), stream_));
    UP_TRY(hipMemsetAsync(P->dc1, 0, ((size_t)n + 1) * sizeof(double), stream_));
    UP_TRY(hipMemsetAsync(P->db, 0, (size_t)ld * sizeof(double), stream_));
    UP_TRY(hipMemsetAsync(dstats, 0, (range_off + 2) * sizeof(int32_t), stream_));
    UP_TRY(hipMemsetAsync(dstats + range_off + 2, 0xFF, 2 * sizeof(int32_t), stream_));
    UP_TRY(hipMemcpyAsync(P->dc, c, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream_));
    UP_TRY(hipMemcpyAsync(P->db, b, (size_t)m * sizeof(double), hipMemcpyHostToDevice, stream_));
    const double one = 1.0;
    UP_TRY(hipMemcpyAsync(P->dc1 + n, &one, sizeof(double), hipMemcpyHostToDevice, stream_));
    launch_transpose_in(dA, n, m, n, P->dAt, ld, stream_);
    launch_col_stats(P->dAt, ld, m, n, dstats, dstats + n, dstats + 2 * n, dstats + 3 * n, reinterpret_cast<unsigned long long *>(dstats + range_off), stream_);
    std::vector<int32_t> hs(range_off + 4);
    UP_TRY(hipMemcpyAsync(hs.data(), dstats, hs.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    UP_TRY(sync_stream());
    UP_TRY(hipGetLastError());
#undef UP_TRY
    P->nnz.assign(hs.begin(), hs.begin() + n);
    P->lastrow.assign(hs.begin() + n, hs.begin() + 2 * n);
    P->allone.assign(hs.begin() + 2 * n, hs.begin() + 3 * n);
    P->hb.assign(b, b + m);
    P->hc.assign(c, c + n);
    {   // spread of the entries (k_col_stats): badly scaled inputs take the careful path (Engine::make_bt_args)
        unsigned long long bits[2];
        memcpy(bits, &hs[range_off], sizeof(bits));
        double amax, amin;
        memcpy(&amax, &bits[0], 8); memcpy(&amin, &bits[1], 8);
        P->scale_span = (bits[0] != 0 && bits[1] != ~0ull && amin > 0 && amin <= amax) ? amax / amin : 1.0;
    }
    P->hA.clear();
    P->lazy_host = false;
    if ((size_t)m * n <= ((size_t)1 << 25)) {  // up to 256 MB: keep A for the general initial-basis path (equality rows, supplied basis)
        // (the flat call skips the copy of a large A — 67 MB, ~5 ms at the metric size — and fetches it from the device if a rare path asks)
        if (lazy_host && (size_t)m * n > ((size_t)1 << 20)) P->lazy_host = true;
        else {
            P->hA.resize((size_t)m * n);
            for (int i = 0; i < m; i++) memcpy(&P->hA[(size_t)i * n], A + (size_t)i * lda, sizeof(double) * (size_t)n);
        }
    }
    // verifyInputs (simplex.go:404-438): rows first, then columns, first offender decides
    P->verify_status = GOMILP_OK;
    for (int i = 0; i < m && P->verify_status == GOMILP_OK; i++)
        if (!hs[(size_t)3 * n + i]) P->verify_status = (b[i] != 0) ? GOMILP_ERR_INFEASIBLE : GOMILP_ERR_ZERO_ROW;
    for (int j = 0; j < n && P->verify_status == GOMILP_OK; j++)
        if (P->nnz[j] == 0) P->verify_status = (c[j] < 0) ? GOMILP_ERR_UNBOUNDED : GOMILP_ERR_ZERO_COLUMN;
    P->seconds_upload = now_s() - t0;
    { static std::atomic<uint64_t> next_serial(1); P->serial = next_serial.fetch_add(1); }
    for (size_t i = 0; i < problems_.size(); i++)
        if (!problems_[i]) { problems_[i] = std::move(P); return (int64_t)i; }
    problems_.push_back(std::move(P));
    return (int64_t)problems_.size() - 1;
}

const Problem *Engine::problem_ptr(int64_t id) {
    std::lock_guard<std::mutex> g(mu_);
    if (id < 0 || (size_t)id >= problems_.size() || !problems_[id]) return nullptr;
    return problems_[id].get();
}

int64_t Engine::upload_child(int64_t root, int K, const int32_t *var, const double *sign, const double *rhs) {
    std::lock_guard<std::mutex> g(mu_);
    if (root < 0 || (size_t)root >= problems_.size() || !problems_[root]) return -GOMILP_ERR_BAD_SHAPE;
    return upload_child_impl(*problems_[root], root, K, var, sign, rhs);
}

int64_t Engine::upload_child_of(Engine &owner, int64_t root, int K, const int32_t *var, const double *sign, const double *rhs) {
    if (&owner == this) return upload_child(root, K, var, sign, rhs);
    if (owner.device_ != device_) return -GOMILP_ERR_BAD_SHAPE;
    const Problem *R = owner.problem_ptr(root);
    if (!R) return -GOMILP_ERR_BAD_SHAPE;
    std::lock_guard<std::mutex> g(mu_);
    return upload_child_impl(*R, -1, K, var, sign, rhs);   // no root link: the host copy of A (general-basis path) is not reachable
}

int64_t Engine::upload_child_impl(const Problem &R, int64_t root, int K, const int32_t *var, const double *sign, const double *rhs) {
    if (K < 0 || (K > 0 && (!var || !sign || !rhs))) return -GOMILP_ERR_BAD_SHAPE;
    const int m0 = R.m, n0 = R.n, m = m0 + K, n = n0 + K;
    const int ld = (m + 1) & ~1;
    for (int k = 0; k < K; k++) if (var[k] < 0 || var[k] >= n0) return -GOMILP_ERR_BAD_SHAPE;
    if (ld > kLdsWindowLd && lds_window_only_) return -GOMILP_ERR_UNSUPPORTED;
    if (hipSetDevice(device_) != hipSuccess) return -GOMILP_ERR_DEVICE;
    if (!stream_ && hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess) return -GOMILP_ERR_DEVICE;
    const double t0 = now_s();
    const size_t need_at = (size_t)(n + 1) * ld, need_c = (size_t)n + 1, need_b = (size_t)ld;
    std::unique_ptr<Problem> P;
    for (size_t i = 0; i < child_pool_.size(); i++) {
        Problem &c = *child_pool_[i];
        if (c.cap_at >= need_at && c.cap_c >= need_c && c.cap_b >= need_b && c.cap_k >= K) {
            P = std::move(child_pool_[i]);
            child_pool_.erase(child_pool_.begin() + i);
            break;
        }
    }
    auto release = [&](Problem &q) {   // a child owns dAt and ONE block holding b | c | c1 | sign | var
        if (q.dAt) hipFree(q.dAt);
        if (q.db) hipFree(q.db);
        q.dAt = q.dc = q.dc1 = q.db = q.dsign = nullptr; q.dvar = nullptr;
    };
    if (!P) {
        P.reset(new Problem);
        P->is_child = true;
        // some head-room so that deeper children of the same root reuse the slot
        const int kcap = K + 8, mcap = m0 + kcap, ncap = n0 + kcap, ldcap = (mcap + 1) & ~1;
        P->cap_at = (size_t)(ncap + 1) * ldcap; P->cap_c = (size_t)ncap + 1; P->cap_b = (size_t)ldcap; P->cap_k = kcap;
        // b | c | c1 | sign (doubles) | var (ints) in one device block, mirrored by the pinned staging block: one copy
        const size_t blk = P->cap_b + 2 * P->cap_c + 2 * (size_t)P->cap_k + 8;
        if (ld > kLdsWindowLd && !device_fits((P->cap_at + blk) * sizeof(double))) return -GOMILP_ERR_UNSUPPORTED;
        if (dmalloc(&P->dAt, P->cap_at) != hipSuccess || dmalloc(&P->db, blk) != hipSuccess) {
            release(*P);
            return -GOMILP_ERR_DEVICE;
        }
        P->dc = P->db + P->cap_b; P->dc1 = P->dc + P->cap_c; P->dsign = P->dc1 + P->cap_c;
        P->dvar = reinterpret_cast<int32_t *>(P->dsign + P->cap_k);
    }
    P->m = m; P->n = n; P->ld = ld;
    auto fail = [&](int code) -> int64_t { release(*P); return -code; };
#define UP_TRY(expr) do { if ((expr) != hipSuccess) return fail(GOMILP_ERR_DEVICE); } while (0)
    P->hc = R.hc; P->hc.resize(n, 0.0);        // c' = [c, 0]   (subproblem.go:110-114)
    P->hb = R.hb; P->hb.insert(P->hb.end(), rhs, rhs + K);  // b' = [b; h]  (:117-119)
    // one pinned staging block with the layout of the child's device block (capacity offsets)
    Work &w = *w_;
    const size_t blk_bytes = (P->cap_b + 2 * P->cap_c + (size_t)P->cap_k) * sizeof(double) + (size_t)P->cap_k * sizeof(int32_t);
    if (w.child_stage_cap < blk_bytes + 64) {
        if (w.child_stage) hipHostFree(w.child_stage);
        w.child_stage_cap = 2 * (blk_bytes + 64);
        UP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w.child_stage), w.child_stage_cap, hipHostMallocDefault));
    }
    double *sb = reinterpret_cast<double *>(w.child_stage);
    double *sc = sb + P->cap_b, *sc1 = sc + P->cap_c, *ss = sc1 + P->cap_c;
    int32_t *sv = reinterpret_cast<int32_t *>(ss + P->cap_k);
    for (int i = 0; i < ld; i++) sb[i] = i < m ? P->hb[i] : 0.0;
    for (int j = 0; j <= n; j++) { sc[j] = j < n ? P->hc[j] : 0.0; sc1[j] = j == n ? 1.0 : 0.0; }
    for (int k = 0; k < K; k++) { ss[k] = sign[k]; sv[k] = var[k]; }
    UP_TRY(hipMemcpyAsync(P->db, sb, blk_bytes, hipMemcpyHostToDevice, stream_));
    launch_child_assemble(R.dAt, R.ld, m0, n0, P->dAt, ld, K, P->dvar, P->dsign, stream_);
    UP_TRY(sync_stream());  // the staging block is reused by the next child
    UP_TRY(hipGetLastError());
#undef UP_TRY
    // column statistics follow from the root's: a branched column gains one entry per constraint on it
    P->nnz = R.nnz; P->lastrow = R.lastrow; P->allone = R.allone;
    P->nnz.resize(n); P->lastrow.resize(n); P->allone.resize(n);
    for (int k = 0; k < K; k++) {
        P->nnz[var[k]] += 1; P->lastrow[var[k]] = m0 + k;
        if (sign[k] != 1.0) P->allone[var[k]] = 0;
        P->nnz[n0 + k] = 1; P->lastrow[n0 + k] = m0 + k; P->allone[n0 + k] = 1;
    }
    // verifyInputs of the child (simplex.go:404-438): branch rows and their slack columns are never empty, so a row verdict of
    // the root stands; a COLUMN verdict is re-derived, because a branch row can fill a column that was empty in the root
    P->verify_status = R.verify_status;
    if (R.verify_status == GOMILP_ERR_ZERO_COLUMN || R.verify_status == GOMILP_ERR_UNBOUNDED) {
        P->verify_status = GOMILP_OK;
        for (int j = 0; j < n && P->verify_status == GOMILP_OK; j++)
            if (P->nnz[j] == 0) P->verify_status = (P->hc[j] < 0) ? GOMILP_ERR_UNBOUNDED : GOMILP_ERR_ZERO_COLUMN;
    }
    // the host copy of [[A0, 0], [G#, I]] is only needed when a solve starts from a non-slack basis: built on demand
    P->hA.clear();
    P->scale_span = R.scale_span;
    P->root = root;
    P->root_ptr = &R;   // (a root resident in another engine of the pool: `root` is -1, the owner keeps it alive)
    P->kvar.assign(var, var + K);
    P->ksign.assign(sign, sign + K);
    P->seconds_upload = now_s() - t0;
    for (size_t i = 0; i < problems_.size(); i++)
        if (!problems_[i]) { problems_[i] = std::move(P); return (int64_t)i; }
    problems_.push_back(std::move(P));
    return (int64_t)problems_.size() - 1;
}

int Engine::free_problem(int64_t id) {
    std::lock_guard<std::mutex> g(mu_);
    if (id < 0 || (size_t)id >= problems_.size() || !problems_[id]) return GOMILP_ERR_BAD_SHAPE;
    hipSetDevice(device_);
    drop_kept(id);
    if (problems_[id]->is_child) {  // keep the buffers for the next child (no hipFree: it synchronises the device)
        child_pool_.push_back(std::move(problems_[id]));
        problems_[id].reset();
        return GOMILP_OK;
    }
    // a root's buffers are kept for the next upload of a fitting shape (at most 4: two shapes in rotation + slack)
    problems_[id]->hA.clear(); problems_[id]->hA.shrink_to_fit();
    root_pool_.push_back(std::move(problems_[id]));
    problems_[id].reset();
    while (root_pool_.size() > 4) {
        Problem &P = *root_pool_.front();
        hipFree(P.dAt); hipFree(P.dc); hipFree(P.dc1); hipFree(P.db);
        root_pool_.erase(root_pool_.begin());
    }
    return GOMILP_OK;
}

LPArgs Engine::make_args(const Problem &P, int phase, double tol, int nn, const double *cost) {
    Work &w = *w_;
    LPArgs a;
    memset(&a, 0, sizeof(a));
    a.m = P.m; a.ld = P.ld; a.nn = nn; a.phase = phase; a.tol = tol;
    a.At = P.dAt; a.cost = cost; a.b = P.db;
    a.binv_cur = w.binv[cur_]; a.binv_next = w.binv[cur_ ^ 1];
    a.xb = w.xb; a.y = w.yb[ycur_]; a.dvec = w.dvec; a.move = w.move; a.rvec = w.rvec;
    a.basic = w.basic; a.nonbasic = w.nonbasic;
    a.pk_price = w.pk_price; a.pi_price = w.pi_price; a.pk_ratio = w.pk_ratio; a.pi_ratio = w.pi_ratio;
    a.pv_price = w.pv_price; a.pd_ratio = w.pd_ratio; a.pb_ratio = w.pb_ratio;
    a.st = w.st;
    a.trace = (trace_on_ || shadow_trace_) ? w.trace : nullptr;
    a.trace_cap = w.trace_cap;
    a.row_chunk2 = row_chunk2(P);
    a.guard = plan_.guard;
    return a;
}

int Engine::row_chunk2(const Problem &P) const {
    if (row_chunk_ > 0) return (int)(row_chunk_ / 2);
    return P.ld > kLdsWindowLd ? kAutoRowChunk / 2 : 0;
}

bool Engine::device_fits(size_t bytes) {
    size_t avail = 0, total = 0;
    if (hipSetDevice(device_) != hipSuccess || hipMemGetInfo(&avail, &total) != hipSuccess) return false;
    return bytes + bytes / 16 + ((size_t)256 << 20) <= avail;   // (head-room: allocation granularity, the runtime's own buffers)
}

// What ensure_work will allocate for P (its head-room formula), beyond what is held already: a solve beyond the LDS window (the
// three-kernel revised simplex, no tableau) is refused up front instead of failing an allocation halfway.  (Buffers that a
// re-allocation releases are not counted as free: conservative.)
bool Engine::large_solve_fits(const Problem &P) {
    const Work &w = *w_;
    const int m = P.m, ncols = P.n + 1;
    size_t dbl = 0;
    if (!(m <= w.cap_m && ncols <= w.cap_cols)) {
        const int nmi = std::max(m + 32 + m / 16, w.cap_m), nci = std::max(ncols + 64 + ncols / 16, w.cap_cols);
        const size_t nm = (size_t)nmi, nc = (size_t)nci, nld = (size_t)std::max((nmi + 1) & ~1, w.cap_ld);
        dbl += 4 * nm * nld + 512 + 200 * nld + 4 * nc + 8 * nm;   // B^-1 x 2, W, Wd; x_B, y, d, move, y scratch, LU panels; r; index lists
    }
    return dbl == 0 || device_fits(dbl * sizeof(double));
}

void Engine::sync_state_to_device() {
    // a snapshot through the staging ring: the host copy may be rewritten before the stream reaches this upload
    stage_upload(w_->st, w_->st_host, sizeof(DevState));
}

int Engine::refresh_xb_y(const Problem &P, const double *cost) {
    Work &w = *w_;
    launch_matvec_rows(w.binv[cur_], P.ld, P.m, P.db, w.xb, stream_, row_chunk2(P));
    launch_y_from_binv(w.binv[cur_], P.ld, P.m, cost, w.basic, w.yscratch, w.yb[ycur_], stream_);
    launches_ += 3;
    return GOMILP_OK;
}

// host copy of A for the general-basis path; children derive it from their root (subproblem.go:81-139)
bool Engine::ensure_host_A(const Problem &P) {
    if (!P.hA.empty()) return true;
    if (!P.is_child && P.lazy_host) {   // flat call: the copy was skipped at upload, At (column-major, resident) has the same numbers
        const int m = P.m, n = P.n;
        std::vector<double> at((size_t)n * P.ld);
        if (hipMemcpyAsync(at.data(), P.dAt, at.size() * sizeof(double), hipMemcpyDeviceToHost, stream_) != hipSuccess || sync_stream() != hipSuccess) return false;
        P.hA.resize((size_t)m * n);
        for (int j = 0; j < n; j++) for (int i = 0; i < m; i++) P.hA[(size_t)i * n + j] = at[(size_t)j * P.ld + i];
        return true;
    }
    if (!P.is_child || !P.root_ptr) return false;
    const Problem &R = *P.root_ptr;
    // the root of a pool child may live in another worker's engine (gomilp_pool_add_root keeps extra roots in worker 0): its host
    // copy was made at upload (roots are never built lazily), read in place
    if (P.root >= 0 ? !ensure_host_A(R) : R.hA.empty()) return false;
    const int m = P.m, n = P.n, m0 = R.m, n0 = R.n, K = (int)P.kvar.size();
    if ((size_t)m * n > ((size_t)1 << 25)) return false;
    P.hA.assign((size_t)m * n, 0.0);
    for (int i = 0; i < m0; i++) memcpy(&P.hA[(size_t)i * n], &R.hA[(size_t)i * n0], sizeof(double) * (size_t)n0);
    for (int k = 0; k < K; k++) { P.hA[(size_t)(m0 + k) * n + P.kvar[k]] = P.ksign[k]; P.hA[(size_t)(m0 + k) * n + n0 + k] = 1.0; }
    return true;
}

// Small host -> device upload from pageable / short-lived memory without a stream sync of its own: the copy is enqueued
// from a slot of a pinned ring.  A slot may be rewritten only after the stream has been fully synchronised since its
// last use: sync_stream() — the engine's only way to wait for the stream — resets the count, and the ring forces a
// sync itself when it would wrap around without one (no per-upload event: with many worker streams the queue
// packets, not the host, are the bottleneck).
hipError_t Engine::sync_stream() {
    const hipError_t e = hipStreamSynchronize(stream_);
    w_->stage_inflight = 0;
    return e;
}

int Engine::stage_upload(void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return GOMILP_OK;
    Work &w = *w_;
    if (w.stage_inflight >= Work::kStageSlots) HIP_TRY(sync_stream());
    const int slot = w.stage_next;
    if (w.stage_cap[slot] < bytes) {
        // slots are sized once per work-buffer generation (ensure_work); an oversized request takes the plain path
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream_));
        HIP_TRY(sync_stream());
        return GOMILP_OK;
    }
    w.stage_next = (slot + 1) % Work::kStageSlots;
    w.stage_inflight++;
    memcpy(w.stage_buf[slot], src, bytes);
    HIP_TRY(hipMemcpyAsync(dst, w.stage_buf[slot], bytes, hipMemcpyHostToDevice, stream_));
    return GOMILP_OK;
}

int Engine::upload_index_lists(const std::vector<int32_t> &basic, const std::vector<int32_t> &nonbasic) {
    Work &w = *w_;
    if (!basic.empty() && !nonbasic.empty()) {
        // the two lists share one device block (basic at 0, nonbasic at cap_m): one copy, one queue packet
        const size_t gap = (size_t)(w.nonbasic - w.basic);
        std::vector<int32_t> both(gap + nonbasic.size(), 0);
        memcpy(both.data(), basic.data(), basic.size() * sizeof(int32_t));
        memcpy(both.data() + gap, nonbasic.data(), nonbasic.size() * sizeof(int32_t));
        return stage_upload(w.basic, both.data(), both.size() * sizeof(int32_t));
    }
    int rc = stage_upload(w.basic, basic.data(), basic.size() * sizeof(int32_t));
    if (rc != GOMILP_OK) return rc;
    return stage_upload(w.nonbasic, nonbasic.data(), nonbasic.size() * sizeof(int32_t));
}

// ------------------------------------------------------------------------------------------------
// replaceBland (simplex.go:347-383), host-driven: candidates are tried one at a time with the FTRAN
// kernel.  Deviation: the `mat.Cond(abTmp,1) < 1e16` guard of :377 is replaced by the
// pivot-magnitude guard |d_replace| >= dRoundTol that move[replace] < +Inf already implies.
// ------------------------------------------------------------------------------------------------
int Engine::host_bland(const Problem &P, LPArgs &a, gomilp_lp_stats *st) {
    Work &w = *w_;
    const int m = P.m, nn = a.nn;
    std::vector<double> r(nn), move(m);
    HIP_TRY(hipMemcpyAsync(w.h_vec, w.rvec, (size_t)nn * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(sync_stream());
    for (int j = 0; j < nn; j++) { r[j] = w.h_vec[j]; if (fabs(r[j]) < 1e-13) r[j] = 0; }  // rRoundTol, :252-256
    for (int i = 0; i < nn; i++) {
        if (r[i] > -1e-14) continue;  // blandNegTol, :352
        w.st_host->done = 0; w.st_host->status = ST_RUNNING;
        sync_state_to_device();
        launch_ftran(a, 0, i, -1, stream_);
        launches_++;
        HIP_TRY(hipMemcpyAsync(w.h_vec, w.move, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(sync_stream());
        for (int k = 0; k < m; k++) move[k] = w.h_vec[k];
        int64_t replace = min_idx(move.data(), m);
        if (move[replace] == std::numeric_limits<double>::infinity()) return GOMILP_ERR_UNBOUNDED;  // computeMove :328
        if (!(fabs(move[replace]) > 1e-12)) {  // blandZeroTol, :362
            replace = -1;
            for (int rp = 0; rp < m; rp++)
                if (!(move[rp] > 1e-12)) { replace = rp; break; }  // :368-379 (cond guard: see header comment)
            if (replace < 0) continue;
        }
        launch_update(a, 0, (int)replace, 0, 1, stream_);
        launches_++;
        cur_ ^= 1;
        if (st) st->bland_steps++;
        // pivots counter is advanced on device by the update kernel
        return GOMILP_OK;
    }
    return GOMILP_ERR_BLAND;
}

// ------------------------------------------------------------------------------------------------
// Pivot loop (simplex.go:233-293): chunks of kernel launches; the kernels stop themselves through
// DevState::done, the host looks at the state after each chunk.
// returns GOMILP_OK when the loop ended at an optimum, else the reference's error class.
// ------------------------------------------------------------------------------------------------
void Engine::account_samples(gomilp_lp_stats *st, const std::vector<int64_t> &sample_t, int64_t executed, int nk) {
    // nk kernels per pivot, each bracketed by its own (start, stop) event pair attached to the dispatch
    if (!st) return;
    Work &w = *w_;
    for (size_t s = 0; s < sample_t.size(); s++) {
        if (sample_t[s] >= executed) break;  // kernels already stopped by DevState::done are not samples
        float ms[3] = {0, 0, 0};
        bool ok = true;
        for (int k = 0; k < nk; k++)
            ok = ok && hipEventElapsedTime(&ms[k], w.sample_ev[(s * 3 + k) * 2], w.sample_ev[(s * 3 + k) * 2 + 1]) == hipSuccess;
        if (!ok) continue;
        if (nk == 3) {
            st->pivot_kernel_seconds[0] += ms[0] * 1e-3; st->pivot_kernel_seconds[1] += ms[1] * 1e-3;
            st->pivot_kernel_seconds[2] += ms[2] * 1e-3;
        } else {
            st->pivot_kernel_seconds[0] += ms[0] * 1e-3; st->pivot_kernel_seconds[2] += ms[1] * 1e-3;
        }
        st->pivot_kernel_seconds[3] += 1.0;  // number of sampled pivots
    }
}

int Engine::run_loop(const Problem &P, int phase, double tol, int nn, const double *cost, gomilp_lp_stats *st) {
    if (plan_.pipeline == 1) return run_loop_fused(P, phase, tol, nn, cost, st);   // (no guard there: general starts stay here)
    Work &w = *w_;
    DevState &hs = *w.st_host;
    hs.done = 0; hs.status = ST_RUNNING; hs.pivots = 0; hs.q = hs.p = -1; hs.rq = hs.dp = hs.mv = 0;
    hs.max_pivots = bt_knobs_.max_pivots;
    hs.lu_singular = 0;
    sync_state_to_device();  // trace_len is cumulative over the solve
    int64_t since_refresh = 0;
    HIP_TRY(hipEventRecord(w.ev[0], stream_));
    int ret = GOMILP_OK;
    const bool sampling = sample_events_ > 0;
    for (;;) {
        const int64_t before = hs.pivots;
        std::vector<int64_t> sample_t;  // chunk-local pivot index of every sampled pivot
        for (int64_t t = 0; t < bt_knobs_.chunk; t++) {
            LPArgs a = make_args(P, phase, tol, nn, cost);
            a.binv_cur = w.binv[(cur_ + t) & 1];
            a.binv_next = w.binv[(cur_ + t + 1) & 1];
            const bool sample = sampling && ((before + t) % sample_events_ == 0);
            hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            if (sample) {
                const size_t e0 = sample_t.size() * 6;
                while (w.sample_ev.size() < e0 + 6) { hipEvent_t ev; HIP_TRY(hipEventCreate(&ev)); w.sample_ev.push_back(ev); }
                for (int k = 0; k < 6; k++) e[k] = w.sample_ev[e0 + k];
                sample_t.push_back(t);
            }
            const int gp = launch_price(a, stream_, e[0], e[1]);
            const int gr = launch_ftran(a, gp, -1, -1, stream_, e[2], e[3]);
            launch_update(a, gr, -1, 0, 0, stream_, e[4], e[5]);
            launches_ += 3;
        }
        HIP_TRY(hipMemcpyAsync(w.st_host, w.st, sizeof(DevState), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(sync_stream());
        HIP_TRY(hipGetLastError());
        const int64_t executed = hs.pivots - before;
        cur_ = (int)((cur_ + executed) & 1);
        since_refresh += executed;
        account_samples(st, sample_t, executed, 3);
        if (!hs.done) {
            if (refresh_ > 0 && since_refresh >= refresh_) {
                refresh_xb_y(P, cost);
                since_refresh = 0;
                if (st) st->refreshes++;
            }
            continue;
        }
        if (hs.status == ST_OPTIMAL) break;
        if (hs.status == ST_UNBOUNDED) { ret = GOMILP_ERR_UNBOUNDED; break; }
        if (hs.status == ST_MAX_PIVOTS) { ret = GOMILP_ERR_UNSUPPORTED; break; }
        if (hs.status == ST_NEED_BLAND) {
            LPArgs a = make_args(P, phase, tol, nn, cost);
            int rc = host_bland(P, a, st);
            if (rc != GOMILP_OK) { ret = rc; break; }
            // resume: the update kernel of the Bland step has been enqueued; read the state back after it
            HIP_TRY(hipMemcpyAsync(w.st_host, w.st, sizeof(DevState), hipMemcpyDeviceToHost, stream_));
            HIP_TRY(sync_stream());
            hs.done = 0; hs.status = ST_RUNNING;
            sync_state_to_device();
            continue;
        }
        if (hs.status == ST_NEED_EXACT) {
            // The guard instances stopped in front of a decision that the rounding noise of the reference's fresh solves takes
            // (LPArgs::guard): the reference's iteration on fresh gonum-order solves decides it (exact_iter, as the blocked tableau's
            // exact step does).  Its y, r and x_B replace the running ones; the pivot it decides runs as a forced pivot on the running
            // B^-1, whose column a_q is checked against the fresh one first (re-inverted beyond 1e-6 of the column's size, up to 1024
            // rows: the tableau's rule).
            const DevState keep = hs;   // (the final solve keeps its singular flag in the same block and reads it back)
            auto check = [&](int, int var, const std::vector<int32_t> &basic, const std::vector<double> &dsol) -> int {
                if (P.m > 1024) return GOMILP_OK;
                launch_matvec_rows(w.binv[cur_], P.ld, P.m, P.dAt + (size_t)var * P.ld, w.dvec, stream_, row_chunk2(P));
                launches_++;
                bool rebuilt = false;
                return exact_column_check(P, basic, dsol, w.dvec, w.binv[cur_], &rebuilt, st);
            };
            int fq = -1, fp = -1;
            const int verdict = exact_iter(P, phase, tol, nn, w.yb[ycur_], w.rvec, nn, check, &fq, &fp, st);
            hs = keep;
            hs.done = 0; hs.status = ST_RUNNING; hs.lu_singular = 0;
            if (verdict < 0) {
                ret = -verdict;
                // an exactly singular basis is the reference's mat.Condition (gonum's ErrSingular is Condition(+Inf): simplex.go:236-239,
                // 289-292 leave the loop with it) — past the reference's own Condition exit, where modes 1 / 2 may go on
                double k1 = 0, kinf = 0;
                if (ret == GOMILP_ERR_LINSOLVE && cond_fresh(P, nullptr, &k1, &kinf) == GOMILP_OK && !(k1 < 1e16)) ret = GOMILP_ERR_CONDITION;
                // strict: the pivot into this basis was decided in the previous exact step, and a singular basis keeps that step's fresh
                // x_B (the reference's receiver keeps its values when Det() == 0, simplex.go:289-292; the epilogue returns it)
                if (ret == GOMILP_ERR_CONDITION && plan_.guard == std::numeric_limits<double>::infinity() && exact_xb_.size() == (size_t)P.m) {
                    const int rc = upload_padded(w.xb, exact_xb_, P.ld);
                    if (rc != GOMILP_OK) ret = rc;
                }
                break;
            }
            if (verdict == 1) { hs.done = 1; hs.status = ST_OPTIMAL; break; }
            if (verdict == 2) { ret = GOMILP_ERR_UNBOUNDED; break; }
            if (verdict != 0 && verdict != 3) { ret = verdict; break; }   // (a runtime failure inside)
            sync_state_to_device();
            LPArgs a = make_args(P, phase, tol, nn, cost);
            if (verdict == 3) {   // (no host copy of A for the kappa_1 test: the host Bland branch on the fresh r / x_B)
                const int rc = host_bland(P, a, st);
                if (rc != GOMILP_OK) { ret = rc; break; }
            } else {
                // st->q / st->rq come from the fresh r (pick_entering reads rvec[q]): commit_pivot updates y with them
                launch_ftran(a, 0, fq, -1, stream_);
                launch_update(a, 0, fp, 0, 0, stream_);
                launches_ += 2;
                cur_ ^= 1;
            }
            HIP_TRY(hipMemcpyAsync(w.st_host, w.st, sizeof(DevState), hipMemcpyDeviceToHost, stream_));
            HIP_TRY(sync_stream());
            hs.done = 0; hs.status = ST_RUNNING;
            sync_state_to_device();
            continue;
        }
        ret = GOMILP_ERR_DEVICE;
        break;
    }
    HIP_TRY(hipEventRecord(w.ev[1], stream_));
    HIP_TRY(hipEventSynchronize(w.ev[1]));
    float ms = 0;
    hipEventElapsedTime(&ms, w.ev[0], w.ev[1]);
    if (st) {
        st->seconds_pivot_loop += ms * 1e-3;
        if (phase == 1) st->pivots_phase1 += hs.pivots; else st->pivots_phase2 += hs.pivots;
    }
    return ret;
}

// Fused two-kernel pipeline (fused_kernels.hip).  Within a segment (since the last restart) launch index t:
//   K_A(t) reads  y = Y[(y0+t-1)&1], row p from B[(c0+t-1)&1]; writes Y[(y0+t)&1]      (t >= 1; t = 0: reads Y[y0])
//   K_B(t) reads  B[(c0+t-1)&1], writes B[(c0+t)&1]                                     (t >= 1; t = 0: reads B[c0])
// After T committed pivots the current buffers are B[(c0+T)&1], Y[(y0+T)&1] whatever stopped the loop.
int Engine::run_loop_fused(const Problem &P, int phase, double tol, int nn, const double *cost, gomilp_lp_stats *st) {
    Work &w = *w_;
    DevState &hs = *w.st_host;
    hs.done = 0; hs.status = ST_RUNNING; hs.pivots = 0; hs.q = hs.p = -1; hs.rq = hs.dp = hs.mv = 0;
    hs.max_pivots = 0;
    hs.lu_singular = 0;
    hs.theta = 0; hs.ent_cur = hs.ent_prev = hs.lea = -1;
    sync_state_to_device();
    int64_t since_refresh = 0;
    HIP_TRY(hipEventRecord(w.ev[0], stream_));
    int ret = GOMILP_OK;
    const bool sampling = sample_events_ > 0;
    int c0 = cur_, y0 = ycur_;
    int64_t seg_start = 0, tseg = 0;  // pivots committed at segment start, launch index inside the segment
    for (;;) {
        const int64_t before = hs.pivots;
        std::vector<int64_t> sample_t;
        int64_t nlaunch = bt_knobs_.chunk;
        if (bt_knobs_.max_pivots > 0) nlaunch = std::min<int64_t>(nlaunch, std::max<int64_t>(1, bt_knobs_.max_pivots - hs.pivots + 1));
        for (int64_t t = 0; t < nlaunch; t++, tseg++) {
            const int pending = tseg > 0;
            LPArgs a = make_args(P, phase, tol, nn, cost);
            const int prev = (int)((tseg + 1) & 1);  // (x + tseg - 1) & 1 == (x + tseg + 1) & 1
            a.binv_cur = w.binv[pending ? ((c0 + prev) & 1) : c0];
            a.binv_next = w.binv[(c0 + tseg) & 1];
            const double *y_in = w.yb[pending ? ((y0 + prev) & 1) : y0];
            double *y_out = w.yb[(y0 + tseg) & 1];
            const bool sample = sampling && ((before + t) % sample_events_ == 0) && pending;
            hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
            if (sample) {
                const size_t e0 = sample_t.size() * 6;
                while (w.sample_ev.size() < e0 + 6) { hipEvent_t ev; HIP_TRY(hipEventCreate(&ev)); w.sample_ev.push_back(ev); }
                for (int k = 0; k < 4; k++) e[k] = w.sample_ev[e0 + k];
                sample_t.push_back(t);
            }
            const int gr = grid_ratio_;
            const int gp = launch_price_fused(a, y_in, y_out, pending, gr, stream_, e[0], e[1]);
            grid_ratio_ = launch_update_ftran_fused(a, pending, gp, stream_, e[2], e[3]);
            launches_ += 2;
        }
        HIP_TRY(hipMemcpyAsync(w.st_host, w.st, sizeof(DevState), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(sync_stream());
        HIP_TRY(hipGetLastError());
        const int64_t executed = hs.pivots - before;
        since_refresh += executed;
        // a sampled launch index t measured K_A(t) (which commits pivot t-1) and K_B(t): valid while t <= executed
        account_samples(st, sample_t, executed + 1, 2);
        const int64_t T = hs.pivots - seg_start;
        if (!hs.done) {
            if (bt_knobs_.max_pivots > 0 && hs.pivots >= bt_knobs_.max_pivots) { cur_ = (c0 + T) & 1; ycur_ = (y0 + T) & 1; ret = GOMILP_ERR_UNSUPPORTED; break; }
            if (refresh_ > 0 && since_refresh >= refresh_) {
                cur_ = (int)((c0 + T) & 1); ycur_ = (int)((y0 + T) & 1);
                refresh_xb_y(P, cost);
                since_refresh = 0;
                if (st) st->refreshes++;
            }
            continue;
        }
        cur_ = (int)((c0 + T) & 1);
        ycur_ = (int)((y0 + T) & 1);
        if (hs.status == ST_OPTIMAL) break;
        if (hs.status == ST_UNBOUNDED) { ret = GOMILP_ERR_UNBOUNDED; break; }
        if (hs.status == ST_NEED_BLAND) {
            // the degenerate pivot has not been committed: B^-1, x_B, y and the index lists are those of the
            // current basis; the Bland step runs on the unfused kernels, then a new fused segment starts
            LPArgs a = make_args(P, phase, tol, nn, cost);
            int rc = host_bland(P, a, st);
            if (rc != GOMILP_OK) { ret = rc; break; }
            HIP_TRY(hipMemcpyAsync(w.st_host, w.st, sizeof(DevState), hipMemcpyDeviceToHost, stream_));
            HIP_TRY(sync_stream());
            hs.done = 0; hs.status = ST_RUNNING;
            sync_state_to_device();
            c0 = cur_; y0 = ycur_; seg_start = hs.pivots; tseg = 0;
            continue;
        }
        ret = GOMILP_ERR_DEVICE;
        break;
    }
    HIP_TRY(hipEventRecord(w.ev[1], stream_));
    HIP_TRY(hipEventSynchronize(w.ev[1]));
    float ms = 0;
    hipEventElapsedTime(&ms, w.ev[0], w.ev[1]);
    if (st) {
        st->seconds_pivot_loop += ms * 1e-3;
        if (phase == 1) st->pivots_phase1 += hs.pivots; else st->pivots_phase2 += hs.pivots;
    }
    return ret;
}

// ------------------------------------------------------------------------------------------------
// simplex() — simplex.go:93-302
// ------------------------------------------------------------------------------------------------
int Engine::solve(int64_t id, double tol, const int64_t *initial_basic, double *opt_f, double *opt_x, int32_t *has_x,
                  int64_t *basis_out, gomilp_lp_stats *stats) {
    std::lock_guard<std::mutex> g(mu_);
    drop_kept(id);   // a kept state belongs to the solve that made it
    return solve_cold_locked(id, tol, initial_basic, opt_f, opt_x, has_x, basis_out, stats);
}

int Engine::solve_cold_locked(int64_t id, double tol, const int64_t *initial_basic, double *opt_f, double *opt_x, int32_t *has_x,
                              int64_t *basis_out, gomilp_lp_stats *stats) {
    xchg_timeout_ = false;
    int rc = solve_locked(id, tol, initial_basic, opt_f, opt_x, has_x, basis_out, stats);
    if (rc == GOMILP_ERR_DEVICE && xchg_timeout_ && bt_knobs_.bt_groups >= 0) {
        // The workgroups of the multi-workgroup block kernel wait for each other; when one of them was not resident within the
        // bounded wait (a crowded device) the launch gives up.  That says nothing about the problem: once more on the
        // single-workgroup kernels, which depend on nobody.
        const int64_t keep = bt_knobs_.bt_groups;
        bt_knobs_.bt_groups = -1;
        rc = solve_locked(id, tol, initial_basic, opt_f, opt_x, has_x, basis_out, stats);
        bt_knobs_.bt_groups = keep;
        if (stats) stats->device_retries = 1;
    }
    return rc;
}

void Engine::open_stats() {
    launches_ = 0;
    fs_device_ = fs_host_ = 0; lu_look_fault_ = 0;
    last_trace_.clear();
    last_trace_total_ = 0;
}

int Engine::close_stats(gomilp_lp_stats *st, double t0, int code) {
    st->seconds_total = now_s() - t0; st->kernel_launches = launches_;
    st->seconds_final_device = fs_device_; st->seconds_final_host = fs_host_;
    st->lu_dense_steps = lu_dense_; st->lu_rounds = lu_rounds_;
    if (lu_look_fault_) st->device_retries = lu_look_fault_;   // (the final solve was repeated with the plain LU schedule)
    return code;
}

// The stages of a solve: validate, the starting basis (scan_start), the plan, x_B of a searched basis (search_start), set-up
// (upload_start), the phase loops of the plan's pipeline, solve_tail.
int Engine::solve_locked(int64_t id, double tol, const int64_t *initial_basic, double *opt_f, double *opt_x, int32_t *has_x,
                         int64_t *basis_out, gomilp_lp_stats *stats) {
    const double t0 = now_s();
    gomilp_lp_stats local;
    gomilp_lp_stats *st = stats ? stats : &local;
    memset(st, 0, sizeof(*st));
    st->device_id = device_;
    if (has_x) *has_x = 0;
    if (opt_f) *opt_f = std::numeric_limits<double>::quiet_NaN();
    if (id < 0 || (size_t)id >= problems_.size() || !problems_[id] || !opt_f || !opt_x || !has_x) return GOMILP_ERR_BAD_SHAPE;
    const Problem &P = *problems_[id];
    st->seconds_upload = P.seconds_upload;
    auto finish = [&](int code) { return close_stats(st, t0, code); };
    open_stats();
    if (P.verify_status != GOMILP_OK) {  // simplex.go:94-100
        if (P.verify_status == GOMILP_ERR_UNBOUNDED) *opt_f = -std::numeric_limits<double>::infinity();
        return finish(P.verify_status);
    }
    const int m = P.m, n = P.n;
    // beyond the LDS window (chunked staging): slack-basis starts only, and only what fits the free device memory
    if (P.ld > kLdsWindowLd && (initial_basic || m >= n || !large_solve_fits(P))) return finish(GOMILP_ERR_UNSUPPORTED);
    int rc = ensure_work(m, n + 1);
    if (rc != GOMILP_OK) return finish(rc);
    w_->st_host->trace_len = 0;
    if (m == n) return finish(solve_square(P, opt_f, opt_x, has_x, st));
    if (m > n) return finish(GOMILP_ERR_SINGULAR);  // findLinearlyIndependent cannot reach m columns (:495-497)

    Start s;
    if ((rc = scan_start(P, initial_basic, s)) != GOMILP_OK) return finish(rc);
    plan_ = SolvePlan::make(m, n, P.ld, s.slack ? SolvePlan::Slack : initial_basic ? SolvePlan::Supplied : SolvePlan::Searched, P.scale_span, knobs_);
    if (plan_.status != GOMILP_OK || (plan_.needs_host_A && !ensure_host_A(P))) return finish(GOMILP_ERR_UNSUPPORTED);
    gen_binv_dev_ = false;
    exact_xb_.clear();
    if (!s.slack && (rc = search_start(P, initial_basic != nullptr, s)) != GOMILP_OK) return finish(rc);
    // small bases starting feasible: record the pivots for the host replay of the reference's condition guards
    // (every pipeline: until round 5 the revised-simplex pipelines — shapes with n - m >= 2m, wide small LPs among them — went without the
    // replay, which is what the one status difference of the badly scaled family, seed 1079, a 2 x 6 LP, came from)
    shadow_trace_ = plan_.replay_if_feasible && s.feasible && ensure_host_A(P);
    const std::vector<int32_t> basic_start = s.basic;
    if ((rc = upload_start(P, s)) != GOMILP_OK) return finish(rc);
    st->pipeline = plan_.pipeline;
    int loop_rc = GOMILP_OK;
    rc = plan_.use_tab ? solve_tableau(P, tol, s, st, &loop_rc) : solve_revised(P, tol, s, st, &loop_rc);
    if (rc != GOMILP_OK) return finish(rc);
    return finish(solve_tail(P, id, loop_rc, s.basic, s.xb, basic_start, s.slack ? &s.rho : nullptr, opt_f, opt_x, has_x, basis_out, st));
}

int Engine::solve_square(const Problem &P, double *opt_f, double *opt_x, int32_t *has_x, gomilp_lp_stats *st) {  // simplex.go:103-119: exactly constrained, one linear solve
    const int n = P.n;
    std::vector<int32_t> ident(n);
    for (int j = 0; j < n; j++) ident[j] = j;
    int rc = upload_index_lists(ident, {});
    if (rc != GOMILP_OK) return rc;
    std::vector<double> xb_exact;
    bool singular = false;
    const double t1 = now_s();
    if ((rc = final_solve(P, xb_exact, &singular)) != GOMILP_OK) return rc;
    st->seconds_final_solve = now_s() - t1;
    if (singular) return GOMILP_ERR_SINGULAR;
    if (knobs_.cond_guard && !P.hA.empty() && n <= 1024) {   // cond > 1e16 is a Condition too: lp.ErrSingular (simplex.go:109-112)
        st->cond_fallbacks++;
        const double kinf = general_cond_inf(P.hA, n);
        if (kinf > 1e16 || kinf != kinf) return GOMILP_ERR_SINGULAR;
    }
    for (int j = 0; j < n; j++)
        if (xb_exact[j] < 0) return GOMILP_ERR_INFEASIBLE;
    *opt_f = dot_unitary(xb_exact.data(), P.hc.data(), n);
    memcpy(opt_x, xb_exact.data(), sizeof(double) * (size_t)n);
    *has_x = 1;
    return GOMILP_OK;
}

// findLinearlyIndependent (simplex.go:611-637), unit-column fast path: the descending scan meets m distinct unit vectors (always true
// for GoMILP's [.. | I] standard forms, subproblem.go:81-139); cond == 1 there, ab = permutation, xb = ab^-1 b exactly
// (initializeFromBasic, simplex.go:447-471).  A supplied basis (simplex.go:147-160; GoMILP itself always passes nil): the caller hands
// over m entries; an index out of range panics in extractColumns, a singular or infeasible set in initializeFromBasic
int Engine::scan_start(const Problem &P, const int64_t *initial_basic, Start &s) {
    const int m = P.m, n = P.n;
    s.basic.assign(m, 0); s.rho.assign(m, 0); s.xb.assign(m, 0.0);
    if (initial_basic) {
        s.slack = false;
        for (int pos = 0; pos < m; pos++) {
            const int64_t j = initial_basic[pos];
            if (j < 0 || j >= n) return GOMILP_ERR_PANIC;
            s.basic[pos] = (int32_t)j;
        }
        return GOMILP_OK;
    }
    std::vector<char> used(m, 0);
    for (int pos = 0; pos < m; pos++) {
        const int j = n - 1 - pos;
        if (!(P.nnz[j] == 1 && P.allone[j]) || used[P.lastrow[j]]) { s.slack = false; return GOMILP_OK; }
        s.rho[pos] = P.lastrow[j]; used[s.rho[pos]] = 1; s.basic[pos] = j;
    }
    for (int pos = 0; pos < m; pos++) { s.xb[pos] = P.hb[s.rho[pos]]; if (s.xb[pos] < -1e-13) s.feasible = false; }
    return GOMILP_OK;
}

// general case (engine_general.cpp): search over a kept copy of A, for the tableau pipelines or the guarded revised loop
int Engine::search_start(const Problem &P, bool supplied, Start &s) {
    const int m = P.m, n = P.n;
    int rc;
    const double t_g0 = now_s();
    if (!supplied) {
        // 96 rows and more (knob general_min_rows): the scan runs on the device — whole solves with the host / the blocked device search,
        // tools/general_small.py: 64 rows 0.96 / 1.08 ms, 96: 1.54 / 1.51, 128: 2.28 / 1.85, 180: 4.5 / 2.9, 224: 6.8 / 3.4, 300: 11.1 / 4.5
        // (until round 5, five launches per candidate: 224 rows)
        rc = plan_.search_on_device ? find_independent_device(P, s.basic, &s.binv_host, &gen_binv_dev_) : general_find_linearly_independent(P.hA, m, n, s.basic, &s.binv_host);
        if (rc != GOMILP_OK) return rc;  // ErrSingular, simplex.go:495-497
    }
    const double t_g1 = now_s();
    if (!gen_binv_dev_ && s.binv_host.size() != (size_t)m * m && !general_basis_inverse(P.hA, m, n, s.basic, n, std::vector<double>(), s.binv_host))
        return supplied ? GOMILP_ERR_PANIC : GOMILP_ERR_SINGULAR;
    const double t_g2 = now_s();
    // xb = ab^-1 b with the reference's own arithmetic (gonum-order LU on the device): the feasibility test of
    // simplex.go:459-469 then sees the same bits
    if ((rc = upload_index_lists(s.basic, {})) != GOMILP_OK) return rc;
    std::vector<double> xb_exact;
    bool sing = false;
    if ((rc = final_solve(P, xb_exact, &sing)) != GOMILP_OK) return rc;
    if (sing) { s.feasible = false; }  // "singular" also sends the reference to Phase I (simplex.go:504-507), xb stays zero
    else { s.xb = xb_exact; for (int pos = 0; pos < m; pos++) if (s.xb[pos] < -1e-13) s.feasible = false; }
    if (supplied && !s.feasible) return GOMILP_ERR_PANIC;  // initializeFromBasic errors panic (:156-158)
    if (GOMILP_DBG_ENV("GOMILP_DEBUG_GS")) fprintf(stderr, "general start: search %.2f ms, host inverse %.2f ms, x_B (gonum-order LU) %.2f ms\n", 1e3 * (t_g1 - t_g0), 1e3 * (t_g2 - t_g1), 1e3 * (now_s() - t_g2));
    return GOMILP_OK;
}

int Engine::upload_start(const Problem &P, const Start &s) {
    Work &w = *w_;
    const int m = P.m;
    int rc;
    cur_ = 0;
    if (s.slack && !plan_.use_tab) {
        HIP_TRY(hipMemsetAsync(w.binv[0], 0, (size_t)m * P.ld * sizeof(double), stream_));
        if ((rc = stage_upload(w.rho, s.rho.data(), (size_t)m * sizeof(int32_t))) != GOMILP_OK) return rc;
        launch_set_binv_perm(w.binv[0], P.ld, m, w.rho, stream_);
    }
    if (plan_.gen_revised) {   // the searched (or supplied) basis' B^-1: in place from the device search, else the host's (the tableau set-up's copy)
        if (!gen_binv_dev_) {
            HIP_TRY(hipMemsetAsync(w.binv[0], 0, (size_t)m * P.ld * sizeof(double), stream_));
            HIP_TRY(hipMemcpy2DAsync(w.binv[0], (size_t)P.ld * sizeof(double), s.binv_host.data(), (size_t)m * sizeof(double), (size_t)m * sizeof(double), m,
                                     hipMemcpyHostToDevice, stream_));
            HIP_TRY(sync_stream());   // (pageable source)
        } else if (P.ld > m) {   // (the K1-K3 rows run over the padding column too)
            HIP_TRY(hipMemset2DAsync(w.binv[0] + m, (size_t)P.ld * sizeof(double), 0, sizeof(double), m, stream_));
        }
    }
    ycur_ = 0;
    if (!plan_.use_tab) {   // the duals only exist on the revised-simplex pipelines
        HIP_TRY(hipMemsetAsync(w.yb[0], 0, (size_t)P.ld * sizeof(double), stream_));
        HIP_TRY(hipMemsetAsync(w.yb[1], 0, (size_t)P.ld * sizeof(double), stream_));
    }
    return upload_padded(w.xb, s.xb, P.ld);
}

int Engine::upload_padded(double *dst, const std::vector<double> &v, int ld) {   // v with its zero padding in one copy
    std::vector<double> pad(ld, 0.0);
    std::copy(v.begin(), v.end(), pad.begin());
    return stage_upload(dst, pad.data(), (size_t)ld * sizeof(double));
}

void build_nonbasic(const std::vector<int32_t> &basic, int ncols, std::vector<int32_t> &nonbasic) {
    std::vector<char> inb(ncols, 0);
    for (int32_t j : basic) inb[j] = 1;
    nonbasic.clear();
    for (int j = 0; j < ncols; j++) if (!inb[j]) nonbasic.push_back(j);
}

// for unit columns one exact "- 1" per row (floats.Sub, :536-542); a searched basis subtracts its full columns, on the device from
// general_min_rows on (k_gs_art: the same subtractions, element by element)
int Engine::phase1_artificial(const Problem &P, const Start &s, int64_t minidx, std::vector<double> &art, gomilp_lp_stats *st) {
    Work &w = *w_;
    const int m = P.m, n = P.n;
    double *row = P.dAt + (size_t)n * P.ld;
    for (int k = 0; k < m; k++) art[k] = P.hb[k];
    if (s.slack) {
        for (int i = 0; i < m; i++) { if (i == minidx) continue; art[s.rho[i]] = -1 * 1.0 + art[s.rho[i]]; }
    } else if (plan_.art_on_device) {
        launch_gs_art(P.dAt, P.ld, m, w.basic, (int)minidx, P.db, row, stream_);
        launches_++;
        HIP_TRY(hipMemcpyAsync(art.data(), row, (size_t)P.ld * sizeof(double), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(sync_stream());
    } else {
        for (int i = 0; i < m; i++) {
            if (i == minidx) continue;
            for (int k = 0; k < m; k++) art[k] = -1 * P.hA[(size_t)k * n + s.basic[i]] + art[k];
        }
    }
    bool art_zero = true;
    for (int k = 0; k < m; k++) if (art[k] != 0) { art_zero = false; break; }
    if (art_zero) { st->wrapped_status = GOMILP_ERR_ZERO_COLUMN; return GOMILP_ERR_PHASE1_WRAPPED; }  // verifyInputs of the recursive call
    return plan_.art_on_device ? GOMILP_OK : stage_upload(row, art.data(), (size_t)P.ld * sizeof(double));
}

int Engine::phase1_art_level(const Problem &P, int added, const std::vector<double> &xb) {
    double xart = added >= 0 ? xb[added] : 0.0;
    if (added >= 0 && fabs(xart) > 1e-13 && fabs(xart) < 1e-11) {
        // too close to phaseIZeroTol to trust the updated x_B: take the reference's own value (fresh gonum-order solve)
        std::vector<double> xe;
        bool sing = false;
        const int rc = final_solve(P, xe, &sing);
        if (rc != GOMILP_OK) return rc;
        if (!sing) xart = xe[added];
    }
    return fabs(xart) > 1e-12 ? GOMILP_ERR_INFEASIBLE : GOMILP_OK;  // phaseIZeroTol, :563-565
}

// keeps the basis nonsingular — a guard on the pivot element instead of the LU condition estimate — and x_B feasible
bool exchange_keeps_feasible(const double *dcol, const std::vector<double> &xb, int added, int m) {
    double dmax = 0;
    for (int i = 0; i < m; i++) dmax = std::max(dmax, fabs(dcol[i]));
    const double dpv = dcol[added];
    if (!(fabs(dpv) > 1e-9 * std::max(1.0, dmax))) return false;
    const double theta = xb[added] / dpv;
    for (int i = 0; i < m; i++) {
        const double v = (i == added) ? theta : xb[i] - theta * dcol[i];
        if (v < -1e-13) return false;
    }
    return true;
}

int Engine::solve_revised(const Problem &P, double tol, Start &s, gomilp_lp_stats *st, int *loop_rc) {
    Work &w = *w_;
    const int m = P.m, n = P.n;
    std::vector<int32_t> &basic = s.basic;
    std::vector<double> &xb = s.xb;
    std::vector<int32_t> nonbasic;
    int rc;
    if (!s.feasible) {
        // ---- Phase I (simplex.go:529-606) ----
        st->phase1_used = 1;
        const int64_t minidx = min_idx(xb.data(), m);
        std::vector<double> art(P.ld, 0.0);   // (w.basic holds a searched basis: uploaded for the x_B solve)
        if ((rc = phase1_artificial(P, s, minidx, art, st)) != GOMILP_OK) return rc;
        // basis := slack basis with position minidx replaced by the artificial: one forced pivot builds its inverse
        w.st_host->done = 0; w.st_host->status = ST_RUNNING; w.st_host->pivots = 0; w.st_host->max_pivots = 0; w.st_host->rq = 0;
        sync_state_to_device();
        {
            LPArgs a = make_args(P, 1, 1e-10, 0, P.dc1);
            launch_ftran(a, 0, -1, n, stream_);
            launch_update(a, 0, (int)minidx, 1, 0, stream_);
            launches_ += 2;
            cur_ ^= 1;
        }
        basic[minidx] = n;
        build_nonbasic(basic, n + 1, nonbasic);
        if ((rc = upload_index_lists(basic, nonbasic)) != GOMILP_OK) return rc;
        refresh_xb_y(P, P.dc1);  // xb = ab^-1 b (initializeFromBasic of the recursive call), y = ab^-T cb
        HIP_TRY(hipMemcpyAsync(w.h_vec, w.xb, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(sync_stream());
        for (int i = 0; i < m; i++) if (w.h_vec[i] < -1e-13) return GOMILP_ERR_PANIC;  // simplex.go:155-158
        rc = run_loop(P, 1, 1e-10, (int)nonbasic.size(), P.dc1, st);
        if (rc == GOMILP_ERR_DEVICE) return rc;
        if (rc != GOMILP_OK) { st->wrapped_status = rc; return GOMILP_ERR_PHASE1_WRAPPED; }  // :557-559
        HIP_TRY(hipMemcpyAsync(w.h_idx, w.basic, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(hipMemcpyAsync(w.h_vec, w.xb, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(sync_stream());
        int added = -1;
        for (int i = 0; i < m; i++) { basic[i] = w.h_idx[i]; xb[i] = w.h_vec[i]; if (basic[i] == n) added = i; }
        if ((rc = phase1_art_level(P, added, xb)) != GOMILP_OK) return rc;
        if (added >= 0) {
            // :581-606 the artificial stayed basic at zero: exchange it for the first nonbasic column that keeps
            // the basis nonsingular and feasible
            bool exchanged = false;
            build_nonbasic(basic, n + 1, nonbasic);   // (the artificial is basic: structural columns only)
            for (size_t c = 0; c < nonbasic.size() && !exchanged; c++) {
                const int j = nonbasic[c];
                w.st_host->done = 0; w.st_host->status = ST_RUNNING; w.st_host->rq = 0;
                sync_state_to_device();
                LPArgs a = make_args(P, 1, 1e-10, 0, P.dc1);
                launch_ftran(a, 0, -1, j, stream_);
                launches_++;
                HIP_TRY(hipMemcpyAsync(w.h_vec, w.dvec, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream_));
                HIP_TRY(sync_stream());
                if (!exchange_keeps_feasible(w.h_vec, xb, added, m)) continue;
                launch_update(a, 0, added, 1, 0, stream_);
                launches_++;
                cur_ ^= 1;
                basic[added] = j;
                exchanged = true;
                st->art_exchanges++;
            }
            if (!exchanged) return GOMILP_ERR_INFEASIBLE;  // :606
        }
    }

    // ---- Phase II (simplex.go:169-293) ----
    build_nonbasic(basic, n, nonbasic);
    if ((rc = upload_index_lists(basic, nonbasic)) != GOMILP_OK) return rc;
    if (st->phase1_used) {
        refresh_xb_y(P, P.dc);
    } else {
        launch_y_from_binv(w.binv[cur_], P.ld, m, P.dc, w.basic, w.yscratch, w.yb[ycur_], stream_);
        launches_ += 2;
    }
    *loop_rc = run_loop(P, 2, tol, (int)nonbasic.size(), P.dc, st);
    return GOMILP_OK;
}

int Engine::fetch_trace(std::vector<DevPivot> &tr) {
    Work &w = *w_;
    HIP_TRY(hipMemcpyAsync(w.st_host, w.st, sizeof(DevState), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(sync_stream());
    const int64_t cnt = std::min<int64_t>(w.st_host->trace_len, w.trace_cap);
    tr.resize((size_t)cnt);
    if (cnt) HIP_TRY(hipMemcpy(tr.data(), w.trace, (size_t)cnt * sizeof(DevPivot), hipMemcpyDeviceToHost));
    return GOMILP_OK;
}

int Engine::solve_tail(const Problem &P, int64_t id, int loop_rc, std::vector<int32_t> &basic, std::vector<double> &xb,
                       const std::vector<int32_t> &basic_start, const std::vector<int32_t> *rho_slack, double *opt_f, double *opt_x,
                       int32_t *has_x, int64_t *basis_out, gomilp_lp_stats *st) {
    const double inf = std::numeric_limits<double>::infinity();
    const int m = P.m, n = P.n;
    Work &w = *w_;
    if (loop_rc == GOMILP_ERR_DEVICE) return loop_rc;
    const bool loop_unbounded = loop_rc == GOMILP_ERR_UNBOUNDED;   // :261-263, :272-274 — after the condition guards below
    if (loop_unbounded && !shadow_trace_) { *opt_f = -inf; return loop_rc; }

    // ---- epilogue (simplex.go:296-301): x_B from a fresh gonum-order solve on the final basis ----
    HIP_TRY(hipMemcpyAsync(w.h_idx, w.basic, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipMemcpyAsync(w.h_vec, w.xb, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(sync_stream());
    for (int i = 0; i < m; i++) { basic[i] = w.h_idx[i]; xb[i] = w.h_vec[i]; }
    std::vector<DevPivot> tr;
    int rc;
    if (shadow_trace_ && (loop_rc == GOMILP_OK || loop_rc == GOMILP_ERR_BLAND || loop_unbounded)) {
        // ---- the reference's LU.Solve guards (mat/lu.go:301,321), replayed on the host with exact condition numbers
        if ((rc = fetch_trace(tr)) != GOMILP_OK) return rc;
        std::vector<std::pair<int, int>> piv;
        for (auto &e : tr) piv.emplace_back((int)e.replace, (int)e.entering);
        std::vector<int32_t> bas = basic_start;
        int cst = GOMILP_OK;
        int64_t evals = 0;
        const int stop = general_condition_replay(P.hA, m, n, bas, piv, loop_unbounded, &cst, &evals);
        st->cond_fallbacks += evals;
        if (cst != GOMILP_OK) {
            // the reference left its loop here with the point of that basis (simplex.go:296-301)
            std::vector<double> xs;
            if (general_solve_basis(P.hA, m, n, bas, P.hb, xs)) {
                return_point(P, bas, xs, opt_f, opt_x, has_x, basis_out);
                st->pivots_phase2 = stop;
                shadow_trace_ = false;
                return cst;
            }
        }
    }
    shadow_trace_ = false;
    if (loop_unbounded) { *opt_f = -inf; return loop_rc; }
    if (keep_id_ == id && loop_rc == GOMILP_OK) keep_capture(P, id, st->pipeline, basic, basic_start, rho_slack);
    rc = epilogue(P, basic, xb, loop_rc, opt_f, opt_x, has_x, basis_out, st);
    if (rc == GOMILP_ERR_DEVICE) return rc;
    if (trace_on_) {
        if (fetch_trace(tr) != GOMILP_OK) return GOMILP_ERR_DEVICE;
        last_trace_total_ = w.st_host->trace_len;
        last_trace_.resize(tr.size());
        for (size_t i = 0; i < tr.size(); i++) {
            last_trace_[i].phase = tr[i].phase; last_trace_[i].bland = tr[i].bland;
            last_trace_[i].min_idx = tr[i].min_idx; last_trace_[i].replace = tr[i].replace;
            last_trace_[i].entering = tr[i].entering; last_trace_[i].leaving = tr[i].leaving;
        }
    }
    return rc;
}

// x_B = ab^-1 b from a fresh gonum-order LU of the final basis (the device list w.basic must hold `basic`), z = DotUnitary,
// scatter (simplex.go:296-301).  Returns loop_rc (or mat.Condition when the final basis is exactly singular).
int Engine::epilogue(const Problem &P, std::vector<int32_t> &basic, std::vector<double> &xb, int loop_rc, double *opt_f,
                     double *opt_x, int32_t *has_x, int64_t *basis_out, gomilp_lp_stats *st) {
    const int m = P.m, n = P.n;
    std::vector<double> xb_exact;
    bool singular = false;
    const double t1 = now_s();
    int rc = final_solve(P, xb_exact, &singular, basic.data());
    if (rc != GOMILP_OK) return rc;
    st->seconds_final_solve = now_s() - t1;
    if (singular) {
        xb_exact = xb;  // the reference keeps its previous x_B when Det()==0 (mat/lu.go:301); ours is the updated one
        if (loop_rc == GOMILP_OK) loop_rc = GOMILP_ERR_CONDITION;
    }
    double drift = 0;
    for (int i = 0; i < m; i++) drift = std::max(drift, fabs(xb[i] - xb_exact[i]));
    st->drift_xb = drift;
    return_point(P, basic, xb_exact, opt_f, opt_x, has_x, basis_out);
    return loop_rc;
}

// z = DotUnitary(c_B, x_B) and the scatter of x_B into x (simplex.go:296-301)
void Engine::return_point(const Problem &P, const std::vector<int32_t> &basic, const std::vector<double> &xb, double *opt_f, double *opt_x,
                          int32_t *has_x, int64_t *basis_out) {
    const int m = P.m;
    std::vector<double> cb(m);
    for (int i = 0; i < m; i++) cb[i] = P.hc[basic[i]];
    *opt_f = dot_unitary(cb.data(), xb.data(), m);
    for (int j = 0; j < P.n; j++) opt_x[j] = 0;
    for (int i = 0; i < m; i++) opt_x[basic[i]] = xb[i];
    *has_x = 1;
    if (basis_out) for (int i = 0; i < m; i++) basis_out[i] = basic[i];
}

bool Engine::root_view(int64_t id, RootView *out) {
    std::lock_guard<std::mutex> g(mu_);
    if (id < 0 || (size_t)id >= problems_.size() || !problems_[id]) return false;
    const Problem &P = *problems_[id];
    out->gen.reset(); out->genrev.reset();   // a view is reused across roots (gomilp_pool_set_root): never keep the previous root's searched basis
    out->m = P.m; out->n = P.n; out->ld = P.ld; out->dAt = P.dAt; out->dc = P.dc; out->db = P.db;
    out->verify_status = P.verify_status; out->serial = P.serial; out->hb = P.hb; out->hc = P.hc; out->scale_span = P.scale_span;
    out->rho0.assign(P.m, 0);
    out->unit_basis = P.m < P.n;
    std::vector<char> used(P.m, 0);
    for (int pos = 0; pos < P.m && out->unit_basis; pos++) {
        const int j = P.n - 1 - pos;
        if (!(P.nnz[j] == 1 && P.allone[j]) || used[P.lastrow[j]]) { out->unit_basis = false; break; }
        out->rho0[pos] = P.lastrow[j]; used[P.lastrow[j]] = 1;
    }
    out->rm.reset();
    if (out->unit_basis && P.verify_status == GOMILP_OK && (size_t)P.m * (size_t)P.n <= ((size_t)1 << 23) && hipSetDevice(device_) == hipSuccess) {
        if (!stream_ && hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess) return true;
        std::shared_ptr<RootView::RowMajor> rm(new RootView::RowMajor);
        rm->lda = (P.n + 1) & ~1;
        if (dmalloc(&rm->dA, (size_t)P.m * rm->lda) == hipSuccess) {
            // "A" of the transposing kernel = At (n rows of ld), its output = m rows of lda: dA[i * lda + j] = At[j * ld + i]
            launch_transpose_in(P.dAt, P.ld, P.n, P.m, rm->dA, rm->lda, stream_);
            if (hipStreamSynchronize(stream_) == hipSuccess) out->rm = rm;
        }
    }
    return true;
}

Engine::RootView::RowMajor::~RowMajor() { if (dA) hipFree(dA); }

Engine::RootView::General::~General() {
    for (void *p : {(void *)dT0, (void *)dxb0, (void *)dbasic0, (void *)dnonbasic0, (void *)dposvar0}) if (p) hipFree(p);
}
Engine::RootView::GeneralRev::~GeneralRev() {
    for (void *p : {(void *)dB0inv, (void *)dxb0, (void *)dbasic0, (void *)dposvar0}) if (p) hipFree(p);
}

bool Engine::root_general(int64_t id, RootView *out) {
    std::lock_guard<std::mutex> g(mu_);
    if (id < 0 || (size_t)id >= problems_.size() || !problems_[id]) return false;
    const Problem &P = *problems_[id];
    const int m = P.m, n = P.n;
    // a wide root (n - m >= 2m) keeps B0^-1 instead of the tableau (GeneralRev), within the limits of SolvePlan::gen_revised
    const bool wide = m < n && (n - m) >= 2 * m;
    if (P.verify_status != GOMILP_OK || m >= n || (wide && !RootView::general_rev_shape(m, n)) || !ensure_host_A(P)) return false;
    if (ensure_work(m, n + 1) != GOMILP_OK) return false;
    Work &w = *w_;
    std::vector<int32_t> basic;
    std::vector<double> binv;
    bool binv_dev = false;
    const int rc = (m >= knobs_.general_min_rows && knobs_.general_device) ? find_independent_device(P, basic, &binv, &binv_dev) : general_find_linearly_independent(P.hA, m, n, basic, &binv);
    if (rc != GOMILP_OK || (int)basic.size() != m) return false;
    if (!binv_dev && binv.size() != (size_t)m * m && !general_basis_inverse(P.hA, m, n, basic, n, std::vector<double>(), binv)) return false;
    std::vector<int32_t> nonbasic, posvar(n);
    build_nonbasic(basic, n, nonbasic);
    const int nn = (int)nonbasic.size();
    for (int i = 0; i < m; i++) posvar[basic[i]] = i;
    for (int jp = 0; jp < nn; jp++) posvar[nonbasic[jp]] = -1 - jp;
    if (upload_index_lists(basic, nonbasic) != GOMILP_OK) return false;
    // x_B of the basis with the reference's own arithmetic (as Engine::solve does for the feasibility test)
    std::vector<double> xb;
    bool sing = false;
    if (final_solve(P, xb, &sing, basic.data()) != GOMILP_OK || sing) return false;
    if (wide) {
        std::shared_ptr<RootView::GeneralRev> R(new RootView::GeneralRev);
        R->m = m; R->ld = P.ld;
        auto ok = [](hipError_t e) { return e == hipSuccess; };
        for (int i = 0; i < m; i++) posvar[basic[i]] = i;
        for (int jp = 0; jp < nn; jp++) posvar[nonbasic[jp]] = -1;
        if (!ok(dmalloc(&R->dB0inv, (size_t)m * P.ld)) || !ok(dmalloc(&R->dxb0, (size_t)m)) || !ok(dmalloc(&R->dbasic0, (size_t)m)) ||
            !ok(dmalloc(&R->dposvar0, (size_t)n))) return false;
        // m x ld with a zeroed padding column: in place from the device search (R^-1 Q^T in the first B^-1 buffer), else the host inverse
        if (!ok(hipMemsetAsync(R->dB0inv, 0, (size_t)m * P.ld * sizeof(double), stream_))) return false;
        if (!ok(binv_dev ? hipMemcpy2DAsync(R->dB0inv, (size_t)P.ld * sizeof(double), w.binv[0], (size_t)P.ld * sizeof(double), (size_t)m * sizeof(double), m,
                                            hipMemcpyDeviceToDevice, stream_)
                         : hipMemcpy2DAsync(R->dB0inv, (size_t)P.ld * sizeof(double), binv.data(), (size_t)m * sizeof(double), (size_t)m * sizeof(double), m,
                                            hipMemcpyHostToDevice, stream_)))
            return false;
        if (!ok(hipMemcpyAsync(R->dxb0, xb.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, stream_)) ||
            !ok(hipMemcpyAsync(R->dbasic0, basic.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, stream_)) ||
            !ok(hipMemcpyAsync(R->dposvar0, posvar.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, stream_)) || !ok(sync_stream())) return false;
        out->genrev = R;
        return true;
    }
    std::shared_ptr<RootView::General> G(new RootView::General);
    G->m = m; G->nn = nn; G->ldt = tab_ld(nn);
    auto ok = [](hipError_t e) { return e == hipSuccess; };
    if (!ok(dmalloc(&G->dT0, (size_t)m * G->ldt)) || !ok(dmalloc(&G->dxb0, (size_t)m)) || !ok(dmalloc(&G->dbasic0, (size_t)m)) ||
        !ok(dmalloc(&G->dnonbasic0, (size_t)std::max(nn, 1))) || !ok(dmalloc(&G->dposvar0, (size_t)n))) return false;
    if (!binv_dev && !ok(hipMemcpy2DAsync(w.binv[0], (size_t)P.ld * sizeof(double), binv.data(), (size_t)m * sizeof(double), (size_t)m * sizeof(double), m, hipMemcpyHostToDevice, stream_))) return false;
    if (!ok(hipMemsetAsync(G->dT0, 0, (size_t)m * G->ldt * sizeof(double), stream_))) return false;
    launch_tab_gemm(w.binv[0], P.ld, P.dAt, P.ld, m, nn, w.nonbasic, G->dT0, G->ldt, false, stream_);
    if (!ok(hipMemcpyAsync(G->dxb0, xb.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, stream_)) ||
        !ok(hipMemcpyAsync(G->dbasic0, basic.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, stream_)) ||
        !ok(hipMemcpyAsync(G->dnonbasic0, nonbasic.data(), (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice, stream_)) ||
        !ok(hipMemcpyAsync(G->dposvar0, posvar.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, stream_)) || !ok(sync_stream())) return false;
    out->gen = G;
    return true;
}

int Engine::finish_from_basis(int64_t id, const int32_t *basic_in, const double *xb_updated, int loop_rc, double *opt_f,
                              double *opt_x, int32_t *has_x, int64_t *basis_out, gomilp_lp_stats *stats) {
    std::lock_guard<std::mutex> g(mu_);
    const double t0 = now_s();
    gomilp_lp_stats local;
    gomilp_lp_stats *st = stats ? stats : &local;
    memset(st, 0, sizeof(*st));
    st->device_id = device_;
    if (has_x) *has_x = 0;
    if (opt_f) *opt_f = std::numeric_limits<double>::quiet_NaN();
    if (id < 0 || (size_t)id >= problems_.size() || !problems_[id] || !opt_f || !opt_x || !has_x || !basic_in || !xb_updated) return GOMILP_ERR_BAD_SHAPE;
    const Problem &P = *problems_[id];
    launches_ = 0; fs_device_ = fs_host_ = 0; lu_look_fault_ = 0;
    int rc = ensure_work(P.m, P.n + 1);
    if (rc != GOMILP_OK) return rc;
    std::vector<int32_t> basic(basic_in, basic_in + P.m);
    std::vector<double> xb(xb_updated, xb_updated + P.m);
    if ((rc = upload_index_lists(basic, {})) != GOMILP_OK) return rc;
    rc = epilogue(P, basic, xb, loop_rc, opt_f, opt_x, has_x, basis_out, st);
    st->seconds_total = now_s() - t0; st->kernel_launches = launches_;
    st->seconds_final_device = fs_device_; st->seconds_final_host = fs_host_;
    st->lu_dense_steps = lu_dense_; st->lu_rounds = lu_rounds_;
    if (lu_look_fault_) st->device_retries = lu_look_fault_;
    return rc;
}

int64_t Engine::last_trace(gomilp_pivot *out, int64_t cap) {
    std::lock_guard<std::mutex> g(mu_);
    const int64_t cnt = std::min<int64_t>((int64_t)last_trace_.size(), cap);
    if (out && cnt > 0) memcpy(out, last_trace_.data(), (size_t)cnt * sizeof(gomilp_pivot));
    return last_trace_total_;
}


// findLinearlyIndependent: the column scan on the device — general_block.hip: 16 / 8 / 4 candidates per four launches (default);
// general_kernels.hip: five launches per candidate (knob general_block = 0, bases beyond 4096 rows, the square step) — one look at the
// state block per chunk of candidates; Q^T and R^-1 live in the two B^-1 buffers of the revised pipelines (free at this point)
int Engine::find_independent_device(const Problem &P, std::vector<int32_t> &basic, std::vector<double> *binv_out, bool *binv_on_device) {
    if (binv_on_device) *binv_on_device = false;
    Work &w = *w_;
    const int m = P.m, n = P.n, ldq = P.ld;
    const double t_gs0 = now_s();
    basic.clear();
    if (!w.gs_state) {
        HIP_TRY(dmalloc(&w.gs_state, 1));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&w.gs_host), sizeof(GsState), hipHostMallocDefault));
    }
    if (w.cap_gs_idx < m) {
        if (w.gs_idx) hipFree(w.gs_idx);
        w.gs_idx = nullptr;
        HIP_TRY(dmalloc(&w.gs_idx, (size_t)m + 64));
        w.cap_gs_idx = m + 64;
    }
    double *QT = w.binv[0], *Rinv = w.binv[1];
    double *wv = w.yscratch, *tv = w.yscratch + P.ld, *yv = w.yscratch + 2 * (size_t)P.ld;   // 64 rows of ld doubles: w, t, 16 partial y
    HIP_TRY(hipMemsetAsync(Rinv, 0, (size_t)m * ldq * sizeof(double), stream_));
    // The scan starts at the slack columns (simplex.go:618).  A unit column e_r after k unit columns with other rows is kept with
    // kappa_1 = 1, one with a row already taken is exactly dependent and dropped; its Householder step only negates a row of Q^T
    // or swaps two (the rank-1 update acts on 0 / +-1 entries: no rounding), so the leading run of unit columns is decided here
    // in O(1) each and the device scan starts behind it with Q^T = that signed permutation, R = R^-1 = diag(beta).
    int col = n - 1, s0 = 0;
    {
        std::vector<int32_t> perm(m), inv(m);
        std::vector<double> sgn(m, 1.0), beta(m, 1.0);
        for (int i = 0; i < m; i++) { perm[i] = i; inv[i] = i; }
        std::vector<int32_t> acc;
        for (; col >= 0 && s0 < m - 1; col--) {
            if (!(P.nnz[col] == 1 && P.allone[col])) break;
            const int r = P.lastrow[col], p = inv[r], k = s0;
            if (p < k) continue;                       // row r already carries an accepted unit column: beta = 0, cond = inf, dropped
            if (p == k) { beta[k] = sgn[k] >= 0 ? -1.0 : 1.0; sgn[k] = -sgn[k]; }
            else {                                     // alpha = 0, beta = -1, v = e_k + sgn[p] e_p: rows k and p trade places
                const int pk = perm[k];
                const double sk = sgn[k], sp = sgn[p];
                beta[k] = -1.0;
                perm[k] = r; sgn[k] = -1.0;
                perm[p] = pk; sgn[p] = -sp * sk;
                inv[r] = k; inv[pk] = p;
            }
            acc.push_back(col);
            s0++;
        }
        if (s0) {
            int rcp = stage_upload(w.gs_idx, acc.data(), (size_t)s0 * sizeof(int32_t));
            if (rcp == GOMILP_OK) rcp = stage_upload(w.lpos, perm.data(), (size_t)m * sizeof(int32_t));
            if (rcp == GOMILP_OK) rcp = stage_upload(yv + 20 * (size_t)P.ld, sgn.data(), (size_t)m * sizeof(double));
            if (rcp == GOMILP_OK) rcp = stage_upload(yv + 21 * (size_t)P.ld, beta.data(), (size_t)m * sizeof(double));
            if (rcp != GOMILP_OK) return rcp;
            launch_gs_init_perm(QT, Rinv, ldq, m, w.lpos, yv + 20 * (size_t)P.ld, yv + 21 * (size_t)P.ld, s0, w.gs_state, stream_);
        } else {
            launch_gs_init(QT, ldq, m, w.gs_state, stream_);
        }
    }
    launches_++;
    bool scan_done = s0 >= m - 1;
    int stop_after_prefix = col;
    // blocked form (general_block.hip): NB candidates per four launches; as many blocks per look at the state as would fill the basis
    // if every candidate were accepted (a rejected candidate costs one more look)
    const int nbw = general_block_ ? gs_block_width(m) : 0;
    int k_known = s0;
    for (; !scan_done;) {
        if (nbw) {
            const int want = std::max(1, std::min(32, (m - 1 - k_known + nbw - 1) / nbw));
            for (int q = 0; q < want && col >= 0; q++) {
                const int nc = std::min(nbw, col + 1);
                launch_gs_block(P.dAt, P.ld, col, nc, QT, Rinv, ldq, m, w.yscratch, w.gs_idx, w.gs_state, stream_);
                col -= nc;
                launches_ += 4;
            }
        } else {
            const int chunk = std::min(col + 1, 128);
            for (int q = 0; q < chunk; q++, col--) launch_gs_candidate(P.dAt + (size_t)col * P.ld, QT, Rinv, ldq, m, wv, tv, yv, col, w.gs_idx, w.gs_state, stream_);
            launches_ += 5 * chunk;
        }
        HIP_TRY(hipMemcpyAsync(w.gs_host, w.gs_state, sizeof(GsState), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(sync_stream());
        HIP_TRY(hipGetLastError());
        if (w.gs_host->done || col < 0) break;
        k_known = w.gs_host->k;
    }
    if (scan_done) {   // the unit columns alone filled m - 1 positions: the device never scanned
        HIP_TRY(hipMemcpyAsync(w.gs_host, w.gs_state, sizeof(GsState), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(sync_stream());
        w.gs_host->stop_col = stop_after_prefix;
    }
    const int k = w.gs_host->k;
    std::vector<int32_t> idx(k);
    if (k) HIP_TRY(hipMemcpy(idx.data(), w.gs_idx, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost));
    basic = idx;
    if (k < m - 1 || !w.gs_host->done) return GOMILP_ERR_SINGULAR;   // the columns ran out: simplex.go:495-497
    const double t_scan = now_s();
    // the square step: the first remaining candidate is taken tentatively on the device (reflector, new column of R^-1), B^-1 =
    // R^-1 Q^T is formed there, and the host judges kappa_1 of the matrix itself, |C|_1 |C^-1|_1 (mat.Cond of a square matrix
    // goes through its LU in the reference).  A rejected candidate sends the rest of the scan to the host form.
    int cand = w.gs_host->stop_col;
    int rcl = GOMILP_ERR_SINGULAR;
    if (cand >= 0) {
        launch_gs_candidate(P.dAt + (size_t)cand * P.ld, QT, Rinv, ldq, m, wv, tv, yv, cand, w.gs_idx, w.gs_state, stream_, 1);
        launch_gs_binv(Rinv, QT, ldq, m, w.W, stream_);
        // the two 1-norms on the device too (absolute column sums of C^-1 in 8 row slices, of the m basis columns out of At): 72 KB
        // come home instead of the matrix — the 8 MB copy, the host's passes over it and over a strided A, and later the upload of the
        // same B^-1 for the tableau set-up were 1.4 of the 1000-row solve's 17.5 ms
        double *nrm = yv, *csum = yv + 8 * (size_t)P.ld;   // (the block search's W rows: free again)
        launch_gs_norms(w.W, ldq, m, nrm, P.dAt, P.ld, w.gs_idx, cand, csum, stream_);
        launches_ += 7;
        const bool keep_dev = binv_on_device != nullptr;
        if (keep_dev) HIP_TRY(hipMemcpyAsync(QT, w.W, (size_t)m * ldq * sizeof(double), hipMemcpyDeviceToDevice, stream_));   // Q^T has served: B^-1 takes its place (the LU that follows overwrites W)
        double *hn = w.h_W;   // (pinned; 9 rows of ld doubles)
        HIP_TRY(hipMemcpyAsync(hn, nrm, (size_t)9 * P.ld * sizeof(double), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(hipMemcpyAsync(w.gs_host, w.gs_state, sizeof(GsState), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(sync_stream());
        HIP_TRY(hipGetLastError());
        double nC = 0, nI = 0;
        bool finite = w.gs_host->beta_last != 0;
        if (finite) {
            const double *hc = hn + 8 * (size_t)P.ld;
            for (int p = 0; p < m; p++) nC = std::max(nC, hc[p]);   // |C|_1: largest absolute column sum over the m basis columns
            for (int c2 = 0; c2 < m; c2++) {
                double sc = 0;
                for (int sl = 0; sl < 8; sl++) sc += hn[(size_t)sl * P.ld + c2];
                if (!std::isfinite(sc)) finite = false;
                nI = std::max(nI, sc);
            }
        }
        const double cond = finite ? nC * nI : std::numeric_limits<double>::infinity();
        if (!(cond > 1e12)) {   // simplex.go:630
            basic.push_back(cand);
            if (keep_dev) *binv_on_device = true;
            else if (binv_out) {   // (a caller that wants the inverse at home)
                HIP_TRY(hipMemcpyAsync(w.h_W, w.W, (size_t)m * ldq * sizeof(double), hipMemcpyDeviceToHost, stream_));
                HIP_TRY(sync_stream());
                binv_out->resize((size_t)m * m);
                for (int r = 0; r < m; r++) memcpy(binv_out->data() + (size_t)r * m, w.h_W + (size_t)r * ldq, (size_t)m * sizeof(double));
            }
            rcl = GOMILP_OK;
        } else {
            rcl = general_finish_last_column(P.hA, m, n, basic, cand - 1, binv_out);
        }
    }
    if (GOMILP_DBG_ENV("GOMILP_DEBUG_GS")) fprintf(stderr, "gs: m %d scanned %d scan %.2f ms last column %.2f ms\n", m, w.gs_host->scanned, 1e3 * (t_scan - t_gs0), 1e3 * (now_s() - t_scan));
    return rcl;
}

int Engine::debug_find_independent(int64_t id, std::vector<int32_t> &idxs) {
    std::lock_guard<std::mutex> g(mu_);
    if (id < 0 || (size_t)id >= problems_.size() || !problems_[id]) return GOMILP_ERR_BAD_SHAPE;
    const Problem &P = *problems_[id];
    HIP_TRY(hipSetDevice(device_));
    int rc = ensure_work(P.m, P.n + 1);
    if (rc != GOMILP_OK) return rc;
    if (!ensure_host_A(P)) return GOMILP_ERR_UNSUPPORTED;
    return find_independent_device(P, idxs, nullptr);
}

}  // namespace gomilp
