// ------------------------------------------------------------------------------------------------
// Final solve x_B = ab^-1 b in gonum's order: LU on the device (k_lu_*), the two triangular solves
// of Dgetrs (lapack/gonum/dgetrs.go:37-45 -> blas/gonum/level3double.go:75-118) on the host (lu_host.cpp),
// because the upper solve is one sequential dependency chain of m^2/2 rounded operations.
// ------------------------------------------------------------------------------------------------
#include <stdio.h>
#include <stdlib.h>

#include "engine_work.hpp"
#include "lu_host.h"

namespace gomilp {

// transpose: the system is ab^T y = rhs (the reference's BTRAN, simplex.go:236: LU of a materialised copy of ab.T()).  The
// column-major image of ab^T is the row-major image of ab, so the two gathers just change places; no column of ab^T is known
// to be a unit vector.  rhs_host (m entries, by basis position; default b): the right-hand side.
int Engine::final_solve(const Problem &P, std::vector<double> &x, bool *singular, const int32_t *basic_host, bool transpose, const double *rhs_host) {
    int rc = lu_factor(P, singular, basic_host, transpose);
    if (rc != GOMILP_OK) return rc;
    return lu_solve(P, x, rhs_host);
}

// ---- the schedule of a factorization
LuPlan LuPlan::make(int m, int64_t lu_blocked, int64_t lu_look, int64_t lu_cross, int64_t lu_large, int64_t bt_fault, size_t small_pack_cap_bytes) {
    LuPlan p;
    p.m = m;
    p.compressed = lu_blocked >= 2 && lu_compressed_supported(m, lu_large != 0);
    p.large = p.compressed && luc_large_rpt(m) > 0;   // knob lu_large: the compressed rounds beyond 4096 rows
    p.blocked = p.compressed || (lu_blocked && lu_blocked_supported(m));
    p.small = p.compressed && m <= 128;
    p.inject_fault = bt_fault == 2;
    // the rows of a panel on the workgroups of one XCD (lu_cross.hip).  1: sixteen slots, the plain schedule.  2: thirty-two slots (half the
    // rounds where a round ends because its slots are used up) in the schedule chosen below — the default where the look-ahead runs (a pool's
    // workers factor side by side and every such panel asks for workgroups of the same XCD: they keep the one-workgroup panel), from
    // the size at which it measures ahead (final solve, 32 slots against the one-workgroup panel: 1100 rows 1.28 / 1.24 ms, 1280 rows
    // 1.40 / 1.41, 1536 rows 1.40 / 1.45, 1792 rows 1.74 / 1.81, 2048 rows 2.13 / 2.19; up to 1024 rows a step of 512 threads is cheaper
    // than the exchange: 1.17 / 1.10 ms)
    const int cross_mode = lu_cross >= 0 ? (int)lu_cross : ((m > 1280 && m <= 2048 && lu_look) ? 2 : 0);
    // beyond 4096 rows (knob lu_large) that panel, several rows per lane on 8 workgroups, is the only one; lu_cross = 1 / 2 there name 16 / 32
    // slots for the four-row instance (default 16 — measured at 4097 rows, 137 dense steps, 5 rounds either way: 1.4 ms against 2.1 ms with
    // 32)
    p.cross_G = p.large ? 8 : ((cross_mode && p.compressed) ? luc_cross_groups(m, 1) : 0);
    p.cross_slots = (p.large ? lu_cross == 2 : cross_mode == 2) ? 32 : 16;
    // look-ahead schedule: where a factorization takes many rounds (measured: 2048 rows 23 rounds 2.20 -> 2.05 ms, 1000 rows 12 rounds
    // 1.10 -> 1.03 ms on the device; 520-row children, 4 rounds: 0.63 -> 0.65 ms, and a wave runs dozens of them side by side)
    // Its launches wait for their own workgroups (bounded), like the loop kernels: two such launches side by side, or one beside a loop
    // kernel, can hold each other's workgroups off the CUs until a wait gives up (measured: four metric LPs finishing together, two of
    // four factorizations fell back after ~50 ms).  So it runs only while this engine holds the device's loop slots, all of them, and
    // only if they are free right now (lu_factor asks); a pool's workers never ask (knob lu_look).
    // (beyond 4096 rows: the plain schedule, no loop slots taken; the cross-workgroup panel: under the look-ahead in mode 2 only)
    p.look_wanted = lu_blocked >= 3 && lu_look && m > 768 && p.compressed && !p.large && !(p.cross_G && cross_mode != 2);
    // Small bases: the packed factors are asked for together with the control block, in ONE host round trip and ONE copy — all m
    // columns (the compact list of dense columns would need the flags first; a unit-column step has zero multipliers and zero
    // off-diagonal U entries, which the solves skip like gonum's do: same bits, m*m instead of m*nd doubles over PCIe), with the
    // diagonal, the row positions, the flags and both control blocks behind them (k_luc_pack_small).  An exact step factors twice and
    // small trees are made of round trips and 3 us copies (60 per relaxation before this).  Should the batch of rounds turn out too
    // short, the general path takes over from where the rounds stand.
    p.oneshot = p.small && !p.cross_G && luc_pack_small_bytes(m) <= small_pack_cap_bytes;
    return p;
}

// A wait inside a look-ahead launch ran out of patience (its workgroups never became resident together): once more, from the basis,
// with the whole update behind each panel.  The cross-workgroup panel under the look-ahead: first the same panel in the plain
// schedule — the rounds stay what they were —, then, should its own exchange give up as well, the one-workgroup panel.  Beyond 4096
// rows there is no one-workgroup panel: one launch per column.  false: nothing is left to give up (or two steps were taken already).
bool LuPlan::step_down() {
    if (steps_down >= 2 || !(look_wanted || cross_G)) return false;
    steps_down++;
    if (look_wanted) look_wanted = false; else cross_G = 0;
    if (large) compressed = blocked = large = false;   // (large: no look-ahead, so this step dropped its panel)
    oneshot = false;
    return true;
}

namespace {

// the device's loop slots, all of them, for the launches of a look-ahead schedule
struct LookSlot {
    int dev; bool held;
    LookSlot(int d, bool want) : dev(d), held(want && Engine::loop_try_acquire_all(d)) {}
    ~LookSlot() { drop(); }
    void drop() { if (held) Engine::loop_release(dev, 4, 0); held = false; }
};

}  // namespace

// the basis columns into W: the compressed schedule keeps L/U column-major (lu_compressed.hip), the other two row-major
int Engine::gather_basis(const Problem &P, const LuPlan &plan, bool transpose) {
    Work &w = *w_;
    if (plan.compressed != transpose) launch_luc_gather(P.dAt, P.ld, P.m, w.basic, w.W, P.ld, stream_);
    else {
        if (transpose) HIP_TRY(hipMemsetAsync(w.W, 0, (size_t)P.m * P.ld * sizeof(double), stream_));   // (k_gather_w leaves the padding of a line alone)
        launch_gather_w(P.dAt, P.ld, P.m, w.basic, w.W, P.ld, stream_);
    }
    return GOMILP_OK;
}

// unit columns of ab (from the column statistics of the upload): the blocked LU skips their elimination steps.  *nonunit: the others
int Engine::upload_unit_rows(const Problem &P, const int32_t *basic_host, bool transpose, int *nonunit) {
    Work &w = *w_;
    const int m = P.m;
    if (!basic_host) {   // the caller has no host copy of the basis positions yet
        HIP_TRY(hipMemcpyAsync(w.h_idx, w.basic, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
        HIP_TRY(sync_stream());
        basic_host = w.h_idx;
    }
    std::vector<int32_t> ur(m);
    *nonunit = 0;
    for (int pos = 0; pos < m; pos++) {
        const int j = basic_host[pos];
        ur[pos] = (!transpose && j < P.n && P.nnz[j] == 1 && P.allone[j]) ? P.lastrow[j] : -1;
        if (ur[pos] < 0) (*nonunit)++;
    }
    return stage_upload(w.unitrow, ur.data(), (size_t)m * sizeof(int32_t));
}

// The rounds of the compressed schedule are data dependent (lu_compressed.hip): enqueue a batch, read the control block, repeat.
// end->gave_up: a launch gave up a wait (the factorization is void); end->landed: the one-shot pack brought everything to the host
int Engine::run_compressed_rounds(const LUArgs &a, const LuPlan &plan, int nonunit, LuRoundsEnd *end) {
    Work &w = *w_;
    const int m = a.m;
    int32_t *h_dense = w.h_idx + w.cap_m;   // landing place of the dense-step flags (h_idx holds nm + nc entries; lpos lands in front)
    launch_luc_init(a, stream_);
    launches_++;
    // The first batch is sized from the number of columns that are dense for sure.
    // measured: steps that do arithmetic ~ 3 x the non-unit columns (each of them usually turns a unit column dense)
    // (the slot panel takes up to nb steps per round whatever the order of the columns; a wrong guess costs one more look at the
    // control block, a generous one a run of empty rounds)
    const int nb = lu_compressed_nb();
    int batch = std::max(1, (std::min(m, (5 * nonunit) / 2) + nb - 1) / nb);
    bool oneshot = plan.oneshot;
    if (oneshot && GOMILP_DBG_ENV("GOMILP_DEBUG_LU_SHORT")) batch = 1;   // (diagnostic flavour: a first batch that is too short — the small-basis block comes too early and the general path takes over)
    int enq = 0;   // rounds enqueued so far: the look-ahead schedule keeps two control blocks, by round parity
    int k_seen = -1;   // steps done when the control block was last read
    const LUCtl *last = w.luctl_host;
    for (;;) {
        launches_ += plan.cross_G ? launch_luc_rounds_cross(a, w.rho, batch, enq, w.luxrec, plan.cross_G, plan.cross_slots, stream_) : launch_luc_rounds(a, w.rho, batch, enq, stream_);
        enq += batch;
        if (oneshot) {
            launch_luc_pack_small(a, w.Wd, stream_);
            launches_++;
            HIP_TRY(hipMemcpyAsync(w.h_W, w.Wd, luc_pack_small_bytes(m), hipMemcpyDeviceToHost, stream_));
            HIP_TRY(sync_stream());
            const double *blk = w.h_W;
            const int32_t *io = reinterpret_cast<const int32_t *>(blk + (size_t)m * m + m);
            memcpy(w.h_vec, blk + (size_t)m * m, (size_t)m * sizeof(double));   // diag
            memcpy(w.h_idx, io, (size_t)m * sizeof(int32_t));                   // lpos
            memcpy(h_dense, io + m, (size_t)m * sizeof(int32_t));
            memcpy(w.luctl_host, io + 2 * m, 2 * sizeof(LUCtl));
            w.st_host->lu_singular = io[2 * m + (int)(2 * sizeof(LUCtl) / sizeof(int32_t))];
        } else {
            HIP_TRY(hipMemcpyAsync(w.luctl_host, w.luctl, 2 * sizeof(LUCtl), hipMemcpyDeviceToHost, stream_));
            // the dense-step flags ride along (final once k_next == m): no separate round trip for them
            HIP_TRY(hipMemcpyAsync(h_dense, w.denseflag, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
            HIP_TRY(sync_stream());
        }
        last = w.luctl_host + (a.look ? ((enq - 1) & 1) : 0);
        if (w.luctl_host[0].fault || last->k_next >= m) break;
        // (every round performs at least the step it starts at — a listed column or a bookkeeping step; a batch that moved nothing
        // would repeat for ever: report it instead)
        if (last->k_next <= k_seen) return GOMILP_ERR_DEVICE;
        k_seen = last->k_next;
        oneshot = false;   // (the batch was too short: that pack came too early)
        batch = std::max(4, (int)(((int64_t)(m - last->k_next) * last->rounds) / std::max(1, last->k_next)) + 2);
        if (batch > 64) batch = 64;
    }
    lu_rounds_ = last->rounds;
    end->gave_up = w.luctl_host[0].fault != 0;
    end->landed = oneshot;
    end->enq = enq;
    if (plan.cross_G && !end->gave_up) { launch_luc_lpos_final(a, stream_); launches_++; }   // (that panel keeps its maps up to the last tied search only)
    return GOMILP_OK;
}

// Only the columns whose elimination step did arithmetic carry non-zero L / off-diagonal U entries (a unit-column
// step has zero multipliers and its column is zero in every earlier pivot row), so the host solves need those
// columns and the diagonal only: m*(nd+1) doubles cross PCIe instead of m*m.  dl: their list; the packed columns land in h_W, the
// diagonal in h_vec, the row positions in h_idx, the singular flag in st_host.
int Engine::pack_and_fetch(const LUArgs &a, const LuPlan &plan, std::vector<int32_t> &dl) {
    Work &w = *w_;
    const int m = a.m;
    int32_t *h_dense = w.h_idx + w.cap_m;
    dl.clear();
    if (plan.blocked) {
        if (!plan.compressed) {
            HIP_TRY(hipMemcpyAsync(h_dense, w.denseflag, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
            HIP_TRY(sync_stream());
        }
        for (int k = 0; k < m; k++) if (h_dense[k]) dl.push_back(k);
    } else {
        for (int k = 0; k < m; k++) dl.push_back(k);
    }
    const int nd = (int)dl.size();
    int rc = stage_upload(w.dlist, dl.data(), (size_t)nd * sizeof(int32_t));
    if (rc != GOMILP_OK) return rc;
    const bool split = plan.split(nd);
    if (split) launch_luc_pack_dense(a, w.dlist, nd, w.rho, w.Wd, w.ludiag, stream_);
    else if (plan.compressed) launch_luc_pack(a, w.dlist, nd, w.Wd, w.ludiag, stream_);
    else launch_lu_pack(a, w.dlist, nd, w.Wd, w.ludiag, stream_);
    launches_++;
    if (nd) HIP_TRY(hipMemcpyAsync(w.h_W, w.Wd, (size_t)(split ? nd : m) * nd * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipMemcpyAsync(w.h_vec, w.ludiag, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipMemcpyAsync(w.h_idx, w.lpos, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    if (plan.small)   // (the state block was not uploaded in front of this factorization: only the flag comes back)
        HIP_TRY(hipMemcpyAsync(&w.st_host->lu_singular, &w.st->lu_singular, sizeof(w.st_host->lu_singular), hipMemcpyDeviceToHost, stream_));
    else
        HIP_TRY(hipMemcpyAsync(w.st_host, w.st, sizeof(DevState), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(sync_stream());
    return GOMILP_OK;
}

// The factorization half of the final solve: gather, gonum-order LU on the device, the packed factors on the host (and, for the large
// bases, what the row kernel needs on the device).  Everything lu_solve needs stays in lu_cache_ / the work buffers until the next
// factorization: an exact step solves for x_B, for the entering column and for every Bland candidate from ONE factorization of ab
// (the reference factors again each time, simplex.go:289,315,356 — same matrix, same bits).
int Engine::lu_factor(const Problem &P, bool *singular, const int32_t *basic_host, bool transpose) {
    Work &w = *w_;
    const double tf0 = now_s();
    const int m = P.m;
    LuPlan plan = LuPlan::make(m, lu_blocked_, lu_look_, lu_cross_, lu_large_, bt_fault_, ((size_t)w.cap_m * w.cap_ld + 512) * sizeof(double));   // (the small-pack block fits Wd / h_W: ensure_work)
    lu_cache_.valid = false;
    int rc = gather_basis(P, plan, transpose);
    if (rc != GOMILP_OK) return rc;
    int nonunit = 0;
    if ((rc = upload_unit_rows(P, basic_host, transpose, &nonunit)) != GOMILP_OK) return rc;
    LookSlot look_slot(device_, plan.look_wanted);
    if (!look_slot.held) plan.look_wanted = false;
    LUArgs a;
    a.W = w.W; a.ldw = P.ld; a.m = m; a.lpos = w.lpos; a.rowstep = w.rowstep;
    for (int t = 0; t < 2; t++) { a.pk[t] = w.lpk[t]; a.pl[t] = w.lpl[t]; a.pr[t] = w.lpr[t]; }
    a.st = w.st;
    a.unit_row = w.unitrow;
    a.dense_flag = plan.blocked ? w.denseflag : nullptr;
    a.ctl = w.luctl; a.Lp = w.luLp; a.Up = w.luUp;
    a.slots = 1; a.look = plan.look_wanted ? 1 : 0;
    a.ctl_prev = a.ctl; a.Lp_prev = a.Lp; a.Up_prev = a.Up;
    a.rowsnap = w.rowstep + w.cap_m; a.rowsnap_prev = a.rowsnap;   // (launch_luc_rounds sets the round's parity)
    a.ctl_base = a.ctl; a.round = 0; a.pad3 = plan.inject_fault ? 1 : 0;
    if (plan.cross_G && !w.luxrec) {
        HIP_TRY(dmalloc(&w.luxrec, luc_cross_doubles()));
        HIP_TRY(hipMemsetAsync(w.luxrec, 0, luc_cross_doubles() * sizeof(double), stream_));
    }
    w.st_host->lu_singular = 0;
    if (!plan.small) sync_state_to_device();   // (small bases: k_luc_init clears the flag on the device, the packed block brings it back)
    lu_rounds_ = 0;
    LuRoundsEnd end;
    if (plan.compressed) {
        for (;;) {
            rc = run_compressed_rounds(a, plan, nonunit, &end);
            look_slot.drop();   // (the rounds are behind the last sync)
            if (rc != GOMILP_OK) return rc;
            if (!end.gave_up) break;
            if (!plan.step_down()) return GOMILP_ERR_DEVICE;
            a.look = 0; a.dense_flag = plan.blocked ? w.denseflag : nullptr;
            lu_look_faults_++; lu_look_fault_++;
            if (w.luxrec) HIP_TRY(hipMemsetAsync(w.luxrec, 0, luc_cross_doubles() * sizeof(double), stream_));   // (a launch that gave up has not recorded how far its sequence numbers went)
            if (GOMILP_DBG_ENV("GOMILP_DEBUG_LOOP")) fprintf(stderr, "final_solve: a look-ahead launch gave up a wait (m %d, rounds enqueued %d, cnt_x %u cnt_u %u cnt_s %u): plain schedule\n", m, end.enq, w.luctl_host[0].cnt_x, w.luctl_host[0].cnt_u, w.luctl_host[0].cnt_s);
            if ((rc = gather_basis(P, plan, transpose)) != GOMILP_OK) return rc;
            if (!plan.compressed) { lu_rounds_ = 0; sync_state_to_device(); launch_lu(a, stream_); launches_ += m + 2; end = LuRoundsEnd(); break; }
        }
    } else if (plan.blocked) launches_ += launch_lu_blocked(a, w.rho, stream_) + 1;
    else { launch_lu(a, stream_); launches_ += m + 2; }
    std::vector<int32_t> dl;
    if (end.landed) {   // everything is on the host already, all m columns
        dl.resize(m);
        for (int k = 0; k < m; k++) dl[k] = k;
        const int32_t *h_dense = w.h_idx + w.cap_m;
        lu_dense_ = 0;   // steps that did arithmetic (stats)
        for (int k = 0; k < m; k++) lu_dense_ += h_dense[k] != 0;
    } else {
        if ((rc = pack_and_fetch(a, plan, dl)) != GOMILP_OK) return rc;
        lu_dense_ = (int64_t)dl.size();
    }
    const int nd = (int)dl.size();
    HIP_TRY(hipGetLastError());
    const double tf1 = now_s();
    fs_device_ += tf1 - tf0;
    std::vector<int32_t> phys(m);
    for (int R = 0; R < m; R++) phys[w.h_idx[R]] = R;
    const double *diag = w.h_vec;
    *singular = w.st_host->lu_singular != 0 || lu_det_is_zero(diag, phys.data(), m);
    if (*singular && GOMILP_DBG_ENV("GOMILP_DEBUG_LOOP")) {
        int nz = 0; double dmin = 1e300, logdet = 0;
        for (int i = 0; i < m; i++) { if (diag[phys[i]] == 0) nz++; dmin = std::min(dmin, fabs(diag[phys[i]])); logdet += log(fabs(diag[phys[i]])); }
        fprintf(stderr, "final_solve: singular (transpose %d, m %d, nd %d, rounds %lld, lu_singular flag %d, logdet %g, zero diagonals %d, min |u_ii| %g, compressed %d)\n",
                (int)transpose, m, nd, (long long)lu_rounds_, (int)w.st_host->lu_singular, logdet, nz, dmin, (int)plan.compressed);
    }
    lu_cache_.m = m; lu_cache_.nd = nd; lu_cache_.split = !end.landed && plan.split(nd); lu_cache_.singular = *singular;
    lu_cache_.phys = phys; lu_cache_.dl = dl;
    lu_cache_.diag.assign(diag, diag + m);   // (h_vec is everybody's landing buffer)
    lu_cache_.args = a;
    lu_cache_.valid = true;
    fs_host_ += now_s() - tf1;
    return GOMILP_OK;
}

// The solve half (Dgetrs, lapack/gonum/dgetrs.go:37-45) from the factors lu_factor left: rhs_host (m entries, by basis position;
// default b).  A singular factorization gives zeros (the caller has the flag).
int Engine::lu_solve(const Problem &P, std::vector<double> &x, const double *rhs_host) {
    Work &w = *w_;
    const LuCache &c = lu_cache_;
    if (!c.valid || c.m != P.m) return GOMILP_ERR_DEVICE;
    const double tf1 = now_s();
    const int m = P.m, nd = c.nd;
    const double *rhs = rhs_host ? rhs_host : P.hb.data();
    x.assign(m, 0.0);
    if (c.singular) return GOMILP_OK;
    if (!c.split) {   // one host pass over all rows
        lu_host_solve(m, nd, c.dl.data(), c.phys.data(), c.diag.data(), w.h_W, rhs, x.data());
        fs_host_ += now_s() - tf1;
        return GOMILP_OK;
    }
    // large bases: only the nd x nd part that couples the dense positions went to the host (lu_compressed.hip, k_luc_pack_dense);
    // every other row is independent of the rest and is solved on the device (k_luc_solve_rows)
    const double *rhs_dev = P.db;
    if (rhs_host) {   // the row kernel reads the right-hand side on the device
        int rcr = stage_upload(w.move, rhs_host, (size_t)m * sizeof(double));
        if (rcr != GOMILP_OK) return rcr;
        rhs_dev = w.move;
    }
    std::vector<double> xdl(nd), xdu(nd);
    lu_host_solve_coupled(nd, c.dl.data(), c.phys.data(), c.diag.data(), w.h_W, rhs, xdl.data(), xdu.data());
    fs_host_ += now_s() - tf1;
    const double tf2 = now_s();
    double *dxl = w.yscratch, *dxu = w.yscratch + P.ld, *dx = w.yscratch + 2 * (size_t)P.ld;   // 64 * ld doubles
    int rcs = stage_upload(dxl, xdl.data(), (size_t)nd * sizeof(double));
    if (rcs == GOMILP_OK) rcs = stage_upload(dxu, xdu.data(), (size_t)nd * sizeof(double));
    if (rcs != GOMILP_OK) return rcs;
    launch_luc_solve_rows(c.args, w.dlist, nd, rhs_dev, dxl, dxu, dx, stream_);
    launches_++;
    HIP_TRY(hipMemcpyAsync(w.h_vec, dx, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIP_TRY(sync_stream());
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < m; i++) x[i] = w.h_vec[i];
    for (int s = 0; s < nd; s++) x[c.dl[s]] = xdu[s];
    fs_device_ += now_s() - tf2;
    return GOMILP_OK;
}

}  // namespace gomilp
