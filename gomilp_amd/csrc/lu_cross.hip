// The panel of the compressed gonum-order LU (lu_compressed.hip) with its ROWS on the workgroups of one XCD (knob lu_cross; the default for bases of 1281 .. 2048 rows).
//
// k_luc_panel_slots runs a round's dense steps on ONE workgroup of sixteen waves: a dense step is the issue time of those waves on the four
// SIMDs of one CU (7.7 k cycles, DESIGN.md section 2.3 "Round 5").  Here G workgroups of four waves (one per SIMD) hold 256 rows each, one
// row per lane, the same NB register slots; everything a step decides is decided by every workgroup from the same values:
//   * the index maps (lpos / rowat / unit / ucol / active) and the slot tables are REPLICATED — every workgroup keeps all m rows' maps in LDS;
//     the bookkeeping runs are off the chain: a row knows the step that retires it, and the interchanges are replayed on the maps (from the
//     log of pivot rows, by every workgroup alike) only when a pivot search finds two rows with the same |a_ik|;
//   * the pivot search is local (four waves), then ONE exchange through the XCD's L2 (bt_loop.h: records of {sequence number, value}
//     slots, sequence-tagged so that no flag separates data from "ready"): the workgroup's candidate posts
//     {max |a_ik|, how many of its rows attain it, one of them, 1 / a_ik, the XCC id, that row's entries in the NB slots}; every wave polls
//     the G records; ONE row in the whole panel attaining the maximum is the pivot row — otherwise (dgetf2.go:38: the first maximum in
//     LAPACK's row order) the maps are brought up to date and a further exchange of logical positions decides — and the pivot row's entries
//     for the elimination came with the same load;
//   * the owner of the pivot row does the global bookkeeping (rowstep, pivrow, the control block's step list, the U row's stores).
// Same arithmetic, same step order, same round structure as the one-workgroup panel (k_luc_usolve / k_luc_trail follow unchanged): the
// schedules are compared bit for bit (tests/test_gpu_parity.py, tests/test_gpu_lu_cross_look.py).  Waits are bounded: a workgroup that runs
// out of patience raises the control block's fault flag, every workgroup leaves, and the host repeats the factorization (below).
// Two widths (knob lu_cross):
//   1  16 register slots, the plain schedule (three launches per round) — the form of round 5, kept as it was;
//   2  32 slots in two register tuples of 16 (a uniform dynamic index reaches 16 doubles; no scratch): one compute unit's registers hold 16
//      slots for 2048 rows, so the one-workgroup panel's rounds end after ~17 of the 32 steps a round may take (every freed slot goes to a
//      column whose step lies far ahead) — 23 rounds at the metric size; with one row per lane there is room for 32: 12 rounds.  The record
//      grows to 37 slots (five 16-byte loads per lane and poll).  Under lu_blocked = 3 this panel is the PANEL ROLE of the look-ahead launch
//      (luc_role.h): blocks 0, 8, .., 8 (G - 1) are the panel, every other block (index remapped) finishes the round before beside it; the
//      panel hands over what k_luc_panel_slots<.., true> hands over — LUCtl::next / nnext (the scan the next panel runs anyway), the rowstep
//      snapshot (every lane knows its own row), Lp / Up / control block by round parity — and waits for cnt_u before its column loads.
//      The legality argument of the look-ahead carries over unchanged: phase T leaves alone the columns the panel
//      loads and the unit columns of rows still active when the round before ended (the only columns this panel writes: a listed column,
//      or the unit column of the row a dense step takes), and every read of the round's pivot rows in phase U's columns is behind cnt_s
//      before workgroup 0 writes their U entries.
// Rows per lane (RPT; workgroup g owns the rows [256 RPT g, 256 RPT (g + 1)), lane t of it the rows 256 RPT g + 256 r + t, r < RPT):
//   1  bases of up to 2048 rows, G = 2 / 4 / 8 workgroups, both widths, both schedules; the maps take 9 bytes per row: 18,432 B of LDS at G = 8;
//   4  bases of 4097 .. 8192 rows (knob lu_large, off by default; luc_large_rpt), eight workgroups, both widths, plain schedule: 73,728 B;
//   8  bases of 8193 .. 16384 rows (lu_large), eight workgroups, 16 slots (one register tuple per row), plain schedule: 147,456 B.
// ONE kernel body serves all three.  What several rows per lane ask for: the local search and the count of rows attaining the maximum
// run over a lane's RPT rows; the poster of a record is one (lane, row) pair — reached by a static unroll over r, never a per-lane
// register index —; every row of a lane takes the elimination update (a row index no lane has an active row at is skipped); the step
// that retires a row is kept per row; with eight rows the entries of column k are read again where they are needed instead of held in
// 16 more registers across the exchange.  With one row per lane all of this folds to a single row's registers.
// Fall-backs (engine_final.cpp LuPlan::step_down, one stats.device_retries each): a look-ahead launch that gave up a wait -> the SAME panel in the plain
// schedule (the rounds stay what they were); an exchange of the panel that gave up -> the one-workgroup panel, or, beyond 4096 rows
// (where there is none), one launch per column.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bt_loop.h"
#include "device_types.h"
#include "kernels_common.h"
#include "luc_role.h"

namespace gomilp {

namespace {

constexpr int kLxSlots = 24;          // slots per record of the 16-slot panel: 4 header values + 16 + the XCC id + 3 spare (three loads per lane and poll)
constexpr int kLxSlots32 = 40;        // ... of the 32-slot panel: 4 + 32 + 1 + 3 spare (five loads)
constexpr int kLxHeader = 16;         // doubles in front of the records: [0] = exchanges completed so far
constexpr int kLxSpinLimit = 400000;  // polls (~1 us each)

__device__ __forceinline__ void lx_load3(const xpair *p0, const xpair *p1, const xpair *p2, xpair (&v)[3]) {
    asm volatile("global_load_dwordx4 %0, %3, off sc1\n\tglobal_load_dwordx4 %1, %4, off sc1\n\tglobal_load_dwordx4 %2, %5, off sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]) : "v"(p0), "v"(p1), "v"(p2) : "memory");
}

__device__ __forceinline__ void lx_load3_fast(const xpair *p0, const xpair *p1, const xpair *p2, xpair (&v)[3]) {   // (never served by L1: the XCD's L2 is the coherence point of its CUs)
    asm volatile("global_load_dwordx4 %0, %3, off nt\n\tglobal_load_dwordx4 %1, %4, off nt\n\tglobal_load_dwordx4 %2, %5, off nt\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]) : "v"(p0), "v"(p1), "v"(p2) : "memory");
}

// five slots of a record, 128 bytes apart (lane l: slots (l & 7) + 8 r of record l >> 3)
__device__ __forceinline__ void lx_load5(const xpair *p, xpair (&v)[5]) {
    asm volatile("global_load_dwordx4 %0, %5, off sc1\n\tglobal_load_dwordx4 %1, %5, off offset:128 sc1\n\tglobal_load_dwordx4 %2, %5, off offset:256 sc1\n\t"
                 "global_load_dwordx4 %3, %5, off offset:384 sc1\n\tglobal_load_dwordx4 %4, %5, off offset:512 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]) : "v"(p) : "memory");
}
__device__ __forceinline__ void lx_load5_fast(const xpair *p, xpair (&v)[5]) {
    asm volatile("global_load_dwordx4 %0, %5, off nt\n\tglobal_load_dwordx4 %1, %5, off offset:128 nt\n\tglobal_load_dwordx4 %2, %5, off offset:256 nt\n\t"
                 "global_load_dwordx4 %3, %5, off offset:384 nt\n\tglobal_load_dwordx4 %4, %5, off offset:512 nt\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]) : "v"(p) : "memory");
}

}  // namespace

#ifdef GOMILP_DEBUG
__device__ unsigned long long g_lux_stamps[4 * 16];
#define LUX_STAMP(S)                                                                      \
    do {                                                                                  \
        unsigned long long t_;                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");        \
        __builtin_amdgcn_sched_barrier(0);                                                \
        if ((S) >= 0) tacc[(S) >= 0 ? (S) : 0] += t_ - tprev;                             \
        tprev = t_;                                                                       \
    } while (0)
#else
#define LUX_STAMP(S) do { } while (0)
#endif

// NB: register slots — 16 (one tuple) or 32 (two tuples of 16 behind a uniform branch: the widest a uniform dynamic index reaches).
// LK: the panel role of the look-ahead launch (luc_role.h): blocks 0, 8, .., 8 (G - 1) are the panel, every other block finishes the round
// before beside it.
// RPT: rows per lane — 1, 4 or 8 (above).
template <int G, int RPT, int NB, int SMAX, bool LK>
__global__ __launch_bounds__(256) void k_luc_panel_x(LUArgs a, int32_t *__restrict__ pivrow, xpair *__restrict__ xrec) {
    constexpr int T = 256, NW = 4, MAXM = 256 * RPT * G;
    static_assert((NB == 16 || NB == 32) && SMAX <= 32 && G <= 8, "register tuples of 16 slots; lane l polls record l >> 3");
    static_assert(RPT == 1 || ((RPT == 4 || RPT == 8) && G == 8), "several rows per lane: the eight-workgroup panel");
    static_assert(!LK || RPT == 1, "the look-ahead role: one row per lane");
    static_assert(RPT < 8 || NB == 16, "eight rows per lane: one tuple of 16 slots");
    static_assert(MAXM <= 16384, "rows below 16384 fit (cnt << 16) | row in redL");
    constexpr bool KEEPX = RPT <= 4;                         // column k's entries are held across the exchange (eight rows: read again, below)
    constexpr int NH = NB / 16;                              // register tuples
    constexpr int NSL = NB == 16 ? kLxSlots : kLxSlots32;    // slots per record
    constexpr int NLD = NSL / 8;                             // loads per lane and poll
    constexpr int NUSE = 5 + NB;                             // slots a record uses: 4 header values, NB entries, the XCC id
    typedef unsigned short idx_t;
    typedef double vec __attribute__((ext_vector_type(16)));
    constexpr idx_t NONE = 0xFFFF;
    const int bx = (int)blockIdx.x;
    if ((bx & 7) || (bx >> 3) >= G) {   // blocks 0, 8, 16, ... land on one XCD (round-robin deal): the panel
        if constexpr (LK) {             // the others: the previous round's U-solve and update (plain launch: they leave at once)
            if (!a.ctl_base->fault) luc_role<T, SMAX, true>(a, bx - min(G, (bx + 7) >> 3), (int)gridDim.x - G);
        }
        return;
    }
    const int g = bx >> 3;
    __shared__ idx_t s_lpos[MAXM];
    __shared__ idx_t s_rowat[MAXM];
    __shared__ idx_t s_unit[MAXM];
    __shared__ idx_t s_ucol[MAXM];
    __shared__ unsigned char s_active[MAXM];
    __shared__ double redM[2][NW];
    __shared__ unsigned int redL[2][NW];
    __shared__ int s_slotcol[NB];
    __shared__ int s_nload, s_stop, s_limit, s_sigma;
    __shared__ __attribute__((aligned(16))) double s_post[NW][NSL];   // a wave's candidate hands its record to the wave's lanes: one store instruction posts it
    if (a.ctl_base->fault) return;
    LUCtl *ctl = a.ctl;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m = a.m;
    const size_t ldw = (size_t)a.ldw;
    const int k0 = a.ctl_prev->k_next;
    if (k0 >= m) {
        if (g == 0 && tid == 0) luc_ctl_empty(ctl, a.ctl_prev, k0, true);
        return;
    }
#ifdef GOMILP_DEBUG
    unsigned long long tacc[16] = {}, tprev = 0;   // segments 0 .. 8: the step loop; 9 index maps, 10 the wait for phase U, 11 column loads, 12 what follows the loop
#endif
    LUX_STAMP(-1);
    for (int R = tid; R < MAXM; R += T) {
        const bool in = R < m;
        s_lpos[R] = (idx_t)(in ? a.lpos[R] : R);
        s_active[R] = (in && a.rowstep[R] < 0) ? 1 : 0;
        const int ur = (in && a.unit_row) ? a.unit_row[R] : -1;
        s_unit[R] = ur < 0 ? NONE : (idx_t)ur;
        s_ucol[R] = NONE;
    }
    __syncthreads();
    for (int R = tid; R < m; R += T) {
        s_rowat[s_lpos[R]] = (idx_t)R;
        if (s_unit[R] != NONE && R >= k0) s_ucol[s_unit[R]] = (idx_t)R;   // column R (still to come) is the unit vector of row s_unit[R]
    }
    for (;;) {   // (two unit columns with the same row — a singular basis —: the FIRST of them is the one whose step retires the row)
        __syncthreads();
        bool again = false;
        for (int R = tid; R < m; R += T)
            if (s_unit[R] != NONE && R >= k0 && R < (int)s_ucol[s_unit[R]]) { s_ucol[s_unit[R]] = (idx_t)R; again = true; }
        if (!__syncthreads_or(again)) break;
    }
    if (w == 0) {   // the columns this round loads
        const int n = luc_scan_dense<NB>(k0, m, s_unit, s_active, s_slotcol);
        if (lane == 0) s_nload = n;
    }
    __syncthreads();
    const int nload = s_nload;
    int myslotcol = (lane < NB && lane < nload) ? s_slotcol[lane < NB ? lane : 0] : 0x7FFFFFFF;
    int myslotin = -1;
    unsigned int live = nload >= 32 ? 0xFFFFFFFFu : ((1u << nload) - 1u);
    const int R0 = g * (T * RPT) + tid;   // this lane's rows: R0 + 256 r
    bool act[RPT];
    int myucol[RPT];   // the step that retires the row unless a dense step takes it first
#pragma unroll
    for (int r = 0; r < RPT; r++) {
        const int R = R0 + T * r;
        act[r] = (R < m) && s_active[R < m ? R : 0];
        const idx_t uc0 = s_ucol[R < m ? R : 0];
        myucol[r] = (act[r] && uc0 != NONE) ? (int)uc0 : 0x7FFFFFFF;
    }
    LUX_STAMP(9);
    if constexpr (LK) {
        // the columns this panel loads are brought up to date by phase U of this launch (luc_role): wait for its workgroups
        if (tid == 0) s_stop = luc_spin(&a.ctl_base->cnt_u, (uint32_t)(a.round + 1) * (uint32_t)((m + 63) / 64)) ? 1 : 0;
        __syncthreads();
        if (!s_stop) {
            if (tid == 0) {
                a.ctl_base->fault = 1;
                if (g == 0) luc_ctl_empty(ctl, a.ctl_prev, k0, true);
            }
            return;
        }
    }
    LUX_STAMP(10);
    vec v[RPT][NH];
#pragma unroll
    for (int r = 0; r < RPT; r++) {
        const double *src = a.W + (act[r] ? R0 + T * r : 0);
        if constexpr (LK) {   // the cells come from phase U of this launch: agent scope
#pragma unroll
            for (int c = 0; c < NB; c++) v[r][c / 16][c % 16] = (act[r] && c < nload) ? luc_ld_agent(&src[(size_t)__builtin_amdgcn_readlane(myslotcol, c) * ldw]) : 0.0;
        } else {
#pragma unroll
            for (int c = 0; c < NB; c++) v[r][c / 16][c % 16] = (act[r] && c < nload) ? src[(size_t)__builtin_amdgcn_readlane(myslotcol, c) * ldw] : 0.0;
        }
    }
    __syncthreads();
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the column loads are retired in front of the loop (see k_luc_panel_slots)
    // exchanges: sequence numbers go on from launch to launch (header slot 0: written by workgroup 0 at the end of a launch)
    unsigned int myxcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(myxcc));
    myxcc &= 0xFu;
    bool fast = false;   // SAFE (sc1) accesses until an exchange has shown that all G workgroups sit on one XCD (slot 4 + NB of a record: the XCC id)
    const double seq0 = xrec[0][0];
    xpair *recs = xrec + kLxHeader / 2;   // [2 parities][G][NSL]
    int nx = 0;
    LUX_STAMP(11);
    int kcur = k0, s = 0, k1 = m;
    int ksync = a.ctl_prev->ksync;   // the index maps (lpos / rowat) hold the interchanges of the steps < ksync: the rest waits in the log (pivrow)
    bool fault = false;
#pragma unroll 1
    for (;;) {
        if (w == 0) {
            const unsigned int key = (lane < NB && ((live >> lane) & 1u)) ? (unsigned int)myslotcol : 0x7FFFFFFFu;
            unsigned int mn = row_min_u32(key);
            if constexpr (NB == 16) mn = (unsigned int)__builtin_amdgcn_readlane((int)mn, 0);
            else mn = min((unsigned int)__builtin_amdgcn_readlane((int)mn, 0), (unsigned int)__builtin_amdgcn_readlane((int)mn, 16));
            const bool listed = live != 0 && s < SMAX;
            const int limit = listed ? (int)mn : m;
            const unsigned long long hit = __ballot(key == mn && lane < NB);
            const int sigma = hit ? (int)__builtin_ctzll(hit) : 0;
            // run of bookkeeping steps [kcur, limit): only its END is needed on the chain — the first column whose step needs arithmetic.  A row
            // knows the step that retires it (myucol); LAPACK's logical row order — all the index maps are for — matters only when two rows tie in
            // a pivot search, and then every workgroup replays the interchanges since the last replay from the log of pivot rows (below).  With
            // ONE wave per SIMD the serial replay (1.8 k cycles per dense step) was on the chain: nobody to hide behind (section 2.3, "Round 5")
            int k = kcur;
            for (;;) {
                const int kk = k + lane;
                const idx_t ur = kk < limit ? s_unit[kk] : NONE;
                const bool triv = ur != NONE && s_active[ur] && (int)s_ucol[ur] == kk;   // (a second unit column of the same row finds it used: arithmetic)
                const unsigned long long nt = __ballot(!triv);
                const int cnt = nt ? (int)__builtin_ctzll(nt) : 64;
                k += cnt;
                if (cnt < 64) break;
            }
            if (lane == 0) { s_stop = k; s_limit = limit; s_sigma = sigma; }
        }
        LUX_STAMP(0);   // wave 0: next column + the run
        __syncthreads();
        LUX_STAMP(1);
        const int kstop = s_stop, limit = s_limit;
        const int sigma = __builtin_amdgcn_readfirstlane(s_sigma) & (NB - 1);
        // the rows of the run leave the active set on every workgroup's copy of the map (every column of the run is the unit column of an active row)
        for (int c = kcur + tid; c < kstop; c += T) s_active[s_unit[c]] = 0;
        // rows of this lane retired by the run (the step of their unit column lies in it): their entries in the listed columns are final U entries
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            if (act[r] && myucol[r] >= kcur && myucol[r] < kstop) {
                const int R = R0 + T * r, kt = myucol[r];
                a.rowstep[R] = kt; pivrow[kt] = R;
                double *dst = a.W + R;
#pragma unroll
                for (int c = 0; c < NB; c++)
                    if ((live >> c) & 1u) dst[(size_t)__builtin_amdgcn_readlane(myslotcol, c) * ldw] = v[r][c / 16][c % 16];
                act[r] = false;
            }
        }
        if (kstop < limit || live == 0 || s >= SMAX) { k1 = kstop; break; }
        const int k = limit;
        LUX_STAMP(2);
        // ---- dense step k on slot sigma: this workgroup's candidate among the RPT rows of every lane
        double xk[KEEPX ? RPT : 1];
        if constexpr (KEEPX) {
#pragma unroll
            for (int r = 0; r < RPT; r++) {
                if constexpr (NH == 1) xk[r] = v[r][0][sigma];   // uniform index
                else {   // (the empty asm keeps the uniform branch a branch: see k_luc_panel_slots)
                    if (sigma < 16) { asm volatile(""); xk[r] = v[r][0][sigma & 15]; }
                    else { asm volatile(""); xk[r] = v[r][NH - 1][sigma & 15]; }
                }
            }
        }
        auto xof = [&](int r) -> double { if constexpr (KEEPX) return xk[r]; else return v[r][0][sigma]; };
        auto xmof = [&](int r) -> double { return act[r] ? -fabs(xof(r)) : __builtin_inf(); };
        double xml = __builtin_inf();   // the lane's maximum over its rows (one row: the value as it is — fmin would turn a NaN into +inf)
        if constexpr (RPT == 1) xml = xmof(0);
        else {
#pragma unroll
            for (int r = 0; r < RPT; r++) xml = fmin(xml, xmof(r));
        }
        // one exchange: the wave that holds the workgroup's candidate hands the record {h0, h1, row, 1 / a_ik, XCC id | the row's entries in the NB
        // slots} to its lanes (LDS, no barrier: one wave), which post it with ONE store instruction; every wave then polls the G records —
        // lane l reads the slots (l & 7), + 8, + 16 (+ 24, + 32 with 32 slots) of record l >> 3.
        // pr: the row (index r) of this lane that posts, -1: this lane does not post
        xpair rv[NLD];
        auto exchange = [&](int pr, double h0, double h1) {
            const double seq = seq0 + (double)(nx + 1);
            xpair *mine = recs + ((size_t)((nx + 1) & 1) * G + g) * NSL;
            if (__any(pr >= 0)) {   // (uniform per wave)
                double *sp = s_post[w];
                if (pr >= 0) {
                    sp[0] = h0; sp[1] = h1;
#pragma unroll
                    for (int r = 0; r < RPT; r++) {
                        if (pr == r) {
                            sp[2] = (double)(R0 + T * r);
                            sp[3] = act[r] ? 1.0 / xof(r) : 0.0;   // dgetf2.go:54-56 scales by the reciprocal
#pragma unroll
                            for (int c = 0; c < NB; c++) sp[4 + c] = v[r][c / 16][c % 16];
                        }
                    }
                    sp[4 + NB] = (double)myxcc;
                }
                __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the candidate's LDS writes have landed (same wave: in order)
                if (lane < NUSE) xstore(mine + lane, xpair{seq, sp[lane]}, fast);
            }
            const xpair *base = recs + (size_t)((nx + 1) & 1) * G * NSL;
            const int g2 = lane >> 3, j0 = lane & 7;
            const bool mineok = g2 < G;
            const xpair *q0 = base + (size_t)(mineok ? g2 : 0) * NSL + j0;
            for (int it = 0;; it++) {
                if constexpr (NLD == 3) { if (fast) lx_load3_fast(q0, q0 + 8, q0 + 16, rv); else lx_load3(q0, q0 + 8, q0 + 16, rv); }
                else { if (fast) lx_load5_fast(q0, rv); else lx_load5(q0, rv); }
                bool ok = true;   // the slots a record uses: 0 .. 4 + NB
#pragma unroll
                for (int r = 0; r < NLD; r++) ok = ok && (j0 + 8 * r >= NUSE || rv[r][0] == seq);
                ok = ok || !mineok;
                if (__all(ok)) break;
                if (it >= kLxSpinLimit) { fault = true; break; }
                __builtin_amdgcn_s_sleep(1);
            }
            nx++;
        };
        const bool head = (lane & 7) == 0 && (lane >> 3) < G;   // a record's header sits in the lanes 8 g2 .. 8 g2 + 4
        // ---- this workgroup's candidate: its maximum, how many of its rows attain it (several rows of one lane count each), and one of them
        // (the smallest physical row)
        const double wm = wave_min_f64(xml);
        unsigned int cntw = 0, lk = 0xFFFFFFFFu;
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            const bool hit = act[r] && xmof(r) == wm;
            cntw += (unsigned int)__popcll(__ballot(hit));
            lk = min(lk, hit ? (unsigned int)(R0 + T * r) : 0xFFFFFFFFu);
        }
        lk = row_min_u32(lk);
        lk = min(min((unsigned int)__builtin_amdgcn_readlane((int)lk, 15), (unsigned int)__builtin_amdgcn_readlane((int)lk, 31)),
                 min((unsigned int)__builtin_amdgcn_readlane((int)lk, 47), (unsigned int)__builtin_amdgcn_readlane((int)lk, 63)));
        double *rm = redM[s & 1];
        unsigned int *rl = redL[s & 1];
        if (lane == 0) { rm[w] = wm; rl[w] = (min(cntw, 2u) << 16) | (lk & 0xFFFFu); }
        LUX_STAMP(3);   // own search
        __syncthreads();
        LUX_STAMP(4);
        const double bx = lane < NW ? rm[lane] : __builtin_inf();
        const double bml = readlane_f64(row_min_f64(bx), 15);
        const unsigned int infol = (lane < NW && bx == bml) ? rl[lane] : 0u;
        const unsigned int cntl = (unsigned int)__popcll(__ballot((infol >> 16) >= 1u)) + (unsigned int)__popcll(__ballot((infol >> 16) >= 2u));   // (0 without an active row)
        const unsigned int rowl = (unsigned int)__builtin_amdgcn_readlane((int)row_min_u32((lane < NW && (infol >> 16) >= 1u) ? (infol & 0xFFFFu) : 0xFFFFFFFFu), 15);
        int pr = -1;
        if (cntl) {
#pragma unroll
            for (int r = 0; r < RPT; r++) pr = (act[r] && (unsigned int)(R0 + T * r) == rowl) ? r : pr;
        } else if (tid == 0) pr = 0;
        exchange(pr, cntl ? bml : __builtin_inf(), (double)min(cntl, 2u));
        if (fault) break;
        LUX_STAMP(5);   // local pick + post + poll
        if (!fast) {   // every record carries its workgroup's XCC id: all equal -> the XCD's L2 is the coherence point, plain stores / nt loads from here on
            const double xc = __shfl(rv[(4 + NB) >> 3][1], (lane & ~7) + 4);   // slot 4 + NB
            fast = __all(!head || xc == (double)myxcc);
        }
        const double wmL = head ? rv[0][1] : __builtin_inf();
        const double bm = wave_min_f64(wmL);
        const double cnL = __shfl(rv[0][1], (lane & ~7) + 1);
        const unsigned long long at1 = __ballot(head && wmL == bm && cnL >= 1.0), at2 = __ballot(head && wmL == bm && cnL >= 2.0);
        int gw;
        if (__popcll(at1) == 1 && at2 == 0) {
            gw = (int)__builtin_ctzll(at1) >> 3;   // ONE row in the whole panel attains the maximum: the pivot row, whatever its logical position
        } else {
            // several rows with the same |a_ik| (or none): dgetf2.go:38 takes the first in LAPACK's logical row order.  (1) an exchange behind
            // which every workgroup's stores to the log have landed; (2) every workgroup replays the interchanges of the steps [ksync, k) on its
            // copy of the maps — the pivot row of step j is pivrow[j], whoever performed it (dlaswp.go); (3) the positions decide: a second
            // exchange of {smallest logical position among the workgroup's tied rows, ...}
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            exchange(tid == 0 ? 0 : -1, 0.0, 0.0);
            if (fault) break;
            if (w == 0) {
                for (int j0 = ksync; j0 < k; j0 += 64) {
                    const int jj = j0 + lane;
                    const int pj = jj < k ? __hip_atomic_load(&pivrow[jj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
                    const int nrep = min(64, k - j0);
                    for (int t = 0; t < nrep; t++) {
                        const int Pj = __builtin_amdgcn_readlane(pj, t);
                        if (lane == 0) {
                            const idx_t jq = s_lpos[Pj], Q = s_rowat[j0 + t];   // dlaswp.go: the row at logical j trades places with the pivot row
                            s_lpos[Q] = jq; s_rowat[jq] = Q;
                            s_lpos[Pj] = (idx_t)(j0 + t); s_rowat[j0 + t] = (idx_t)Pj;
                        }
                    }
                }
            }
            ksync = k;
            __syncthreads();
            unsigned int lpmine = 0xFFFFFFFFu;   // the smallest logical position among this lane's tied rows, and which row it is
            int rmine = 0;
#pragma unroll
            for (int r = 0; r < RPT; r++) {
                const bool tied = act[r] && xmof(r) == bm;
                const unsigned int lpr = tied ? (unsigned int)s_lpos[tied ? R0 + T * r : 0] : 0xFFFFFFFFu;
                rmine = lpr < lpmine ? r : rmine;
                lpmine = min(lpmine, lpr);
            }
            unsigned int lp = row_min_u32(lpmine);
            lp = min(min((unsigned int)__builtin_amdgcn_readlane((int)lp, 15), (unsigned int)__builtin_amdgcn_readlane((int)lp, 31)),
                     min((unsigned int)__builtin_amdgcn_readlane((int)lp, 47), (unsigned int)__builtin_amdgcn_readlane((int)lp, 63)));
            unsigned int *rt = redL[(s & 1) ^ 1];
            if (lane == 0) rt[w] = lp;
            __syncthreads();
            const unsigned int lpl = (unsigned int)__builtin_amdgcn_readlane((int)row_min_u32(lane < NW ? rt[lane] : 0xFFFFFFFFu), 15);
            const bool any_l = lpl != 0xFFFFFFFFu;
            exchange(any_l ? (lpmine == lpl ? rmine : -1) : (tid == 0 ? 0 : -1), any_l ? (double)lpl : __builtin_inf(), 0.0);
            if (fault) break;
            const double lpL = head ? rv[0][1] : __builtin_inf();
            const double blp = wave_min_f64(lpL);
            const unsigned long long won = __ballot(head && lpL == blp);
            gw = won ? ((int)__builtin_ctzll(won) >> 3) : 0;
        }
        const int P = (int)readlane_f64(rv[0][1], 8 * gw + 2);
        const double rinv = readlane_f64(rv[0][1], 8 * gw + 3);
        // lane c: the pivot row's value in slot c = record slot 4 + c: lane 8 gw + ((4 + c) & 7), register (4 + c) >> 3
        double prl;
        {
            const int c = lane & (NB - 1);
            const int src = 8 * gw + ((4 + c) & 7), rr = (4 + c) >> 3;
            prl = __shfl(rv[0][1], src);
#pragma unroll
            for (int r = 1; r < NLD; r++) {
                const double br = __shfl(rv[r][1], src);
                prl = rr == r ? br : prl;
            }
        }
        LUX_STAMP(6);   // pick
        // the pivot row leaves the active set on every workgroup's copy of the map; the interchange itself (dlaswp.go) waits in the log
        if (tid == 0 && P >= 0 && P < MAXM) s_active[P] = 0;
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            if (act[r] && R0 + T * r == P) {   // the owner of the pivot row
                act[r] = false;
                a.rowstep[P] = k; pivrow[k] = P;
                if (a.dense_flag) a.dense_flag[k] = 1;
                ctl->steps[s] = k; ctl->prow[s] = P;
                double *dst = a.W + (R0 + T * r);   // the pivot row's U entries (slot sigma holds column k); the lane's own address: with the uniform P the scalar unit forms all NB of them, one after the other
#pragma unroll
                for (int cc = 0; cc < NB; cc++)
                    if ((live >> cc) & 1u) dst[(size_t)__builtin_amdgcn_readlane(myslotcol, cc) * ldw] = v[r][cc / 16][cc % 16];
                if (readlane_f64(prl, sigma) == 0) a.st->lu_singular = 1;
            }
        }
        const idx_t uc = (P >= 0 && P < MAXM) ? s_ucol[P] : NONE;
        const int k2 = (uc != NONE && (int)uc > k) ? (int)uc : -1;   // taking row P makes its unit column (if still to come) dense
        LUX_STAMP(7);   // pick + bookkeeping
        const double piv = readlane_f64(prl, sigma);
        const bool singular = (piv == 0);  // dgetf2.go:48-49
        double *wcol = a.W + (size_t)k * ldw;
        double *lcol = a.Lp + (size_t)s * ldw;
        const unsigned int others = live & ~(1u << sigma);
        const double prz = (lane < NB && ((others >> (lane & 31)) & 1u)) ? prl : 0.0;
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            const int R = R0 + T * r;
            double nl = 0.0;
            if (act[r]) {
                const double xr = xof(r);
                const double l = singular ? xr : __dmul_rn(xr, rinv);
                wcol[R] = l;
                nl = singular ? 0.0 : -l;
                lcol[R] = nl;
            } else if (R < a.ldw) lcol[R] = 0.0;
            if (!singular && __any(act[r])) {   // (a row index at which no lane of the wave has an active row is not read again)
#pragma unroll
                for (int c = 0; c < NB; c++) {
                    const double pc = readlane_f64(prz, c);
                    v[r][c / 16][c % 16] = __dadd_rn(__dmul_rn(nl, pc), v[r][c / 16][c % 16]);
                }
            }
            if (k2 >= 0) {
                const double vn = (act[r] && !singular) ? __dadd_rn(__dmul_rn(nl, 1.0), 0.0) : 0.0;
                if constexpr (NH == 1) { asm volatile(""); v[r][0][sigma] = vn; }   // (the uniform branch on k2 stays a branch too: not a select over the tuple)
                else {
                    if (sigma < 16) { asm volatile(""); v[r][0][sigma & 15] = vn; }
                    else { asm volatile(""); v[r][NH - 1][sigma & 15] = vn; }
                }
            }
        }
        if (k2 >= 0) {
            if (lane == sigma) { myslotcol = k2; myslotin = k; }
        } else live = others;
        s++;
        kcur = k + 1;
        LUX_STAMP(8);   // elimination
    }
    if (fault) {
        if (lane == 0) a.ctl_base->fault = 1;
        return;
    }
    if constexpr (LK) {
        // rowstep as this round leaves it, for the update workgroups that run beside the next panel: every lane knows its own row (the step
        // that took it was stored by this lane, or by an earlier launch)
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            const int R = R0 + T * r;
            if (R < m) a.rowsnap[R] = act[r] ? -1 : a.rowstep[R];
        }
    }
    if (g != 0) return;
    __syncthreads();   // the last run's rows have left s_active (the scan below reads it)
    for (int R2 = tid; R2 < m; R2 += T) a.lpos[R2] = s_lpos[R2];
    int ndl = 0;
    if (w == 0) {
        if constexpr (LK) {
            // the columns the next round's panel will load: its own scan (above), run on the state this round leaves
            const int n = luc_scan_dense<NB>(k1, m, s_unit, s_active, ctl->next);
            if (lane == 0) ctl->nnext = n;
        } else if (lane == 0) ctl->nnext = 0;
        const bool on = lane < NB && ((live >> lane) & 1u);
        const unsigned long long msk = __ballot(on);
        ndl = __popcll(msk);
        if (on) {
            const int at = __popcll(msk & ((1ull << lane) - 1ull));
            ctl->dropcol[at] = myslotcol; ctl->dropin[at] = myslotin; ctl->dropout[at] = k1;
        }
    }
    if (tid == 0) {
        ctl->k0 = k0; ctl->k1 = k1; ctl->k_next = k1; ctl->nsteps = s; ctl->ndrop = ndl;
        ctl->rounds = a.ctl_prev->rounds + 1; ctl->ksync = ksync;
        xrec[0] = xpair{seq0 + (double)nx, 0.0};
    }
    LUX_STAMP(12);
#ifdef GOMILP_DEBUG
    if (lane == 0) {   // (workgroup 0; a launch that gave up a wait is not counted)
        for (int sg = 0; sg < 13; sg++) atomicAdd(&g_lux_stamps[w * 16 + sg], tacc[sg]);
        if (w == 0) { atomicAdd(&g_lux_stamps[15], (unsigned long long)s); atomicAdd(&g_lux_stamps[14], 1ull); }
    }
#endif
}

// once every step is done a row's logical position is the step that took it — what the solves and the host read (the panel's maps hold the
// interchanges up to its last replay only)
__global__ void k_luc_lpos_final(LUArgs a) {
    const int R = blockIdx.x * blockDim.x + threadIdx.x;
    if (R < a.m) a.lpos[R] = a.rowstep[R];
}
void launch_luc_lpos_final(const LUArgs &a, hipStream_t s) { hipLaunchKernelGGL(k_luc_lpos_final, dim3((a.m + 255) / 256), dim3(256), 0, s, a); }

// ---- host side
size_t luc_cross_doubles() { return (size_t)kLxHeader + 2 * 2 * 8 * kLxSlots32; }   // header + two parities of eight records (xpairs = 2 doubles) of the wider form
int luc_cross_groups(int m, int want) {   // workgroups for a basis of m rows (0: not this schedule)
    if (want <= 0 || m < 64) return 0;
    const int need = (m + 255) / 256;
    if (need > 8) return 0;
    return need <= 2 ? 2 : (need <= 4 ? 4 : 8);
}
// knob lu_large: rows per lane of the eight-workgroup panel for a basis of m rows — 4 for 4097 .. 8192 rows, 8 for 8193 .. 16384, 0 outside
// (the one place that states the two ranges: lu_compressed_supported and the launcher below read it)
int luc_large_rpt(int m) { return (m <= 4096 || m > 16384) ? 0 : (m <= 8192 ? 4 : 8); }
// slots: 16 or 32 register slots (eight rows per lane: 16); nrole > 0: the look-ahead launch (32 slots, one row per lane, G >= 4) with
// that many workgroups beside the panel's
template <int G, int RPT>
static void luc_cross_panel(const LUArgs &a, int32_t *pivrow, double *xrec, int slots, int nrole, hipStream_t s) {
    xpair *xr = reinterpret_cast<xpair *>(xrec);
    constexpr bool look = RPT == 1 && G >= 4;
    if (slots != 32 || RPT == 8) hipLaunchKernelGGL((k_luc_panel_x<G, RPT, 16, 32, false>), dim3(8 * G), dim3(256), 0, s, a, pivrow, xr);
    else if constexpr (RPT < 8) {
        if (nrole <= 0 || !look) hipLaunchKernelGGL((k_luc_panel_x<G, RPT, 32, 32, false>), dim3(8 * G), dim3(256), 0, s, a, pivrow, xr);
        else if constexpr (look) hipLaunchKernelGGL((k_luc_panel_x<G, 1, 32, 32, true>), dim3(G + (nrole > 8 * G ? nrole : 8 * G)), dim3(256), 0, s, a, pivrow, xr);   // (every panel block 8 g lies inside the grid)
    }
}
// G: the workgroups of a basis of up to 2048 rows (luc_cross_groups); beyond 4096 rows (luc_large_rpt) there are eight, with several rows per lane
void launch_luc_cross_panel(const LUArgs &a, int32_t *pivrow, double *xrec, int G, int slots, int nrole, hipStream_t s) {
    const int rpt = luc_large_rpt(a.m);
    if (rpt == 8) luc_cross_panel<8, 8>(a, pivrow, xrec, slots, nrole, s);
    else if (rpt == 4) luc_cross_panel<8, 4>(a, pivrow, xrec, slots, nrole, s);
    else if (G == 2) luc_cross_panel<2, 1>(a, pivrow, xrec, slots, nrole, s);   // (bases of up to 512 rows: below the look-ahead's range)
    else if (G == 4) luc_cross_panel<4, 1>(a, pivrow, xrec, slots, nrole, s);
    else luc_cross_panel<8, 1>(a, pivrow, xrec, slots, nrole, s);
}
#ifdef GOMILP_DEBUG
void lux_stamps_read(unsigned long long *out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lux_stamps), sizeof(unsigned long long) * 64); }
#endif

}  // namespace gomilp
