// The look-ahead schedule of the compressed gonum-order LU (lu_compressed.hip): what the workgroups BESIDE a round's panel do, shared by the
// panels that carry it — the one-workgroup slot panel (lu_compressed.hip k_luc_panel_slots) and the cross-workgroup panel (lu_cross.hip
// k_luc_panel_x) — and the bounded waits / agent-scope accesses both sides of a launch use.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"

namespace gomilp {

constexpr int kLucSpinLimit = 200000;   // polls (1.5 us each and more: seconds, against the milliseconds another kernel can hold the device)
__device__ __forceinline__ bool luc_spin(const uint32_t *p, uint32_t target) {
    for (int it = 0; it < kLucSpinLimit; it++) {
        const uint32_t v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((int)(v - target) >= 0) return true;
        __builtin_amdgcn_s_sleep(8);
    }
    return false;
}
__device__ __forceinline__ double luc_ld_agent(const double *p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void luc_st_agent(double *p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- what every panel does at the edges of a round ---------------------------------------------------------------------------------
// The first NB columns >= k that are dense for sure (not the unit column of a row still active: unit / active are the panel's LDS maps,
// 0xFFFF = no unit column), ascending, into out[]; returns how many, NB at the most.  Called by ONE whole wave, the result is uniform.
// The start of a round lists the columns it loads with it, the look-ahead hand-over (LUCtl::next) the columns the next round will.
template <int NB>
__device__ __forceinline__ int luc_scan_dense(int k, int m, const unsigned short *unit, const unsigned char *active, int *out) {
    const int lane = (int)threadIdx.x & 63;
    int n = 0;
    for (int base = k; base < m && n < NB; base += 64) {
        const int kk = base + lane;
        bool dense = false;
        if (kk < m) {
            const unsigned short ur = unit[kk];
            dense = ur == 0xFFFF || !active[ur];
        }
        const unsigned long long mask = __ballot(dense);
        const int rank = __popcll(mask & ((1ull << lane) - 1ull));
        if (dense && n + rank < NB) out[n + rank] = kk;
        n += __popcll(mask);
    }
    return n < NB ? n : NB;
}
// The control block of a round that does nothing (no step left, or a wait that was given up): the next round starts where this one did.
// ksync: the cross-workgroup panel's replay mark travels along.
__device__ __forceinline__ void luc_ctl_empty(LUCtl *ctl, const LUCtl *prev, int k0, bool ksync) {
    ctl->nsteps = 0; ctl->ndrop = 0; ctl->nnext = 0; ctl->k_next = k0; ctl->k0 = k0; ctl->k1 = k0; ctl->rounds = prev->rounds;
    if (ksync) ctl->ksync = prev->ksync;
}

// ---- the trailing update of a round, cell by cell (look-ahead schedule) ------------------------------------------------------------
// a[R][j] += sum_s Lp[s][R] * Up[s][j] in ascending s, zero multipliers skipped — the arithmetic of k_luc_trail (lu_compressed.hip), with the
// round's panels read straight from L2 (no staging, no barrier): the body of every 256-thread group of the workgroups that run
// BESIDE the next round's panel (luc_role, phase T) — hidden behind the panel's steps, so the efficiency of these loads does not matter.
// 4 x 4 cells per thread: rows R0 + 4 tx .. (consecutive lanes walk down a column), columns by `colj`.
template <int NB, int UNR>
__device__ __forceinline__ void luc_trail_cells(const LUArgs &a, const LUCtl *__restrict__ c, const double *__restrict__ Lp,
                                                const double *__restrict__ Up, const int32_t *__restrict__ rowstep, int ns, int k0,
                                                const int (&colj)[4], int R0, int tx) {
    const int m = a.m;
    const size_t ldw = (size_t)a.ldw;
    const int Rb = R0 + tx * 4;
    int rs[4], cls[4];
    bool anyrow = false;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
        const int R = Rb + rr;
        rs[rr] = R < m ? rowstep[R] : 0;
        cls[rr] = R < m ? (rs[rr] < 0 ? 1 : (rs[rr] >= k0 ? 2 : 0)) : 0;   // 1 active, 2 left during the round, 0 finished earlier
        anyrow = anyrow || cls[rr] > 0;
    }
    bool anycol = false;
#pragma unroll
    for (int cc = 0; cc < 4; cc++) anycol = anycol || colj[cc] >= 0;
    if (!anyrow || !anycol) return;
    int din[4] = {0, 0, 0, 0}, dout[4] = {0, 0, 0, 0};   // rows that left at steps [din, dout) are final in the column
    const int nd = c->ndrop;
    for (int t = 0; t < nd; t++) {
        const int dc = c->dropcol[t], di = c->dropin[t], dq = c->dropout[t];
#pragma unroll
        for (int cc = 0; cc < 4; cc++)
            if (dc == colj[cc]) { din[cc] = di; dout[cc] = dq; }
    }
    double acc[4][4];   // [cc][rr]
    bool live[4][4];
#pragma unroll
    for (int cc = 0; cc < 4; cc++) {
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            live[cc][rr] = cls[rr] > 0 && colj[cc] >= 0 && !(cls[rr] == 2 && rs[rr] >= din[cc] && rs[rr] < dout[cc]);
            acc[cc][rr] = live[cc][rr] ? a.W[(size_t)colj[cc] * ldw + Rb + rr] : 0.0;
        }
    }
#pragma unroll UNR
    for (int s = 0; s < ns; s++) {   // (UNR steps' loads in flight: 4 where the registers are there, 2 beside a 1024-thread panel)
        double l[4], u[4];
#pragma unroll
        for (int rr = 0; rr < 4; rr++) l[rr] = (Rb + rr) < m ? Lp[(size_t)s * ldw + Rb + rr] : 0.0;
#pragma unroll
        for (int cc = 0; cc < 4; cc++) u[cc] = colj[cc] >= 0 ? luc_ld_agent(&Up[(size_t)s * ldw + colj[cc]]) : 0.0;   // (written by phase S of this launch)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const bool nz = l[rr] != 0;
#pragma unroll
            for (int cc = 0; cc < 4; cc++) acc[cc][rr] = nz ? __dadd_rn(__dmul_rn(l[rr], u[cc]), acc[cc][rr]) : acc[cc][rr];
        }
    }
#pragma unroll
    for (int cc = 0; cc < 4; cc++) {
#pragma unroll
        for (int rr = 0; rr < 4; rr++)
            if (live[cc][rr]) a.W[(size_t)colj[cc] * ldw + Rb + rr] = acc[cc][rr];
    }
}

// ---- look-ahead schedule: ONE launch per round -----------------------------------------------------------------------------------
// One launch holds the panel of round r (one workgroup, k_luc_panel_slots; or the G panel workgroups of k_luc_panel_x) and nrole
// workgroups that finish round r-1 beside it, from the record round r-1 left (control block, multiplier panel, rowstep snapshot: all
// by round parity, the running panel writes the other parity).  The panel hands each of them its index b among the nrole:
//   phase U  (workgroups 0 .. nrt - 1, 64 rows each): U-solve + update of the columns panel r LOADS (ctl_prev->next) — the only part
//            of the update on the critical path; the panel sets up its index maps meanwhile and waits for cnt_u before it loads.
//            Two forms.  !SELF (beside the one-workgroup panel): workgroup 0 solves and hands the U rows to the others through
//            Up_prev and cnt_x; the update takes the round's pivot rows along.  SELF (beside the cross-workgroup panel): every
//            workgroup solves for itself, nothing is handed over, and the update leaves the round's pivot rows out.
//   phase S  (the same workgroups): the U-solve of one 64-column tile of all other columns -> Up_prev, then cnt_s.
//   phase T  (every workgroup, behind cnt_s): the update of all other columns, hidden behind the panel's steps.  Not touched: the
//            columns of phase U, and the unit columns of rows that were still active when round r-1 ended — the running panel may take
//            such a row, build the column in registers and write it, while the round's U rows are exactly zero in it (the update
//            would add l * 0 to every cell).  SELF: workgroup 0 first writes the U entries of the round's pivot rows in phase U's columns.
// What crosses workgroups INSIDE the launch (the cells of phase U -> the panel's loads, Up_prev -> phase T) moves with agent-scope
// stores / loads and an arrival counter, as in the loop kernels (bt_loop.h); everything else crossed a launch boundary.  Waits are
// bounded: whoever runs out of patience (a role workgroup on cnt_x or cnt_s, the panel on cnt_u) raises ctl_base->fault, every later
// launch returns at once, and the host repeats the factorization: with the same panel in the plain schedule, and, should the
// cross-workgroup panel's own exchange give up there as well, once more with the one-workgroup panel.
template <int T, int NB, bool SELF>
__device__ void luc_role(const LUArgs &a, const int b, const int nrole) {   // b: this workgroup among the nrole workgroups beside the panel
    static_assert(T % 256 == 0 && NB == 32, "groups of 256 threads; 32 steps per round");
    const LUCtl *__restrict__ c = a.ctl_prev;
    LUCtl *base = a.ctl_base;
    const int tid = threadIdx.x;
    const int m = a.m, nrt = (m + 63) / 64;
    const size_t ldw = (size_t)a.ldw;
    const int ns = c->nsteps, k0 = c->k0, k1 = c->k1, nn = c->nnext, nd = c->ndrop;
    const bool work = ns > 0 && k1 < m;
    // phases U and S share the staging area (S starts behind U's last barrier)
    __shared__ double s_ln[NB][NB + 1];
    __shared__ double s_xa[SELF ? NB * 65 : 2 * NB * 33];   // U: X[s][33] (pivot rows x listed columns; SELF: the solve turns it into the U rows in place, else Us[s][33] behind it); S: X[s][65]
    static_assert(2 * NB * 33 >= NB * 65, "staging area of phase S");
    __shared__ double s_ls[NB][64];
    __shared__ int Ps[NB], Ss[NB], Dc[NB], Di[NB], Do[NB], Nx[NB];
    __shared__ int s_go;
    const double *__restrict__ Lp = a.Lp_prev;
    if (b < nrt) {
        if (work) {
            if (tid < NB) {
                Ps[tid] = tid < ns ? c->prow[tid] : 0;
                Ss[tid] = tid < ns ? c->steps[tid] : 0x7fffffff;
                Dc[tid] = tid < nd ? c->dropcol[tid] : -1;
                Di[tid] = tid < nd ? c->dropin[tid] : 0;
                Do[tid] = tid < nd ? c->dropout[tid] : 0;
                Nx[tid] = tid < nn ? c->next[tid] : -1;
            }
            __syncthreads();
            for (int idx = tid; idx < NB * NB; idx += T) {
                const int s2 = idx / NB, t = idx % NB;
                s_ln[s2][t] = (s2 < ns && t < s2) ? Lp[(size_t)t * ldw + Ps[s2]] : 0.0;
            }
        }
        // ---- phase U
        bool ok = true;
        if constexpr (SELF) {
            // The U-solve of the listed columns reads the round's pivot rows in them, and the update would WRITE those cells (a pivot row's
            // update is its U-solve).  EVERY workgroup solves for itself, from the cells the launch before left, and nobody writes them in
            // this phase: the update below leaves the round's pivot rows out, and workgroup 0 writes their U entries in phase T — behind
            // cnt_s, when every workgroup has read them (a workgroup that starts late — other kernels on the device — still finds the
            // original cells).  So nothing is handed from workgroup to workgroup in front of the panel's wait: that chain was one solve, an
            // arrival counter, a spin and 1024 agent-scope loads long (cnt_x; one thread per column solved, 496 dependent steps).
            if (work && nn > 0) {
                double (*X)[33] = reinterpret_cast<double (*)[33]>(s_xa);   // pivot rows x listed columns; the solve turns it into the U rows in place
                __shared__ unsigned char s_piv[64];                          // this tile's rows that are pivot rows of the round
                const int R0 = b * 64;
                if (tid < 64) s_piv[tid] = 0;
                for (int idx = tid; idx < NB * 64; idx += T) {
                    const int s2 = idx / 64, r = idx % 64;
                    s_ls[s2][r] = (s2 < ns && R0 + r < m) ? Lp[(size_t)s2 * ldw + R0 + r] : 0.0;
                }
                for (int idx = tid; idx < NB * 32; idx += T) {
                    const int s2 = idx / 32, ci = idx % 32;
                    X[s2][ci] = (s2 < ns && ci < nn) ? a.W[(size_t)Nx[ci] * ldw + Ps[s2]] : 0.0;
                }
                __syncthreads();
                if (tid < ns) {
                    const int r = Ps[tid] - R0;
                    if (r >= 0 && r < 64) s_piv[r] = 1;
                }
                if (tid < 256) {
                    // the U-solve of k_luc_usolve: u_s = x_s + sum_{t < s} l_st u_t in ascending t, zero multipliers skipped.  Lane = (step s, one of
                    // two columns), four column pairs per wave; by the time step t is handed round (one lane's value to the 32 lanes of its
                    // column), every term of u_t has been added: s_ln[s][t] is zero for t >= s
                    const int ln = tid & 63, wv = tid >> 6, s2 = ln & 31;
                    double x[4];
                    bool ex[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int ci = wv * 8 + q * 2 + (ln >> 5);
                        const int jq = Nx[ci];
                        int din = 0, dout = 0;
                        for (int t = 0; t < nd; t++)
                            if (Dc[t] == jq) { din = Di[t]; dout = Do[t]; }
                        x[q] = X[s2][ci];
                        ex[q] = Ss[s2] >= din && Ss[s2] < dout;   // (a pivot row that left while the panel listed the column: final already)
                    }
#pragma unroll 1
                    for (int t = 0; t < ns; t++) {
                        const double l = s_ln[s2][t];
                        const bool on = l != 0;
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const double ut = __shfl(x[q], (ln & 32) + t);
                            x[q] = (on && !ex[q]) ? __dadd_rn(__dmul_rn(l, ut), x[q]) : x[q];
                        }
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int ci = wv * 8 + q * 2 + (ln >> 5);
                        X[s2][ci] = x[q];
                        if (b == 0 && s2 < ns && ci < nn) luc_st_agent(const_cast<double *>(a.Up_prev) + (size_t)s2 * ldw + Nx[ci], x[q]);   // (for phase T: the pivot rows' cells)
                    }
                }
                __syncthreads();
                if (tid < 256) {   // 64 rows x 32 listed columns, 4 x 2 cells per thread
                    const int tx = tid & 15, ty = tid >> 4;
                    const int Rb = R0 + tx * 4;
                    int rs[4], cls[4], colj[2], din[2] = {0, 0}, dout[2] = {0, 0};
#pragma unroll
                    for (int rr = 0; rr < 4; rr++) {
                        const int R = Rb + rr;
                        rs[rr] = R < m ? a.rowsnap_prev[R] : 0;
                        cls[rr] = R < m ? (rs[rr] < 0 ? 1 : (rs[rr] >= k0 ? 2 : 0)) : 0;
                        if (s_piv[tx * 4 + rr]) cls[rr] = 0;   // (phase T, workgroup 0)
                    }
#pragma unroll
                    for (int cc = 0; cc < 2; cc++) colj[cc] = Nx[ty * 2 + cc];
                    for (int t = 0; t < nd; t++) {
#pragma unroll
                        for (int cc = 0; cc < 2; cc++)
                            if (Dc[t] == colj[cc]) { din[cc] = Di[t]; dout[cc] = Do[t]; }
                    }
                    double acc[2][4];
                    bool live[2][4];
#pragma unroll
                    for (int cc = 0; cc < 2; cc++) {
#pragma unroll
                        for (int rr = 0; rr < 4; rr++) {
                            live[cc][rr] = cls[rr] > 0 && colj[cc] >= 0 && !(cls[rr] == 2 && rs[rr] >= din[cc] && rs[rr] < dout[cc]);
                            acc[cc][rr] = live[cc][rr] ? a.W[(size_t)colj[cc] * ldw + Rb + rr] : 0.0;
                        }
                    }
#pragma unroll
                    for (int s2 = 0; s2 < NB; s2++) {
                        if (s2 < ns) {
                            double l[4], u[2];
#pragma unroll
                            for (int rr = 0; rr < 4; rr++) l[rr] = s_ls[s2][tx * 4 + rr];
#pragma unroll
                            for (int cc = 0; cc < 2; cc++) u[cc] = X[s2][ty * 2 + cc];
#pragma unroll
                            for (int rr = 0; rr < 4; rr++) {
                                const bool nz = l[rr] != 0;
#pragma unroll
                                for (int cc = 0; cc < 2; cc++) acc[cc][rr] = nz ? __dadd_rn(__dmul_rn(l[rr], u[cc]), acc[cc][rr]) : acc[cc][rr];
                            }
                        }
                    }
#pragma unroll
                    for (int cc = 0; cc < 2; cc++) {
#pragma unroll
                        for (int rr = 0; rr < 4; rr++)
                            if (live[cc][rr]) luc_st_agent(&a.W[(size_t)colj[cc] * ldw + Rb + rr], acc[cc][rr]);
                    }
                }
            }
        } else {
            // The U-solve of the listed columns reads the round's pivot rows in them, and the update WRITES those cells (a pivot row's
            // update is its U-solve): ONE workgroup solves, before anybody writes, and hands the U rows over through Up_prev (otherwise
            // unused in these columns) and cnt_x; a workgroup that starts late — other kernels on the device — finds everything it needs.
            if (work && nn > 0) {
                double (*X)[33] = reinterpret_cast<double (*)[33]>(s_xa);
                double (*Us)[33] = reinterpret_cast<double (*)[33]>(s_xa + NB * 33);
                double *Upw = const_cast<double *>(a.Up_prev);
                const int R0 = b * 64;
                for (int idx = tid; idx < NB * 64; idx += T) {
                    const int s2 = idx / 64, r = idx % 64;
                    s_ls[s2][r] = (s2 < ns && R0 + r < m) ? Lp[(size_t)s2 * ldw + R0 + r] : 0.0;
                }
                if (b == 0) {
                    for (int idx = tid; idx < NB * 32; idx += T) {
                        const int s2 = idx / 32, ci = idx % 32;
                        X[s2][ci] = (s2 < ns && ci < nn) ? a.W[(size_t)Nx[ci] * ldw + Ps[s2]] : 0.0;
                    }
                    __syncthreads();
                    if (tid < nn) {   // the U-solve of k_luc_usolve, one listed column per thread
                        const int j = Nx[tid];
                        int din = 0, dout = 0;
                        for (int t = 0; t < nd; t++)
                            if (Dc[t] == j) { din = Di[t]; dout = Do[t]; }
                        double u[NB];
#pragma unroll
                        for (int s2 = 0; s2 < NB; s2++) {
                            double x = 0;
                            if (s2 < ns) {
                                x = X[s2][tid];
                                if (!(Ss[s2] >= din && Ss[s2] < dout)) {
#pragma unroll
                                    for (int t = 0; t < s2; t++) {
                                        const double l = s_ln[s2][t];
                                        x = (l != 0) ? __dadd_rn(__dmul_rn(l, u[t]), x) : x;
                                    }
                                }
                                luc_st_agent(Upw + (size_t)s2 * ldw + j, x);
                            }
                            u[s2] = x;
                            Us[s2][tid] = x;
                        }
                    }
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
#ifdef GOMILP_DEBUG
                    if (a.pad3) ok = false;   // fault injection: this workgroup never arrives, the others run out of patience
                    else
#endif
                    if (tid == 0) __hip_atomic_fetch_add(&base->cnt_x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else {
                    if (tid == 0) s_go = luc_spin(&base->cnt_x, (uint32_t)(a.round + 1)) ? 1 : 0;
                    __syncthreads();
                    ok = s_go != 0;
                    if (ok) {
                        for (int idx = tid; idx < NB * 32; idx += T) {
                            const int s2 = idx / 32, ci = idx % 32;
                            Us[s2][ci] = (s2 < ns && ci < nn) ? luc_ld_agent(Upw + (size_t)s2 * ldw + Nx[ci]) : 0.0;
                        }
                    } else if (tid == 0) base->fault = 1;
                    __syncthreads();
                }
                if (ok && tid < 128) {   // 64 rows x 32 listed columns, 4 x 4 cells per thread
                    const int tx = tid & 15, ty = tid >> 4;
                    const int Rb = R0 + tx * 4;
                    int rs[4], cls[4], colj[4], din[4] = {0, 0, 0, 0}, dout[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int rr = 0; rr < 4; rr++) {
                        const int R = Rb + rr;
                        rs[rr] = R < m ? a.rowsnap_prev[R] : 0;
                        cls[rr] = R < m ? (rs[rr] < 0 ? 1 : (rs[rr] >= k0 ? 2 : 0)) : 0;
                    }
#pragma unroll
                    for (int cc = 0; cc < 4; cc++) colj[cc] = Nx[ty * 4 + cc];
                    for (int t = 0; t < nd; t++) {
#pragma unroll
                        for (int cc = 0; cc < 4; cc++)
                            if (Dc[t] == colj[cc]) { din[cc] = Di[t]; dout[cc] = Do[t]; }
                    }
                    double acc[4][4];
                    bool live[4][4];
#pragma unroll
                    for (int cc = 0; cc < 4; cc++) {
#pragma unroll
                        for (int rr = 0; rr < 4; rr++) {
                            live[cc][rr] = cls[rr] > 0 && colj[cc] >= 0 && !(cls[rr] == 2 && rs[rr] >= din[cc] && rs[rr] < dout[cc]);
                            acc[cc][rr] = live[cc][rr] ? a.W[(size_t)colj[cc] * ldw + Rb + rr] : 0.0;
                        }
                    }
#pragma unroll
                    for (int s2 = 0; s2 < NB; s2++) {
                        if (s2 < ns) {
                            double l[4], u[4];
#pragma unroll
                            for (int rr = 0; rr < 4; rr++) l[rr] = s_ls[s2][tx * 4 + rr];
#pragma unroll
                            for (int cc = 0; cc < 4; cc++) u[cc] = Us[s2][ty * 4 + cc];
#pragma unroll
                            for (int rr = 0; rr < 4; rr++) {
                                const bool nz = l[rr] != 0;
#pragma unroll
                                for (int cc = 0; cc < 4; cc++) acc[cc][rr] = nz ? __dadd_rn(__dmul_rn(l[rr], u[cc]), acc[cc][rr]) : acc[cc][rr];
                            }
                        }
                    }
#pragma unroll
                    for (int cc = 0; cc < 4; cc++) {
#pragma unroll
                        for (int rr = 0; rr < 4; rr++)
                            if (live[cc][rr]) luc_st_agent(&a.W[(size_t)colj[cc] * ldw + Rb + rr], acc[cc][rr]);
                    }
                }
            } else if (b == 0) {
                if (tid == 0) __hip_atomic_fetch_add(&base->cnt_x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (one arrival per launch, work or not)
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's cells have landed
        __syncthreads();
#ifdef GOMILP_DEBUG
        if (!(SELF && a.pad3 && b == 0 && work && nn > 0))   // fault injection (SELF): the workgroup that solves for the others' pivot rows never arrives, the panel runs out of patience
#endif
        if (tid == 0) __hip_atomic_fetch_add(&base->cnt_u, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // ---- phase S: column tile b of the columns behind the round
        const int j0 = k1 + b * 64;
        if (work && j0 < m) {
            double (*X)[65] = reinterpret_cast<double (*)[65]>(s_xa);
            for (int idx = tid; idx < NB * 64; idx += T) {
                const int s2 = idx / 64, ci = idx % 64;
                const int j = j0 + ci;
                bool listed = false;   // (phase U's columns: not needed, and their cells are being written)
                for (int t = 0; t < nn; t++) listed = listed || Nx[t] == j;
                X[s2][ci] = (s2 < ns && j < m && !listed) ? a.W[(size_t)j * ldw + Ps[s2]] : 0.0;
            }
            __syncthreads();
            const int j = j0 + tid;
            bool mine = tid < 64 && j < m;
            if (mine)
                for (int t = 0; t < nn; t++) mine = mine && Nx[t] != j;   // (phase U's columns: their U rows in Up_prev are phase U's)
            if (mine) {
                int din = 0, dout = 0;
                for (int t = 0; t < nd; t++)
                    if (Dc[t] == j) { din = Di[t]; dout = Do[t]; }
                double u[NB];
#pragma unroll
                for (int s2 = 0; s2 < NB; s2++) {
                    if (s2 < ns) {
                        double x = X[s2][tid];
                        if (!(Ss[s2] >= din && Ss[s2] < dout)) {
#pragma unroll
                            for (int t = 0; t < s2; t++) {
                                const double l = s_ln[s2][t];
                                x = (l != 0) ? __dadd_rn(__dmul_rn(l, u[t]), x) : x;
                            }
                        }
                        u[s2] = x;
                        luc_st_agent(const_cast<double *>(a.Up_prev) + (size_t)s2 * ldw + j, x);
                    } else u[s2] = 0;
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(&base->cnt_s, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!work) return;
    // ---- phase T
    if (tid == 0) s_go = luc_spin(&base->cnt_s, (uint32_t)(a.round + 1) * (uint32_t)nrt) ? 1 : 0;
    __syncthreads();
    if (!s_go) {
        if (tid == 0) base->fault = 1;
        return;
    }
    if (SELF && b == 0 && nn > 0) {
        // the round's pivot rows in the columns of phase U: their U entries (every workgroup has read the cells: it arrived at cnt_s)
        for (int idx = tid; idx < NB * 32; idx += T) {
            const int s2 = idx / 32, ci = idx % 32;
            if (s2 < ns && ci < nn) a.W[(size_t)Nx[ci] * ldw + Ps[s2]] = luc_ld_agent(a.Up_prev + (size_t)s2 * ldw + Nx[ci]);
        }
    }
    constexpr int G = T / 256;
    const int g = tid >> 8, t256 = tid & 255;
    const int tx = t256 & 15, ty = t256 >> 4;
    const int nct = (m - k1 + 63) / 64;
    const int ngroups = nrole * G;
    for (int tile = b * G + g; tile < nct * nrt; tile += ngroups) {
        const int ct = tile / nrt, rt = tile % nrt;   // neighbouring groups: the row tiles of one column tile
        int colj[4];
#pragma unroll
        for (int cc = 0; cc < 4; cc++) {
            int j = k1 + ct * 64 + ty * 4 + cc;
            if (j >= m) j = -1;
            if (j >= 0) {
                const int ur = a.unit_row ? a.unit_row[j] : -1;
                if (ur >= 0 && a.rowsnap_prev[ur] < 0) j = -1;
            }
            colj[cc] = j;
        }
        for (int t = 0; t < nn; t++) {
            const int nj = c->next[t];
#pragma unroll
            for (int cc = 0; cc < 4; cc++)
                if (colj[cc] == nj) colj[cc] = -1;
        }
        luc_trail_cells<NB, (T > 512 ? 2 : 4)>(a, c, a.Lp_prev, a.Up_prev, a.rowsnap_prev, ns, k0, colj, rt * 64, tx);
    }
}

}  // namespace gomilp
