/*
 * gomilp_lp.h — C-ABI of the MI355X-native LP-relaxation engine.
 *
 * Drop-in boundary for GoMILP's one hot path: the call
 *     z, x, err = lp.Simplex(c, A, b, 0, nil)
 * at /root/reference/subproblem.go:154 (branch-and-bound child) and :172 (root), i.e.
 * /root/reference/vendor/gonum.org/v1/gonum/optimize/convex/lp/simplex.go:88.
 * The Go side binds these entry points through cgo (INTEGRATION.md shows the stub); all
 * arguments are plain pointers and sizes, the caller owns every host buffer, nothing is
 * retained after return (cgo pointer rules), and every entry point is thread-safe.
 *
 * There is no CPU fallback: without a usable HIP device every solve returns
 * GOMILP_ERR_DEVICE.
 */
#ifndef GOMILP_LP_H
#define GOMILP_LP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes.  1..7 are the lp.Err* sentinels of simplex.go:26-34 that the Go wrapper maps
 * back to the SAME sentinel values (GoMILP tests them by identity: ilp.go:37-40, tree.go:77,266-273). */
typedef enum {
    GOMILP_OK = 0,
    GOMILP_ERR_BLAND = 1,          /* lp.ErrBland       simplex.go:27 */
    GOMILP_ERR_INFEASIBLE = 2,     /* lp.ErrInfeasible  simplex.go:28 */
    GOMILP_ERR_LINSOLVE = 3,       /* lp.ErrLinSolve    simplex.go:29 */
    GOMILP_ERR_UNBOUNDED = 4,      /* lp.ErrUnbounded   simplex.go:30 — opt_f = -Inf, no x */
    GOMILP_ERR_SINGULAR = 5,       /* lp.ErrSingular    simplex.go:31 */
    GOMILP_ERR_ZERO_COLUMN = 6,    /* lp.ErrZeroColumn  simplex.go:32 */
    GOMILP_ERR_ZERO_ROW = 7,       /* lp.ErrZeroRow     simplex.go:33 */
    GOMILP_ERR_CONDITION = 8,      /* mat.Condition out of a mid-loop solve, simplex.go:236-239,289-292 */
    GOMILP_ERR_PHASE1_WRAPPED = 9, /* fmt.Errorf("lp: error finding feasible basis: %s"), simplex.go:558 */
    GOMILP_ERR_BAD_SHAPE = 10,     /* the reference panics: simplex.go:387-398 */
    GOMILP_ERR_PANIC = 11,         /* any other reference panic (simplex.go:150,157) */
    GOMILP_ERR_DEVICE = 12,        /* HIP runtime failure / no device / extension not built for it */
    GOMILP_ERR_UNSUPPORTED = 13    /* input outside what this round's device path covers */
} gomilp_status;

/* Per-solve statistics (all optional output). */
typedef struct gomilp_lp_stats {
    int64_t pivots_phase1;      /* pivots of the Phase-I recursive simplex (simplex.go:556) */
    int64_t pivots_phase2;      /* pivots of the Phase-II loop (simplex.go:233-293) */
    int64_t bland_steps;        /* degenerate steps routed through replaceBland (simplex.go:269-277) */
    int64_t refreshes;          /* times x_B / y were recomputed from B^-1 */
    int64_t kernel_launches;    /* pivot-loop kernel launches enqueued */
    int32_t phase1_used;        /* 1 when the initial basis was infeasible and Phase I ran */
    int32_t device_id;
    int32_t wrapped_status;     /* inner status when the result is GOMILP_ERR_PHASE1_WRAPPED */
    int32_t pipeline;           /* pivot pipeline that ran: 0 three-kernel, 1 fused two-kernel, 2 single-kernel tableau,
                                   3 blocked tableau (deferred rank-K updates) */
    double seconds_total;       /* host wall clock of the call (upload included for the flat call) */
    double seconds_upload;      /* host->device copies + layout conversion */
    double seconds_pivot_loop;  /* HIP-event time of all pivot-loop kernels (Phase I + II) */
    double seconds_final_solve; /* gonum-order LU on device + host triangular solves */
    double drift_xb;            /* max |x_B(updated) - x_B(fresh LU)| at termination: accuracy of the B^-1 updates */
    double pivot_kernel_seconds[4]; /* HIP-event time of sampled pivots: [0] pricing kernel, [1] ftran kernel (0 when fused),
                                       [2] update(+ftran) kernel, [3] number of sampled pivots */
    double seconds_final_device; /* part of seconds_final_solve: gather + LU kernels + device->host copy */
    double seconds_final_host;   /* part of seconds_final_solve: the two triangular solves on the host */
    int64_t lu_dense_steps;      /* elimination steps of the final LU that did arithmetic (the rest hit the unit-column fast path) */
    int64_t lu_rounds;           /* panel rounds of the compressed LU schedule (0 for the other schedules) */
    int64_t art_exchanges;       /* 1 when a zero-level artificial was exchanged out of the basis after Phase I (simplex.go:581-606) */
    int64_t cond_fallbacks;      /* exact condition-number evaluations made because a cheap guard was near a threshold */
    int64_t device_retries;      /* 1 when a transient device condition (a workgroup of the multi-workgroup block kernel, or of a look-ahead
                                    launch of the final solve's LU, was not resident in time) made the engine repeat the solve on the
                                    single-workgroup kernels, resp. the factorization with the plain LU schedule */
    double cond1_final;          /* exact kappa_1 / kappa_inf of the basis the Phase-II loop ended with, from the resident tableau (slack-basis */
    double condinf_final;        /* starts beyond 64 rows; 0: not evaluated): kappa_1 > 1e16 -> GOMILP_ERR_CONDITION like mat/lu.go:321 */
} gomilp_lp_stats;

/* One record per pivot, execution order (Phase I first).  Same fields as the oracle's trace. */
typedef struct gomilp_pivot {
    int32_t phase;    /* 1 = Phase I, 2 = Phase II, 3 = dual pivot of a warm start (gomilp_lp_solve_warm) */
    int32_t bland;    /* 1 when chosen by the Bland rule */
    int64_t min_idx;  /* position in nonBasicIdx (simplex.go:247) */
    int64_t replace;  /* position in basicIdxs   (simplex.go:268) */
    int64_t entering; /* variable id entering */
    int64_t leaving;  /* variable id leaving */
} gomilp_pivot;

/* ------------------------------------------------------------------------------------------
 * Flat drop-in: signature-isomorphic to
 *   func Simplex(c []float64, A mat.Matrix, b []float64, tol float64, initialBasic []int)
 *        (optF float64, optX []float64, err error)                          — simplex.go:88
 * A is the RawMatrix() of the *mat.Dense GoMILP always passes: row-major m x n, stride lda.
 * opt_x (length n, caller-owned) is written only when *has_x = 1 (the reference returns nil x on
 * most errors); a mid-loop failure returns the error AND the current point, like the reference.
 * basis_out (nullable, length m) receives the final basicIdxs in positional order.
 * initial_basic (nullable, exactly m entries; GoMILP passes nil): a supplied feasible basis skips Phase I
 * (simplex.go:147-160); an index out of range, a singular or an infeasible set return GOMILP_ERR_PANIC (the
 * reference panics); like any non-slack starting basis it needs the host copy of A, kept for m * n <= 2^25
 * (GOMILP_ERR_UNSUPPORTED above): the column search runs on the device from 96 rows on.  Such a start runs on the tableau
 * pipelines while the tableau row fits the 64 KB LDS window (n - m <= 8191), on the three-kernel revised simplex with the exact-step
 * guard beyond (up to 8192 rows).
 * ---------------------------------------------------------------------------------------- */
int gomilp_lp_simplex(const double *c, const double *A, int64_t lda, const double *b, int64_t m, int64_t n,
                      double tol, const int64_t *initial_basic, double *opt_f, double *opt_x, int32_t *has_x,
                      int64_t *basis_out, gomilp_lp_stats *stats);

/* ------------------------------------------------------------------------------------------
 * Handle API: one context per (thread, GPU); problems stay resident in HBM so that a B&B
 * frontier uploads the root (c, A0, b0) once (subproblem.go:20-29 shares them by pointer).
 * ---------------------------------------------------------------------------------------- */
typedef struct gomilp_ctx gomilp_ctx;

/* device < 0: current HIP device.  Returns NULL (and *status) on failure. */
gomilp_ctx *gomilp_ctx_create(int device, int *status);
void gomilp_ctx_destroy(gomilp_ctx *ctx);
int gomilp_ctx_device(const gomilp_ctx *ctx);
/* knobs: "chunk" (pivots enqueued between host checks), "refresh" (pivots between x_B/y recomputations, 0 = never),
 * "trace" (1 = record pivots), "max_pivots" (safety cap, 0 = none).  Developer knobs of the pivot pipelines (tests force
 * kernel instances with them; results do not depend on them): "tableau", "blocked", "block_k", "bt_nt" (threads of the
 * single-workgroup block kernel), "bt_groups" (-1: single-workgroup block kernels only, 0: by shape, 2 / 4 / 8: that many
 * workgroups, 16: the loop-kernel shapes also below 600 rows), "bt_old", "bt_stamps", "sample_events" — which block kernel a shape takes under
 * which of these and of the loop kernel's knobs is ONE table, DESIGN.md section 2.1 ("BtPlan"; probe: gomilp_debug_bt_plan below);
 * of the persistent loop kernel: "bt_lag" (0: the launch pairs of round 2),
 * "loop_chunk" (pivots per launch), "loop_g" (8 / 16 pivot workgroups), "loop_k" (8 / 12 / 16 pivots per block), "loop_upd"
 * (update workgroups that take part), "loop_grid", "poll_delay", "loop_rep" (default 0, opt-in: the pivot role with replicated reduced costs, ONE exchange
 * per pivot — bit-identical pivots, measured slower: DESIGN.md section 2.1d); "loop_wave_rec" (default 1: the 16 x 128 instance posts one exchange record per wave,
 * 0: one per workgroup — bit-identical pivots: DESIGN.md section 2.1c); "bt_stamps" = 2 stamps that instance instead of the 8 x 256 one; of the bit-exact final solve: "lu_blocked" (3 default: compressed rounds
 * in the look-ahead schedule — one launch per round, the panel beside the previous round's update — for bases beyond 768 rows while the
 * engine holds the device's loop slots, 2: compressed rounds with the whole update behind each panel, 1: blocked panels, 0: one launch per
 * column — all bit-identical), "lu_look" (0: never the look-ahead schedule; a pool sets it on its workers), "lu_large" (default 0;
 * any non-zero value is 1: with "lu_blocked" >= 2 the bases of 4097 .. 16384 rows take the compressed rounds as well, in the plain schedule
 * — three launches per round — on a panel of eight workgroups of one XCD with four (up to 8192 rows) or eight rows per lane, bit-identical
 * to one launch per column; a panel exchange that gives up a wait falls back to one launch per column in the same call,
 * stats.device_retries + 1; a pool accepts the knob and keeps it at 0 on its workers).  The
 * diagnostic flavour of the library (libgomilp_hip_debug.so, GOMILP_DEBUG_BUILD=1) adds "bt_fault" and the GOMILP_DEBUG_* / GOMILP_LUC_*
 * environment hooks; the product library has none of them.  Knobs that DO change what is decided, and how faithfully:
 * "exact_degenerate" (0 never, 1 default: bases of up to 256 rows, non-slack starts and badly scaled inputs, 2 always — degenerate,
 * tied and tiny pivots are decided on fresh gonum-order solves; 3 strict: EVERY pivot and the stop test are the
 * reference's iteration on fresh gonum-order solves with its condition guard, simplex.go:233-293 — milliseconds per pivot, the mode that
 * follows the reference wherever the rounding noise of its solves leads).  The exact steps exist on the BLOCKED tableau pipeline and,
 * for non-slack starts (equality rows, initial_basic) that the tableau does not take (n - m > 8191, or "tableau" = 0), on the
 * three-kernel revised simplex.  A wide slack-basis LP (n - m >= 2m) whose mode asks for them takes the blocked tableau instead of the
 * revised pipelines when that pipeline takes the shape; with "tableau" = 0 or "blocked" = 0 a slack-basis start runs modes 1 / 2
 * WITHOUT them (A/B knobs), and mode 3 returns GOMILP_ERR_UNSUPPORTED from the solve whenever neither of the two runs.  "cond_guard" (1 default: gonum's
 * mat.Condition guard, from a pivot-by-pivot replay up to 64 rows and from the tableau's exact condition numbers beyond — at every exact
 * step (Phase I too), on the final basis, and in front of any pivot whose element is of rounding-noise size).
 * "row_chunk" (doubles; 0 default): the revised-simplex kernels stage one m-long vector per workgroup in LDS — in one pass up to
 * 8192 rows, in chunks of 4096 doubles beyond (bit-identical either way); a multiple of 512 up to 8192 forces the chunked form with
 * that many doubles per chunk at every size (tests).
 * Returns GOMILP_OK or GOMILP_ERR_BAD_SHAPE. */

/* Row limit.  Upload accepts m < 2^20 rows; the device memory decides what solves.  Up to 8192 rows every path below applies,
 * non-slack starts of any width n included (the three-kernel revised simplex with exact steps where the tableau row does not fit,
 * while m * n <= 2^25).
 * Beyond 8192 rows ("Beyond 8192 rows") a single context solves SLACK-BASIS starts — every row has its own
 * unit column, GoMILP's inequality form [G | I] — with Phase I where b has negative entries, through gomilp_lp_simplex,
 * gomilp_lp_upload + gomilp_lp_solve_resident, and gomilp_lp_upload_child on such a root; with the statuses, trace, basis and point
 * semantics of the same pipelines at 8192 rows.  A shape whose buffers (A^T, the two B^-1 copies, the final solve's matrices, the
 * tableau) do not fit the free device memory returns GOMILP_ERR_UNSUPPORTED before anything is allocated; the context stays usable.
 * Warm starts on a context (gomilp_lp_solve_warm) work there too: the dual loop runs on the same chunked revised-simplex kernels.
 * Frontier pools take such roots with the pool knob "large_rows" = 1 (gomilp_pool_set: wide waves on the batched revised simplex in its
 * chunked kernels, warm starts included; everything else on the workers).
 * Still GOMILP_ERR_UNSUPPORTED beyond 8192 rows: non-slack starts (equality rows, a supplied initial_basic, m >= n), on a context and in
 * a pool alike; frontier pools with "large_rows" = 0, the default (gomilp_pool_set_root, their waves and their warm starts); and
 * exact_degenerate = 3 (the blocked tableau does not run there).  The final
 * solve of the bases beyond 4096 rows takes the one-launch-per-column LU (k_lu_step): seconds, not milliseconds — unless "lu_large" is
 * set, which gives the bases of 4097 .. 16384 rows the compressed rounds (beyond 16384 rows the knob changes nothing). */
int gomilp_ctx_set(gomilp_ctx *ctx, const char *key, int64_t value);

/* Upload a standard-form LP (row-major A, stride lda) and keep it resident.  Returns a problem id >= 0, or
 * -(gomilp_status) on failure.  Replaces the per-call operands of simplex.go:88. */
int64_t gomilp_lp_upload(gomilp_ctx *ctx, const double *c, const double *A, int64_t lda, const double *b, int64_t m,
                         int64_t n);
int gomilp_lp_free(gomilp_ctx *ctx, int64_t problem);

/* Solve a resident problem (inputs already in HBM: the timed region of bench.py).  Same outputs as the flat call. */
int gomilp_lp_solve_resident(gomilp_ctx *ctx, int64_t problem, double tol, const int64_t *initial_basic,
                             double *opt_f, double *opt_x, int32_t *has_x, int64_t *basis_out,
                             gomilp_lp_stats *stats);

/* Pivot trace of the last solve on this context (needs "trace" = 1).  Copies up to cap records, returns the
 * total number of pivots performed. */
int64_t gomilp_lp_last_trace(gomilp_ctx *ctx, gomilp_pivot *out, int64_t cap);

/* Child of a resident root problem, assembled on the device: the K branch-and-bound rows
 * G#_k = sign_k * e_{var_k}, h#_k = rhs_k of /root/reference/subproblem.go:36-44,245-255 are appended exactly like
 * convertToEqualities (subproblem.go:81-139) does: A' = [[A0, 0], [G#, I_K]], c' = [c0, 0], b' = [b0; h#].
 * Returns a problem id (solve it with gomilp_lp_solve_resident; x has n0 + K entries, the caller keeps the
 * first n0 like subproblem.go:157-159) or -(gomilp_status). */
int64_t gomilp_lp_upload_child(gomilp_ctx *ctx, int64_t root_problem, int32_t K, const int32_t *var, const double *sign,
                               const double *rhs);

/* ------------------------------------------------------------------------------------------
 * Warm start on a context: a child starts from the kept final state of its parent — the parent's basis
 * plus the slacks of the new branch rows, dual feasible — and a dual simplex on the revised-simplex kernels repairs the rows the
 * parent violates; a primal Phase-II loop (usually 0 pivots) and the usual final solve follow.  At every row count a context
 * solves, beyond 8192 rows included.  Parity (as gomilp_frontier_solve_warm): status, branching decisions, |z - z_cold| <= 1e-9
 * max(1, |z_cold|); not the reference's pivot path.
 * ---------------------------------------------------------------------------------------- */
typedef struct gomilp_warm_stats {
    int32_t warm_started;   /* 1: the solve started from the parent's basis */
    int32_t fallback;       /* why it ran cold: 0 none, 1 parent < 0, 2 parent has no kept state, 3 not a descendant,
                               4 dual-pivot budget spent (then solved cold in the same call), 5 mode / shape without a warm path */
    int32_t new_rows;       /* J: branch rows the problem has beyond the parent */
    int32_t kept;           /* 1: this problem's final state is now kept (keep != 0, status OK, and it fit in device memory) */
    int64_t pivots_dual;
    int64_t keep_bytes;
    double seconds_setup;   /* building the child's B^-1 / x_B from the parent's state */
    double seconds_dual;    /* dual loop (HIP events) */
} gomilp_warm_stats;

/* Solve `problem`, warm from `parent`, and keep its final state when `keep` != 0.
 *   parent < 0       a cold solve, bit for bit gomilp_lp_solve_resident, plus keeping (how a root gets kept).
 *   keep != 0        when the status is GOMILP_OK the final positional basis and an explicit B^-1 (m x ld doubles: 538 MB at
 *                    8200 rows) stay on the device with the problem, if they fit the free device memory; gomilp_lp_free(problem)
 *                    and the next solve of the same problem drop them.
 *   descendant       `problem` was assembled by gomilp_lp_upload_child from `parent` itself (J = its K rows), or both come from
 *                    the same root and the parent's (var, sign, rhs) rows are a bitwise prefix of the problem's (J = K - K_parent).
 *                    Any J >= 1.  Anything else runs cold with fallback = 3 (not an error).
 *   dual_budget      dual pivots before the call gives up the warm start (0: 64) and solves the problem cold, fallback = 4: the
 *                    result is then bit-identical to gomilp_lp_solve_resident.
 *   A child the dual loop proves infeasible returns GOMILP_ERR_INFEASIBLE without x.  exact_degenerate = 3, and parents that
 *   started from a non-slack basis on a tableau pipeline, run cold with fallback = 5.
 *   Dual pivots are recorded in the trace with phase = 3, ahead of the Phase-II pivots; stats->pivots_phase2 counts the latter.
 *   wstats may be NULL. */
int gomilp_lp_solve_warm(gomilp_ctx *ctx, int64_t problem, int64_t parent, int32_t keep, int32_t dual_budget, double tol,
                         double *opt_f, double *opt_x, int32_t *has_x, int64_t *basis_out,
                         gomilp_lp_stats *stats, gomilp_warm_stats *wstats);

/* ------------------------------------------------------------------------------------------
 * Frontier API: one FIFO level of the enumeration tree (independent relaxations sharing the root data,
 * tree.go:98-100,196-205) solved by a pool of `workers` contexts on ONE GPU, each on its own HIP stream.
 * Multi-GPU runs use one pool per process/GPU and shard the children by index (bench.py).
 * ---------------------------------------------------------------------------------------- */
typedef struct gomilp_pool gomilp_pool;

typedef struct gomilp_frontier_stats {
    int64_t relaxations;
    int64_t pivots_phase1, pivots_phase2, bland_steps, phase1_runs;
    int64_t kernel_launches;
    int32_t workers, device_id;
    double seconds_total;       /* host wall clock of the call */
    double seconds_busy_sum;    /* sum over workers of time spent inside solves */
    int64_t batched_relaxations; /* relaxations whose pivot loops ran in the device-batched schedule (one launch per kernel type
                                    for the whole wave) */
    int64_t host_fallbacks;      /* relaxations the batched schedule handed to a worker's single-relaxation engine */
    int64_t supersteps;          /* host round trips of the batched schedule for the WHOLE wave */
    double seconds_batch;        /* wall clock of the batched schedule */
    int64_t blocks;              /* block steps of the batched schedule (one batched inner launch + one batched update launch each) */
    int64_t blocks_sampled;      /* of which timed with HIP events (pool knob "sample_batch") */
    double seconds_inner_kernels;  /* HIP-event time of the sampled batched inner launches (k_bt_inner2_batch) */
    double seconds_update_kernels; /* ... of the sampled batched update launches (k_bt_update_tiled_batch) */
    /* warm start (gomilp_frontier_solve_warm) */
    int64_t warm_started;        /* relaxations that started from their parent's basis */
    int64_t warm_fallbacks;      /* of which handed back to the cold path (dual-pivot budget spent) */
    int64_t warm_kept;           /* final states kept for children */
    int64_t pivots_dual;         /* dual-simplex pivots of the warm starts (not counted in pivots_phase1 / 2) */
    int64_t art_exchanges;       /* zero-level artificial exchanges (simplex.go:581-606) done inside the batched revised schedule (pool knob
                                    "rev_exchange"); those of relaxations solved on a worker are not counted */
} gomilp_frontier_stats;

gomilp_pool *gomilp_pool_create(int device, int workers, int *status);
void gomilp_pool_destroy(gomilp_pool *pool);
/* knobs: "split_phase" (default 1: in a wave of >= 16 the relaxations that start feasible — the long Phase-II chains — and those that need
 * Phase I run as two schedules side by side, the long chains on the higher-priority stream), "batch_loop" (default 1: whenever the active
 * relaxations of a schedule fit one launch their block steps run in the persistent kernel k_b_loop — per relaxation one pivot workgroup and
 * seven update workgroups, the rank-4 update of block t beside block t + 1), "batch_virt" (default 1: a WIDE wave of slack-start
 * relaxations runs its set-up pivot and its first block of 8 pivots on computed tableau entries and writes out only the tableaus that are
 * still alive behind that block — bit-identical), "batch_res" (default 0, opt-in: narrow waves in the
 * register-resident kernel k_b_res instead of k_b_loop — bit-identical, slower: DESIGN.md section 2.5d), "split_large" (default 1: a wave of >= 4 relaxations beyond 1024 rows runs as two interleaved schedules), "sample_batch" (1: time every batched block launch with HIP events), "batched" (default 1: the pivot loops of a wave run device-batched — grid.x = relaxation, O(1) host round trips per
 * superstep for the whole wave; 0: one host thread + stream per relaxation), "batch_revised" (default 1: a WIDE wave, n - m >= 2m, whose
 * relaxations a worker would run on the unguarded revised-simplex pipelines — slack starts of more than 256 rows at exact_degenerate = 1,
 * any size above 64 rows at = 0 — runs on the device-batched revised simplex: the three-kernel pipeline with the relaxation as a grid
 * dimension, Phase I and the Bland rule on the device, bit-identical to the worker path; 0: such waves on the workers, one relaxation per
 * stream.  Several roots: the test runs over the roots the wave USES, each with the row counts of its own children, and the wave runs as one
 * schedule when all of them pass; roots the pool merely holds do not count.  DESIGN.md section 2.5e), "rev_roots" (default 1: a wide wave of
 * gomilp_frontier_solve_roots that uses more than one root, or a root other than the gomilp_pool_set_root problem, takes that schedule when
 * every root it uses passes its test — bit-identical results; 0: such a wave runs on the workers, whole, as it did before the knob
 * existed.  Waves of root 0 alone never look at it), "rev_exchange" (default 1: on that schedule a relaxation whose Phase I ends with the artificial basic at level
 * zero exchanges it on the device — every nonbasic column tried at once by the worker's acceptance rule, the smallest passing id taken, one
 * forced pivot, then Phase II: the column the worker takes, bit-identical results, counted in art_exchanges; 0: such a relaxation is handed
 * to a worker's whole solve and counted in host_fallbacks.  Either way the schedule hands over a relaxation whose artificial ends Phase I
 * with 1e-13 < |x_art| < 1e-11: that verdict needs a fresh gonum-order solve), "warm_revised" (default 0, opt-in: a gomilp_frontier_solve_warm call whose wave passes the routing
 * test of "batch_revised" runs on that schedule too — relaxations whose parent was kept by it start from the parent's B^-1 with a batched
 * dual simplex, the others cold in the same run, final states are kept as B^-1 + basis list; 0: such a call runs on the workers, cold, and
 * keeps nothing.  Cold calls never look at it.  DESIGN.md section 2.6b), "large_rows" (default 0, opt-in: the pool takes roots and
 * children beyond 8192 rows.  The workers accept there what a context accepts — slack-basis roots that fit the device memory; a root
 * without a slack basis stays GOMILP_ERR_UNSUPPORTED — and a wide wave of such relaxations passes the routing test of "batch_revised": that
 * schedule's kernels then stream their m-long vectors through LDS in chunks of 4096 doubles, bit-identical to the worker path, and its warm
 * starts ("warm_revised") are no longer limited to 4096 rows.  A relaxation there costs its own A^T and two copies of B^-1 (8200 x 24648:
 * 1.6 GB + 2 x 0.54 GB); a wave whose buffers do not fit the free device memory runs on the workers, whole — correct, one relaxation per
 * stream on the chunked three-kernel loop — and a final state that does not fit is not kept (warm_kept), which is no error.  With the
 * knob at 1 the pool also stages in chunks of the worker knob "row_chunk" where that is set, at any row count (tests).  0: pools keep the
 * 8192-row limit and never look at "row_chunk"; clearing the knob while the pool holds a root beyond 8192 rows returns
 * GOMILP_ERR_BAD_SHAPE.  DESIGN.md section 2.5e), "rev_inplace" (default 0, opt-in: a run of that schedule assembles no per-child copy of
 * A^T — (n + 1) x ld doubles per relaxation, most of a wave's memory: 3.6 MB of 5 MB at 300 x 1500 — but reads the root's resident A^T in
 * place and synthesises the K branch entries and unit columns while it reads, with one ld-long row per relaxation for the Phase-I
 * artificial column: the same arithmetic in the same order, bit-identical results, one launch less per wave, and wider waves fit the
 * device.  Routing does not depend on it; 0: the launches as they were.  gomilp_debug_rev_footprint gives both footprints),
 * "rev_mem_limit" (MiB, default 0: none; a negative value is GOMILP_ERR_BAD_SHAPE: where it is below the free device memory it takes its
 * place in that schedule's test of whether a wave's buffers fit — a cap on the wave buffers for a caller on a shared card; a wave that does
 * not fit runs on the workers, whole), "rev_general" (default 1: a WIDE wave of a root WITHOUT a slack basis — equality rows, the
 * standard form [[A, 0], [G, I]] — takes that schedule too.  The column search runs once per root (gomilp_pool_set_root /
 * gomilp_pool_add_root keep the searched basis, its inverse and its x_B); a child starts from that basis and its K branch slacks, built on
 * the device by copies and sign flips, runs the loops with the exact-step guard of such starts (1e-9), and is handed to a worker's whole
 * solve — counted in host_fallbacks — wherever its start or a pivot has to be decided on a fresh gonum-order solve.  Bit-identical to the
 * worker path.  Cold calls, exact_degenerate 1 or 2, one-pass staging (not with "large_rows" and "row_chunk" set), roots of up to 2^25
 * entries, children of up to 96 rows — where a 24-child wave runs as fast as on eight workers; 2: children of up to 300 rows, measured 11 %
 * slower at 160 and 43 % slower at 300 rows than the workers, which solve such children on the blocked tableau.  Everything else, and the
 * knob at 0: such waves on the workers, whole, as before; other values are GOMILP_ERR_BAD_SHAPE.  DESIGN.md section 2.5e); any gomilp_ctx_set key is forwarded to the worker contexts ("row_chunk" is remembered
 * by the pool as well). */
int gomilp_pool_set(gomilp_pool *pool, const char *key, int64_t value);
/* Upload the root standard form (row-major A0, stride lda) to every worker context of the pool. */
int gomilp_pool_set_root(gomilp_pool *pool, const double *c0, const double *A0, int64_t lda, const double *b0, int64_t m0,
                         int64_t n0);
/* Solve `count` children.  Child i owns the triples [koff[i], koff[i+1]) of (var, sign, rhs) (koff has count+1 entries).
 * Outputs, all caller-owned: z_out[count]; x_out[count*n0] (root width, subproblem.go:157-159); status_out[count]
 * (gomilp_status); has_x_out[count].  Returns GOMILP_OK unless the call itself could not run. */
int gomilp_frontier_solve(gomilp_pool *pool, int64_t count, const int64_t *koff, const int32_t *var, const double *sign,
                          const double *rhs, double tol, double *z_out, double *x_out, int32_t *status_out,
                          int32_t *has_x_out, gomilp_frontier_stats *stats);

/* ------------------------------------------------------------------------------------------
 * Incumbent exchange of a frontier sharded over GPUs, one process per GPU: the only state the
 * reference's workers share is the incumbent (/root/reference/tree.go:207-263; pruning at :228-230).  One RCCL
 * all-reduce(min) of 2 * world doubles per wave over xGMI.  The caller ships the 128-byte id from rank 0 to the
 * other ranks by whatever transport it has (the Go host: its own RPC; bench.py: torch.distributed).
 * ---------------------------------------------------------------------------------------- */
typedef struct gomilp_comm gomilp_comm;
#define GOMILP_COMM_ID_BYTES 128
#define GOMILP_NO_INCUMBENT ((int64_t)1 << 52)   /* index meaning "this rank has no integer-feasible candidate" */
/* rank 0: fill id_out[GOMILP_COMM_ID_BYTES] (ncclGetUniqueId). */
int gomilp_comm_unique_id(char *id_out);
/* every rank, with rank 0's id; collective (ncclCommInitRank).  device < 0: current HIP device. */
gomilp_comm *gomilp_comm_create(int rank, int world, const char *id, int device, int *status);
void gomilp_comm_destroy(gomilp_comm *comm);
int gomilp_comm_rank(const gomilp_comm *comm);
int gomilp_comm_world(const gomilp_comm *comm);
/* global_z = min over ranks of local_z, global_index = the smallest child index among the ranks that attain it
 * (ties resolved like the reference's FIFO order would); a rank without a candidate passes (+Inf, GOMILP_NO_INCUMBENT).
 * Collective: every rank of the communicator calls it once per wave. */
int gomilp_incumbent_allreduce(gomilp_comm *comm, double local_z, int64_t local_index, double *global_z,
                               int64_t *global_index);
/* the host logic of the exchange (no GPU): lexicographic minimum of a table of `world` (z, index) pairs, +Inf = none */
void gomilp_incumbent_pick(const double *table, int world, double *global_z, int64_t *global_index);

/* The root relaxation (subproblem.go:172) on the pool's first worker. */
int gomilp_pool_solve_root(gomilp_pool *pool, double tol, double *opt_f, double *opt_x, int32_t *has_x, gomilp_lp_stats *stats);

/* Warm start from the parent's basis — OPT-IN (/root/reference/README.md TODO "initiate the simplex at solution of
 * parent?"; the reference's own hook would be initialBasic, simplex.go:147-161).  As gomilp_frontier_solve, plus per relaxation:
 *   tag[i]     caller-chosen id (>= 0; the B&B node id) under which the relaxation's final state stays resident when keep[i] != 0 and it
 *              ends GOMILP_OK inside the device-batched schedule (2-3 MB of HBM per 520-row relaxation; gomilp_pool_release_warm drops it,
 *              gomilp_pool_set_root drops all);
 *   parent[i]  tag of a kept relaxation that is THIS relaxation minus its last branch row, or < 0.  With a parent the relaxation starts
 *              from the parent's final basis + the slack of the new row: dual feasible, primal infeasible at most in that row — a dual-
 *              simplex loop on the device (k_bt_inner2_dual_batch) repairs it or proves the row infeasible; a new row the parent's
 *              optimum already satisfies costs no pivot.  After `dual_budget` dual pivots (0: default 64) the relaxation is handed to the
 *              cold path of this same call (the reference's Phase I), so the worst case is cold + budget.
 * Parity in this mode (it does not follow the reference's pivot path): status, branching / pruning decisions and |z - z_ref| <= 1e-9
 * max(1, |z_ref|); x is the gonum-order solve of the final basis, as always — the same vertex reached through another basis order can
 * differ in the last bits.  Without parents (parent == NULL or all < 0) the call is gomilp_frontier_solve + keeping.
 * WIDE waves (n - m >= 2m; the waves of pool knob "batch_revised"): with pool knob "warm_revised" = 1 the call runs on the device-batched
 * revised simplex.  A kept state is the final B^-1 (m x ld doubles: 0.6 MB per 270-row relaxation), the positional basis list and the
 * relaxation's branch triples.  Relaxation i starts warm when parent[i] names a state kept by this schedule for the current root and its
 * (var, sign, rhs) rows extend that parent's rows — a bitwise prefix of its own, the rule of gomilp_lp_solve_warm — by J >= 1 rows:
 * B^-1 = [[B_p^-1, 0], [R, I_J]], a dual simplex on the batched revised-simplex kernels, then Phase II.  Everything else in the wave (no
 * parent, an unknown tag, a state kept by the tableau schedule, not a prefix) starts cold in the same run, and so does a narrow relaxation
 * whose parent was kept here: neither is an error.  A warm start that spends dual_budget is re-initialised in place and solved cold by
 * the same call, bit for bit what the cold call returns (warm_fallbacks).  Relaxations handed to a worker (host_fallbacks: the |x_art| band; with "rev_exchange" = 0 the zero-level artificial
 * exchange too) keep nothing, one that exchanged its artificial on the device is kept like any other; waves with more
 * than 4096 rows run on this schedule cold, with keeping, unless the pool knob "large_rows" is 1: then they start warm like any other wave
 * (the dual pricing kernel streams its two vectors through LDS in chunks), beyond 8192 rows too.  With the knob at 0 (default) a wide warm call runs on the workers, cold,
 * warm_started = 0.  Same parity contract. */
int gomilp_frontier_solve_warm(gomilp_pool *pool, int64_t count, const int64_t *koff, const int32_t *var, const double *sign,
                               const double *rhs, const int64_t *parent, const int64_t *tag, const int32_t *keep, int32_t dual_budget,
                               double tol, double *z_out, double *x_out, int32_t *status_out, int32_t *has_x_out,
                               gomilp_frontier_stats *stats);
int gomilp_pool_release_warm(gomilp_pool *pool, int64_t tag);   /* tag < 0: all */

/* Several roots in one pool: relaxation i of a wave is a child (K_i >= 0 rows) of root root_of[i]; index 0 is the root of
 * gomilp_pool_set_root, gomilp_pool_add_root returns 1, 2, ... (or -(gomilp_status)).  Independent LPs of similar shape
 * are children with K = 0 of different roots: they advance together through the device-batched schedule (one launch per
 * kernel type for all of them) — narrow relaxations (n - m < 2m) on the tableau schedule, WIDE ones (n - m >= 2m: slack
 * starts, and with pool knob "rev_general" roots without a slack basis) on the batched revised simplex of pool knob
 * "batch_revised" (pool knob "rev_roots"), where the roots may differ in rows and columns and a wave may mix the two kinds of
 * wide roots: one schedule, the exact-step guard per relaxation.  Which schedule takes the wave is decided over the roots the wave uses; a wave that mixes roots of both
 * kinds, or uses a root no schedule takes, runs on the workers, whole (one relaxation per stream): it is not split.
 * gomilp_frontier_solve_warm names no roots: its wave is one of root 0, whatever else the pool holds.
 * x_out has row stride ldx >= the widest root; gomilp_pool_set_root drops the added roots. */
int gomilp_pool_add_root(gomilp_pool *pool, const double *c, const double *A, int64_t lda, const double *b, int64_t m, int64_t n);
int gomilp_frontier_solve_roots(gomilp_pool *pool, int64_t count, const int32_t *root_of, const int64_t *koff, const int32_t *var,
                                const double *sign, const double *rhs, double tol, double *z_out, double *x_out, int64_t ldx,
                                int32_t *status_out, int32_t *has_x_out, gomilp_frontier_stats *stats);

/* Diagnostic, host only: the column search of findLinearlyIndependent (simplex.go:611-637) as the engine performs it for
 * non-slack starting bases (exact kappa_1 instead of the Hager estimate).  fast = 1: one Householder QR carried along,
 * O(m^2 n); fast = 0: a fresh factorisation per candidate, O(m^4).  idx_out has room for m entries; returns their count. */
int64_t gomilp_debug_find_independent(const double *A, int64_t lda, int64_t m, int64_t n, int64_t *idx_out, int fast);
/* the same search with the column scan on the device, on a resident problem (tests compare the two) */
int64_t gomilp_debug_find_independent_device(gomilp_ctx *ctx, int64_t problem, int64_t *idx_out, int64_t cap);
/* Diagnostic (host only): the condition-number estimate behind the engine's mat.Condition verdicts (mat/lu.go:321 with
 * lapack/gonum/dgecon.go:26-81, dlacn2.go:24-136) for a row-major n x n matrix: 1-norm (inf = 0) or infinity norm (inf = 1);
 * -1 when B is singular to working precision.  Tests compare it with the checker's Dgecon. */
double gomilp_debug_cond_estimate(const double *B, int64_t n, int inf);
/* Diagnostic (host only): what gonum's mat.LU holds after Factorize(M) (transposed = 1: Factorize(M.T())) for a row-major n x n matrix with
 * n <= 64 — *cond = 1 / Dgecon(MaxRowSum) on the factors of Dgetf2 (mat/lu.go:29-50,70-84), bit for bit; returns 1 when LU.Solve's
 * Det() == 0 test fires (mat/lu.go:301), 0 when not, -1 for n out of range.  The host replay of the reference's guards for bases of up
 * to 64 rows uses exactly this (engine_general.cpp general_condition_replay); tests compare it with the checker's restatement. */
int gomilp_debug_gonum_lu_cond(const double *M, int64_t n, int transposed, double *cond);
/* Diagnostic (host only): the host half of the bit-exact final solve on packed LU factors (gomilp_amd/csrc/lu_host.h) — Dlaswp and the two
 * Dtrsm of Dgetrs (lapack/gonum/dgetrs.go:37-45) in gonum's rounding order.  dl: the nd logical positions (ascending) whose column of the
 * in-place L\U has off-diagonal entries; phys[i]: the physical row at logical position i; diag[R]: u_ii of physical row R; rhs: m entries
 * by physical row.  coupled = 0: W is m x nd (row R: those columns of physical row R), x gets m entries by logical position.  coupled = 1:
 * W is nd x nd (row s: logical position dl[s] restricted to those columns), x gets the nd entries of the solution at dl.  Returns 1 when
 * LU.Solve's Det() == 0 test fires (mat/lu.go:301; x is zeroed), 0 when not, -1 for bad arguments.  Tests compare it with the checker's SolveVec. */
int gomilp_debug_lu_host_solve(int64_t m, int64_t nd, const int32_t *dl, const int32_t *phys, const double *diag, const double *W, int coupled,
                               const double *rhs, double *x);
/* Diagnostic (host only, no device): which block kernel the blocked tableau would run for a relaxation of m rows and ldt tableau columns
 * under the given knobs (nknobs key / value pairs, taken through the same range checks as gomilp_ctx_set; only the knobs of the routing
 * table) on a device of ncu compute units — the fields of the engine's BtPlan (gomilp_amd/csrc/engine.hpp) as
 * integers, in the order of BT_PLAN_FIELDS in gomilp_amd/lp.py.  out has room for GOMILP_BT_PLAN_FIELDS entries; returns their count, or
 * -GOMILP_ERR_BAD_SHAPE for a bad shape, key or value. */
#define GOMILP_BT_PLAN_FIELDS 23
int gomilp_debug_bt_plan(int64_t m, int64_t ldt, int64_t nknobs, const char *const *keys, const int64_t *values, int64_t ncu, int64_t *out);

/* Diagnostic (host only, no device): where a single solve of an m x n problem (m < n) goes from a starting basis of kind `start` (0 slack:
 * the last m columns are unit columns, 1 searched: findLinearlyIndependent, 2 supplied by the caller) with Problem scale span
 * scale_span (max |a_ij| / min nonzero |a_ij|) under the given knobs (key / value pairs through the range checks of gomilp_ctx_set; only
 * the routing knobs tableau, blocked, fused, exact_degenerate, cond_guard, general_min_rows, general_device) — the fields of the engine's
 * SolvePlan (gomilp_amd/csrc/engine.hpp; the table of DESIGN.md section 2.4) as doubles, in the order of SOLVE_PLAN_FIELDS in
 * gomilp_amd/lp.py.  out has room for GOMILP_SOLVE_PLAN_FIELDS entries; returns their count, or -GOMILP_ERR_BAD_SHAPE for a bad shape,
 * key or value. */
#define GOMILP_SOLVE_PLAN_FIELDS 13
int gomilp_debug_solve_plan(int64_t m, int64_t n, int32_t start, double scale_span, int64_t nknobs, const char *const *keys, const int64_t *values, double *out);

/* Diagnostic (host only, no device): where a pool that holds the given roots would send one frontier wave under the given pool knobs
 * (nknobs key / value pairs of gomilp_pool_set's own keys) — the routing table of DESIGN.md section 2.5f.  A root is its m, n,
 * scale_span and GOMILP_WP_ROOT_* flags (a root with B_NEGATIVE has some b_i < 0; one with GENERAL carries its searched basis as
 * gomilp_pool_set_root would give it: the tableau of a narrow root, the inverse of a wide one with m n <= 2^25 — pool knob "rev_general");
 * the wave is count / root_of (NULL: all of root 0) /
 * koff / var / rhs as gomilp_frontier_solve_roots takes them.  warm_call: the wave comes through gomilp_frontier_solve_warm; then warm[i]
 * != 0 says that relaxation i names a parent whose kept tableau is resident, and spent[0 .. nspent) lists warm starts that spend their
 * dual budget and come back into the cold part.  Out: *route (0 workers, 1 batched revised simplex, 2 tableau schedule), *cut (how the
 * tableau schedule cuts the cold part: 0 none, 1 one run on the caller's arrays, 2 one run on gathered lists, 3 feasible starts beside
 * Phase-I starts, 4 two halves), group[i], a GOMILP_WP_GROUP_* per relaxation, and pos[i], its place in the list of that group as the
 * schedule gets it.  Returns GOMILP_OK, or
 * -GOMILP_ERR_BAD_SHAPE for a bad shape, key or list. */
enum { GOMILP_WP_ROOT_UNIT_BASIS = 1, GOMILP_WP_ROOT_GENERAL = 2, GOMILP_WP_ROOT_B_NEGATIVE = 4, GOMILP_WP_ROOT_VERIFY_BAD = 8 };
enum { GOMILP_WP_GROUP_WHOLE = 0, GOMILP_WP_GROUP_WARM = 1, GOMILP_WP_GROUP_FEASIBLE = 2, GOMILP_WP_GROUP_PHASE1 = 3, GOMILP_WP_GROUP_HALF0 = 4,
       GOMILP_WP_GROUP_HALF1 = 5 };
int gomilp_debug_wave_plan(int64_t nroots, const int64_t *root_m, const int64_t *root_n, const int32_t *root_flags, const double *root_scale_span,
                           int64_t count, const int32_t *root_of, const int64_t *koff, const int32_t *var, const double *rhs, int32_t warm_call,
                           const int32_t *warm, int64_t nspent, const int64_t *spent, int64_t nknobs, const char *const *keys, const int64_t *values,
                           int32_t *route, int32_t *cut, int32_t *group, int32_t *pos);

/* Diagnostic (host only, no device): the device memory a wave takes on the batched revised simplex of pool knob "batch_revised", as that
 * schedule itself lays it out (the function its run sizes its buffers from).  Roots by shape, the wave as count / root_of (NULL: all of
 * root 0) / koff of gomilp_frontier_solve_roots; inplace: the value of pool knob "rev_inplace".  With m_i, n_i the child's rows and
 * columns and ld_i = m_i rounded up to even: out[0], doubles of the arena of assembled A^T copies, is the sum of (n_i + 1) * ld_i, or 0
 * with inplace; out[1], doubles of the work arena (both B^-1, the vectors, the lists), is larger by the sum of ld_i with inplace — the
 * rows of the artificial columns.  The schedule takes the wave when (out[0] + out[1]) * 8 bytes, plus a sixteenth, plus 256 MiB fit the
 * free device memory (or pool knob "rev_mem_limit").  The probe describes roots with a slack basis; a child of a root without one (pool knob
 * "rev_general") takes 4 * kMaxPartials doubles more of the work arena, the runner-up keys of its guarded pivots.  Returns GOMILP_OK, or -GOMILP_ERR_BAD_SHAPE for a bad shape or list. */
int gomilp_debug_rev_footprint(int64_t nroots, const int64_t *root_m, const int64_t *root_n, int64_t count, const int32_t *root_of,
                               const int64_t *koff, int32_t inplace, int64_t *out /* [2] */);

/* Library / device probes (no compute): used by the loader checks and by __graft_entry__. */
const char *gomilp_version(void);
int gomilp_device_count(void);
/* Name of the gfx target the kernels were compiled for ("gfx950"). */
const char *gomilp_compiled_arch(void);

#ifdef __cplusplus
}
#endif
#endif /* GOMILP_LP_H */
