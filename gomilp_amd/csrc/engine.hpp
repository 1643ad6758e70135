// Host-side engine of the gfx950 LP-relaxation path: owns the HBM-resident problem and work buffers,
// enqueues the pivot kernels in chunks on one HIP stream, and reproduces the control flow of
// gonum's simplex() (vendor/gonum.org/v1/gonum/optimize/convex/lp/simplex.go:93-302) around them.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gomilp_lp.h"
#include "device_types.h"

namespace gomilp {

// The revised-simplex kernels stage one m-long vector (ld doubles) per workgroup in LDS.  Up to kLdsWindowLd (64 KB) it is staged
// in one pass; beyond it the chunked form streams it kAutoRowChunk doubles at a time (simplex_kernels.hip).
constexpr int kLdsWindowLd = 8192;
constexpr int kAutoRowChunk = 4096;

// A standard-form LP resident in HBM.
struct Problem {
    int m = 0, n = 0, ld = 0;
    double *dAt = nullptr;    // (n+1) x ld : row j = column j of A; row n is reserved for the Phase-I artificial column
    double *dc = nullptr;     // n+1 : c, then 0
    double *dc1 = nullptr;    // n+1 : Phase-I cost e_n
    double *db = nullptr;     // ld  : b, zero padded
    std::vector<double> hb, hc;
    mutable std::vector<double> hA;   // host copy of A (row-major m x n), kept for small problems: general initial basis (S7);
                                      // a child builds it from its root only when a solve needs it (ensure_host_A)
    std::vector<int32_t> nnz, lastrow, allone;  // per column of A
    int verify_status = GOMILP_OK;              // verifyInputs, simplex.go:385-439
    double seconds_upload = 0;
    uint64_t serial = 0;      // unique per upload (device buffers are recycled: a pointer does not identify a problem)
    // children are recycled: their device buffers go back to a per-engine pool instead of hipFree (which synchronises
    // the whole device and would serialise the worker streams of a frontier pool)
    bool lazy_host = false;   // no host copy of A was kept at upload: ensure_host_A downloads it (flat call only)
    double scale_span = 1.0;  // max |a_ij| / min nonzero |a_ij| of A: beyond 1e9 the solve keeps the degenerate-pivot guard on at every size
    bool is_child = false;
    size_t cap_at = 0, cap_c = 0, cap_b = 0;    // capacities in doubles
    int32_t *dvar = nullptr;                    // child: branched variables / signs on the device
    double *dsign = nullptr;
    int cap_k = 0;
    int64_t root = -1;                          // child: the problem it was assembled from, its branching rows
    const Problem *root_ptr = nullptr;          //   (the same as a pointer: also set when the root lives in another engine)
    std::vector<int32_t> kvar;
    std::vector<double> ksign;
};

// Which kernels one factorization of the final solve runs (engine_final.cpp): decided once, at the top of Engine::lu_factor, from the row
// count, the knobs lu_blocked / lu_look / lu_cross / lu_large / bt_fault and the capacity of the buffer the small pack lands in —
// before anything is launched or acquired.  Afterwards only two things change it: the loop slots that could not be had
// (look_wanted) and step_down().
struct LuPlan {
    int m = 0;
    bool compressed = false;    // the compressed rounds (lu_compressed.hip, L/U column-major); else L/U row-major:
    bool blocked = false;       //   the blocked panels (lu_kernels.hip), or — neither — one launch per column.  Both skip unit-column steps
    bool large = false;         // knob lu_large: the compressed rounds on the eight-workgroup panel with several rows per lane
    bool small = false;         // compressed, few rows: k_luc_init clears the singular flag on the device and only the flag comes back
    bool look_wanted = false;   // the look-ahead schedule (LUArgs::look), while the engine holds the device's loop slots
    int cross_G = 0;            // workgroups of the cross-workgroup panel (lu_cross.hip); 0: the one-workgroup panel
    int cross_slots = 16;       // its register slots, 16 or 32
    bool oneshot = false;       // one batch of rounds and the small pack (k_luc_pack_small) in one host round trip
    bool inject_fault = false;  // diagnostic flavour, knob bt_fault = 2 (LUArgs::pad3)
    int steps_down = 0;
    // large bases: only the nd x nd part that couples the dense positions goes to the host (lu_compressed.hip,
    // k_luc_pack_dense / k_luc_solve_rows); small ones take one host pass over all rows (one round trip fewer)
    bool split(int nd) const { return compressed && m >= 1024 && nd > 0; }
    static LuPlan make(int m, int64_t lu_blocked, int64_t lu_look, int64_t lu_cross, int64_t lu_large, int64_t bt_fault, size_t small_pack_cap_bytes);
    bool step_down();   // after a launch gave up a wait: the next plainer schedule (false: there is none)
};
struct LuRoundsEnd { bool gave_up = false, landed = false; int enq = 0; };   // Engine::run_compressed_rounds

// The knobs that decide which block kernel runs a relaxation, and in which shape (gomilp_ctx_set; the routing table of DESIGN.md §2.1).
struct BtKnobs {
    int64_t chunk = 32, max_pivots = 0;           // pivots enqueued between host checks; safety cap (0 = none)
    int64_t block_k = 0, bt_nt = 0, bt_old = 0;   // single-workgroup block kernel: pivots per block and threads (0 = by shape; tests force the 1024-thread instance), first generation only
    int64_t bt_groups = 0;                        // -1 never several workgroups, 0 by shape, 2 / 4 / 8 forced where the shape fits, 16 the loop shapes also below 600 rows
    int64_t bt_stamps = 0;                        // diagnostic builds with cycle sums per wave: 1 the 8 x 256 loop instance, 2 the production shape (16 x 128 up to 2048 rows)
    int64_t bt_lag = 1, loop_chunk = 512;         // persistent loop kernel where the multi-workgroup block kernel runs (0: launch pairs); its pivots per launch
    int64_t loop_grid = 0, loop_upd = 0;          // its workgroups (0: by shape, one per CU at most); its update workgroups that take part (0: the instance's default)
    int64_t loop_g = 0, loop_k = 0;               // its pivot workgroups (8 / 16) and pivots per block (8 / 12 / 16) where instantiated, 0 = by shape
    int64_t loop_wave_rec = 1, loop_rep = 0;      // 16 x 128 instance: one exchange record per wave; opt-in role with replicated reduced costs (btr_kernels.hip)
    int set(const std::string &key, int64_t v);   // GOMILP_OK, GOMILP_ERR_BAD_SHAPE (value out of range), -1: not one of these knobs
};

// Which block kernel runs the pivot loop of a relaxation on the blocked tableau, and in which shape (the table of DESIGN.md §2.1): ONE
// value, a pure function of (m, ldt) and the knobs above (engine_tableau.cpp), made whenever the engine sets ldt_.  Set-up pivots,
// make_bt_args, the loop and the launchers read it; nothing downstream looks at a knob or calls bt_group_cfg again.
struct BtPlan {
    enum Pipeline : int { kSingle, kGroups, kLoop } pipeline = kSingle;   // block kernel of one workgroup / of several + update launches; persistent loop kernel
    int m = 0, ldt = 0;
    int K = 8;                                         // pivots per block
    bool tiled = false, tiled_forced = false;          // T in 4x4 tiles inside the pivot loop; for a block of one forced pivot (set-up, artificial exchange)
    BtGroupCfg cfg = {0, 0, 0};                        // bt_group_cfg's shape: set-up / forced pivots, make_bt_args (groups 0: one workgroup)
    BtLoop loop = BtLoop::None;                        // kLoop: the instance that runs,
    int slot_weight = 4, upd_cap = 0;                  //   the device slots it takes (1 shares the device with up to three others, 4 runs alone) and BTArgs::upd_cap
    BtLoop rep = BtLoop::None;                         // knob loop_rep: the replicated role that runs INSTEAD if Engine::loop_try_acquire_all gives the device right now
    int rep_upd_cap = 0;
    int64_t blocks_per_chunk = 1, loop_grid = 0;       // blocks between two looks at the device state (loop: per launch); knob loop_grid
    bool is_loop() const { return pipeline == kLoop; }
    int grid(int ncu, BtLoop inst) const;              // workgroups of a loop launch on a device of ncu CUs
    static BtPlan make(int m, int ldt, const BtKnobs &k);
};

// The knobs that decide where a single solve goes (gomilp_ctx_set; the table of DESIGN.md §2.4 "Where a solve goes").
struct SolveKnobs {
    int64_t tableau = 1, blocked = 1, fused = 1;       // A/B knobs: 0 keeps a solve off the tableau pipelines / the block kernels / the fused revised pipeline
    int64_t exact_degenerate = 1;                      // 0 never, 1 bases of up to 256 rows, non-slack starts and badly scaled inputs, 2 always: pivots whose winning ratio is (nearly) zero are decided on a fresh gonum-order x_B; 3 strict: EVERY pivot and the stop test are
    int64_t cond_guard = 1;                            // the condition guards of the reference: a host replay for bases of up to 64 rows, measured from the tableau beyond
    int64_t general_min_rows = 96, general_device = 1; // non-slack starts: from this many rows the column search and the artificial column are made on the device
    int set(const std::string &key, int64_t v);        // GOMILP_OK, GOMILP_ERR_BAD_SHAPE (value out of range), -1: not one of these knobs
};

// Where one solve goes: ONE value, a pure function of the shape, the kind of starting basis, Problem::scale_span and the knobs above
// (engine.cpp; no HIP call, no device query, no Problem; tests/test_solve_plan.py), made at the top of Engine::solve_locked /
// warm_locked.  Everything downstream — set-up, make_args, make_bt_args, the loops, the tail — reads it; nothing looks at a routing knob
// again.  What needs the device or the host copy of A (large_solve_fits, ensure_host_A) stays with the caller.
struct SolvePlan {
    enum StartKind : int { Slack, Searched, Supplied };   // the descending scan met m unit columns; findLinearlyIndependent; the caller's basis
    int status = GOMILP_OK;           // GOMILP_ERR_UNSUPPORTED: nothing takes the solve (strict mode off the exact steps, non-slack starts beyond the LDS window or beyond both the tableau row and the host copy of A)
    int pipeline = 0;                 // stats.pipeline: 0 three-kernel revised, 1 fused revised, 2 single-kernel tableau, 3 blocked tableau
    bool use_tab = false, blocked = false;
    bool gen_start = false;           // a searched or supplied (non-slack) basis: the degenerate-pivot guard stays on
    bool gen_revised = false;         // ... on the three-kernel revised loop (beyond the tableau's LDS row, or knob tableau = 0)
    bool badly_scaled = false;        // the entries of A span more than nine decades: guard on, tableau checked
    double guard = 0.0;               // BTArgs::guard / LPArgs::guard: 0, 1e-9, or +Inf (strict); 0 on every pipeline without exact steps
    double cguard = 0.0;              // BTArgs::cguard, and whether the exact steps and the end of the tableau loop measure the condition numbers (slack starts beyond 64 rows)
    bool replay_if_feasible = false;  // bases of up to 64 rows: a feasible start records its pivots for the host replay of the condition guards
    bool search_on_device = false, art_on_device = false;   // non-slack starts: the column search / the Phase-I artificial column on the device
    bool needs_host_A = false;        // the solve cannot start without the host copy of A (Engine::ensure_host_A)
    // does this solve decide degenerate pivots on fresh solves — the ONE statement of knob exact_degenerate (also RevBatchEngine::eligible,
    // BatchEngine).  Non-slack starts: a tree's repeated branch rows make nearly dependent tableau rows on equality forms, and a pivot on
    // their 1e-12 drift walks into a singular basis; badly scaled inputs: the updated tableau loses digits, the exact steps check and rebuild it
    static bool exact_wanted(int64_t mode, int m, bool slack_start, double scale_span) {
        return mode == 3 || mode == 2 || (mode == 1 && (m <= 256 || !slack_start || scale_span > 1e9));
    }
    static SolvePlan make(int m, int n, int ld, StartKind start, double scale_span, const SolveKnobs &k);   // m < n
    static SolvePlan warm(int ld, double scale_span, const SolveKnobs &k);   // the dual loop + Phase II of a warm start: the revised pipelines, no guard
};

class Engine {
   public:
    explicit Engine(int device);
    ~Engine();
    int device() const { return device_; }
    static int loop_acquire(int dev, int weight);          // slots for persistent loop kernels on a device (engine.cpp): returns the slot
    static void loop_release(int dev, int weight, int slot);
    static bool loop_try_acquire_all(int dev);             // the whole device, if nobody holds a slot right now (no waiting); release: loop_release(dev, 4, 0)
    int set(const std::string &key, int64_t v);

    // lazy_host: do not keep a host copy of a large A at upload (the flat call: the context is the caller's alone, and the copy is
    // only read on rare paths — ensure_host_A fetches it from the device then)
    int64_t upload(const double *c, const double *A, int64_t lda, const double *b, int64_t m, int64_t n, bool lazy_host = false);
    int free_problem(int64_t id);
    // child of a resident root: K branch-and-bound rows (var, sign, rhs) appended on the device (subproblem.go:141-159)
    int64_t upload_child(int64_t root, int K, const int32_t *var, const double *sign, const double *rhs);
    // the same with the root resident in ANOTHER engine of the same device (read in place: device buffers are immutable
    // after upload); the owner must not free the root before the child is freed
    int64_t upload_child_of(Engine &owner, int64_t root, int K, const int32_t *var, const double *sign, const double *rhs);
    int solve(int64_t id, double tol, const int64_t *initial_basic, double *opt_f, double *opt_x, int32_t *has_x,
              int64_t *basis_out, gomilp_lp_stats *stats);
    // gomilp_lp_solve_warm (engine_warm.cpp): a dual simplex from the kept state of `parent` (< 0: cold), keeping this problem's
    // final state when `keep`
    int solve_warm(int64_t id, int64_t parent, int keep, int dual_budget, double tol, double *opt_f, double *opt_x, int32_t *has_x,
                   int64_t *basis_out, gomilp_lp_stats *stats, gomilp_warm_stats *wstats);
   private:
    int solve_locked(int64_t id, double tol, const int64_t *initial_basic, double *opt_f, double *opt_x, int32_t *has_x,
                     int64_t *basis_out, gomilp_lp_stats *stats);
    // solve_locked, repeated once on the single-workgroup kernels after an exchange timeout (Engine::solve)
    int solve_cold_locked(int64_t id, double tol, const int64_t *initial_basic, double *opt_f, double *opt_x, int32_t *has_x,
                          int64_t *basis_out, gomilp_lp_stats *stats);
    // everything after the Phase-II loop of a solve (engine.cpp): the condition replay of small bases, the epilogue, the trace; keeps the
    // final state when keep_id_ asks for it.  rho_slack: the rows of the slack-basis start (basic_start), null for other starts
    int solve_tail(const Problem &P, int64_t id, int loop_rc, std::vector<int32_t> &basic, std::vector<double> &xb,
                   const std::vector<int32_t> &basic_start, const std::vector<int32_t> *rho_slack, double *opt_f, double *opt_x,
                   int32_t *has_x, int64_t *basis_out, gomilp_lp_stats *st);
    // ---- single-context warm start (engine_warm.cpp) ----
    struct Kept {                    // the final state of a solved problem: positional basis + explicit B^-1 (m x ld)
        double *d = nullptr;         // null: nothing kept (no_warm: the pipeline that ran has no way to give its B^-1)
        size_t cap = 0;              // doubles
        int m = 0, ld = 0;
        bool no_warm = false;
        std::vector<int32_t> basic;
    };
    std::map<int64_t, Kept> kept_;                        // by problem id
    std::vector<std::pair<double *, size_t>> keep_pool_;  // released B^-1 buffers (no hipFree per node: it synchronises the device)
    int64_t keep_id_ = -1;                                // the solve running keeps its final state under this id
    void keep_capture(const Problem &P, int64_t id, int pipeline, const std::vector<int32_t> &basic, const std::vector<int32_t> &basic_start,
                      const std::vector<int32_t> *rho_slack);
    void drop_kept(int64_t id);
    bool descendant(const Problem &P, int64_t parent, int *J) const;
    int warm_locked(int64_t id, const Kept &K, int J, int dual_budget, double tol, double *opt_f, double *opt_x, int32_t *has_x,
                    int64_t *basis_out, gomilp_lp_stats *st, gomilp_warm_stats *ws);
    int run_dual_loop(const Problem &P, double tol, int nn, int dual_budget, gomilp_warm_stats *ws);
   public:
    int64_t last_trace(gomilp_pivot *out, int64_t cap);

    // ---- hooks of the device-batched frontier (engine_batch.cpp) ----
    // device pointers / statistics of a resident problem: the batch engine reads the root's columns where they lie
    struct RootView {
        int m = 0, n = 0, ld = 0;
        const double *dAt = nullptr, *dc = nullptr, *db = nullptr;
        double scale_span = 1.0;          // Problem::scale_span of the root
        bool unit_basis = false;          // the descending scan of simplex.go:618-635 meets m distinct unit columns
        std::vector<int32_t> rho0;        // their rows, by basis position
        int verify_status = GOMILP_OK;
        uint64_t serial = 0;              // identifies the upload (device buffers are recycled)
        std::vector<double> hb, hc;       // host copies of b and c (final solves on another engine's behalf)
        // no slack basis (equality rows): the result of the column search (simplex.go:611-637) and the tableau of that basis,
        // computed ONCE per root (root_general) — a child's starting basis is this one + its K branch slacks, so the batched
        // schedule takes such children too instead of repeating the search per node
        struct General {
            int m = 0, nn = 0, ldt = 0;
            double *dT0 = nullptr, *dxb0 = nullptr;                              // m x ldt row-major B0^-1 A_N0; x_B of the basis
            int32_t *dbasic0 = nullptr, *dnonbasic0 = nullptr, *dposvar0 = nullptr;
            ~General();
        };
        std::shared_ptr<General> gen;     // null: slack basis, or no usable basis (the single-relaxation engine reports why)
        // the same search for a WIDE root (n - m >= 2m: the tableau row is what does not fit): the searched basis with its inverse instead
        // of its tableau, for the batched revised simplex (k_rv_gen_start of batch_revised.hip builds a child's B^-1 from it by copies and
        // sign flips).  Within the limits of SolvePlan::gen_revised only (general_rev_shape)
        struct GeneralRev {
            int m = 0, ld = 0;
            double *dB0inv = nullptr, *dxb0 = nullptr;       // m x ld row-major B0^-1, padding column zero; x_B0 of the gonum-order solve
            int32_t *dbasic0 = nullptr, *dposvar0 = nullptr; // m basis positions; per variable (n) its basis position, -1: nonbasic
            ~GeneralRev();
        };
        std::shared_ptr<GeneralRev> genrev;   // null: slack basis, a narrow root, outside the limits, or no usable basis
        // does a root of this shape get a GeneralRev: wide, the host copy of A within 2^25 entries, the rows within the LDS window
        static bool general_rev_shape(int64_t m, int64_t n) {
            return m < n && (n - m) >= 2 * m && m * n <= ((int64_t)1 << 25) && ((m + 1) & ~(int64_t)1) <= kLdsWindowLd;
        }
        // the root's A row-major on the device (one transposing copy per root): rows of the virtual tableau of a wide wave (BatchLP::A0r)
        struct RowMajor { double *dA = nullptr; int lda = 0; ~RowMajor(); };
        std::shared_ptr<RowMajor> rm;     // null: not made (large roots)
    };
    bool root_view(int64_t id, RootView *out);
    // fills out->gen (narrow roots) or out->genrev (wide roots) for a root without a slack basis (false: not possible — too large for the
    // host copy of A, singular, ...)
    bool root_general(int64_t id, RootView *out);
    // epilogue of simplex() (simplex.go:296-301) for a relaxation whose pivot loop ran elsewhere: final basis positions
    // `basic` (m entries) and updated x_B in, gonum-order solve of that basis, z, x out; `loop_rc` as Engine::solve
    int finish_from_basis(int64_t id, const int32_t *basic, const double *xb_updated, int loop_rc, double *opt_f, double *opt_x,
                          int32_t *has_x, int64_t *basis_out, gomilp_lp_stats *stats);
    // diagnostic: the device column search on a resident problem (tests compare it with the host forms)
    int debug_find_independent(int64_t id, std::vector<int32_t> &idxs);

    // pools, batched waves and warm starts keep the row limit of one-pass LDS staging (ld <= kLdsWindowLd)
    // (a pool lifts it with its knob large_rows: the workers then take what a context takes)
    void limit_rows_to_lds_window(bool on = true) { std::lock_guard<std::mutex> g(mu_); lds_window_only_ = on; }

   private:
    struct Work;  // device work buffers, sized for the largest problem seen
    int row_chunk2(const Problem &P) const;   // LPArgs::row_chunk2 for this problem (0: the one-pass kernels)
    bool device_fits(size_t bytes);           // free device memory (hipMemGetInfo) holds `bytes` with a margin
    bool large_solve_fits(const Problem &P);  // the work set of a solve beyond the LDS window fits the free memory
    int ensure_work(int m, int ncols);
    const Problem *problem_ptr(int64_t id);
    int64_t upload_child_impl(const Problem &R, int64_t root_id, int K, const int32_t *var, const double *sign, const double *rhs);
    LPArgs make_args(const Problem &P, int phase, double tol, int nn, const double *cost);
    int run_loop(const Problem &P, int phase, double tol, int nn, const double *cost, gomilp_lp_stats *st);
    int run_loop_fused(const Problem &P, int phase, double tol, int nn, const double *cost, gomilp_lp_stats *st);
    int run_loop_tab(const Problem &P, int phase, double tol, int nn, gomilp_lp_stats *st);
    int host_bland_tab(const Problem &P, int phase, double tol, int nn, gomilp_lp_stats *st, int *par_out);
    TabArgs make_tab_args(const Problem &P, int phase, double tol, int nn);
    int tab_forced_pivot(const Problem &P, int phase, double tol, int nn, int q, int ent, double rq, int p, double dp, double xp,
                         int lea, int flags, long long t);
    // The stages of solve_locked between the plan and solve_tail.  Start: the starting basis as the reference builds it
    struct Start {
        std::vector<int32_t> basic, rho;   // positions; slack start: the row of each position's unit column
        std::vector<double> xb, binv_host; // x_B = ab^-1 b; non-slack start: B^-1 from the host (empty when it is resident: gen_binv_dev_)
        bool slack = true, feasible = true;
    };
    int solve_square(const Problem &P, double *opt_f, double *opt_x, int32_t *has_x, gomilp_lp_stats *st);   // m == n: one linear solve
    int scan_start(const Problem &P, const int64_t *initial_basic, Start &s);    // the unit-column scan, or the caller's basis
    int search_start(const Problem &P, bool supplied, Start &s);                 // non-slack: column search, B^-1, x_B and its feasibility
    int upload_start(const Problem &P, const Start &s);                          // B^-1 / duals of the revised pipelines, x_B
    // Phase I / Phase II of the revised pipelines (engine.cpp) and of the tableau pipelines (engine_tableau.cpp): on return s.basic /
    // s.xb hold the final basis positions and updated x_B, *loop_rc the Phase-II loop result
    int solve_revised(const Problem &P, double tol, Start &s, gomilp_lp_stats *st, int *loop_rc);
    int solve_tableau(const Problem &P, double tol, Start &s, gomilp_lp_stats *st, int *loop_rc);
    int ensure_tableau_work(const Problem &P, int ldt);
    // Phase I, written once for both (engine.cpp).  phase1_artificial: a_{n+1} = b - sum_{i != minidx} a_{basic_i} into art (P.ld doubles)
    // and row n of dAt — w.basic must hold s.basic; GOMILP_ERR_PHASE1_WRAPPED for a zero column.  phase1_art_level: the artificial's level
    // at position `added` (-1: it left the basis) against phaseIZeroTol, GOMILP_ERR_INFEASIBLE beyond it
    int phase1_artificial(const Problem &P, const Start &s, int64_t minidx, std::vector<double> &art, gomilp_lp_stats *st);
    int phase1_art_level(const Problem &P, int added, const std::vector<double> &xb);
    int upload_padded(double *dst, const std::vector<double> &v, int ld);
    void return_point(const Problem &P, const std::vector<int32_t> &basic, const std::vector<double> &xb, double *opt_f, double *opt_x,
                      int32_t *has_x, int64_t *basis_out);
    int fetch_trace(std::vector<DevPivot> &tr);   // the device state into w.st_host, the recorded pivots (at most trace_cap) into tr
    void open_stats();                            // per-solve counters, at the top of solve_locked / warm_locked;
    int close_stats(gomilp_lp_stats *st, double t0, int code);   // ... and into the caller's stats on every way out (returns code)
    void bt_layout(const Problem &P, bool tiled);
    BTArgs make_bt_args(const Problem &P, int phase, double tol, int nn, int kmax);
    // the tableau's row length, and with it the plan of the blocked pipeline
    void set_ldt(const Problem &P, int ldt) { ldt_ = ldt; bt_plan_ = BtPlan::make(P.m, ldt, bt_knobs_); }
    int bt_forced_pivot(const Problem &P, int phase, double tol, int nn, int q, int p, int nocommit);
    int run_loop_bt(const Problem &P, int phase, double tol, int nn, gomilp_lp_stats *st);
    void account_samples(gomilp_lp_stats *st, const std::vector<int64_t> &sample_t, int64_t executed, int nk);
    int host_bland(const Problem &P, LPArgs &a, gomilp_lp_stats *st);
    int refresh_xb_y(const Problem &P, const double *cost);
    int epilogue(const Problem &P, std::vector<int32_t> &basic, std::vector<double> &xb, int loop_rc, double *opt_f, double *opt_x,
                 int32_t *has_x, int64_t *basis_out, gomilp_lp_stats *st);
    // the bit-exact final solve (engine_final.cpp)
    int final_solve(const Problem &P, std::vector<double> &xb_exact, bool *singular, const int32_t *basic_host = nullptr,
                    bool transpose = false, const double *rhs_host = nullptr);
    // its two halves: one factorization, any number of right-hand sides
    int lu_factor(const Problem &P, bool *singular, const int32_t *basic_host = nullptr, bool transpose = false);
    int lu_solve(const Problem &P, std::vector<double> &x, const double *rhs_host = nullptr);
    // the steps of lu_factor
    int gather_basis(const Problem &P, const LuPlan &plan, bool transpose);
    int upload_unit_rows(const Problem &P, const int32_t *basic_host, bool transpose, int *nonunit);
    int run_compressed_rounds(const LUArgs &a, const LuPlan &plan, int nonunit, LuRoundsEnd *end);
    int pack_and_fetch(const LUArgs &a, const LuPlan &plan, std::vector<int32_t> &dl);
    // What lu_solve needs of the last factorization, besides the packed factors themselves: those stay where lu_factor landed them, in
    // Work::h_W (m x nd by physical row; split: nd x nd by dense position), between lu_factor and any number of lu_solve calls.
    struct LuCache {
        bool valid = false, split = false, singular = false;
        int m = 0, nd = 0;
        std::vector<int32_t> phys, dl;   // physical row at a logical position; the positions whose step did arithmetic
        std::vector<double> diag;        // u_ii by physical row
        LUArgs args;
    } lu_cache_;
    // one iteration of the reference on fresh solves (engine_tableau.cpp): the decision a degenerate or tied pivot needs — exact_iter,
    // shared by the blocked tableau (exact_step) and the three-kernel revised loop of non-slack starts (run_loop)
    int exact_step(const Problem &P, int phase, double tol, int nn, int *q_out, int *p_out, gomilp_lp_stats *st);
    int exact_iter(const Problem &P, int phase, double tol, int nn, double *y_dev, double *r_dev, int ldr,
                   const std::function<int(int, int, const std::vector<int32_t> &, const std::vector<double> &)> &check_column, int *q_out,
                   int *p_out, gomilp_lp_stats *st);
    int exact_column_check(const Problem &P, const std::vector<int32_t> &basic, const std::vector<double> &dsol, const double *col_dev,
                           double *binv_dst, bool *rebuilt, gomilp_lp_stats *st);
    int cond_check(const Problem &P, int nn, double *k1, double *kinf);
    int cond_fresh(const Problem &P, const int32_t *basic_host, double *k1, double *kinf);   // from a fresh host inverse of the basis
    bool ensure_host_A(const Problem &P);
    // findLinearlyIndependent with the scan on the device (general_kernels.hip) and the last, square step on the host
    int find_independent_device(const Problem &P, std::vector<int32_t> &basic, std::vector<double> *binv_out, bool *binv_on_device = nullptr);
    int stage_upload(void *dst, const void *src, size_t bytes);
    hipError_t sync_stream();
    int upload_index_lists(const std::vector<int32_t> &basic, const std::vector<int32_t> &nonbasic);
    void sync_state_to_device();

    int device_;
    hipStream_t stream_ = nullptr;
    int ncu_ = 256;   // compute units of the device (grid of the persistent loop kernel)
    std::mutex mu_;
    std::vector<std::unique_ptr<Problem>> problems_;
    std::vector<std::unique_ptr<Problem>> child_pool_;  // released children, buffers kept
    // released root problems and the staging buffers of upload(), kept for the next upload of a fitting shape: the flat
    // lp.Simplex drop-in uploads and frees once per call, and hipFree synchronises the whole device (it would serialise
    // the concurrent callers of the drop-in)
    std::vector<std::unique_ptr<Problem>> root_pool_;
    double *up_dA_ = nullptr; size_t up_dA_cap_ = 0;
    int32_t *up_stats_ = nullptr; size_t up_stats_cap_ = 0;
    std::unique_ptr<Work> w_;
    // knobs (Engine::set)
    BtKnobs bt_knobs_;             // which block kernel runs, in which shape
    SolveKnobs knobs_;             // where a single solve goes
    int64_t refresh_ = 0, trace_on_ = 0, sample_events_ = 0, bt_upd_valu_ = 0, bt_fault_ = 0;
    int64_t poll_delay_ = 0;       // loop kernel: 64-cycle units between a wave's post and its first poll of an exchange
    int64_t general_block_ = 1, lu_blocked_ = 3, lu_cross_ = -1;
    int64_t lu_look_ = 1;          // 0 = never the look-ahead schedule (the workers of a pool)
    int64_t lu_large_ = 0;         // 1 = bases of 4097 .. 16384 rows take the compressed rounds on the eight-workgroup panel with several rows per lane (lu_cross.hip); 0 (default, and the workers of a pool) = one launch per column there
    int64_t row_chunk_ = 0;        // doubles per LDS chunk of the revised-simplex kernels' staged vectors; 0: one-pass staging up to ld = kLdsWindowLd, chunks of kAutoRowChunk beyond
    int64_t lu_look_faults_ = 0;   // final solves repeated with the plain schedule after a look-ahead launch gave up a wait
    int lu_look_fault_ = 0;        // ... in the running solve, one per fall-back (stats.device_retries)
    bool lds_window_only_ = false;   // refuse problems beyond the one-pass LDS window, as before the chunked form (pool workers)
    bool gen_binv_dev_ = false;   // the searched basis' B^-1 = R^-1 Q^T is resident in the first B^-1 buffer (the device judged the square step): no upload
    std::vector<double> exact_xb_;   // the fresh x_B of the last exact step (exact_iter)
    bool xchg_timeout_ = false;   // the last pivot loop ended in ST_XCHG_TIMEOUT (Engine::solve repeats the solve once)
    bool shadow_trace_ = false;   // this solve records its pivots for the replay even when the caller did not ask for a trace
    // per-solve state
    SolvePlan plan_;   // where the running solve goes
    int cur_ = 0;   // which Binv buffer is current
    int ycur_ = 0;  // which y buffer is current
    int grid_ratio_ = 1;
    int tcur_ = 0, rcur_ = 0, ldt_ = 0;   // tableau pipelines: current T / r buffer, row length of T (set_ldt)
    BtPlan bt_plan_;         // blocked tableau: the plan for (the problem being solved, ldt_)
    bool t_tiled_ = false;   // layout of T[tcur_]: 4x4 tiles (blocked pipeline, register-resident kernel) or row-major
    int64_t launches_ = 0;
    double fs_device_ = 0, fs_host_ = 0;
    int64_t lu_dense_ = 0, lu_rounds_ = 0;
    std::vector<gomilp_pivot> last_trace_;
    int64_t last_trace_total_ = 0;
};

// engine_general.cpp
// ascending ids below ncols that are not in the basis (simplex.go:174-184); the acceptance test of a candidate for the exchange of a
// zero-level artificial at position `added` (simplex.go:581-606): dcol = B^-1 a_j
void build_nonbasic(const std::vector<int32_t> &basic, int ncols, std::vector<int32_t> &nonbasic);
bool exchange_keeps_feasible(const double *dcol, const std::vector<double> &xb, int added, int m);
int general_find_linearly_independent(const std::vector<double> &A, int m, int n, std::vector<int32_t> &idxs, std::vector<double> *binv_out = nullptr);
int general_finish_last_column(const std::vector<double> &A, int m, int n, std::vector<int32_t> &idxs, int start_col, std::vector<double> *binv_out);
int general_find_linearly_independent_slow(const std::vector<double> &A, int m, int n, std::vector<int32_t> &idxs);
bool general_basis_inverse(const std::vector<double> &A, int m, int n, const std::vector<int32_t> &basic, int ncols_with_art,
                           const std::vector<double> &art, std::vector<double> &binv);

int general_condition_replay(const std::vector<double> &A, int m, int n, std::vector<int32_t> &basic, const std::vector<std::pair<int, int>> &pivots,
                             bool ended_in_compute_move, int *status_out, int64_t *evaluations);
double general_cond_inf(const std::vector<double> &A, int n);
bool general_invert(const std::vector<double> &B, int m, std::vector<double> &inv);
double inverse_norm1_estimate(const std::vector<double> &M, int n, bool transposed);
// gonum_cond.cpp: what gonum's mat.LU reports for a row-major n x n matrix (transposed: for its transpose) — cond = 1 / Dgecon(MaxRowSum) of the
// factors, and the Det() == 0 test of LU.Solve — bit for bit, for n <= kGonumCondMax (the range Dgetrf does not block); false beyond it
constexpr int kGonumCondMax = 64;
bool gonum_lu_cond(const double *M, int n, int ldm, bool transposed, double *cond, bool *det_zero);
bool gonum_lu_solve(const double *M, int n, int ldm, const double *b, double *x);   // LU.SolveVec's result (the point returned with a mat.Condition error)
double general_basis_cond1(const std::vector<double> &A, int m, int n, const std::vector<int32_t> &basic, const std::vector<double> &art);
bool general_solve_basis(const std::vector<double> &A, int m, int n, const std::vector<int32_t> &basic, const std::vector<double> &b, std::vector<double> &x);

int device_count();
const char *compiled_arch();

// launch wrappers implemented in simplex_kernels.hip
int launch_price(const LPArgs &a, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
int launch_ftran(const LPArgs &a, int nparts_price, int forced_pos, int forced_var, hipStream_t s, hipEvent_t e0 = nullptr,
                 hipEvent_t e1 = nullptr);
void launch_update(const LPArgs &a, int nparts_ratio, int forced_p, int no_swap, int bland, hipStream_t s,
                   hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// dual_kernels.hip (warm start)
void launch_dual_leave(const double *xb, int m, double tol, DevState *st, hipStream_t s);
int launch_dual_price(const LPArgs &a, hipStream_t s);
void launch_warm_binv(const double *Bp, int ldp, int mp, double *B, int ld, int m, const int32_t *kpos, const double *ksign, hipStream_t s);
void launch_tab_to_binv(const double *T, int ldt, bool tiled, int m, const int32_t *src, double *B, int ld, hipStream_t s);
// fused_kernels.hip
bool fused_supported(int ld);
int launch_price_fused(const LPArgs &a, const double *y_in, double *y_out, int pending, int nparts_ratio, hipStream_t s,
                       hipEvent_t e0, hipEvent_t e1);
int launch_update_ftran_fused(const LPArgs &a, int pending, int nparts_price, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
// tableau_kernels.hip
int tab_ld(int nn);
int launch_tableau_pivot(const TabArgs &a, int flags, int nparts, long long t, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
void launch_tab_gather(const double *At, int ld, int m, int nn, const int32_t *nonbasic, const int32_t *rho, double *T, int ldt,
                       bool tiled, hipStream_t s);
void launch_tab_gemm(const double *Binv, int ldb, const double *At, int ld, int m, int nn, const int32_t *nonbasic, double *T, int ldt, bool tiled, hipStream_t s);
void launch_tab_permute_cols(const double *Tin, int ld_in, double *Tout, int ld_out, int m, int nn_out, const int32_t *srcpos,
                             bool tiled, hipStream_t s);
int tab_r_chunks(int m);
void launch_tab_r(const double *T, int ldt, int m, int nn, const double *cost, const int32_t *basic, const int32_t *nonbasic,
                  double *scratch, double *r, bool tiled, hipStream_t s);
void launch_tab_row_colmax(const double *T, int ldt, int m, int nn, int row, double *out, bool tiled, hipStream_t s);
void launch_tab_column(const double *T, int ldt, int m, int jp, const double *xb, double *dvec, double *move, bool tiled, hipStream_t s);
void launch_cond_check(const double *T, int ldt, int m, int nn, const int32_t *nonbasic, const int32_t *basic, const double *At, int ld, int slack0, int nvar,
                       double *scratch, bool tiled, hipStream_t s);
void launch_exact_r(const double *At, int ld, int m, int nn, const int32_t *nonbasic, const double *y, const double *cost, double *r, int ldt, hipStream_t s);
// general_kernels.hip
void launch_gs_init(double *QT, int ldq, int m, GsState *st, hipStream_t s);
void launch_gs_init_perm(double *QT, double *Rinv, int ldq, int m, const int32_t *perm, const double *sgn, const double *beta, int s0, GsState *st, hipStream_t s);
void launch_gs_candidate(const double *acol, double *QT, double *Rinv, int ldq, int m, double *w, double *t, double *ypart, int cand, int32_t *idxs, GsState *st, hipStream_t s,
                         int last = 0);
int launch_luc_rounds_cross(const LUArgs &base, int32_t *pivrow, int nrounds, int round_base, double *xrec, int G, int slots, hipStream_t s);
void launch_luc_cross_panel(const LUArgs &a, int32_t *pivrow, double *xrec, int G, int slots, int nrole, hipStream_t s);   // lu_cross.hip: one panel launch of those rounds
size_t luc_cross_doubles();
void launch_luc_lpos_final(const LUArgs &a, hipStream_t s);
int luc_cross_groups(int m, int want);
int luc_large_rpt(int m);   // rows per lane of the lu_large panel (0: m is outside 4097 .. 16384)
int gs_scratch_rows();
int gs_block_width(int m);
int gs_block_scratch_rows();
void launch_gs_block(const double *At, int ld, int col0, int ncand, double *QT, double *Rinv, int ldq, int m, double *scratch, int32_t *idxs, GsState *st, hipStream_t s);
void launch_gs_binv(const double *Rinv, const double *QT, int ldq, int m, double *C, hipStream_t s);
void launch_gs_art(const double *At, int ld, int m, const int32_t *basic, int minidx, const double *b, double *art, hipStream_t s);
void launch_gs_norms(const double *C, int ldq, int m, double *out, const double *At, int ld, const int32_t *idxs, int cand, double *colsum, hipStream_t s);
// bt_kernels.hip
bool bt_supported(int m, int nn);
int bt_max_k();
int bt_reg_k(int m, int ldt, int nt_force);
bool bt_tiled(int m, int ldt, int kmax, int nt_force, bool old_only);
// btg_kernels.hip: the block kernel over G workgroups of one XCD
BtGroupCfg bt_group_cfg(int m, int ldt, int knob);
size_t bt_xbuf_doubles();
void launch_bt_inner_groups(const BTArgs &a, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
const char *bt_group_kernel_name(int G, int ri);
constexpr int kBtStampSegs = 16;   // cycle sums per wave written by the diagnostic build of k_bt_inner2
void launch_bt_tile(const double *src, double *dst, int m, int ldt, bool to_tiles, hipStream_t s);
void launch_bt_inner(const BTArgs &a, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
void launch_bt_update(const BTArgs &a, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
bool bt_loop_supported(const BtGroupCfg &c);
bool launch_bt_loop(BtLoop inst, const BTArgs &a, int grid, hipStream_t s, hipEvent_t e0, hipEvent_t e1);   // false: not an instance of k_bt_loop, or a grid below BtLoopShape::min_grid
// btr_kernels.hip
bool bt_loop_rep_supported(int m, int ldt);
int bt_loop_rep_threads(int m, int ldt);
long long bt_loop_rep_launches();
long long bt_loop_wave_rec_launches();
bool launch_bt_loop_rep(BtLoop inst, const BTArgs &a, int grid, hipStream_t s, hipEvent_t e0, hipEvent_t e1);   // (the Rep* instances)
bool bt_batch_supported(int m_max, int ldt_max);
int bt_batch_k(int m_max, int ldt_max);
void launch_bt_inner_batch(const BatchLP *lps, const int *ids, const int *count, int nlp, int m_max, int ldt_max, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr, int xcd_off = 0);
void launch_bt_update_batch(const BatchLP *lps, const int *ids, const int *count, int nlp, int m_max, int ldt_max, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
const char *bt_batch_kernel_name(int m_max, int ldt_max);
// the batched block kernel on a virtual tableau (bt_kernels.hip k_bt_inner2_virt_batch; BatchLP::virt)
bool bt_virt_batch_supported(int m_max, int ldt_max);
void launch_bt_inner_virt_batch(const BatchLP *lps, const int *ids, const int *count, int nlp, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// batched persistent loop kernel (bt_kernels.hip k_b_loop): relaxations per launch on a device with ncu CUs; shapes it takes
int b_loop_slots(int ncu);
bool b_loop_supported(int m_max, int ldt_max);
void launch_b_loop(const BatchLP *lps, const int *ids, const int *count, int nlp, int nblocks, int par, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// res_kernels.hip: the register-resident tableau kernel for the long chains of a narrow wave (G workgroups per relaxation on one XCD)
size_t b_res_slot_bytes();
int b_res_max_slots();
int b_res_groups(int m_max, int nn_max, int ldt_max);
void launch_b_res(const BatchLP *lps, const int *ids, const int *count, int nlp, int G, int nb, double seq0, void *xbase, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// batch_kernels.hip
int batch_ldt(int nn);
void launch_b_setup(BatchLP *lps, int nlp, hipStream_t s);
void launch_b_setup_warm(BatchLP *lps, int nlp, hipStream_t s);
void launch_b_posvar(const int32_t *basic, int m, const int32_t *nonbasic, int nn, int32_t *posvar, hipStream_t s);
bool bt_dual_batch_supported(int m_max, int ldt_max);
void launch_bt_inner_dual_batch(const BatchLP *lps, const int *ids, const int *count, int nlp, int m_max, int ldt_max, hipStream_t s);
void launch_b_gather(const BatchLP *lps, int nlp, int m_max, int ldt_max, int mode, hipStream_t s);   // mode: batch_kernels.hip k_b_gather
void launch_b_write_virt(const BatchLP *lps, const int *ids, const int *count, int *list, int *nalive, int bound, int m_max, int ldt_max, int ncu, hipStream_t s);          // the survivors of a virtual first block (= mode 3, one tile per thread)
void launch_b_ctrl(BatchLP *lps, const int *ids_in, const int *count_in, int bound, int n_max, BatchOut *outs, int *ids_out, int *count_out, int loop_par, hipStream_t s);
void launch_b_init_ids(int *ids, int *count, int nlp, hipStream_t s);
void launch_b_permute(const BatchLP *lps, const int *ids, const int *count, int bound, int m_max, int ldt_max, hipStream_t s);
void launch_b_tab_r(const BatchLP *lps, const int *ids, const int *count, int bound, int m_max, int ldt_max, hipStream_t s);
void launch_transpose_in(const double *A, int64_t lda, int m, int n, double *At, int ld, hipStream_t s);
void launch_col_stats(const double *At, int ld, int m, int n, int32_t *nnz, int32_t *lastrow, int32_t *allone, int32_t *rowflag, unsigned long long *range,
                      hipStream_t s);
void launch_set_binv_perm(double *binv, int ld, int m, const int32_t *rho, hipStream_t s);
void launch_child_assemble(const double *At0, int ld0, int m0, int n0, double *At1, int ld1, int K, const int32_t *var,
                           const double *sign, hipStream_t s);
void launch_matvec_rows(const double *M, int ld, int m, const double *vec, double *out, hipStream_t s, int row_chunk2 = 0);
int y_chunks(int m);
void launch_y_from_binv(const double *binv, int ld, int m, const double *cost, const int32_t *basic, double *scratch,
                        double *y, hipStream_t s);
void launch_gather_w(const double *At, int ld, int m, const int32_t *basic, double *W, int ldw, hipStream_t s);
int lu_grid(int m);
void launch_lu(const LUArgs &a, hipStream_t s);
// lu_kernels.hip
bool lu_blocked_supported(int m);
int launch_lu_blocked(const LUArgs &a, int32_t *pivrow, hipStream_t s);
// lu_compressed.hip
bool lu_compressed_supported(int m, bool large);   // large: knob lu_large (4097 .. 16384 rows: lu_cross.hip luc_large_rpt)
int lu_compressed_nb();   // dense steps a round can take
void launch_luc_init(const LUArgs &a, hipStream_t s);
int launch_luc_rounds(const LUArgs &a, int32_t *pivrow, int nrounds, int round_base, hipStream_t s);
void launch_luc_gather(const double *At, int ld, int m, const int32_t *basic, double *W, int ldw, hipStream_t s);
void launch_luc_pack_dense(const LUArgs &a, const int32_t *dlist, int nd, const int32_t *pivrow, double *Wdd, double *diag, hipStream_t s);
void launch_luc_solve_rows(const LUArgs &a, const int32_t *dlist, int nd, const double *b, const double *xdL, const double *xdU,
                           double *x, hipStream_t s);
void launch_luc_pack(const LUArgs &a, const int32_t *dlist, int nd, double *Wd, double *diag, hipStream_t s);
void launch_luc_pack_small(const LUArgs &a, double *out, hipStream_t s);   // small bases: factors, diagonal, row positions, flags, control blocks in one block
size_t luc_pack_small_bytes(int m);
void launch_lu_pack(const LUArgs &a, const int32_t *dlist, int nd, double *Wd, double *diag, hipStream_t s);

}  // namespace gomilp
