/*
 * lpg.h — C-ABI of the MI355X (gfx950) dense-tableau simplex pivot engine.
 *
 * This is the drop-in boundary for the pivot loop that the reference
 * (SomeBottle/LinearProgramming) is missing. The reference's solver driver
 * `void newSimplex(LPModel *model)` (Source/simplex.h:13, Source/simplex.c:27-73)
 * builds the tableau with
 *   `SimplexMatrix CreateSMatrix(LPModel *model, size_t **lack, short int *valid)`
 *   (Source/matrix.h:23, Source/matrix.c:19-91)
 * and frees it with `void RevokeSMatrix(SimplexMatrix *)` (matrix.h:25,
 * matrix.c:97-123) without ever pivoting (the loop belongs between
 * simplex.c:40 and simplex.c:65). Every entry point below replaces a piece of
 * that missing loop, or of the SimplexMatrix (matrix.h:13-21) storage it would
 * have run on; the binding a maintainer adds to simplex.c is in INTEGRATION.md.
 *
 * Tableau layout (row-major fp64, same as SimplexMatrix.cMatrix flattened):
 *   rows 0..m-1  constraint rows  [b_i | a_i1 .. a_iN]   (matrix.c:42-48, 62-66)
 *   row  m       objective row    [z   | d_1  .. d_N ]   d_j = z_j - c_j
 *   (LPG_FLAG_BIG_M: row m = M part, row m+1 = real part; d_j = dM_j M + dR_j)
 *   columns      0 = b, 1..N = variables in LPAlign order (simplex.c:238-260)
 * The reference maximises (LPStandardize turns min into max, simplex.c:99-106),
 * so the engine maximises; the optimum is reached when every d_j >= -eps_opt.
 *
 * Conventions follow the reference's C style: plain pointers and sizes, caller
 * owns host buffers (they are copied), the context owns device memory. Return
 * codes: 0 = success, < 0 = error (lpg_last_error has the text); a host
 * wrapper maps this onto the reference's `short int valid` (valid = rc == 0).
 * One context per host thread; not reentrant.
 *
 * Multi-GPU: one process per GPU. Each rank creates its context with
 * lpg_create_dist() and owns the row block [row0, row0 + nrows) of the m
 * constraint rows (row0 = floor(m*rank/world)); the objective row and the
 * basis are replicated. Per pivot the ranks exchange the ratio-test
 * candidates and the normalised pivot row. Default for world > 1 (round 3):
 * the owner push (lpg_comm_init_push*: the owner stores the row straight into
 * every rank's IPC-mapped buffer over xGMI, flag per chunk). With a
 * communicator only (or env LPG_EXCHANGE=rccl): RCCL collectives, an
 * allgather of the candidates and an allreduce of the owner's row and zeros
 * (= a broadcast from a device-resident root).
 */
#ifndef LPG_H
#define LPG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes ---- */
#define LPG_OK           0
#define LPG_ERR_ARG     -1
#define LPG_ERR_DEVICE  -2
#define LPG_ERR_OOM     -3
#define LPG_ERR_STATE   -4
#define LPG_ERR_COMM    -5

/* ---- solve status (SURVEY.md §5 failure detection) ---- */
#define LPG_RUNNING      0
#define LPG_OPTIMAL      1
#define LPG_UNBOUNDED    2
#define LPG_INFEASIBLE   3
#define LPG_ITER_LIMIT   4
#define LPG_NUMERIC      5

/* ---- pricing rules ---- */
#define LPG_RULE_DANTZIG 0   /* k = argmin d_j, ties -> smallest j; ratio ties -> smallest row */
#define LPG_RULE_BLAND   1   /* k = min{j : d_j < -eps}; ratio ties -> smallest basic column */

/* ---- synthetic generators (device-side) ---- */
#define LPG_GEN_DENSE      0  /* A_ij = u, b_i = n/8 (1+u), c_j = 1+u, <= rows, slack basis */
#define LPG_GEN_DEGENERATE 1  /* lower-triangular KM-style rows (a_ii = 1, a_ij = u/(i+1)), b_i = 0 on even rows */
#define LPG_GEN_DUAL       3  /* dual-simplex LP: min c.x, A x >= b (A = u, b = n/8 (1+u), c = 1+u) as
                                 rows [-b | -A | I], objective row [0 | c | 0] */
#define LPG_GEN_ARTIFICIAL 2  /* config 5: KM-style; even rows `<= 0` (a_ij = -u/(i+1)), odd rows equalities whose
                                 unit columns are artificials at columns 1+n+ceil(m/2) .. N */

/* ---- lpg_create flags ---- */
#define LPG_FLAG_NO_LOG  0x1u  /* do not record the (entering, leaving) pivot log */
#define LPG_FLAG_NO_SKIP 0x2u  /* update every column (no skipping of P[j] == 0 slices). A context does so on its own
                                  once lpg_load_rows has given it a -0 or a non-finite entry or lpg_solve_dual has run
                                  (negative pivots make -0s): skipping a column is bit for bit the full update only
                                  on a tableau free of both. lpg_generate, or loading the whole tableau clean, starts
                                  again. Forced pivots on negative elements (lpg_pivot) are not tracked. */
#define LPG_FLAG_BIG_M   0x4u  /* two objective rows: row m = M part, row m+1 = real part (Big-M) */
#define LPG_FLAG_EAGER   0x8u  /* one rank-1 update pass per pivot instead of deferred (blocked) updates */

/* Deferred updates (default): the constraint rows are brought up to date in
 * one HBM pass per block of up to LPG_DEFER_MAX pivots. Default K (decided
 * from the largest rank's tableau bytes): 96 in region mode (lpg_info.region)
 * from 2 GB on one rank and from 1 GB on the ranks of a row partition, where
 * the region-mode slices hold 96 slots (config 3); 96 from 16 GB (the
 * two-kernel pair, config 4); 64 from 200 MB; 32 below. Env LPG_DEFER=K picks
 * K, K in 1 .. 128; 0 = eager. The persistent pivot kernel takes blocks of up
 * to 96 slots where its slices fit (lpg_info.pivot_wg > 0), else the pair
 * runs the pivots. Values,
 * pivot sequence and log are bitwise those of eager updates; every call that
 * reads or replaces the tableau (lpg_get_rows, lpg_get_column0, lpg_load_rows,
 * lpg_set_basis, lpg_set_objective*, lpg_sync, lpg_device_sync, the end of
 * lpg_solve) applies the pending block first. Single-rank contexts may keep the
 * columns in a different physical order between such calls (nonbasic columns
 * contiguous); every call that exposes or takes columns sees caller order. */
#define LPG_DEFER_MAX    128

typedef struct lpg_ctx lpg_ctx;

/* Same field layout as oracle/lpo.h's lpo_result. */
typedef struct {
    int32_t status;       /* LPG_* status */
    int32_t rule;         /* rule of the last solve */
    int64_t pivots;       /* pivots applied so far */
    double  objective;    /* T[m][0]: z without the objective constant (matrix.c:23-28) */
    int64_t entering;     /* last pivot's column (1-based, like cMatrix columns), -1 if none */
    int64_t leaving;      /* last pivot's row (0-based), -1 if none */
} lpg_result;

typedef struct {
    int64_t m, ncols, ld;       /* constraint rows, N+1 columns, row pitch (doubles) */
    int64_t row0, nrows;        /* this rank's constraint-row block */
    int32_t world, rank, device;
    int32_t nobj;               /* objective rows (1) */
    int32_t defer_k;            /* pivots per deferred block (0: eager updates) */
    int32_t pivot_wg;           /* workgroups of the persistent pivot kernel (one launch per run of
                                   pivots, lpg_block.hip); 0: two kernels per pivot */
    double  bytes_per_pivot;    /* algorithmic HBM bytes of one rank-1 update on this rank:
                                   16 * (nrows + nobj) * ncols (one read + one write) */
    int32_t exchange;           /* per-pivot exchange of a multi-rank context: 0 collectives (or none),
                                   1 owner push, 2 owner push into uncached exchange buffers */
    int32_t column_trade;       /* 1: the deferred path keeps the nonbasic columns contiguous (a column
                                   trade at every block's end; default from 2 GB per single rank, env
                                   LPG_NO_REORDER=0/1) */
    int32_t residency_fallbacks;  /* persistent pivot launches that found their grid (every rank's) not resident
                                     at once -- another kernel or process held CUs -- and handed the loop to the
                                     two-kernel pair (pivot_wg is 0 from then on) */
    int32_t region;             /* 1: the persistent pivot kernel runs in region mode -- its slices hold only the
                                   block start's nonbasic columns plus a spare slot per pending pivot for the
                                   column leaving the basis then (one rank, one objective row, column trade on;
                                   the default where it fits, env LPG_REGION=0 turns it off) */
    int32_t region_recoveries;  /* region-mode launches that found a block's column trade incomplete
                                   (DevState::rbad), ran no pivot and were re-run after a region rebuild */
} lpg_info_t;

typedef struct {
    double  update_ms;          /* summed device time of the update kernel (eager: rank-1 update per
                                   pivot; deferred: the block flush) */
    double  select_ms;          /* summed device time of pricing + ratio-test kernels (eager mode;
                                   deferred mode times the flushes only and reports 0) */
    double  comm_ms;            /* summed device time of the collectives */
    int64_t update_count;       /* update / flush launches timed */
    double  update_bytes;       /* bytes the update / flush kernels read + wrote (8 B x 2 per tableau
                                   entry in a column not skipped); eager: equals update_count *
                                   bytes_per_pivot when nothing is skipped */
} lpg_timing;

/* Host-staged collectives supplied by the caller (tests, non-RCCL transports).
 * Buffers are HOST memory; calls block until complete. */
typedef struct {
    void *user;
    int (*allgather)(void *user, const void *send, void *recv, size_t bytes_per_rank);
    int (*allreduce_sum_f64)(void *user, double *buf, size_t count);
} lpg_host_comm_ops;

/* ---- lifecycle ---- */
int  lpg_device_count(int *count);
/* Single-GPU engine for an m x ncols tableau (ncols = N+1).
 * Replaces the SimplexMatrix allocation of CreateSMatrix (matrix.c:33-48). */
int  lpg_create(lpg_ctx **out, int device, int64_t m, int64_t ncols, uint32_t flags);
/* One rank of a row-block partitioned engine; attach a communicator next. */
int  lpg_create_dist(lpg_ctx **out, int device, int world, int rank,
                     int64_t m, int64_t ncols, uint32_t flags);
int  lpg_comm_unique_id(void *uid, size_t len);              /* RCCL id, len >= 128 */
/* Attach an RCCL communicator (all ranks call it together). A world-1
 * context may attach one too: the per-pivot collectives then run for real on
 * a 1-rank communicator (used to test and time the exchange on one GPU). */
int  lpg_comm_init_rccl(lpg_ctx *ctx, const void *uid, size_t len);
int  lpg_comm_init_host(lpg_ctx *ctx, const lpg_host_comm_ops *ops);
/* Owner-push exchange for the deferred multi-rank loop (the north star's
 * pivot-row broadcast and candidate all-reduce, SURVEY.md §8(e), without a
 * collective per pivot): the owner of the pivot row stores it straight into
 * every rank's exchange buffer and raises per-chunk flags, every rank stores
 * its ratio candidates into every rank's buffer as self-validating tagged
 * words. Attach a communicator first (setup and bootstrap still use it),
 * then give every rank all ranks' buffers: IPC handles between processes
 * (lpg_comm_push_handle -> exchange -> lpg_comm_init_push), device pointers
 * between ranks of one process (lpg_comm_push_base -> lpg_comm_init_push_local).
 * Waits are bounded (2 s): a rank that waits longer ends the solve with
 * LPG_NUMERIC and lpg_last_error names the exchange. With the push attached,
 * each block (<= 96 pivots; region mode with K = 96 from 1 GB per rank, see
 * above) runs as one persistent launch per block on every
 * rank (lpg_info.pivot_wg > 0; each rank needs its own GPU, or launches
 * small enough to be resident together; env LPG_PERSIST_MR=0: two kernels
 * per pivot). The exchange's kernels spin-wait on their peers, so attaching
 * is refused (LPG_ERR_STATE, lpg_last_error names the reason) when ranks
 * would depend on each other for hardware queues or CUs: ranks that are
 * threads of one process (lpg_comm_init_push_local, world > 1), or ranks of
 * several processes on one GPU (same PCI bus id). Nothing has pivoted then:
 * the caller keeps the collectives. Env LPG_PUSH_SHARED_QUEUES=1 /
 * LPG_PUSH_SHARED_DEVICE=1 acknowledge the sharing (tests on one GPU). */
#define LPG_PUSH_HANDLE_BYTES 64
int  lpg_comm_push_handle(lpg_ctx *ctx, void *handle, size_t len);
int  lpg_comm_push_base(lpg_ctx *ctx, void **base);
int  lpg_comm_init_push(lpg_ctx *ctx, const void *handles, size_t len);
int  lpg_comm_init_push_local(lpg_ctx *ctx, void *const *bases, int world);
/* Replaces RevokeSMatrix (matrix.c:97-123). NULL is a no-op. */
void lpg_destroy(lpg_ctx *ctx);
int  lpg_info(const lpg_ctx *ctx, lpg_info_t *out);
const char *lpg_last_error(const lpg_ctx *ctx);
/* The source stamp this library was built from (16 hex digits: sha256 over
 * the engine's csrc/ files and this header, linearprogramming_amd/_stamp.py).
 * No reference counterpart: a loader compares it with the sources beside the
 * library and refuses a stale binary. */
const char *lpg_build_stamp(void);

/* ---- loading (host buffers are copied) ---- */
/* Rows [row0, row0+nrows) in GLOBAL numbering, each [b | a_1..a_N] with pitch
 * ld >= ncols. Row index m is the objective row. Rows outside this rank's
 * block are skipped. Replaces CreateSMatrix's cell fill (matrix.c:42-66). */
int  lpg_load_rows(lpg_ctx *ctx, int64_t row0, int64_t nrows, const double *rows, int64_t ld);
/* basis[i] = 1-based column of row i's basic variable (all m rows, every
 * rank). Replaces SimplexMatrix.basicVars (matrix.c:67-78). */
int  lpg_set_basis(lpg_ctx *ctx, const int64_t *basis);
/* Objective row from costs c[0..N-1] of `max c.x` and the current basis:
 * d_j = sum_i c_B(i) T[i][j] - c_j, z = sum_i c_B(i) b_i, summed in global
 * row order with fma (bitwise independent of the partition). Replaces
 * SimplexMatrix.ofCosts / basicCosts (matrix.c:55-57, 76-77). The pivot
 * count and log are kept (phase I -> phase II). */
int  lpg_set_objective(lpg_ctx *ctx, const double *c);
/* Big-M contexts: the M-part objective row from M-part costs (the real row
 * comes from lpg_set_objective). */
int  lpg_set_objective_m(lpg_ctx *ctx, const double *costM);
int  lpg_set_tolerances(lpg_ctx *ctx, double eps_piv, double eps_opt);
/* Price only columns 1..nact (e.g. to exclude artificials). */
int  lpg_set_active_columns(lpg_ctx *ctx, int64_t nact);
/* Device-side synthetic LP with n structural columns (ncols == n + m + 1). */
int  lpg_generate(lpg_ctx *ctx, int64_t n, uint64_t seed, int kind);

/* ---- the pivot loop (the part simplex.c:40-65 lacks) ---- */
/* Pivot until optimal / unbounded / numeric trouble or max_pivots more
 * pivots; blocks; fills *out. A status of LPG_ITER_LIMIT means the budget
 * ran out first. */
int  lpg_solve(lpg_ctx *ctx, int64_t max_pivots, int rule, lpg_result *out);
/* Asynchronous form for benchmarking: enqueue exactly npivots pivots on the
 * context's stream without any host synchronisation (pivots after the LP
 * finishes are no-ops on the device); lpg_sync waits and reports. */
int  lpg_enqueue(lpg_ctx *ctx, int64_t npivots, int rule);
/* Waits for everything enqueued, applies any pending deferred block (so the
 * tableau is current) and reports. */
int  lpg_sync(lpg_ctx *ctx, lpg_result *out);
/* Pre-size the device pivot log for npivots more pivots so that no
 * reallocation (and host synchronisation) happens inside a timed region. */
int  lpg_reserve_log(lpg_ctx *ctx, int64_t npivots);
/* Build, ahead of the pivot loop, the replayed HIP graph that lpg_enqueue /
 * lpg_solve use for runs of at least two blocks under this rule (capture +
 * instantiate, ~0.5 ms of host time), so that it does not land inside a timed
 * region. No pivot runs; a pending deferred block is applied first. A no-op
 * where the loop does not replay graphs (graphs disabled, eager timing, a
 * host communicator). */
int  lpg_prepare(lpg_ctx *ctx, int rule);

/* Apply one caller-chosen pivot (entering column k, 1-based; leaving row r,
 * 0-based) with the same arithmetic as the loop; |T[r][k]| must exceed
 * eps_piv (either sign). Counts as a pivot and is logged. On a row partition
 * every rank calls it with the same (k, r). */
int  lpg_pivot(lpg_ctx *ctx, int64_t k, int64_t r);
/* Two-phase method for a tableau whose columns art_first..N are artificial
 * unit columns basic in the rows that lacked an identity column
 * (reference: the empty `case 2:` of simplex.c:61-62, lack list from
 * matrix.c:80-89). Phase I maximises -sum(artificials); a negative optimum
 * means LPG_INFEASIBLE. Artificials left basic at zero are pivoted out on the
 * first usable original column of their row. Phase II prices columns
 * 1..art_first-1 only, with the objective row recomputed from cost[0..N-1]
 * (cost NULL: -1 x the objective row as loaded, i.e. a slack-form -c row).
 * On a row partition every rank calls it with the same arguments (it is
 * collective): the |b| sum of the feasibility test runs over the ranks in
 * global row order, and each artificial row's owner finds its column and
 * shares it through the communicator before every rank pivots (round 3). */
int  lpg_solve_two_phase(lpg_ctx *ctx, int64_t art_first, const double *cost, int64_t max_pivots, int rule,
                         lpg_result *out);

/* Big-M method (reference: the empty `case 1:` of simplex.c:58-60, constant
 * M of dataReader.c:165-173) on a LPG_FLAG_BIG_M context: artificial columns
 * art_first..N cost -M, kept symbolic as a second objective row, so pricing
 * is lexicographic (M part first) exactly like the reference's Number with a
 * constant (numOprts.h:15-37); no numeric M is ever formed. An optimum with a
 * negative M part means LPG_INFEASIBLE. cost NULL: -1 x the real objective
 * row as loaded. */
int  lpg_solve_big_m(lpg_ctx *ctx, int64_t art_first, const double *cost, int64_t max_pivots, int rule,
                     lpg_result *out);

/* Dual simplex (reference: router option 2, router.c:32-34, a no-op; the
 * tableau LPStandardize(model, 1) builds by flipping >= rows, simplex.c:178-179).
 * Needs a dual-feasible basis (every d_j >= -eps_opt, else LPG_ERR_STATE).
 * Leaving row: most negative b_i < -eps_opt (ties: smallest row); entering
 * column: min d_j / (-a_rj) over a_rj < -eps_piv (ties: smallest j); none ->
 * LPG_INFEASIBLE; no negative b -> LPG_OPTIMAL. Same update kernel and
 * arithmetic as the primal loop. On a row partition (round 3) every rank
 * calls it (collective) and the deferred form runs: the row candidates are
 * allgathered and the leaving row is summed from its owner; LPG_FLAG_EAGER
 * is single rank. */
int  lpg_solve_dual(lpg_ctx *ctx, int64_t max_pivots, lpg_result *out);

/* ---- readout ---- */
int  lpg_get_rows(lpg_ctx *ctx, int64_t row0, int64_t nrows, double *out, int64_t ld);
int  lpg_get_basis(lpg_ctx *ctx, int64_t *basis);            /* m entries */
int  lpg_get_column0(lpg_ctx *ctx, double *xB);               /* local rows' b (x_B) */
int64_t lpg_get_log(lpg_ctx *ctx, int64_t *k, int64_t *r, int64_t max);

/* ---- measurement ---- */
int  lpg_set_timing(lpg_ctx *ctx, int enable);
int  lpg_get_timing(lpg_ctx *ctx, lpg_timing *out);          /* syncs; resets the sums */
int  lpg_device_sync(lpg_ctx *ctx);

/* ---- batches: many small LPs in one launch ----
 * An lpg_ctx spreads ONE tableau over the chip; a caller with a thousand
 * small LPs (parameter sweeps, scenario sets, the node LPs of a
 * branch-and-bound tree, SURVEY.md:72) would loop create / solve / destroy.
 * An lpg_batch holds `count` tableaus of one shape, each (m+1) x ncols as
 * above (one objective row), back to back in device memory with row pitch
 * lpg_batch_info_t.ld, and solves them in one launch: one workgroup per LP
 * (lpg_batch.hip k_batch_solve), no communication between workgroups, the
 * chip filled by the batch. Each LP has its own basis, status, pivot count,
 * last (entering, leaving) and pivot log, and computes bit for bit what
 * lpg_solve / lpg_solve_dual (and oracle/lpo.c) compute for it alone.
 *
 * Tier: where a whole tableau plus its pivot row, pivot column and basis fit
 * the 150 KiB dynamic LDS cap, the tableau stays in LDS while its LP runs
 * (LPG_BATCH_TIER_LDS); else it stays in device memory and only the pivot
 * row and column are staged in LDS (LPG_BATCH_TIER_GLOBAL; m + 1 <= 8192 and
 * ncols <= 8192 -- larger tableaus belong to lpg_create). Env
 * LPG_BATCH_TIER=global forces the second tier.
 *
 * Bounded launches: a launch applies at most lpg_batch_info_t.chunk pivots
 * per LP (default 4096, fewer for large global-tier tableaus; env
 * LPG_BATCH_CHUNK); the host relaunches until no LP is still running. A
 * cycling LP therefore ends at its budget (LPG_ITER_LIMIT), never in an
 * unbounded kernel.
 *
 * Two-phase: lpg_batch_solve_two_phase runs lpg_solve_two_phase's algorithm
 * on every LP (lpg_batch.hip k_batch_two_phase): phase I, the feasibility
 * test, the drive-out of basic artificials and phase II all happen in the
 * workgroup that owns the LP, an LDS-tier tableau staying in LDS across the
 * transition, so an LP that finishes phase I early goes on at once. A launch
 * is bounded here too (a pivot, drive-outs included, or an objective
 * computation is one unit of `chunk`); the per-LP phase and drive-out cursor
 * round-trip with the rest of the state and the next launch resumes there.
 *
 * Big-M: a batch from lpg_batch_create_big_m holds (m+2) x ncols tableaus,
 * the M part of the objective in row m and the real part in row m + 1 (the
 * layout of an LPG_FLAG_BIG_M context), and lpg_batch_solve_big_m runs
 * lpg_solve_big_m's algorithm on every LP (lpg_batch.hip k_batch_big_m: both
 * objective rows in the rank-1 update, lexicographic pricing). The extra row
 * counts in the LDS footprint, so the tier boundary lies one row earlier than
 * for a plain batch. The two kinds of batch are kept apart: the other solve
 * calls refuse a Big-M batch and lpg_batch_solve_big_m a plain one
 * (LPG_ERR_STATE, nothing has pivoted).
 *
 * Ragged batches: a batch from lpg_batch_create_ragged holds LPs of
 * different shapes, LP q being (m_q + nobj) x ncols_q (nobj 1, or 2 for a
 * Big-M batch; one kind per batch). Every solve call runs on it as on a batch
 * of one shape -- one workgroup per LP, the same kernels, every LP bit for bit
 * what it computes alone -- with the geometry, the tier (lpg_batch_shape) and
 * the LDS layout decided per LP. A round of a solve call is one launch per
 * tier in use: the global-tier LPs (group 0), then the LDS-tier LPs (group
 * 1) with the dynamic LDS of the largest of them, in each the LPs with the
 * most update work first. `chunk` and the log capacity,
 * 2 * (max m + max ncols) by default, hold for the whole batch. Tableaus,
 * bases and costs move in the packed layout: LP after LP, each dense with no
 * padding (lpg_batch_load_packed and the other _packed / _ragged calls); the
 * calls that take one shape or one pitch (lpg_batch_load, _get_rows,
 * _get_basis, _set_objective, _set_active_columns, the generators, the scalar
 * _solve_two_phase and _solve_big_m) return LPG_ERR_STATE on a ragged batch
 * and name the call to use, and the packed calls refuse a batch of one shape
 * in the same way; nothing is moved and nothing pivots.
 *
 * LPG_FLAG_NO_LOG is the only flag.
 * Every argument is validated on the host before any launch. One batch per
 * host thread; not reentrant. */
#define LPG_BATCH_TIER_LDS    0
#define LPG_BATCH_TIER_GLOBAL 1
#define LPG_BATCH_MAX_DIM     8192   /* m + 1 (Big-M: m + 2, goal: m + K) and ncols of a batch */

typedef struct lpg_batch lpg_batch;

typedef struct {
    int64_t count, m, ncols, ld;  /* LPs, constraint rows, N+1 columns, device row pitch (doubles) */
    int32_t tier;                 /* LPG_BATCH_TIER_* */
    int32_t chunk;                /* pivots per LP and launch */
    int64_t lds_bytes;            /* dynamic LDS of one workgroup */
    int64_t log_capacity;         /* pivots recorded per LP (0 with LPG_FLAG_NO_LOG) */
    int32_t nobj;                 /* objective rows per tableau: 1, 2 for a Big-M batch, K for a goal batch */
    /* ragged: 1 for a batch from lpg_batch_create_ragged (m, ncols, ld and
     * lds_bytes above are then the largest of any LP, tier is
     * LPG_BATCH_TIER_GLOBAL if any LP is on it), else 0 */
    int32_t pad;
} lpg_batch_info_t;

/* One LP of a ragged batch (lpg_batch_shape) */
typedef struct {
    int64_t m, ncols, ld;         /* constraint rows, N+1 columns, device row pitch (doubles) */
    int32_t tier;                 /* LPG_BATCH_TIER_* of this LP */
    int32_t group;                /* its launch group: 0 on the global tier, 1 on the LDS tier */
    int64_t lds_bytes;            /* dynamic LDS its workgroup uses */
    int64_t tableau_offset;       /* of its (m + nobj) x ncols tableau in the packed tableaus of the whole batch (doubles) */
    int64_t basis_offset;         /* of its m entries in the packed bases */
    int64_t cost_offset;          /* of its ncols - 1 entries in the packed costs */
} lpg_batch_shape_t;

/* count >= 1 LPs of m constraint rows and ncols = N+1 columns; flags: 0 or
 * LPG_FLAG_NO_LOG (anything else: LPG_ERR_ARG). All tableaus start as zeros
 * with status LPG_RUNNING; load or generate them next. */
int  lpg_batch_create(lpg_batch **out, int device, int64_t count, int64_t m, int64_t ncols, uint32_t flags);
/* The same for a Big-M batch: every tableau is (m+2) x ncols, row m the M
 * part and row m + 1 the real part of the objective; m + 2 <= LPG_BATCH_MAX_DIM.
 * Arguments, flags and refusals as lpg_batch_create. lpg_batch_load and
 * lpg_batch_get_rows then move m + 2 rows per LP, and
 * lpg_batch_generate_artificial puts the objective into row m + 1 (the M row
 * is zero). */
int  lpg_batch_create_big_m(lpg_batch **out, int device, int64_t count, int64_t m, int64_t ncols, uint32_t flags);
/* A ragged batch: LP q has m[q] constraint rows and ncols[q] columns; nobj =
 * 1 (a plain batch) or 2 (a Big-M batch) for all of them. LPG_ERR_ARG, with
 * a message that names the first offending LP, before any device work: NULL
 * arrays, count < 1, an LP with m < 1, ncols < 2 or m + nobj or ncols over
 * LPG_BATCH_MAX_DIM, flags other than LPG_FLAG_NO_LOG, another nobj, more
 * than 2^31 - 1 rows in all. */
int  lpg_batch_create_ragged(lpg_batch **out, int device, int64_t count, const int64_t *m, const int64_t *ncols,
                             int nobj, uint32_t flags);
/* LP lp of a ragged batch (a batch of one shape: LPG_ERR_STATE, see lpg_batch_info) */
int  lpg_batch_shape(const lpg_batch *b, int64_t lp, lpg_batch_shape_t *out);
/* lpg_batch_load / _get_rows / _get_basis / _set_objective for a ragged
 * batch, in the packed layout: LP q's tableau is (m_q + nobj) x ncols_q,
 * row-major without padding, the LPs one after another from `first`; bases
 * m_q entries each (validated: 1..N_q; NULL keeps them); costs ncols_q - 1
 * entries each, for the whole batch. */
int  lpg_batch_load_packed(lpg_batch *b, int64_t first, int64_t n, const double *tableaus, const int64_t *basis);
int  lpg_batch_get_rows_packed(lpg_batch *b, int64_t first, int64_t n, double *out);
int  lpg_batch_get_basis_packed(lpg_batch *b, int64_t first, int64_t n, int64_t *basis);
int  lpg_batch_set_objective_packed(lpg_batch *b, const double *cost);
/* lpg_batch_solve_two_phase / lpg_batch_solve_big_m on a ragged batch:
 * art_first[q] in 2..N_q for LP q, cost packed or NULL (as the scalar calls').
 * After the two-phase call LP q's active columns are 1..art_first[q]-1. */
int  lpg_batch_solve_two_phase_ragged(lpg_batch *b, const int64_t *art_first, const double *cost,
                                      int64_t max_pivots, int rule, lpg_result *out);
int  lpg_batch_solve_big_m_ragged(lpg_batch *b, const int64_t *art_first, const double *cost,
                                  int64_t max_pivots, int rule, lpg_result *out);
void lpg_batch_destroy(lpg_batch *b);                        /* NULL is a no-op */
const char *lpg_batch_last_error(const lpg_batch *b);        /* NULL: this thread's last create error */
int  lpg_batch_info(const lpg_batch *b, lpg_batch_info_t *out);
/* LPs [first, first + n): tableaus = n x (m+1) rows (Big-M batch: m+2)
 * [b | a_1..a_N] of pitch ld >= ncols, objective row(s) last; basis = n x m 1-based basic columns
 * (validated: 1..N), or NULL to keep the current ones. The LPs loaded start
 * again: status LPG_RUNNING, no pivots, empty log. */
int  lpg_batch_load(lpg_batch *b, int64_t first, int64_t n, const double *tableaus, int64_t ld,
                    const int64_t *basis);
/* LP i = lpg_generate(n_struct, seed + i, kind) for every LP of the batch
 * (ncols == n_struct + m + 1); kind: LPG_GEN_DENSE, LPG_GEN_DEGENERATE or
 * LPG_GEN_DUAL (LPG_GEN_ARTIFICIAL: lpg_batch_generate_artificial). */
int  lpg_batch_generate(lpg_batch *b, int64_t n_struct, uint64_t seed, int kind);
int  lpg_batch_set_tolerances(lpg_batch *b, double eps_piv, double eps_opt);
int  lpg_batch_set_active_columns(lpg_batch *b, int64_t nact);   /* price columns 1..nact of every LP */
/* Log capacity per LP (default 2 * (m + ncols)), before the first pivot
 * (LPG_ERR_STATE afterwards). Pivots beyond it are applied and counted but
 * not recorded. */
int  lpg_batch_reserve_log(lpg_batch *b, int64_t npivots);
/* Up to max_pivots MORE pivots per LP, as lpg_solve; out[count] (may be
 * NULL). A finished LP keeps its status in later calls; an LP whose budget
 * runs out on its last pivot still reports LPG_OPTIMAL. */
int  lpg_batch_solve(lpg_batch *b, int64_t max_pivots, int rule, lpg_result *out);
/* The dual simplex with lpg_solve_dual's rules. Every LP must be dual
 * feasible: else LPG_ERR_STATE, the message names the first offending LP
 * and nothing has pivoted. */
int  lpg_batch_solve_dual(lpg_batch *b, int64_t max_pivots, lpg_result *out);
/* lpg_solve_two_phase on every LP, whatever its earlier status: artificial
 * columns art_first..N (one art_first in 2..N for the whole batch); cost =
 * count x N real costs of pitch ld_cost >= N, LP by LP, or NULL: -1 x each
 * LP's objective row as it stands at the call. Phase I may apply max_pivots
 * pivots, phase II max(0, max_pivots - the LP's pivots so far); drive-out
 * pivots are counted and logged but not charged. A second call starts phase
 * I again from the current basis. Per LP: LPG_INFEASIBLE (or the phase-I
 * LPG_ITER_LIMIT / LPG_NUMERIC) with the phase-I tableau, else the phase-II
 * result. Afterwards the batch's active columns are 1..art_first-1 (as after
 * lpg_batch_set_active_columns(b, art_first - 1)). Bad art_first, rule,
 * ld_cost or max_pivots < 0: LPG_ERR_ARG, the message names the argument and
 * nothing has pivoted. */
int  lpg_batch_solve_two_phase(lpg_batch *b, int64_t art_first, const double *cost, int64_t ld_cost,
                               int64_t max_pivots, int rule, lpg_result *out);
/* lpg_solve_big_m on every LP of a Big-M batch, whatever its earlier status:
 * artificial columns art_first..N; cost as lpg_batch_solve_two_phase's, or
 * NULL: -1 x each LP's row m + 1 as it stands at the call; the entries from
 * art_first on are taken as 0 in the real row and -1 in the M row. Both
 * objective rows are recomputed from the current basis, then up to max_pivots
 * MORE pivots per LP are applied, all columns 1..N priced lexicographically
 * (M part first). An LP that ends LPG_OPTIMAL or LPG_UNBOUNDED with the M
 * part of its objective still negative (T[m][0] < -1e-9 max(1, sum |b_i|)) is
 * LPG_INFEASIBLE. out[].objective is T[m+1][0]. A budget-limited solve goes
 * on with another call. Argument errors as lpg_batch_solve_two_phase's; a
 * batch from lpg_batch_create: LPG_ERR_STATE. */
int  lpg_batch_solve_big_m(lpg_batch *b, int64_t art_first, const double *cost, int64_t ld_cost,
                           int64_t max_pivots, int rule, lpg_result *out);

/* ---- goal programmes: K priority rows priced on the device ----
 * Preemptive goal programming: hard constraints, goal rows with deviation
 * variables d- / d+, and K priority levels P1 >> P2 >> ... >> PK, solved by the
 * simplex with K rows of check numbers instead of one. A Big-M batch is the
 * case K = 2 (the M part is level 0) and a plain batch the case K = 1; a goal
 * batch is nevertheless a kind of its own.
 *
 * Layout. A goal batch holds `count` tableaus of (m + K) x ncols,
 * 1 <= K <= LPG_GOAL_MAX_LEVELS, in max form like every other batch: rows
 * 0..m-1 the constraints (column 0 the right-hand side) with a basis, row
 * m + k the objective row of priority level k, level 0 the highest.
 *
 * Costs. The caller gives K rows of N = ncols - 1 costs per LP; a minimised
 * weighted deviation is a negative cost on d- / d+ at its level.
 *
 * One call of lpg_batch_solve_goal, per LP, whatever its earlier status:
 *  1. for k = 0..K-1 row m + k becomes lpo_set_objective(cost_k) from the
 *     current basis: acc = fma(cost_k[basis[i]-1], T[i][j], acc) over
 *     i = 0..m-1 in order, then acc - cost_k[j-1] for j >= 1;
 *  2. the pivot loop is lpg_solve's over columns 1..N, with the pricing class
 *     of column j found by scanning k = 0, 1, ...: d_k[j] < -eps_opt: the class
 *     is k and the value d_k[j]; else d_k[j] <= eps_opt: go on to the next
 *     level; else (positive, or NaN) the column is not eligible. A column with
 *     no class is not eligible;
 *  3. the entering column: LPG_RULE_DANTZIG the least class, then the least
 *     value, then the smallest column; LPG_RULE_BLAND the first eligible column.
 * The ratio test, the LPG_NUMERIC rule, the update (all K objective rows take
 * part in it), the log and the order of the checks (price: LPG_OPTIMAL; budget
 * spent: LPG_ITER_LIMIT; ratio: LPG_UNBOUNDED; LPG_NUMERIC; apply) are
 * lpg_batch_solve_big_m's, and every call starts from fresh objective rows and
 * a fresh budget of max_pivots. There is no LPG_INFEASIBLE at this layer: a
 * caller that puts artificials at level 0 reads attain[q][0].
 *
 * Results: lpg_result as elsewhere with objective = T[m + K - 1][0], and
 * attain[q * K + k] = T[m + k][0] of LP q.
 *
 * lpg_batch_load, _get_rows, _get_basis, _get_log, _info (nobj = K),
 * _set_tolerances, _reserve_log and _destroy serve a goal batch as they serve a
 * Big-M batch's m + 2 rows. Every other lpg_batch_* call refuses it
 * (LPG_ERR_STATE, the message names lpg_batch_solve_goal), and
 * lpg_batch_solve_goal refuses plain and Big-M batches. The tier is decided by
 * the LDS footprint of m + K rows; there are no ragged goal batches. */
#define LPG_GOAL_MAX_LEVELS   8
/* count >= 1 goal programmes of m constraint rows, ncols = N+1 columns and
 * nlevels priority levels. LPG_ERR_ARG before any device work: nlevels outside
 * 1..LPG_GOAL_MAX_LEVELS, a bad shape, m + nlevels or ncols over
 * LPG_BATCH_MAX_DIM, count * (m + nlevels) over 2^31 - 1, flags other than
 * LPG_FLAG_NO_LOG. */
int  lpg_batch_create_goal(lpg_batch **out, int device, int64_t count, int64_t m, int64_t ncols, int nlevels,
                           uint32_t flags);
/* The call described above. Level k's cost of column j of LP q is
 * cost[q * ld_lp + k * ld_level + (j - 1)], ld_level >= N and
 * ld_lp >= nlevels * ld_level; the padding is never read. res[count] and
 * attain[count x nlevels] may be NULL. NULL cost, a bad rule, ld_level, ld_lp
 * or max_pivots < 0: LPG_ERR_ARG, the message names the argument and nothing
 * has pivoted; a batch that is not a goal batch: LPG_ERR_STATE. */
int  lpg_batch_solve_goal(lpg_batch *b, const double *cost, int64_t ld_lp, int64_t ld_level, int64_t max_pivots,
                          int rule, lpg_result *res, double *attain /* count x nlevels, or NULL */);

/* lpg_set_objective on every LP: cost = count x N of pitch ld_cost >= N; the
 * objective row of LP i becomes d_j = sum_r c_B(r) T[r][j] - c_j from its
 * current basis, and the LP's status LPG_RUNNING. */
int  lpg_batch_set_objective(lpg_batch *b, const double *cost, int64_t ld_cost);
/* LP i = lpg_generate(n_struct, seed + i, LPG_GEN_ARTIFICIAL);
 * *art_first (may be NULL) = 1 + n_struct + ceil(m / 2). */
int  lpg_batch_generate_artificial(lpg_batch *b, int64_t n_struct, uint64_t seed, int64_t *art_first);
/* n x (m+1) rows (Big-M batch: m+2) of pitch ld >= ncols / n x m basis entries of LPs [first, first + n) */
int  lpg_batch_get_rows(lpg_batch *b, int64_t first, int64_t n, double *out, int64_t ld);
int  lpg_batch_get_basis(lpg_batch *b, int64_t first, int64_t n, int64_t *basis);
/* LP lp's log: copies min(recorded, max) pivots, returns the number recorded
 * (= min(pivots, log capacity)), < 0 on error. */
int64_t lpg_batch_get_log(lpg_batch *b, int64_t lp, int64_t *k, int64_t *r, int64_t max);
/* LP lp's active columns 1..*nact (what lpg_batch_solve and _solve_dual price)
 * and, for a ragged batch, the art_first recorded by its last two-phase or
 * Big-M call (a batch of one shape: ncols); either pointer may be NULL. */
int  lpg_batch_active_columns(const lpg_batch *b, int64_t lp, int64_t *nact, int64_t *art_first);

/* ---- branching: the step between two levels of a branch-and-bound tree ----
 *
 * The node LPs of a tree are the LPs of a batch. lpg_batch_branch_select picks
 * the branching variable of every LP (lpg_batch.hip k_batch_branch_select, one
 * workgroup per LP over its basis), lpg_batch_branch makes the batch of the
 * children on the device (k_batch_branch, one workgroup per child): a child is
 * its parent's tableau in the parent's current basis plus one bound row, so it
 * is dual feasible wherever the parent was LPG_OPTIMAL and
 * lpg_batch_solve_dual(child) re-optimises it. No tableau crosses the host.
 * Both calls work on batches of one shape and on ragged ones and refuse a
 * Big-M batch (LPG_ERR_STATE). Only floor, ceil, one subtraction, one
 * negation and comparisons are used, so a host restatement reproduces both
 * bit for bit (tests/branch_cases.py). */
#define LPG_BRANCH_MOST_FRACTIONAL 0   /* largest distance to an integer; ties -> smallest column */
#define LPG_BRANCH_FIRST           1   /* smallest fractional integer column */
typedef struct { int64_t row, col; double value; } lpg_branch_t;   /* row = col = -1: every integer column integral */
/* out[q] for every LP q: column j (1-based) is integer-constrained in LP q iff
 * j <= nmask && mask[q * ld_mask + j - 1] (ld_mask == 0: one mask of nmask
 * bytes for every LP; else ld_mask >= nmask). Of the rows i whose basic
 * column is integer-constrained, with v = T[i][0], f = v - floor(v) and
 * dist = min(f, 1 - f), those with dist > int_tol are candidates; `rule`
 * picks one, out[q] = (its row, its basic column, v). LPG_ERR_ARG before any
 * device work: NULL arguments, nmask outside 1..ncols-1 (ragged: the largest
 * ncols), 0 < ld_mask < nmask, int_tol not in [0, 0.5), another rule. */
int  lpg_batch_branch_select(lpg_batch *b, const uint8_t *mask, int64_t nmask, int64_t ld_mask,
                             double int_tol, int rule, lpg_branch_t *out /* count */);
/* *child = a new batch of n LPs: child c is LP src[c] of `parent` with one
 * more row and one more column, the bound x <= floor(v) (dir[c] = -1) or
 * x >= ceil(v) (dir[c] = +1) on the variable x basic in row[c], v = T[row][0].
 * With nact the source's active columns: columns 0..nact are copied, the new
 * slack column is nact + 1 (zero in every other row, the objective row
 * included, 1 in the new row), the source's columns beyond nact (the inert
 * artificials of a two-phase solve) move right by one and basis entries
 * beyond nact grow by one. Constraint rows 0..m-1 are copied, the new row is
 * row m with basis[m] = nact + 1, the objective row becomes row m + 1. The
 * new row is -T[row][j] with right-hand side floor(v) - v (dir -1) or
 * +T[row][j] with v - ceil(v) (dir +1), the entry in x's own column exactly
 * 0. The child's active columns are 1..nact+1 (a ragged child's recorded
 * art_first grows by one as well); it inherits the parent's tolerances and
 * flags; its LPs are fresh: LPG_RUNNING, no pivots, empty log. A parent of
 * one shape gives a child of one shape (m + 1, ncols + 1), a ragged parent a
 * ragged child. The parent is unchanged. Before any device work, with a
 * message that names the first offending index: n < 1, NULL arrays, a src
 * outside the parent, a row outside 0..m_src-1, a dir other than -1 / +1, a
 * child dimension over LPG_BATCH_MAX_DIM (LPG_ERR_ARG); a Big-M parent
 * (LPG_ERR_STATE). On any error *child is NULL. */
int  lpg_batch_branch(lpg_batch **child, lpg_batch *parent, int64_t n, const int64_t *src, const int64_t *row,
                      const int8_t *dir);

/* ---- cuts: a round of Gomory mixed-integer cuts on the LPs of a batch ----
 *
 * The other way from a fractional optimum towards an integer one: instead of
 * two children with one bound row each, one child with k cut rows, each of
 * which the fractional vertex violates and no integer point does. The shape of
 * the work is lpg_batch_branch's: the child is the parent's tableau in its
 * current basis plus rows with basic slacks and negative right-hand sides, dual
 * feasible wherever the parent was LPG_OPTIMAL, so lpg_batch_solve_dual(child)
 * re-optimises it, and no tableau crosses the host. Both calls work on batches
 * of one shape and on ragged ones and refuse a Big-M batch (LPG_ERR_STATE).
 *
 * The cut (Gomory mixed-integer, GMI) of LP s from row r, whose basic column is
 * integer-constrained; 1..nact the active columns, B the basis, v = T[r][0]:
 *     frac(x) = x - floor(x), and 0.0 where that difference is >= 1.0 (a tiny
 *               negative x rounds to exactly 1.0 otherwise)
 *     f0  = frac(v)
 *     rho = f0 / (1.0 - f0)                         one IEEE division per cut
 * and for column j in 1..nact with a = T[r][j]
 *     j basic in any row of the LP (by membership in B, not by value):
 *                                  g = 0.0
 *     j integer-constrained:       f = frac(a), g = f <= f0 ? f : rho * (1.0 - f)
 *     otherwise (continuous):      g = a >= 0.0 ? a : rho * (-a)
 * and g = 0.0 for the columns behind nact (the inert artificials of a two-phase
 * parent). The new row holds -g_j in column j, -f0 in column 0, 1.0 in its own
 * new slack column and 0.0 in the other new slack columns. It is valid for any
 * real coefficients given only the mask: slacks, branch slacks and the slacks
 * of earlier cuts count as continuous. Only floor, subtraction, one division,
 * multiplication, negation and comparisons are used, each a single rounding
 * (nothing is contracted into an fma, the division is the IEEE one), so a host
 * restatement reproduces every bit (tests/cut_cases.py). */
#define LPG_BATCH_MAX_CUTS 1024   /* cuts per child: their (f0, rho) records and the basic-column byte map share the LDS */
/* The cut rows of every LP q (k_batch_cut_select, one workgroup per LP): the
 * candidates are lpg_batch_branch_select's (basic column masked, min(f, 1 - f)
 * > int_tol, the mask addressed as there); ncut[q] = min(max_cuts, candidates)
 * and rows[q * max_cuts ..] lists that many in LPG_BRANCH_MOST_FRACTIONAL
 * order, largest distance first, ties to the smallest column; unused slots are
 * -1. LPG_ERR_ARG before any device work: NULL arguments, max_cuts outside
 * 1..LPG_BATCH_MAX_CUTS, int_tol not in [0, 0.5) (these three before the batch
 * is looked at), nmask outside 1..ncols-1, 0 < ld_mask < nmask. */
int  lpg_batch_cut_select(lpg_batch *b, const uint8_t *mask, int64_t nmask, int64_t ld_mask,
                          double int_tol, int64_t max_cuts,
                          int64_t *ncut /* count */, int64_t *rows /* count * max_cuts */);
/* *child = a new batch of n LPs: child c is LP src[c] of `parent` plus one cut
 * per row in rows[first[c] .. first[c+1]) (first has n + 1 entries, first[0] =
 * 0), k_c = first[c+1] - first[c] of them: 1 <= k_c <= LPG_BATCH_MAX_CUTS, the
 * rows distinct and inside 0..m_src-1. The mask is the parent's, LP src[c] at
 * mask + src[c] * ld_mask (ld_mask == 0: one mask for every LP). The layout
 * follows lpg_batch_branch: columns 0..nact keep their place, the new slacks
 * are columns nact+1 .. nact+k, what lay behind nact moves right by k, as do
 * basis entries > nact; the new rows are m .. m+k-1 in the order of `rows`,
 * the basis of new row t is nact+1+t, the objective row becomes row m+k. The
 * child's active columns are 1..nact+k (a ragged parent's recorded art_first
 * grows by k as well); it inherits tolerances and flags; its LPs are fresh. The
 * child is ragged if the parent is ragged or the k_c differ, else of one shape
 * (m + k, ncols + k). The parent is unchanged. Every argument is checked before
 * any device work, with a message that names the call and the first offending
 * index; first the checks that need no parent: n < 1, NULL arrays, first[0] !=
 * 0, a first[c+1] <= first[c]; then a src outside the parent, a k_c over the
 * cap, a row out of range or listed twice, a child dimension over
 * LPG_BATCH_MAX_DIM, the mask's nmask / ld_mask as above (all LPG_ERR_ARG); a
 * Big-M parent (LPG_ERR_STATE). On any error *child is NULL. */
int  lpg_batch_cut(lpg_batch **child, lpg_batch *parent, int64_t n, const int64_t *src,
                   const int64_t *first /* n + 1 offsets into rows */, const int64_t *rows,
                   const uint8_t *mask, int64_t nmask, int64_t ld_mask);

/* ---- scenarios: the same LPs under other right-hand sides ----
 *
 * For parameter sweeps and scenario sets: LPs that differ only in b. A solved
 * tableau carries B^-1 in the columns that were the identity when the LP was
 * stated, so for a new right-hand side b' column 0 is B^-1 b'; the objective
 * row's entries d_j do not change, the LP stays dual feasible, and
 * lpg_batch_solve_dual re-optimises it in a few pivots where a cold solve
 * would start from the slack or artificial basis again. No tableau crosses
 * the host. Both calls work on batches of one shape and on ragged ones and
 * refuse a Big-M batch (LPG_ERR_STATE).
 *
 * `ident` states the frame the right-hand sides are given in: ident[i] of LP
 * q is the column (1..N_q) that was the unit vector e_i in that frame; for a
 * loaded LP the basis it was loaded with, for the generators the slack or
 * artificial column of row i. It is laid out like the bases: m entries per LP,
 * count x m for a batch of one shape, packed as lpg_batch_get_basis_packed's
 * for a ragged one. For every row r = 0..m of the LP, the objective row
 * included:
 *     acc = 0.0; for i = 0..m-1: acc = acc + T[r][ident[i]] * rhs[i]
 *     T[r][0] = acc
 * i ascending, the product and the sum one rounding each (nothing contracted
 * into an fma), so a host restatement reproduces every bit
 * (tests/scenario_cases.py). The objective row's column 0 is the objective of
 * the new basic solution only where the ident columns cost 0: slacks do, and
 * so do artificials in phase II; otherwise follow with lpg_batch_set_objective.
 * Nothing checks that an LP was LPG_OPTIMAL: lpg_batch_solve_dual refuses an
 * LP that is not dual feasible. A lane per row gathers the row's entries;
 * LPG_SCENARIO_WALK=tile reads them tile by tile through LDS instead, which
 * was measured and is slower at the shapes tried; the bits are the same. */
/* *child = a new batch of n LPs: child c is LP src[c] of `parent` unchanged
 * (shape, basis, active columns, a ragged parent's art_first, the inert
 * artificial columns behind nact, which are the B^-1 of their rows) except for
 * column 0, restated for rhs: packed, child c's m_src[c] values behind child
 * c-1's; ident is the parent's. The child inherits tolerances and flags; its
 * LPs are fresh: LPG_RUNNING, no pivots, empty log. A parent of one shape gives
 * a child of one shape, a ragged parent a ragged child. The parent is
 * unchanged. One launch (k_batch_scenario, one workgroup per child) copies
 * the parent and computes the column. Before any device work, with a message
 * that names the call and the first offending index: `child` NULL, n < 1, NULL
 * src / ident / rhs, NULL parent (LPG_ERR_ARG, in this order, none of them
 * looks at the parent); then a Big-M parent (LPG_ERR_STATE), a src outside the
 * parent, an ident entry outside 1..N_q, a rhs entry that is not finite
 * (LPG_ERR_ARG). On any error *child is NULL. */
int  lpg_batch_scenario(lpg_batch **child, lpg_batch *parent, int64_t n, const int64_t *src,
                        const int64_t *ident, const double *rhs);
/* The same column on every LP of `b`, in place (k_batch_set_rhs): ident is
 * the batch's own, rhs holds LP q's m_q values, LP after LP. Column 0 is only
 * written and the other columns only read. The LPs start again as after
 * lpg_batch_load; B^-1 survives any number of dual pivots, so a sweep in steps
 * needs no new batch. Refusals as lpg_batch_scenario's. */
int  lpg_batch_set_rhs(lpg_batch *b, const int64_t *ident, const double *rhs);

/* ---- ranging: shadow prices, and how far costs and right-hand sides can move ----
 *
 * The sensitivity report of every solved LP of a batch, computed on the device
 * (lpg_batch.hip k_batch_ranging, one workgroup per LP) from the tableau the
 * solve left there: no tableau crosses the host. It works on batches of one
 * shape and on ragged ones, refuses a Big-M batch (LPG_ERR_STATE) and changes
 * nothing: statuses, pivots, logs, bases and tableaus stay as they were.
 *
 * Notation for LP q: T its tableau as lpg_batch_get_rows returns it, B its
 * basis, 1..nact its active columns, N = ncols - 1, m its constraint rows,
 * eps the batch's eps_piv, ident[i] in 1..N_q as in "scenarios" above (same
 * meaning, same layout, same validation). "None" is 0 for a column index
 * (columns are 1-based) and -1 for a row index.
 *
 * An LP whose status is not LPG_OPTIMAL is not ranged: every double of its
 * outputs is NaN, every index none. For an LPG_OPTIMAL LP:
 *
 * Dual values. dual[i] = T[m][ident[i]], i = 0..m-1, the bits as they stand.
 * This is the shadow price of row i where column ident[i] costs 0 (slacks, and
 * artificials in phase II); otherwise the caller adds that column's cost.
 *
 * One ratio. Every bound is q = (-x) / a over candidates (x, a, index): the
 * negation exact, the division the one IEEE division, nothing contracted. An
 * entry is a candidate for the lower bound iff a > eps, for the upper bound
 * iff a < -eps (both strict), and never one whose q is NaN. The lower bound is
 * the largest candidate q, the upper bound the smallest; among candidates that
 * compare equal (-0 and +0 do) the one with the smallest index wins, and its
 * bits and its index are reported. With no candidate the bound is -inf or +inf
 * and the index none. The order is total, so the result does not depend on how
 * the candidates are grouped.
 *
 * Cost ranging. For column j = 1..N, at index j - 1 (the layout of the costs):
 * the interval [cost_lo, cost_hi] of changes to the max-form cost c_j for
 * which the basis stays optimal, and the column that limits each end.
 *     j > nact:     (-inf, +inf), both indices none
 *     j nonbasic (not in B, by membership, not by value):
 *                   lo = -inf, index none; hi = T[m][j], hi_at = j
 *     j basic in row r: the candidates are the columns k in 1..nact not in B,
 *                   x = T[m][k], a = T[r][k], index k
 * A row whose basic column lies behind nact (a kept artificial) ranges
 * nothing. A basis that lists a column twice is the caller's error: the entry
 * is that of one of the rows. The column that limits an end is the one that
 * enters there.
 *
 * Right-hand-side ranging. For frame row i = 0..m-1, at index i (the layout of
 * the bases): the interval [rhs_lo, rhs_hi] of changes to b_i for which the
 * basis stays feasible. With h = ident[i] the candidates are the constraint
 * rows r = 0..m-1, x = T[r][0], a = T[r][h], index r; the variable basic in
 * the limiting row is the one that leaves there.
 *
 * Nothing is clamped: a d_k in [-eps_opt, 0) gives a bound on the wrong side
 * of zero, as the numbers say. tests/ranging_cases.py restates all of this in
 * numpy, operation for operation, and the device is held to it bit for bit. */
typedef struct {
    double  *dual;                                   /* m per LP, laid out as the bases */
    double  *cost_lo, *cost_hi;                      /* ncols - 1 per LP, laid out as the costs */
    int64_t *cost_lo_at, *cost_hi_at;
    double  *rhs_lo, *rhs_hi;                        /* m per LP */
    int64_t *rhs_lo_at, *rhs_hi_at;
} lpg_ranging_t;
/* The three groups (dual; the four cost_* arrays; the four rhs_* arrays) are
 * each wanted or not as a whole: NULL pointers leave a group out, and it is
 * then not computed. The layouts are count x m and count x (ncols - 1), dense,
 * for a batch of one shape, and packed as lpg_batch_get_basis_packed's and
 * lpg_batch_set_objective_packed's for a ragged one. Before any device work,
 * with a message that names the call and the argument: `out` NULL, `ident`
 * NULL, `b` NULL, a group given in part or no group at all (LPG_ERR_ARG, in
 * this order, the first three without looking at the batch); then a Big-M
 * batch (LPG_ERR_STATE); then an ident entry outside 1..N_q, naming the LP and
 * the row (LPG_ERR_ARG). */
int  lpg_batch_ranging(lpg_batch *b, const int64_t *ident, const lpg_ranging_t *out);

/* ---- assignment: batches of n x n (and nr x nc) assignment problems ----
 *
 * The reference's README lists the assignment problem by the Hungarian method
 * among the things it meant to solve. Stated as an LP it has nr + nc equality
 * rows and nr * nc columns, an O(n^3) tableau for an O(n^2) problem at a vertex
 * as degenerate as they come. An lpg_assign holds `count` cost matrices of one
 * shape instead, nr rows by nc columns with 1 <= nr <= nc <= LPG_BATCH_MAX_DIM,
 * row-major fp64, and solves them in one launch by the primal-dual (shortest
 * augmenting path) Hungarian method (lpg_assign.hip): every row is assigned to
 * a distinct column and the sum of the chosen costs is minimal, or maximal with
 * LPG_ASSIGN_MAXIMIZE. Only subtraction, addition and comparison are used, so a
 * host restatement reproduces every bit (tests/assign_cases.py). Ragged
 * assignment batches are not provided.
 *
 * Costs. An entry of +inf forbids the pair. A maximisation negates the finite
 * costs as they are loaded, which is exact (+inf still forbids), and negates u
 * and v back on the way out. NaN, -inf and finite entries above
 * LPG_ASSIGN_COST_CAP = 2^1000 in magnitude are refused by lpg_assign_load
 * (LPG_ERR_ARG, the message names the problem and the entry) before any device
 * work. The cap keeps every potential finite: in exact arithmetic -v[j] is the
 * length of an alternating path of at most 2 nr <= 2^14 edges, each a cost of
 * magnitude <= cap, so |v[j]| <= 2^14 cap and |u[i]| <= cap + max |v| < 2^1015;
 * a problem makes fewer than 2^41 roundings, each off by at most 2^-53 of a
 * magnitude below 2^1016, which moves those bounds by less than a factor of
 * two, and 2^1017 is far below the overflow threshold 2^1024. With finite u
 * and v no reduced cost is NaN (+inf minus a finite number is +inf) and delta
 * is always finite.
 *
 * The algorithm, operation for operation. C is the matrix as loaded (negated
 * for a maximisation). "None" is -1. u[nr] and v[nc] start at 0.0, rowof[nc]
 * at none, steps at 0. For row i = 0 .. nr-1:
 *   1. minv[j] = +inf, way[j] = none, used[j] = false for every j; i0 = i,
 *      j0 = none.
 *   2. Step (steps = steps + 1):
 *        if j0 is a column, used[j0] = true;
 *        for every unused j: cur = (C[i0][j] - u[i0]) - v[j], two roundings in
 *          this order; if cur < minv[j] (strict): minv[j] = cur, way[j] = j0;
 *        j1 = the unused column with the smallest minv under `<` (-0 and +0
 *          compare equal), ties to the smallest j; delta = minv[j1], the bits
 *          as they stand;
 *        no unused column with minv < +inf: the problem is LPG_INFEASIBLE and
 *          ends here, u and v as they stand.
 *   3. Update, one rounding each:
 *        u[i] = u[i] + delta;
 *        for every used j: u[rowof[j]] = u[rowof[j]] + delta, v[j] = v[j] - delta;
 *        for every unused j: minv[j] = minv[j] - delta;
 *        j0 = j1; if rowof[j0] is a row: i0 = rowof[j0], go to 2.
 *   4. Augment: while j0 is a column: rowof[j0] = (way[j0] is a column ?
 *      rowof[way[j0]] : i), then j0 = way[j0].
 * Row i's search marks a new column used in every step and ends at the first
 * free one, so it makes at most i + 1 steps and steps <= nr (nr + 1) / 2,
 * whatever the arithmetic does: a launch is bounded without relaunches.
 *
 * Per problem: status (LPG_OPTIMAL or LPG_INFEASIBLE); col[nr], the 0-based
 * column of every row, -1 throughout for an infeasible problem; u[nr] and
 * v[nc] in the caller's sense (for a maximisation the negation of each, so 0.0
 * comes back as -0.0); objective = 0.0, then for i ascending objective +
 * (the caller's C[i][col[i]]), one rounding per addition, NaN if infeasible;
 * steps. On integer costs the certificate holds exactly: u[i] + v[j] <=
 * C[i][j] with equality on assigned pairs, v <= 0, and v[j] == 0 on unassigned
 * columns (a minimisation; mirrored for a maximisation).
 *
 * Two points decide the bits. The reduced costs are non-negative in exact
 * arithmetic only: in fp64 a minv can be slightly negative or -0, so the
 * argmin does not use block_argmin_cand's packed key ("the bits of theta >=
 * 0"); it maps the bits to a total order with -0 and +0 made equal FOR THE KEY
 * ONLY, and delta is the winner's own bits, because -0 + -0 and -0 + +0 differ.
 * And every compare-and-keep is a branch-free per-field select (lpg_device.h
 * tells why).
 *
 * Forms. nc <= 64: one wave per problem, four problems per workgroup, a column
 * per lane, column state in registers, C and u in LDS (the wave form). Else one
 * workgroup per problem, columns strided over 256 threads, their state in
 * registers up to 256 columns and in LDS beyond (in device memory where even
 * that does not fit); C in LDS where u, C and that state fit the 150 KiB
 * dynamic LDS cap (LPG_BATCH_TIER_LDS, up to 138 x 138), else in device memory
 * with one coalesced row read per step (LPG_BATCH_TIER_GLOBAL). Env
 * LPG_ASSIGN_TIER=global forces the second tier (and with it the workgroup
 * form, the only one that has it), env LPG_ASSIGN_FORM=workgroup the workgroup
 * form at nc <= 64; both are read by lpg_assign_create. Every form computes the same bits.
 *
 * Every argument is checked on the host before any device work: the device is
 * first touched by the first lpg_assign_load, _generate or _solve that passes
 * its checks. The messages name the call and the first offending index; NULL
 * handles are errors (lpg_assign_last_error(NULL): this thread's last one).
 * One batch per host thread; not reentrant. */
#define LPG_ASSIGN_MAXIMIZE        0x1u
#define LPG_ASSIGN_FORM_WAVE       0
#define LPG_ASSIGN_FORM_WORKGROUP  1
#define LPG_ASSIGN_COST_CAP        0x1p1000

typedef struct lpg_assign lpg_assign;
typedef struct { int32_t status, pad; int64_t steps; double objective; } lpg_assign_result;
typedef struct {
    int64_t count, nr, nc;
    int32_t tier;                 /* LPG_BATCH_TIER_*: where C lives while a problem runs */
    int32_t form;                 /* LPG_ASSIGN_FORM_* */
    int64_t lds_bytes;            /* dynamic LDS of one workgroup */
    double  kernel_ms;            /* device time of the last lpg_assign_solve's kernel (events around the launch) */
} lpg_assign_info_t;

/* count >= 1 problems of nr x nc, 1 <= nr <= nc <= LPG_BATCH_MAX_DIM; flags: 0
 * or LPG_ASSIGN_MAXIMIZE. Anything else: LPG_ERR_ARG and *out = NULL. */
int  lpg_assign_create(lpg_assign **out, int device, int64_t count, int64_t nr, int64_t nc, uint32_t flags);
/* Problems [first, first + n), n >= 1: n x nr rows of nc costs at pitch ld >=
 * nc. Refused as a whole (nothing is loaded) on a bad entry, see "Costs". */
int  lpg_assign_load(lpg_assign *a, int64_t first, int64_t n, const double *costs, int64_t ld);
/* Problem q, entry (i, j) = floor(uniform01(seed + q, i * nc + j) * range),
 * the engine's generator draw (oracle lpo_uniform): exact integers in
 * 0..range-1; range in 1..2^53. */
int  lpg_assign_generate(lpg_assign *a, uint64_t seed, int64_t range);
/* Solves every problem, whatever an earlier call found; out[count] may be
 * NULL. LPG_ERR_STATE while a problem has no costs. May be called again after
 * another load. */
int  lpg_assign_solve(lpg_assign *a, lpg_assign_result *out);
/* Of problems [first, first + n) after a solve: col n x nr, u n x nr, v n x nc,
 * dense; each may be NULL, not all three. */
int  lpg_assign_get(lpg_assign *a, int64_t first, int64_t n, int64_t *col, double *u, double *v);
int  lpg_assign_info(const lpg_assign *a, lpg_assign_info_t *out);
const char *lpg_assign_last_error(const lpg_assign *a);
void lpg_assign_destroy(lpg_assign *a);                        /* NULL is a no-op */

/* ---- 0-1 programs: batches of small binary programs by implicit enumeration ----
 *
 * The reference's README lists 0-1 integer programs by implicit enumeration
 * among the things it meant to solve. An lpg_binary holds `count` problems of
 * one shape, n variables (1 <= n <= LPG_BINARY_MAX_N = 64) and m rows (1 <= m
 * <= LPG_BINARY_MAX_M = 256):
 *
 *     minimise (LPG_BINARY_MAXIMIZE: maximise)  c.x
 *     subject to  a_i.x  {<=, =, >=}  b_i   (sense[i] = -1, 0, +1),  x in {0,1}^n
 *
 * and solves each by a depth-first walk over partial assignments with interval
 * tests per row and a bound on the objective (lpg_binary.hip): no tableau, no
 * division, no multiplication. Ragged batches are not provided.
 *
 * Data and caps. Every entry of A, b and c is a finite integer-valued fp64;
 * for every row sum_j |a_ij| <= LPG_BINARY_SUM_CAP = 2^52 and |b_i| <=
 * LPG_BINARY_RHS_CAP = 2^53; sum_j |c_j| <= LPG_BINARY_SUM_CAP. lpg_binary_load
 * refuses anything else (a fraction, NaN, an infinity, a cap exceeded, a sense
 * outside {-1, 0, 1}) with LPG_ERR_ARG before any device work; the message
 * names the problem, the row and the entry, and nothing is loaded. -0.0 is
 * loaded as +0.0. A maximisation negates c as it is loaded (exact) and the
 * objective back on the way out (objective = 0.0 - inc, so a zero comes back
 * as +0.0). Why the caps make every operation exact: every quantity below (lo,
 * hi, comp, z, and every intermediate of their updates) is a sum of a subset
 * of one row's entries or of the costs, each taken with a sign, so it is an
 * integer of magnitude at most 2^52 < 2^53, and fp64 adds, subtracts and
 * compares such integers without rounding. The order in which lanes or the
 * host form a sum therefore cannot change a bit, and subtracting a term that
 * was added restores the bits that stood before.
 *
 * The algorithm, operation for operation (numpy: tests/binary_cases.py). Per
 * row the two-sided form L_i <= a_i.x <= U_i: `<=` gives L = -inf, U = b; `>=`
 * gives L = b, U = +inf; `=` gives L = U = b. c is the internal, minimising
 * cost. The preferred value of column j is p_j = (c_j < 0). A search carries:
 * the depth d (columns 0..d-1 fixed, the rest free); the fixed values x; per
 * level whether it is on its second value; per row lo_i and hi_i, the smallest
 * and largest activity any completion can reach, and comp_i, the activity of
 * the completion with every free column at its preferred value; z, the cost of
 * that completion (the lower bound of the subtree); the incumbent (inc, inc_x),
 * +inf and none at the start; the count `nodes`. At the root
 *     lo_i = sum_j min(0, a_ij), hi_i = sum_j max(0, a_ij),
 *     comp_i = sum_j p_j a_ij,   z = sum_j min(0, c_j).
 *   1. Visit: nodes += 1. Prune if z >= inc. Else prune if any row has lo_i >
 *      U_i or hi_i < L_i. Else, if every row has L_i <= comp_i <= U_i: the
 *      incumbent becomes (z, x with the free columns at p), and prune.
 *      Otherwise descend: fix column d at p_d (its first value), d += 1, visit.
 *   2. Fix column j at value v: v = 1: lo_i += max(0, a_ij), hi_i += min(0,
 *      a_ij); v = 0: lo_i += max(0, -a_ij), hi_i -= max(0, a_ij); and if v !=
 *      p_j: comp_i += (v ? a_ij : -a_ij), z += |c_j|. Unfixing subtracts the
 *      same terms (exact, so no per-level copies of the row state exist).
 *   3. Prune (backtrack): while the deepest fixed level is on its second value,
 *      unfix it; if no level is left the search has ended; otherwise unfix the
 *      deepest level, fix it at the other value, mark it second, and visit.
 * At d = n lo = hi = comp, so step 1 always ends at a leaf. A subtree is cut
 * only when it holds no strictly better leaf, so the reported x is the first
 * optimal point in the search order (preferred value first, column 0
 * outermost): a property of the problem, not of the schedule. There are no
 * fixing tests and no surrogate constraints.
 *
 * Split. lpg_binary_create takes `split` in 0..min(n, LPG_BINARY_MAX_SPLIT =
 * 10): problem q is searched as 2^split independent sub-searches; sub-search k
 * starts at depth `split` with column t < split fixed at its first value (bit
 * t of k clear) or its second (bit t set), and never unfixes those. The
 * sub-searches share no incumbent. Reduction (on the host, over the records
 * copied back): sub-searches are taken in search order, i.e. ordered by (bit
 * 0, bit 1, ..., bit split-1) of k lexicographically; the problem's inc is the
 * smallest inc, its x that of the first sub-search in that order that reaches
 * it, its nodes the sum, found = any. Objective and x are the same for every
 * split; nodes is not.
 *
 * Budgets. A launch visits at most `chunk` nodes per sub-search (default
 * LPG_BINARY_DEFAULT_CHUNK, env LPG_BINARY_CHUNK read at create); the whole
 * state of a sub-search round-trips through device memory between launches.
 * lpg_binary_solve(b, max_nodes, out) relaunches until no sub-search is
 * running, or until every running sub-search has visited max_nodes nodes in
 * this call (max_nodes <= 0: no budget). A sub-search is "running" while it
 * stands before a node it has not visited; the backtrack after a visit belongs
 * to that visit, so a search whose last visit exhausts the budget has ended.
 * Per problem: status LPG_ITER_LIMIT while a sub-search of it is running (with
 * the incumbent so far: found = 0 or 1, objective NaN if none), else
 * LPG_OPTIMAL if found, else LPG_INFEASIBLE. Another call continues where the
 * last one stopped; any number of budgeted calls ends in the same bits as one
 * unbudgeted call. A load or generate resets every search.
 *
 * Generator. lpg_binary_generate(b, seed, LPG_BINARY_GEN_BANDED): problem q
 * draws u(k) = uniform01(seed + q, k) (the engine's generator draw). With w =
 * min(3, n) and s_i = (m > 1 && n > 3) ? floor(i (n - 3) / (m - 1)) : 0, row i
 * has a[i][s_i + t] = floor(u(4 i + t) * 9) - 4 for t < w and zeros elsewhere;
 * the planted point is xp_j = (u(4 m + j) < 0.5); act_i = a_i.xp; with r =
 * u(4 i + 3): r < 0.5: sense 0, b = act; r < 0.75: sense -1, b = act + 1;
 * else sense +1, b = act - 1. c_j = floor(u(4 m + n + j) * 19) - 9 (the
 * caller's cost: a maximisation negates it like a loaded one). Every problem
 * is feasible at xp.
 *
 * Kernel. One wave per sub-search, four waves per workgroup; row i lives on
 * lane i mod 64 with 1, 2 or 4 rows per lane (m <= 64, 128, 256), lo, hi,
 * comp, L, U in registers for a launch; A transposed [n][m] so a node's
 * column read is contiguous across lanes; A^T and c in LDS where the
 * workgroup's problems fit the 150 KiB dynamic cap (LPG_BATCH_TIER_LDS;
 * sub-searches of one problem in a workgroup share one copy), else in device
 * memory (LPG_BATCH_TIER_GLOBAL; env LPG_BINARY_TIER=global forces it).
 *
 * Every argument is checked on the host before any device work: the device is
 * first touched by the first lpg_binary_load, _generate, _solve or _occupancy
 * that passes its checks. The messages name the call and the first offending
 * index; NULL handles are errors (lpg_binary_last_error(NULL): this thread's
 * last one). One batch per host thread; not reentrant. */
#define LPG_BINARY_MAXIMIZE        0x1u
#define LPG_BINARY_MAX_N           64
#define LPG_BINARY_MAX_M           256
#define LPG_BINARY_MAX_SPLIT       10
#define LPG_BINARY_SUM_CAP         0x1p52
#define LPG_BINARY_RHS_CAP         0x1p53
#define LPG_BINARY_GEN_BANDED      0
#define LPG_BINARY_DEFAULT_CHUNK   4096

typedef struct lpg_binary lpg_binary;
typedef struct { int32_t status, found; int64_t nodes; double objective; } lpg_binary_result;
typedef struct {
    int64_t count, m, n;
    int32_t split;                /* 2^split sub-searches per problem */
    int32_t rows_per_lane;        /* 1, 2 or 4: the kernel instantiation */
    int32_t tier;                 /* LPG_BATCH_TIER_*: where A^T and c live while a search runs */
    int32_t chunk;                /* nodes per sub-search per launch */
    int64_t lds_bytes;            /* dynamic LDS of one workgroup */
    int64_t launches;             /* kernel launches of the last lpg_binary_solve */
    double  kernel_ms;            /* device time of those launches, summed */
} lpg_binary_info_t;

/* count >= 1, 1 <= m <= 256, 1 <= n <= 64, 0 <= split <= min(n, 10), count *
 * 2^split <= 2^31 - 1; flags 0 or LPG_BINARY_MAXIMIZE. Anything else:
 * LPG_ERR_ARG and *out = NULL. */
int  lpg_binary_create(lpg_binary **out, int device, int64_t count, int64_t m, int64_t n, int32_t split, uint32_t flags);
/* Problems [first, first + np), np >= 1: A np x m rows of n entries at pitch
 * ldA >= n, sense np x m, rhs np x m, c np x n, dense. Refused as a whole on a
 * bad entry (see "Data and caps"). */
int  lpg_binary_load(lpg_binary *b, int64_t first, int64_t np, const double *A, int64_t ldA, const int32_t *sense,
                     const double *rhs, const double *c);
int  lpg_binary_generate(lpg_binary *b, uint64_t seed, int kind);
/* out[count] may be NULL. LPG_ERR_STATE while a problem has no data. */
int  lpg_binary_solve(lpg_binary *b, int64_t max_nodes, lpg_binary_result *out);
/* x of problems [first, first + np) after a solve, np x n of 0 / 1; -1
 * throughout for a problem with nothing found. */
int  lpg_binary_get(lpg_binary *b, int64_t first, int64_t np, int8_t *x);
int  lpg_binary_info(const lpg_binary *b, lpg_binary_info_t *out);
/* The waves of this batch's kernel instantiation that the device holds at once
 * (the occupancy query times the compute units times four). */
int  lpg_binary_occupancy(lpg_binary *b, int64_t *resident_waves);
const char *lpg_binary_last_error(const lpg_binary *b);
void lpg_binary_destroy(lpg_binary *b);                        /* NULL is a no-op */

/* ---- transportation: batches of balanced transportation problems ----
 *
 * Between duality and integer programming the textbook course behind the
 * reference's README has the transportation problem, solved by the tableau
 * method: a start by the northwest-corner or least-cost rule, potentials u, v
 * (MODI) with a pricing of the non-basic cells, and a closed-loop adjustment
 * of the flows. Stated as an LP a problem of nr sources and nc sinks has nr +
 * nc equality rows over nr * nc columns at a maximally degenerate vertex. An
 * lpg_transport holds `count` problems of one shape instead, 1 <= nr, 1 <= nc,
 * nr + nc <= LPG_TRANSPORT_MAX_NODES = 4096:
 *
 *     minimise (LPG_TRANSPORT_MAXIMIZE: maximise)  sum_ij c_ij x_ij
 *     subject to  sum_j x_ij = s_i,  sum_i x_ij = d_j,  x >= 0
 *
 * and solves them by that method (lpg_transport.hip). Unbalanced problems,
 * forbidden routes and ragged batches are not provided here (frontend.py
 * solve_transportation handles the first two).
 *
 * Data and caps. Every cost, supply and demand is a finite integer-valued fp64
 * with |c_ij| <= LPG_TRANSPORT_COST_CAP = 2^40, s_i >= 0, d_j >= 0, sum s = sum
 * d <= 2^53 and max |c| * sum s <= 2^53 (checked in integer arithmetic).
 * lpg_transport_load refuses anything else with LPG_ERR_ARG before any device
 * work; the message names the problem and the entry (for an unbalanced problem
 * both sums), and nothing is loaded. Zero supplies and demands are allowed. A
 * minimisation loads c + 0.0 and a maximisation 0.0 - c (exact, and no -0.0
 * inside); a maximisation reports 0.0 - u, 0.0 - v and 0.0 - objective. Why
 * the caps make every operation exact: a potential is an alternating sum of at
 * most nr + nc - 1 < 2^12 costs along a tree path, so below 2^52 in magnitude;
 * a reduced cost is a cost less two potentials, below 2^53; a flow is at most
 * sum s; the objective is at most max |c| * sum s. fp64 adds, subtracts,
 * multiplies and compares such integers without rounding, so no order of
 * evaluation can change a bit.
 *
 * The method, operation for operation (numpy: tests/transport_cases.py). Cell
 * (i, j) has index i * nc + j. The basis is a list of exactly nr + nc - 1
 * cells with their flows, a spanning tree of the bipartite graph of rows and
 * columns; a cell with flow 0 may be basic.
 *   Start, LPG_TRANSPORT_START_NORTHWEST. Begin at (0, 0) with rs = s_0, rd =
 *     d_0. nr + nc - 1 times: x = min(rs, rd); the cell becomes basic with
 *     flow x; rs -= x, rd -= x; after the last cell stop; otherwise if rs == 0
 *     and i < nr - 1 move down (i += 1, rs = s_i), else move right (j += 1,
 *     rd = d_j).
 *   Start, LPG_TRANSPORT_START_LEAST_COST (the default). All rows and columns
 *     are open, rs = s, rd = d. nr + nc - 1 times: take the open cell (row and
 *     column open) of smallest cost, ties to the smallest cell index; x =
 *     min(rs_i, rd_j); the cell becomes basic with flow x; rs_i -= x, rd_j -=
 *     x; after the last cell stop; otherwise close exactly one line: the row
 *     if rs_i == 0 and (rd_j != 0 or more than one row is open), else the
 *     column. (On balanced data an open cell always exists.)
 *   Iteration.
 *   1. Potentials. u_0 = 0. Along the tree a known row gives v_j = c_ij - u_i
 *      over a basic cell, a known column u_i = c_ij - v_j. The tree path from
 *      row 0 is unique, so the order of discovery does not matter.
 *   2. Pricing. delta_ij = (c_ij - u_i) - v_j over all cells. LPG_RULE_DANTZIG
 *      takes the smallest delta, ties to the smallest cell index;
 *      LPG_RULE_BLAND the smallest cell index with delta < 0. No delta < 0:
 *      the problem is LPG_OPTIMAL. Else, if the call has applied max_iters
 *      iterations to this problem: LPG_ITER_LIMIT, the state stays and a later
 *      call continues from it.
 *   3. Closed loop. Take the tree path from column j* to row i* of the
 *      entering cell; its 1st, 3rd, ... cells are the minus cells, the others
 *      the plus cells. theta is the smallest flow on a minus cell; the leaving
 *      cell is the minus cell with flow == theta and the smallest cell index.
 *      Minus cells lose theta, plus cells gain it; the entering cell takes the
 *      leaving cell's slot with flow theta. iterations += 1.
 * These rules do not exclude cycling at a degenerate vertex, so
 * lpg_transport_solve takes max_iters >= 1 and has no unbounded form.
 *
 * Per problem: status (LPG_OPTIMAL, LPG_ITER_LIMIT; LPG_NUMERIC would mean the
 * cell list is no tree, which the method cannot produce); iterations;
 * objective = sum c x in the caller's sense; the dense flows x[nr][nc]; u[nr]
 * and v[nc] of the basis as it stands; the basic cell indices ascending.
 * After LPG_OPTIMAL the certificate holds exactly: u_i + v_j <= c_ij (>= for a
 * maximisation) with equality on basic cells.
 *
 * Budgets. A launch applies at most `chunk` iterations per problem (default
 * LPG_TRANSPORT_DEFAULT_CHUNK, env LPG_TRANSPORT_CHUNK read at create) and the
 * host relaunches while a problem is unfinished and the call has budget left.
 * What crosses a launch is the cell list with its flows, the iteration count
 * and the status; potentials and tree are rebuilt from the cell list in every
 * iteration. Any sequence of budgets ends in the bits of one sufficient call.
 * A load or generate resets the problems it writes.
 *
 * Generator. lpg_transport_generate(t, seed, range, qmax): problem q draws
 * U(k) = uniform01(seed + q, k) (the engine's generator draw, oracle
 * lpo_uniform): c_ij = floor(U(i nc + j) range), s_i = 1 + floor(U(nr nc + i)
 * qmax), d_j = 1 + floor(U(nr nc + nr + j) qmax); the side with the smaller
 * sum gets the difference added to its last entry. range in 1..2^40 + 1, qmax
 * >= 1, (range - 1) max(nr, nc) qmax <= 2^53.
 *
 * Forms. nr + nc <= 64: one wave per problem, four problems per workgroup, no
 * workgroup barrier (the wave form). Else, or with env
 * LPG_TRANSPORT_FORM=workgroup, one workgroup of 256 threads per problem. Both
 * run one kernel body: 32 bytes of LDS per node (potential, flow, cell,
 * predecessor, depth, loop sign), the cells strided over the problem's threads
 * for the start and the pricing, the argmin by the DPP reductions over the
 * total-order key of the value and the cell index. C sits in LDS where it fits
 * the 150 KiB dynamic cap beside the node state (LPG_BATCH_TIER_LDS, up to 134
 * x 134), else in device memory, read coalesced (LPG_BATCH_TIER_GLOBAL; env
 * LPG_TRANSPORT_TIER=global forces it, and with it the workgroup form). Every
 * form and tier computes the same bits. The least-cost start is nr + nc - 1
 * sweeps over C inside the first launch.
 *
 * Every argument is checked on the host before any device work: the device is
 * first touched by the first lpg_transport_load, _generate or _solve that
 * passes its checks. The messages name the call and the first offending
 * index; NULL handles are errors (lpg_transport_last_error(NULL): this
 * thread's last one). One batch per host thread; not reentrant. */
#define LPG_TRANSPORT_MAXIMIZE          0x1u
#define LPG_TRANSPORT_START_LEAST_COST  0x0u
#define LPG_TRANSPORT_START_NORTHWEST   0x2u
#define LPG_TRANSPORT_FORM_WAVE         0
#define LPG_TRANSPORT_FORM_WORKGROUP    1
#define LPG_TRANSPORT_MAX_NODES         4096
#define LPG_TRANSPORT_COST_CAP          0x1p40
#define LPG_TRANSPORT_DEFAULT_CHUNK     1024

typedef struct lpg_transport lpg_transport;
/* started: 0 until the problem's start has been made (the library's own) */
typedef struct { int32_t status, started; int64_t iterations; double objective; } lpg_transport_result;
typedef struct {
    int64_t count, nr, nc;
    int32_t tier;                 /* LPG_BATCH_TIER_*: where C lives while a problem runs */
    int32_t form;                 /* LPG_TRANSPORT_FORM_* */
    int32_t start;                /* LPG_TRANSPORT_START_* */
    int32_t chunk;                /* iterations per problem per launch */
    int64_t lds_bytes;            /* dynamic LDS of one workgroup */
    int64_t launches;             /* kernel launches of the last lpg_transport_solve */
    double  kernel_ms;            /* device time of those launches, summed */
} lpg_transport_info_t;

/* count >= 1 problems of nr x nc, nr >= 1, nc >= 1, nr + nc <= 4096, count *
 * nr * nc <= 2^31 - 1; flags: LPG_TRANSPORT_MAXIMIZE, LPG_TRANSPORT_START_*.
 * Anything else: LPG_ERR_ARG and *out = NULL. */
int  lpg_transport_create(lpg_transport **out, int device, int64_t count, int64_t nr, int64_t nc, uint32_t flags);
/* Problems [first, first + n), n >= 1: n x nr rows of nc costs at pitch ld >=
 * nc, supply n x nr, demand n x nc, dense. Refused as a whole (nothing is
 * loaded) on a bad entry, see "Data and caps". */
int  lpg_transport_load(lpg_transport *t, int64_t first, int64_t n, const double *costs, int64_t ld, const double *supply,
                        const double *demand);
int  lpg_transport_generate(lpg_transport *t, uint64_t seed, int64_t range, int64_t qmax);
/* Continues every problem that is not LPG_OPTIMAL by at most max_iters >= 1
 * iterations; rule: LPG_RULE_DANTZIG or LPG_RULE_BLAND; out[count] may be
 * NULL. LPG_ERR_STATE while a problem has no data. */
int  lpg_transport_solve(lpg_transport *t, int64_t max_iters, int rule, lpg_transport_result *out);
/* Of problems [first, first + n) after a solve: x n x nr x nc, u n x nr, v n x
 * nc, basis n x (nr + nc - 1), dense; each may be NULL, not all four. */
int  lpg_transport_get(lpg_transport *t, int64_t first, int64_t n, double *x, double *u, double *v, int64_t *basis);
int  lpg_transport_info(const lpg_transport *t, lpg_transport_info_t *out);
const char *lpg_transport_last_error(const lpg_transport *t);
void lpg_transport_destroy(lpg_transport *t);                  /* NULL is a no-op */

#ifdef __cplusplus
}
#endif
#endif
