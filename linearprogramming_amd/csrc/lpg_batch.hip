// lpg_batch.hip — many small LPs in one launch: one workgroup per LP
// (include/lpg.h, "batches"); of one shape, or each of its own (a ragged batch).
//
// The context of lpg_ctx.hip spreads one tableau over the chip and pays a
// launch-sized cost per pivot whatever the tableau size. Here the chip is
// filled by the batch instead: workgroup b owns LP b for the whole launch,
// there is no protocol between workgroups (so no residency requirement: the
// hardware scheduler balances LPs of different pivot counts), and per pivot
// the workgroup does what oracle/lpo.c's lpo_solve / lpo_solve_dual do, with
// the same arithmetic (built with -ffp-contract=off, every fma explicit):
//   pricing (block argmin) -> ratio test (block argmin)
//   P[j] = T[r][j] / T[r][k],  C[i] = T[i][k]               (LDS buffers)
//   T[i][j] = fma(-C[i], P[j], T[i][j])  for i != r,  T[r] = P,  basis[r] = k
// so every LP is bitwise the oracle's, whatever else is in the batch.
//
// TIER_LDS: the whole tableau sits in dynamic LDS for the launch (row pitch
// odd in doubles: the ratio test's column read, lane = row, then touches 32
// different 8-byte bank pairs per 32-lane group; row-wise work, lane =
// column, is conflict-free at any pitch). TIER_GLOBAL: the tableau stays in
// device memory (one LP's working set is L2-sized), only P and C in LDS.
//
// Bounded launches: a launch applies at most `chunk` pivots per LP and the
// state round-trips through device memory; the host relaunches while the
// device counter of still-running LPs is non-zero. A workgroup whose LP is
// finished exits at once.
//
// Big-M batches (lpg_batch_create_big_m) carry two objective rows per LP, the
// M part in row m and the real part in row m + 1, and are solved by
// k_batch_big_m with lexicographic pricing (lpo.c lpo_solve_big_m).
//
// Goal batches (lpg_batch_create_goal) carry K <= LPG_GOAL_MAX_LEVELS objective
// rows per LP, row m + k the row of priority level k (level 0 the highest),
// and are solved by k_batch_goal: Big-M's loop with a pricing class per level
// (batch_price_goal), which at K = 2 is k_batch_big_m's pricing and at K = 1
// k_batch_solve's.
//
// The four solve kernels (k_batch_solve, k_batch_two_phase, k_batch_big_m,
// k_batch_goal) are their method's state machine over one set of parts: BatchView (where
// the LP lives, load / store, apply a pivot), batch_primal_step (one step of
// lpo_solve), batch_objective (an objective row) and batch_write_back.
//
// Ragged batches (lpg_batch_create_ragged): every LP has its own m and ncols,
// kept in a BatchShape record in device memory. A workgroup reads which LP it
// owns (BatchGeo::order) and that LP's record once at kernel entry (lp_geo;
// both addresses depend on blockIdx.x alone, so the fields are scalar) and from
// there on runs the code of a uniform batch. RG, the last template parameter
// of the solve kernels, says which of the two a launch is: a uniform batch
// runs the instantiations it ran before there were ragged ones.
//
// Branching (lpg_batch_branch_select, lpg_batch_branch) and cuts
// (lpg_batch_cut_select, lpg_batch_cut): the step between two levels of a
// branch-and-bound tree whose node LPs are a batch, and a round of Gomory
// mixed-integer cuts on a batch. Both are one path with two policies.
// Selection: frac_candidate says what a fractional row of the basis is;
// k_batch_branch_select picks every LP's best one, k_batch_cut_select lists
// its most fractional ones. Children: grow_copy makes a child from its
// parent's tableau plus k rows and k slack columns by a copy in device memory;
// k_batch_branch calls it with the one bound row, k_batch_cut, behind a
// prologue in LDS of its own, with one cut row per listed row. On the host
// stage_mask uploads the integer mask of all three calls that take one,
// grow_create makes the child batch and grow_finish launches the copy; what
// lpg_batch_branch and lpg_batch_cut keep is their own argument checks and
// job arrays.
//
// Scenarios (lpg_batch_scenario, lpg_batch_set_rhs): the same LPs under other
// right-hand sides. k_batch_scenario is grow_copy by no row plus
// scenario_column, which restates column 0 from the columns that hold B^-1;
// k_batch_set_rhs is scenario_column in place.
//
// Ranging (lpg_batch_ranging): the sensitivity report of the solved LPs.
// k_batch_ranging reads the tableau the solve left in device memory and
// reduces ratios under one total order (range_better): the cost ranges a wave
// per basic row, the right-hand-side ranges a lane per frame row, the dual
// values a gather. It writes only its own output arrays.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "../../include/lpg.h"
#include "lpg_internal.h"
#include "lpg_device.h"
#include "lpg_host.h"

namespace lpg {

constexpr int kBatchMaxLds = 150 * 1024;   // dynamic LDS cap, as lpg_block.hip's kMaxLds
constexpr int kBatchChunk = 4096;          // default pivots per LP and launch
constexpr int MODE_DUAL = 2;               // k_batch_solve's MODE: RULE_DANTZIG, RULE_BLAND or this
constexpr int TIER_LDS = LPG_BATCH_TIER_LDS, TIER_GLOBAL = LPG_BATCH_TIER_GLOBAL;

struct BatchLP {              // 64 B of state per LP
    int32_t status;           // of the current solve call (ITER_LIMIT once its budget is spent)
    int32_t pstatus;          // the primal loop's sticky status (lpo_ctx.status): RUNNING or final
    int64_t pivots;
    int64_t last_k, last_r;
    int64_t budget;           // pivots the current solve call may still apply
    double  objective;        // the (real) objective row's column 0 after the last launch
    int32_t phase;            // two-phase, Big-M: where the LP stands (PH_*); round-trips between launches
    int32_t pad;
    int64_t cursor;           // two-phase: the next row the drive-out looks at
};
static_assert(sizeof(BatchLP) == 64, "BatchLP is 64 bytes");

// k_batch_two_phase's per-LP state machine: a launch may end
// in front of any of these steps and the next one resumes there
enum : int32_t {
    PH_OBJ1 = 0,              // save the costs (cost == NULL), phase-I objective
    PH_LOOP1,                 // phase-I pivots, then the feasibility test
    PH_DRIVE,                 // drive basic artificials out, row `cursor` next
    PH_OBJ2,                  // phase-II objective from the real costs, phase-II budget
    PH_LOOP2,                 // phase-II pivots
};
// k_batch_big_m reuses the first two: PH_OBJ1 = both objective rows are still
// to be set (costs saved first when cost == NULL), PH_LOOP1 = in the pivot loop

struct TwoPhase {
    double *cost;             // count x N real costs (written by the kernel when save_cost)
    int64_t art_first, max_pivots;
    int32_t save_cost;        // cost == NULL: the costs are -1 x the objective row at the call
};

// One LP of a ragged batch: where it lives in the batch's arrays, and its geometry
struct BatchShape {           // 64 B per LP
    int64_t t_off, b_off, c_off;   // its tableau in T (doubles), its basis, its row of the cost buffer
    int32_t m, ncols;
    int32_t ld;               // the tableau's row pitch in device memory, (ncols + 63) & ~63
    int32_t pitch, txs;       // as BatchGeo's
    int32_t nact;             // columns 1..nact are priced by k_batch_solve
    int32_t art_first;        // of the last two-phase / Big-M call
    int32_t pad[3];
};
static_assert(sizeof(BatchShape) == 64, "BatchShape is 64 bytes");

struct BatchGeo {
    double  *T;               // count x (m + nobj) x ld (ragged: LP q at shape[q].t_off)
    int64_t *basis;           // count x m (ragged: LP q at shape[q].b_off)
    BatchLP *lp;              // count
    int32_t *logk, *logr;     // count x logcap, or null
    int32_t *running;         // LPs still RUNNING after this launch
    int64_t  ld, m, ncols, nact, logcap;
    double   eps_piv, eps_opt;
    int32_t  chunk;
    int32_t  pitch;           // TIER_LDS: row pitch in LDS (doubles, odd)
    int32_t  txs;             // update tile: 1 << txs lanes along a row, 256 >> txs rows at a time
    int32_t  nobj;            // objective rows: 1, 2 for a Big-M batch (M part in row m, real part in row m + 1), K of a goal batch
    const BatchShape *shape;  // ragged: one record per LP (then ld, m, ncols, nact, pitch, txs above are not read); else null
    const int32_t *order;     // ragged: workgroup w of this launch owns LP order[w]
};

// The LP of a workgroup and its geometry: the batch's one shape and LP =
// workgroup, or the LP's BatchShape record
struct LpGeo {
    int64_t lp, t_off, b_off, c_off, m, ncols, ld, nact, art_first;
    int32_t pitch, txs;
};

// the LP that workgroup blockIdx.x of a solve launch owns
template <bool RG>
__device__ __forceinline__ int64_t lp_index(const BatchGeo &g) {
    return RG ? (int64_t)g.order[blockIdx.x] : (int64_t)blockIdx.x;
}

// geometry of LP `lp` (uniform in the workgroup); nobj and art_first are the caller's for a uniform batch
template <bool RG>
__device__ __forceinline__ LpGeo lp_geo(const BatchGeo &g, int64_t lp, int64_t nobj, int64_t art_first) {
    LpGeo s;
    s.lp = lp;
    if (RG) {
        const BatchShape r = g.shape[lp];
        s.t_off = r.t_off;
        s.b_off = r.b_off;
        s.c_off = r.c_off;
        s.m = r.m;
        s.ncols = r.ncols;
        s.ld = r.ld;
        s.nact = r.nact;
        s.art_first = r.art_first;
        s.pitch = r.pitch;
        s.txs = r.txs;
    } else {
        s.t_off = lp * (g.m + nobj) * g.ld;
        s.b_off = lp * g.m;
        s.c_off = lp * (g.ncols - 1);
        s.m = g.m;
        s.ncols = g.ncols;
        s.ld = g.ld;
        s.nact = g.nact;
        s.art_first = art_first;
        s.pitch = g.pitch;
        s.txs = g.txs;
    }
    return s;
}

// geometry of LP `lp` of a plain batch, whatever its layout: for the kernels that are not built per layout
__device__ __forceinline__ LpGeo lp_geo_any(const BatchGeo &g, int64_t lp) {
    return g.shape ? lp_geo<true>(g, lp, 1, 0) : lp_geo<false>(g, lp, 1, 0);
}

// ------------------------------------------------------------------------
// generator: LP b = lpo_generate(n, seed + b, kind), one block per row
// ------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_batch_generate(BatchGeo g, int64_t n, uint64_t seed, int kind) {
    const int64_t rows = g.m + g.nobj;
    const int64_t b = (int64_t)blockIdx.x / rows, i = (int64_t)blockIdx.x % rows;
    const uint64_t s = seed + (uint64_t)b;
    const uint64_t kA = splitmix64(s ^ (1 * 0xD1B54A32D192ED03ull)), kB = splitmix64(s ^ (2 * 0xD1B54A32D192ED03ull)),
                   kC = splitmix64(s ^ (3 * 0xD1B54A32D192ED03ull));
    double *row = g.T + (b * rows + i) * g.ld;
    const double bscale = (double)n / 8.0;
    for (int64_t j = threadIdx.x; j < g.ld; j += kBlock) {
        double x = 0.0;
        if (i < g.m) {
            if (j == 0) {
                if (kind == 0 || kind == 3 || (i & 1)) x = bscale * (1.0 + uniform01(kB, (uint64_t)i));
                if (kind == 3) x = -x;
            } else if (j <= n) {
                const int64_t jj = j - 1;
                if (kind == 0 || kind == 3) {
                    x = uniform01(kA, (uint64_t)(i * n + jj));
                    if (kind == 3) x = -x;
                } else {
                    if (jj < i) {
                        x = uniform01(kA, (uint64_t)(i * n + jj)) / (double)(i + 1);
                        if (kind == 2 && !(i & 1)) x = -x;     // artificial: even rows are feasible `<= 0` rows
                    } else if (jj == i) x = 1.0;
                }
            } else if (j == unit_column(g.m, n, i, kind)) {
                x = 1.0;
            }
        } else if (i == rows - 1 && j >= 1 && j <= n) {   // (real) objective row; a Big-M M row stays zero
            x = 1.0 + uniform01(kC, (uint64_t)(j - 1));
            if (kind != 3) x = -x;                     // kind 3: max -c.x, d_j = +c_j (dual feasible)
        }
        row[j] = x;
    }
    if (i < g.m && threadIdx.x == 0) g.basis[b * g.m + i] = unit_column(g.m, n, i, kind);
}

// LPs [first, first + n) start again
__global__ void k_batch_reset(BatchLP *lp, int64_t first, int64_t n) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    BatchLP z{};
    z.last_k = z.last_r = -1;
    lp[first + q] = z;
}

// a solve call begins: the budget, and the status the oracle's loop would
// start from (primal: its sticky status; dual: derived anew every call)
__global__ void k_batch_begin(BatchLP *lp, int64_t count, int64_t budget, int dual) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= count) return;
    lp[q].budget = budget;
    lp[q].status = dual ? RUNNING : lp[q].pstatus;
}

// a two-phase or Big-M call begins: every LP starts at PH_OBJ1 again, whatever its status
__global__ void k_batch_begin_two_phase(BatchLP *lp, int64_t count, int64_t budget) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= count) return;
    lp[q].budget = budget;
    lp[q].status = RUNNING;
    lp[q].phase = PH_OBJ1;
    lp[q].cursor = 0;
}

// dual feasibility of every LP: bad[0] = the first LP with a d_j < -eps_opt
// (workgroup b looks at LP b, whatever the order of the solve launches)
__global__ __launch_bounds__(kBlock) void k_batch_dual_check(BatchGeo g, unsigned long long *bad) {
    const int64_t b = blockIdx.x;
    const LpGeo s = lp_geo_any(g, b);
    const double *obj = g.T + s.t_off + s.m * s.ld;
    bool any = false;
    for (int64_t j = 1 + threadIdx.x; j <= s.nact; j += kBlock) any |= obj[j] < -g.eps_opt;
    if (any) atomicMin(bad, (unsigned long long)b);
}

// ------------------------------------------------------------------------
// the parts the three solve kernels are made of (whole-block calls from
// uniform control flow; results uniform)
// ------------------------------------------------------------------------

// lpo_pivot's arithmetic on (k, r) with pivot element piv; the caller records
// the basis and the log and puts a barrier behind them
__device__ __forceinline__ void batch_pivot(double *T, int64_t tp, int64_t rows, int64_t ncols, double *sP, double *sC,
                                            int64_t k, int64_t r, double piv, int tid, int tx, int ty, int j0, int i0) {
    // P, C
    for (int64_t j = tid; j < ncols; j += kBlock) sP[j] = T[r * tp + j] / piv;
    for (int64_t i = tid; i < rows; i += kBlock) sC[i] = T[i * tp + k];
    __syncthreads();
    // rank-1 update (lpo_pivot)
    // a thread keeps its column's P[j] and walks the rows four at a time:
    // the four loads are issued before the first store, so their latencies
    // overlap (the compiler cannot reorder them itself: T, P and C may alias)
    for (int64_t j = j0; j < ncols; j += tx) {
        const double pj = sP[j];
        double *col = T + j;
        int64_t i = i0;
        for (; i + 3 * ty < rows; i += 4 * ty) {
            double c[4], t[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                c[u] = sC[i + u * ty];
                t[u] = col[(i + u * ty) * tp];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) col[(i + u * ty) * tp] = (i + u * ty == r) ? pj : fma(-c[u], pj, t[u]);
        }
        for (; i < rows; i += ty) col[i * tp] = (i == r) ? pj : fma(-sC[i], pj, col[i * tp]);
    }
}

// The LP of this workgroup: where its tableau and basis are worked on during
// the launch, and the moves every method makes on them. `rows` = m + nobj.
// LDS: [tableau (TIER_LDS)] P[ncols] C[rows] [basis as int32 (TIER_LDS)]
template <int TIER>
struct BatchView {
    double *T, *gT;           // the tableau of the launch (LDS or gT), the LP's tableau in device memory
    int64_t tp, ld;           // their row pitches
    int64_t *gB;              // the basis in device memory
    int32_t *sB;              // TIER_LDS: its mirror
    double *sP, *sC;
    int32_t *logk, *logr;     // the LP's log, or null
    int64_t logcap, m, rows, ncols;
    int tid, tx, ty, j0, i0;  // update tile coordinates (BatchGeo::txs)

    // the LDS layout is this LP's own: the launch's dynamic LDS is an upper bound of it
    static __device__ __forceinline__ BatchView make(const BatchGeo &g, const LpGeo &s, int64_t rows) {
        extern __shared__ double smem[];
        BatchView v;
        v.gT = g.T + s.t_off;
        v.ld = s.ld;
        v.tp = TIER == TIER_LDS ? (int64_t)s.pitch : s.ld;
        v.T = TIER == TIER_LDS ? smem : v.gT;
        v.gB = g.basis + s.b_off;
        v.sP = TIER == TIER_LDS ? smem + rows * v.tp : smem;
        v.sC = v.sP + s.ncols;
        v.sB = (int32_t *)(v.sC + rows);
        v.logk = g.logk ? g.logk + s.lp * g.logcap : nullptr;
        v.logr = g.logk ? g.logr + s.lp * g.logcap : nullptr;
        v.logcap = g.logcap;
        v.m = s.m;
        v.rows = rows;
        v.ncols = s.ncols;
        v.tid = threadIdx.x;
        v.tx = 1 << s.txs;
        v.ty = kBlock >> s.txs;
        v.j0 = v.tid & (v.tx - 1);
        v.i0 = v.tid >> s.txs;
        return v;
    }

    __device__ __forceinline__ void load() const {
        if (TIER == TIER_LDS) {
            for (int64_t i = i0; i < rows; i += ty)
                for (int64_t j = j0; j < ncols; j += tx) T[i * tp + j] = gT[i * ld + j];
            for (int64_t i = tid; i < m; i += kBlock) sB[i] = (int32_t)gB[i];
        }
        __syncthreads();
    }

    // the tableau back to device memory, where the launch changed it
    __device__ __forceinline__ void store(bool worked) const {
        if (TIER == TIER_LDS && worked) {
            for (int64_t i = i0; i < rows; i += ty)
                for (int64_t j = j0; j < ncols; j += tx) gT[i * ld + j] = T[i * tp + j];
        }
    }

    __device__ __forceinline__ int64_t basis(int64_t i) const { return TIER == TIER_LDS ? (int64_t)sB[i] : gB[i]; }

    // (k, r) with pivot element piv: the update, the basis, its mirror, entry `q` of the log
    __device__ __forceinline__ void apply(int64_t k, int64_t r, double piv, int64_t q) const {
        batch_pivot(T, tp, rows, ncols, sP, sC, k, r, piv, tid, tx, ty, j0, i0);
        if (tid == 0) {
            gB[r] = k;
            if (TIER == TIER_LDS) sB[r] = (int32_t)k;
            if (logk && q < logcap) {
                logk[q] = (int32_t)k;
                logr[q] = (int32_t)r;
            }
        }
        __syncthreads();
    }

    // the phase-I / M objective says artificials are still positive (lpo.c's
    // feasibility test); every thread adds the same column in row order
    __device__ __forceinline__ bool artificials_positive() const {
        double bsum = 0;
        for (int64_t i = 0; i < m; i++) bsum += fabs(T[i * tp]);
        return T[m * tp] < -1e-9 * (bsum > 1.0 ? bsum : 1.0);
    }
};

// pricing over columns 1..nact of the objective row (lpo.c price): the entering column or -1
template <int RULE>
__device__ __forceinline__ int64_t batch_price(const double *obj, int64_t nact, double eps_opt, int tid) {
    PricePart pb{0.0, -1, 0, 0};
    for (int64_t j = 1 + tid; j <= nact; j += kBlock) {
        const double d = obj[j];
        PricePart c{d, d < -eps_opt ? j : -1, 0, (int32_t)j};
        pp_take(pb, c, pp_better<RULE>(c, pb));
    }
    pb = block_argmin_pp<RULE>(pb);
    return pb.j;
}

// Big-M pricing over columns 1..nact of the two objective rows (lpo.c
// price_class): class 0 where the M part dM < -eps (value dM), class 1 where
// dM <= eps and the real part dR < -eps (value dR); pp_better and
// block_argmin_pp order by class first. A NaN dM makes a column ineligible.
template <int RULE>
__device__ __forceinline__ int64_t batch_price_big_m(const double *objM, const double *objR, int64_t nact, double eps_opt,
                                                     int tid) {
    PricePart pb{0.0, -1, 0, 0};
    for (int64_t j = 1 + tid; j <= nact; j += kBlock) {
        const double dM = objM[j], dR = objR[j];
        const bool c0 = dM < -eps_opt, c1 = (dM <= eps_opt) & (dR < -eps_opt);
        PricePart c{c0 ? dM : dR, (c0 | c1) ? j : -1, c0 ? 0 : 1, (int32_t)j};
        pp_take(pb, c, pp_better<RULE>(c, pb));
    }
    pb = block_argmin_pp<RULE>(pb);
    return pb.j;
}

// block_argmin_pp<RULE_DANTZIG> for partials of more than two classes (its
// key has one bit for the class): the least class of the wave first, then
// block_argmin_pp's (value, column) key among the lanes that hold it; the four
// waves meet in LDS through (class, key). Whole-wave calls only (wave_min_*).
template <int NW = kBlock / 64>
__device__ PricePart block_argmin_pp_cls(const PricePart &p) {
    const bool valid = p.j >= 0;
    const uint32_t c = valid ? (uint32_t)p.cls : ~0u;
    const uint32_t cm = wave_min_u32(c);
    const bool in = valid & (c == cm);
    uint64_t h = in ? (~(uint64_t)__double_as_longlong(p.v) & 0x7fffffffffffffffull) : ~0ull;
    uint32_t l = in ? (uint32_t)p.j : ~0u;
    const uint64_t mh = h;
    const uint32_t ml = l;
    wave_min_key(h, l);
    const int src = winner_lane(in && mh == h && ml == l);
    PricePart o{0.0, -1, 0, 0};
    if (src >= 0) {      // wave-uniform
        o.j = (int64_t)l;
        o.v = __longlong_as_double((long long)rdl64((uint64_t)__double_as_longlong(p.v), src));
        o.cls = (int32_t)cm;
        o.pad = (int32_t)rdl32((uint32_t)p.pad, src);
    }
    __shared__ PricePart sw[NW];
    __shared__ uint64_t sh[NW];
    __shared__ uint32_t sl[NW], sc[NW];
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        sw[w] = o;
        sh[w] = h;
        sl[w] = l;
        sc[w] = cm;
    }
    __syncthreads();
    int bi = 0;
    uint32_t bc = sc[0];
    uint64_t bh = sh[0];
    uint32_t bl = sl[0];
#pragma unroll
    for (int i = 1; i < NW; i++) {
        const bool t = sc[i] < bc || (sc[i] == bc && key_less(sh[i], sl[i], bh, bl));
        bc = t ? sc[i] : bc;
        bh = t ? sh[i] : bh;
        bl = t ? sl[i] : bl;
        bi = t ? i : bi;
    }
    return sw[bi];
}

// Goal pricing over columns 1..nact of the nlev objective rows at obj, obj +
// tp, ... (include/lpg.h, "goal programmes"): the class of a column is the
// first level k whose d_k < -eps (value d_k), every level before it within
// [-eps, eps]; a level before it that is positive or NaN makes the column
// ineligible. The levels are walked from the last to the first (a scalar
// loop: nlev is uniform), level k overwriting what the later levels left, by
// selects on its two predicates: no branch diverges per lane.
template <int RULE>
__device__ __forceinline__ int64_t batch_price_goal(const double *obj, int64_t tp, int nlev, int64_t nact, double eps_opt,
                                                    int tid) {
    PricePart pb{0.0, -1, 0, 0};
    for (int64_t j = 1 + tid; j <= nact; j += kBlock) {
        double val = 0.0;
        int32_t cls = 0;
        bool ok = false;
        for (int k = nlev - 1; k >= 0; k--) {
            const double d = obj[k * tp + j];
            const bool neg = d < -eps_opt, blocks = !(d <= eps_opt);
            val = neg ? d : val;
            cls = neg ? k : cls;
            ok = neg | (ok & !blocks);
        }
        PricePart c{val, ok ? j : -1, cls, (int32_t)j};
        pp_take(pb, c, pp_better<RULE>(c, pb));
    }
    pb = RULE == RULE_BLAND ? block_argmin_pp<RULE_BLAND>(pb) : block_argmin_pp_cls(pb);
    return pb.j;
}

// ratio test of column k (lpo.c ratio_block, cand_less): row < 0 when there is none
template <int RULE, int TIER>
__device__ __forceinline__ Cand batch_ratio(const BatchView<TIER> &v, int64_t k, double eps_piv) {
    Cand cb{0.0, 0.0, 0, -1};
    for (int64_t i = v.tid; i < v.m; i += kBlock) {
        const double a = v.T[i * v.tp + k], bi = v.T[i * v.tp];
        Cand c;
        c.theta = bi > 0.0 ? bi / a : 0.0;
        c.piv = a;
        c.key = RULE == RULE_BLAND ? v.basis(i) : i;
        c.row = a > eps_piv ? i : -1;
        cand_take(cb, c, cand_better(c, cb));
    }
    return block_argmin_cand(cb);
}

// What a step of a pivot loop returns: STEP_APPLIED (a pivot was applied and
// (k, r) set), RUNNING (the launch's work is spent: the loop goes on in the
// next launch), or the loop's final status.
constexpr int32_t STEP_APPLIED = -1;

// One step of lpo_solve. price() gives the entering column and is also the
// final peek when the budget is spent; `budget` pivots are left to the call
// and `room` units of work to the launch; the pivot becomes entry `q` of the
// log. The order of the checks is the oracle's.
template <int RULE, int TIER, class Price>
__device__ __forceinline__ int32_t batch_primal_step(const BatchView<TIER> &v, Price price, double eps_piv, int64_t budget,
                                                     int64_t room, int64_t q, int64_t &k, int64_t &r) {
    const int64_t kk = price();
    if (kk < 0) return OPTIMAL;
    if (budget == 0) return ITER_LIMIT;
    if (room <= 0) return RUNNING;
    const Cand cb = batch_ratio<RULE, TIER>(v, kk, eps_piv);
    if (cb.row < 0) return UNBOUNDED;
    if (!isfinite(cb.piv) || !isfinite(v.T[cb.row * v.tp])) return NUMERIC;
    v.apply(kk, cb.row, cb.piv, q);
    k = kk;
    r = cb.row;
    return STEP_APPLIED;
}

// One step of lpo_solve_dual on the objective row m, arguments as batch_primal_step's
template <int TIER>
__device__ __forceinline__ int32_t batch_dual_step(const BatchView<TIER> &v, int64_t nact, double eps_piv, double eps_opt,
                                                   int64_t budget, int64_t room, int64_t q, int64_t &k, int64_t &r) {
    // leaving row: most negative b_i, ties -> smallest row
    PricePart pb{0.0, -1, 0, 0};
    for (int64_t i = v.tid; i < v.m; i += kBlock) {
        const double bi = v.T[i * v.tp];
        PricePart c{bi, bi < -eps_opt ? i : -1, 0, (int32_t)i};
        pp_take(pb, c, pp_better<RULE_DANTZIG>(c, pb));
    }
    pb = block_argmin_pp<RULE_DANTZIG>(pb);
    const int64_t rr = pb.j;
    if (rr < 0) return OPTIMAL;
    if (budget == 0) return ITER_LIMIT;
    if (room <= 0) return RUNNING;
    // entering column: min d_j / -a_rj over a_rj < -eps_piv, ties -> smallest j
    Cand cb{0.0, 0.0, 0, -1};
    for (int64_t j = 1 + v.tid; j <= nact; j += kBlock) {
        const double a = v.T[rr * v.tp + j], d = v.T[v.m * v.tp + j];
        Cand c;
        c.theta = d > 0.0 ? d / -a : 0.0;
        c.piv = a;
        c.key = j;
        c.row = a < -eps_piv ? j : -1;
        cand_take(cb, c, cand_better(c, cb));
    }
    cb = block_argmin_cand(cb);
    if (cb.row < 0) return INFEASIBLE;
    v.apply(cb.row, rr, cb.piv, q);
    k = cb.row;
    r = rr;
    return STEP_APPLIED;
}

// The cost c_j of column j >= 0 (no column, no cost: a batch that was never
// given a basis holds zeros) under the three rules of lpo.c's objectives
enum : int {
    COST_ART,                 // phase I, the Big-M M part: -1 on the artificial columns (art_first on), 0 before
    COST_REAL,                // phase II: cost[j - 1]
    COST_REAL_NO_ART,         // the Big-M real part: cost[j - 1], the artificial columns forced to 0
};
template <int COST>
__device__ __forceinline__ double batch_cost(const double *cost, int64_t art_first, int64_t j) {
    if (COST == COST_ART) return j >= art_first ? -1.0 : 0.0;
    if (COST == COST_REAL) return j >= 1 ? cost[j - 1] : 0.0;
    return (j >= 1 && j < art_first) ? cost[j - 1] : 0.0;
}

// sC[i] = c_B(i), the cost of row i's basic column
template <int COST, int TIER>
__device__ __forceinline__ void batch_stage_cb(const BatchView<TIER> &v, const double *cost, int64_t art_first) {
    for (int64_t i = v.tid; i < v.m; i += kBlock) v.sC[i] = batch_cost<COST>(cost, art_first, v.basis(i));
    __syncthreads();
}

// lpo.c set_objective_row into row `row`: d_j = sum_i c_B(i) T[i][j] - c_j,
// per column one fma chain over the rows 0..m-1 in order (lane = column:
// conflict-free in LDS, coalesced in device memory; rows are never reduced
// across lanes)
template <int COST, int TIER>
__device__ __forceinline__ void batch_objective(const BatchView<TIER> &v, int64_t row, const double *cost, int64_t art_first) {
    batch_stage_cb<COST>(v, cost, art_first);
    const double *cB = v.sC;
    double *T = v.T;
    const int64_t tp = v.tp, m = v.m;
    for (int64_t j = v.tid; j < v.ncols; j += kBlock) {
        double acc = 0.0;
#pragma unroll 4
        for (int64_t i = 0; i < m; i++) acc = fma(cB[i], T[i * tp + j], acc);
        if (j > 0) acc = acc - batch_cost<COST>(cost, art_first, j);
        T[row * tp + j] = acc;
    }
    __syncthreads();
}

// Thread 0 at the end of a launch: the fields every method owns (phase and
// cursor are their kernels' own), the objective from the last row, and the
// count of LPs that go on
template <int TIER>
__device__ __forceinline__ void batch_write_back(const BatchGeo &g, const BatchView<TIER> &v, BatchLP *lp, int32_t status,
                                                 int32_t pstatus, int64_t pivots, int64_t last_k, int64_t last_r,
                                                 int64_t budget) {
    lp->status = status;
    lp->pstatus = pstatus;
    lp->pivots = pivots;
    lp->last_k = last_k;
    lp->last_r = last_r;
    lp->budget = budget;
    lp->objective = v.T[(v.rows - 1) * v.tp];
    if (status == RUNNING) atomicAdd(g.running, 1);
}

// ------------------------------------------------------------------------
// the pivot loop of one LP (lpo.c lpo_solve, lpo_solve_dual)
// ------------------------------------------------------------------------
template <int MODE, int TIER, bool RG = false>
__global__ __launch_bounds__(kBlock) void k_batch_solve(BatchGeo g) {
    const int64_t lpi = lp_index<RG>(g);
    BatchLP *lp = g.lp + lpi;
    if (lp->status != RUNNING) return;            // finished in an earlier launch (or call): uniform
    const LpGeo s = lp_geo<RG>(g, lpi, 1, 0);
    const BatchView<TIER> v = BatchView<TIER>::make(g, s, s.m + 1);
    int32_t pst = lp->pstatus;
    int64_t pivots = lp->pivots, budget = lp->budget, last_k = lp->last_k, last_r = lp->last_r;
    v.load();

    int32_t status;                               // RUNNING where the launch ends in front of a pivot
    int64_t work = 0;
    for (;;) {
        if constexpr (MODE != MODE_DUAL) {
            auto price = [&] { return batch_price<MODE>(v.T + v.m * v.tp, s.nact, g.eps_opt, v.tid); };
            status = batch_primal_step<MODE>(v, price, g.eps_piv, budget, g.chunk - work, pivots, last_k, last_r);
        } else {
            status = batch_dual_step(v, s.nact, g.eps_piv, g.eps_opt, budget, g.chunk - work, pivots, last_k, last_r);
        }
        if (status != STEP_APPLIED) break;
        pivots++;
        budget--;
        work++;
    }
    if (MODE != MODE_DUAL && status != RUNNING && status != ITER_LIMIT) pst = status;   // lpo_ctx.status

    v.store(work > 0);
    if (v.tid == 0) batch_write_back(g, v, lp, status, pst, pivots, last_k, last_r, budget);
}

// ------------------------------------------------------------------------
// two-phase simplex of one LP (lpo.c lpo_solve_two_phase), both phases and
// the transition between them in the workgroup that owns the LP
// ------------------------------------------------------------------------

// Work of a launch: a pivot (drive-outs included) or an objective computation
// is one unit, and a launch ends in front of the unit that would exceed
// g.chunk. `budget` is the oracle's: phase I may apply max_pivots pivots,
// phase II max(0, max_pivots - pivots of the LP); drive-outs are not charged.
template <int RULE, int TIER, bool RG = false>
__global__ __launch_bounds__(kBlock) void k_batch_two_phase(BatchGeo g, TwoPhase t) {
    const int64_t lpi = lp_index<RG>(g);
    BatchLP *lp = g.lp + lpi;
    if (lp->status != RUNNING) return;            // finished in an earlier launch of this call: uniform
    const LpGeo s = lp_geo<RG>(g, lpi, 1, t.art_first);
    const BatchView<TIER> v = BatchView<TIER>::make(g, s, s.m + 1);
    const int64_t m = s.m, ncols = s.ncols, af = s.art_first, chunk = g.chunk;
    double *cost = t.cost + s.c_off;
    int32_t phase = lp->phase, pst = lp->pstatus;
    int64_t cursor = lp->cursor, pivots = lp->pivots, budget = lp->budget, last_k = lp->last_k, last_r = lp->last_r;
    v.load();

    int64_t nact = 0;
    auto price = [&] { return batch_price<RULE>(v.T + m * v.tp, nact, g.eps_opt, v.tid); };
    int32_t status = RUNNING;                     // stays RUNNING where the launch ends in front of a unit
    int64_t work = 0;
    for (;;) {
        if (phase == PH_OBJ1 || phase == PH_OBJ2) {
            if (work >= chunk) break;
            if (phase == PH_OBJ1 && t.save_cost) {
                for (int64_t j = 1 + v.tid; j < ncols; j += kBlock) cost[j - 1] = -v.T[m * v.tp + j];
            }
            if (phase == PH_OBJ1) batch_objective<COST_ART>(v, m, cost, af);
            else batch_objective<COST_REAL>(v, m, cost, af);
            pst = RUNNING;                        // lpo_set_objective
            if (phase == PH_OBJ2) budget = t.max_pivots > pivots ? t.max_pivots - pivots : 0;
            phase++;
            work++;
            continue;
        }
        if (phase == PH_LOOP1 || phase == PH_LOOP2) {
            // lpo_solve over columns 1..N (phase I) or 1..art_first-1 (phase II)
            nact = phase == PH_LOOP1 ? ncols - 1 : af - 1;
            int32_t st;
            while ((st = batch_primal_step<RULE>(v, price, g.eps_piv, budget, chunk - work, pivots, last_k, last_r)) ==
                   STEP_APPLIED) {
                pivots++;
                budget--;
                work++;
            }
            if (st == RUNNING) break;             // the launch's work is done; this loop goes on in the next
            if (st != ITER_LIMIT) pst = st;       // lpo_ctx.status
            if (phase == PH_LOOP2 || st == ITER_LIMIT || st == NUMERIC) {
                status = st;
                break;
            }
            if (st == UNBOUNDED) {                // the phase-I objective is bounded: arithmetic went wrong
                status = NUMERIC;
                break;
            }
            if (v.artificials_positive()) {
                status = INFEASIBLE;
                break;
            }
            phase = PH_DRIVE;
            cursor = 0;
            continue;
        }
        // PH_DRIVE: a basic artificial leaves on the first real column with a usable entry in its
        // row, of either sign (b_i is zero there; no ratio test); a row without one keeps it
        bool full = false;
        for (; cursor < m; cursor++) {
            if (v.basis(cursor) < af) continue;
            PricePart pb{0.0, -1, 0, 0};
            for (int64_t j = 1 + v.tid; j < af; j += kBlock) {
                const double a = v.T[cursor * v.tp + j];
                PricePart c{a, fabs(a) > g.eps_piv ? j : -1, 0, (int32_t)j};
                pp_take(pb, c, pp_better<RULE_BLAND>(c, pb));
            }
            pb = block_argmin_pp<RULE_BLAND>(pb);  // the smallest such column
            if (pb.j < 0) continue;
            if (work >= chunk) {
                full = true;
                break;
            }
            v.apply(pb.j, cursor, pb.v, pivots);
            last_k = pb.j;
            last_r = cursor;
            pivots++;
            work++;
        }
        if (full) break;
        phase = PH_OBJ2;
    }

    v.store(work > 0);
    if (v.tid == 0) {
        batch_write_back(g, v, lp, status, pst, pivots, last_k, last_r, budget);
        lp->phase = phase;
        lp->cursor = cursor;
    }
}

// ------------------------------------------------------------------------
// Big-M simplex of one LP (lpo.c lpo_solve_big_m): tableaus of m + 2 rows,
// the M part of the objective in row m, the real part in row m + 1
// ------------------------------------------------------------------------

// Work of a launch as k_batch_two_phase's: a pivot or the computation of the
// two objective rows is one unit. `t.cost` holds the real costs (written here
// from row m + 1 when save_cost); lp->phase is PH_OBJ1 until the objective
// rows are set and PH_LOOP1 from then on, so a launch that ends in front of
// any unit is resumed bitwise by the next.
template <int RULE, int TIER, bool RG = false>
__global__ __launch_bounds__(kBlock) void k_batch_big_m(BatchGeo g, TwoPhase t) {
    const int64_t lpi = lp_index<RG>(g);
    BatchLP *lp = g.lp + lpi;
    if (lp->status != RUNNING) return;            // finished in an earlier launch of this call: uniform
    const LpGeo s = lp_geo<RG>(g, lpi, 2, t.art_first);
    const BatchView<TIER> v = BatchView<TIER>::make(g, s, s.m + 2);
    const int64_t m = s.m, ncols = s.ncols, af = s.art_first, chunk = g.chunk;
    double *cost = t.cost + s.c_off;
    int32_t phase = lp->phase, pst = lp->pstatus;
    int64_t pivots = lp->pivots, budget = lp->budget, last_k = lp->last_k, last_r = lp->last_r;
    v.load();

    int64_t work = 0;
    if (phase == PH_OBJ1) {
        // lpo_set_objective_m, lpo_set_objective: each row from the current basis (rows 0..m-1 only)
        if (t.save_cost) {
            for (int64_t j = 1 + v.tid; j < ncols; j += kBlock) cost[j - 1] = -v.T[(m + 1) * v.tp + j];
            __syncthreads();                      // the costs of the basic columns are read by other threads
        }
        batch_objective<COST_ART>(v, m, cost, af);
        batch_objective<COST_REAL_NO_ART>(v, m + 1, cost, af);
        pst = RUNNING;                            // lpo_set_objective
        phase = PH_LOOP1;
        work = 1;
    }
    // lpo_solve over columns 1..N, priced on both rows
    auto price = [&] {
        return batch_price_big_m<RULE>(v.T + m * v.tp, v.T + (m + 1) * v.tp, ncols - 1, g.eps_opt, v.tid);
    };
    int32_t status;                               // RUNNING where the launch ends in front of a unit
    while ((status = batch_primal_step<RULE>(v, price, g.eps_piv, budget, chunk - work, pivots, last_k, last_r)) ==
           STEP_APPLIED) {
        pivots++;
        budget--;
        work++;
    }
    if (status != RUNNING && status != ITER_LIMIT) pst = status;   // lpo_ctx.status
    if ((status == OPTIMAL || status == UNBOUNDED) && v.artificials_positive()) status = INFEASIBLE;

    v.store(work > 0);
    if (v.tid == 0) {
        batch_write_back(g, v, lp, status, pst, pivots, last_k, last_r, budget);
        lp->phase = phase;
    }
}

// ------------------------------------------------------------------------
// preemptive goal programme of one LP (include/lpg.h, "goal programmes"):
// tableaus of m + K rows, row m + k the objective row of priority level k
// ------------------------------------------------------------------------

struct GoalArgs {
    const double *cost;       // count x K x N: level k of LP q at (q * K + k) * N
    double *attain;           // count x K: column 0 of the objective rows after the launch
};

// k_batch_big_m's state machine with K = g.nobj rows: PH_OBJ1 = the K
// objective rows are still to be set (one unit of work), PH_LOOP1 = in the
// pivot loop, so a launch that ends in front of any unit is resumed bitwise.
template <int RULE, int TIER>
__global__ __launch_bounds__(kBlock) void k_batch_goal(BatchGeo g, GoalArgs a) {
    const int64_t lpi = blockIdx.x;
    BatchLP *lp = g.lp + lpi;
    if (lp->status != RUNNING) return;            // finished in an earlier launch of this call: uniform
    const int nlev = g.nobj;
    const LpGeo s = lp_geo<false>(g, lpi, nlev, 0);
    const BatchView<TIER> v = BatchView<TIER>::make(g, s, s.m + nlev);
    const int64_t m = s.m, N = s.ncols - 1, chunk = g.chunk;
    const double *cost = a.cost + lpi * nlev * N;
    int32_t phase = lp->phase, pst = lp->pstatus;
    int64_t pivots = lp->pivots, budget = lp->budget, last_k = lp->last_k, last_r = lp->last_r;
    v.load();

    int64_t work = 0;
    if (phase == PH_OBJ1) {
        // lpo_set_objective with level k's costs into row m + k, each from the current basis (rows 0..m-1 only)
        for (int k = 0; k < nlev; k++) batch_objective<COST_REAL>(v, m + k, cost + k * N, 0);
        pst = RUNNING;                            // lpo_set_objective
        phase = PH_LOOP1;
        work = 1;
    }
    // lpo_solve over columns 1..N, priced on the K rows
    auto price = [&] { return batch_price_goal<RULE>(v.T + m * v.tp, v.tp, nlev, N, g.eps_opt, v.tid); };
    int32_t status;                               // RUNNING where the launch ends in front of a unit
    while ((status = batch_primal_step<RULE>(v, price, g.eps_piv, budget, chunk - work, pivots, last_k, last_r)) ==
           STEP_APPLIED) {
        pivots++;
        budget--;
        work++;
    }
    if (status != RUNNING && status != ITER_LIMIT) pst = status;   // lpo_ctx.status

    v.store(work > 0);
    if (v.tid == 0) {
        batch_write_back(g, v, lp, status, pst, pivots, last_k, last_r, budget);
        lp->phase = phase;
        for (int k = 0; k < nlev; k++) a.attain[lpi * nlev + k] = v.T[(m + k) * v.tp];
    }
}

// lpo_set_objective on every LP, costs as k_batch_two_phase's (count x N)
__global__ __launch_bounds__(kBlock) void k_batch_set_objective(BatchGeo g, const double *costs) {
    const int64_t b = blockIdx.x;
    const LpGeo s = lp_geo_any(g, b);
    const int64_t m = s.m, ld = s.ld;
    double *T = g.T + s.t_off;
    const int64_t *gB = g.basis + s.b_off;
    const double *cost = costs + s.c_off;
    for (int64_t j = threadIdx.x; j < s.ncols; j += kBlock) {
        double acc = 0.0;
        for (int64_t i = 0; i < m; i++) acc = fma(gB[i] >= 1 ? cost[gB[i] - 1] : 0.0, T[i * ld + j], acc);
        T[m * ld + j] = j == 0 ? acc : acc - cost[j - 1];
    }
    if (threadIdx.x == 0) g.lp[b].status = g.lp[b].pstatus = RUNNING;
}

// ------------------------------------------------------------------------
// branching (include/lpg.h, "branching"): the step between two levels of a
// branch-and-bound tree, on the tableaus where the solve calls left them
// ------------------------------------------------------------------------

struct BranchPick {           // lpg_branch_t
    int64_t row, col;
    double value;
};
static_assert(sizeof(BranchPick) == sizeof(lpg_branch_t), "BranchPick is lpg_branch_t");

// Row i as a candidate of the select kernels: a row whose basic column bj is
// integer-constrained (mk, the LP's nmask mask bytes) is one when
// dist = min(f, 1 - f) > int_tol, f = v - floor(v), v = T[i][0], and the
// caller's also(-dist, bj) holds. A candidate is a pricing partial (v = -dist
// < 0, j = its column, pad = its row; j = -1: none), so the block argmin of
// the solve kernels picks among them: RULE_DANTZIG the largest dist, ties ->
// the smallest column; RULE_BLAND the smallest column (the basic columns of
// an LP differ).
template <class Also>
__device__ __forceinline__ PricePart frac_candidate(const int64_t *gB, const double *T, int64_t ld, const uint8_t *mk,
                                                    int64_t nmask, double int_tol, int64_t i, Also also) {
    const int64_t bj = gB[i];
    const bool integer = (bj >= 1) & (bj <= nmask) && mk[bj - 1] != 0;
    const double v = T[i * ld];
    const double f = v - floor(v), f1 = 1.0 - f;
    const double dist = f < f1 ? f : f1;
    return PricePart{-dist, (integer & (dist > int_tol) & also(-dist, bj)) ? bj : -1, 0, (int32_t)i};
}

// The branching row of LP blockIdx.x: the best candidate under RULE (mask:
// nmask bytes per LP at pitch ld_mask, 0: one for all)
template <int RULE>
__global__ __launch_bounds__(kBlock) void k_batch_branch_select(BatchGeo g, const uint8_t *mask, int64_t nmask, int64_t ld_mask,
                                                                double int_tol, BranchPick *out) {
    const int64_t q = blockIdx.x;
    const LpGeo s = lp_geo_any(g, q);
    const double *T = g.T + s.t_off;
    const int64_t *gB = g.basis + s.b_off;
    const uint8_t *mk = mask + q * ld_mask;
    PricePart pb{0.0, -1, 0, 0};
    for (int64_t i = threadIdx.x; i < s.m; i += kBlock) {
        const PricePart c = frac_candidate(gB, T, s.ld, mk, nmask, int_tol, i, [](double, int64_t) { return true; });
        pp_take(pb, c, pp_better<RULE>(c, pb));
    }
    pb = block_argmin_pp<RULE>(pb);
    if (threadIdx.x == 0) {
        BranchPick o{-1, -1, 0.0};
        if (pb.j >= 0) {
            o.row = pb.pad;
            o.col = pb.j;
            o.value = T[(int64_t)pb.pad * s.ld];
        }
        out[q] = o;
    }
}

struct BranchJob {            // child c of lpg_batch_branch: validated on the host
    int32_t src, row, dir, pad;
};

// entry j of a bound row from the branching row's entry x in column j of the
// parent: one negation; the right-hand side and the zero in the branching
// variable's own column bj are exact
__device__ __forceinline__ double branch_entry(double x, int64_t j, int64_t bj, bool down, double rhs) {
    const double y = down ? -x : x;
    return j == 0 ? rhs : (j == bj ? 0.0 : y);
}

// The copy that makes a child of branching or of a round of cuts: the child
// (c, cs) is the parent (p, ps) plus k rows behind its rows and k slack
// columns behind its active ones. Child row i is the parent's row i (i < m),
// new row t = i - m (m <= i < m + k) or the parent's objective row
// (i = m + k); new row t is made from the parent's row src_row(t), entry by
// entry: row_entry(t), asked for once per row and lane, is the function that
// gives its entry from that row's x in the parent's column j as (x, j). The
// parent's tableau is streamed from device memory row by row into the child's
// rows at the child's pitch. Columns 0..nact keep their place: both pitches
// are multiples of 64 doubles and both tableaus start on one, so the even part
// of them moves as 16-byte loads and stores, consecutive lanes on consecutive
// pairs of a row. The rest of a row (the k slack columns nact + 1.., new row
// t's 1 in slack t; behind them the parent's columns nact + 1.. moved right
// by k, which an odd k takes off the 16-byte grid) moves as doubles. The
// child's padding columns stay the zeros of its allocation. The child's basis
// is the parent's with the same shift, and slack t basic in new row t.
template <class SrcRow, class RowEntry>
__device__ __forceinline__ void grow_copy(const BatchGeo &p, const LpGeo &ps, const BatchGeo &c, const LpGeo &cs, int64_t k,
                                          SrcRow src_row, RowEntry row_entry) {
    const double *pT = p.T + ps.t_off;
    double *cT = c.T + cs.t_off;
    const int64_t *pB = p.basis + ps.b_off;
    int64_t *cB = c.basis + cs.b_off;
    const int64_t m = ps.m, nc = ps.ncols, nact = ps.nact, pld = ps.ld, cld = cs.ld;
    const int tid = threadIdx.x;

    // a tile of 1 << txs lanes along a row (enough for its pairs, 256 at the most) and 256 >> txs rows at a
    // time: the row and column of a lane come from shifts, and a narrow LP still fills the workgroup
    const int npair = (int)((nact + 1) >> 1), w0 = 2 * npair;      // columns [0, w0) as pairs
    int txs = 0;
    while ((1 << txs) < npair && txs < 8) txs++;
    const int tx = 1 << txs, ty = kBlock >> txs, j0 = tid & (tx - 1), i0 = tid >> txs;
    for (int64_t i = i0; i < m + k + 1; i += ty) {
        const bool fresh = (i >= m) & (i < m + k);
        const int64_t t = fresh ? i - m : 0;
        const int64_t si = i < m ? i : (fresh ? (int64_t)src_row(t) : m);
        const auto entry = row_entry(t);                           // row 0's on a copied row, where it is not called
        const double *prow = pT + si * pld;
        double *crow = cT + i * cld;
        for (int j = 2 * j0; j < w0; j += 2 * tx) {
            d2 x = *(const d2 *)(prow + j);
            if (fresh) {
                x.x = entry(x.x, j);
                x.y = entry(x.y, (int64_t)j + 1);
            }
            *(d2 *)(crow + j) = x;
        }
        // child columns [w0, nc + k): at most one unshifted column, the slacks, the shifted columns
        for (int64_t j = w0 + j0; j < nc + k; j += tx) {
            double y;
            if (j > nact && j <= nact + k) y = (fresh && j == nact + 1 + t) ? 1.0 : 0.0;
            else {
                const int64_t pj = j <= nact ? j : j - k;
                y = prow[pj];
                if (fresh) y = entry(y, pj);
            }
            crow[j] = y;
        }
    }
    for (int64_t i = tid; i < m + k; i += kBlock) cB[i] = i >= m ? nact + 1 + (i - m) : (pB[i] > nact ? pB[i] + k : pB[i]);
}

// Child blockIdx.x of `c` from LP job.src of `p` (RG: both ragged, as the
// parent is): grow_copy by the one bound row, made from the branching row.
// No LDS and nothing in front of the copy.
template <bool RG>
__global__ __launch_bounds__(kBlock) void k_batch_branch(BatchGeo p, BatchGeo c, const BranchJob *jobs) {
    const BranchJob job = jobs[blockIdx.x];
    const LpGeo ps = lp_geo<RG>(p, job.src, 1, 0), cs = lp_geo<RG>(c, blockIdx.x, 1, 0);
    const int64_t r = job.row;
    const bool down = job.dir < 0;
    const double v = p.T[ps.t_off + r * ps.ld];
    const int64_t bj = p.basis[ps.b_off + r];
    const double rhs = down ? floor(v) - v : v - ceil(v);
    grow_copy(p, ps, c, cs, 1, [&](int64_t) { return r; },
              [&](int64_t) { return [&](double x, int64_t j) { return branch_entry(x, j, bj, down, rhs); }; });
}

// ------------------------------------------------------------------------
// cuts (include/lpg.h, "cuts"): a round of Gomory mixed-integer cuts on the
// tableaus where the solve calls left them. Every operation of the cut is one
// rounding (the file is built with -ffp-contract=off; the product and the
// quotient are spelled __dmul_rn / __ddiv_rn), so tests/cut_cases.py
// reproduces every bit.
// ------------------------------------------------------------------------

// x - floor(x), and 0 where that difference rounds to 1 (a tiny negative x)
__device__ __forceinline__ double cut_frac(double x) {
    const double f = x - floor(x);
    return f >= 1.0 ? 0.0 : f;
}

// The cut rows of LP blockIdx.x: the candidates of k_batch_branch_select
// (frac_candidate), the `max_cuts` best in LPG_BRANCH_MOST_FRACTIONAL order,
// by repeated extraction: round t takes the block argmin over the candidates
// that come strictly behind pick t - 1 in that order (a total one: the basic
// columns of an LP differ).
__global__ __launch_bounds__(kBlock) void k_batch_cut_select(BatchGeo g, const uint8_t *mask, int64_t nmask, int64_t ld_mask,
                                                             double int_tol, int64_t max_cuts, int64_t *ncut, int64_t *rows) {
    const int64_t q = blockIdx.x;
    const LpGeo s = lp_geo_any(g, q);
    const double *T = g.T + s.t_off;
    const int64_t *gB = g.basis + s.b_off;
    const uint8_t *mk = mask + q * ld_mask;
    int64_t *out = rows + q * max_cuts;
    double last_v = 0.0;
    int64_t last_j = -1, t = 0;
    for (; t < max_cuts; t++) {
        PricePart pb{0.0, -1, 0, 0};
        auto behind = [&](double v, int64_t bj) { return (t == 0) | (v > last_v) | ((v == last_v) & (bj > last_j)); };
        for (int64_t i = threadIdx.x; i < s.m; i += kBlock) {
            const PricePart c = frac_candidate(gB, T, s.ld, mk, nmask, int_tol, i, behind);
            pp_take(pb, c, pp_better<RULE_DANTZIG>(c, pb));
        }
        pb = block_argmin_pp<RULE_DANTZIG>(pb);
        if (pb.j < 0) break;                                   // uniform: every thread holds the block's pick
        last_v = pb.v;
        last_j = pb.j;
        if (threadIdx.x == 0) out[t] = pb.pad;
    }
    if (threadIdx.x == 0) ncut[q] = t;
    for (int64_t u = t + threadIdx.x; u < max_cuts; u += kBlock) out[u] = -1;
}

struct CutJob {               // child c of lpg_batch_cut: validated on the host
    int32_t src, first, k, pad;   // its source LP, its rows at rows[first .. first + k)
};

// entry j of a cut row from the source row's entry a in column j of the
// parent (include/lpg.h, "cuts"): -f0 in column 0, else -g_j
__device__ __forceinline__ double cut_entry(double a, int64_t j, int64_t nact, const uint8_t *basic, const uint8_t *mk,
                                            int64_t nmask, double f0, double rho) {
    if (j == 0) return -f0;
    double g;
    if (j > nact || basic[j]) g = 0.0;
    else if (j <= nmask && mk[j - 1]) {
        const double f = cut_frac(a);
        g = f <= f0 ? f : __dmul_rn(rho, 1.0 - f);
    } else g = a >= 0.0 ? a : __dmul_rn(rho, -a);
    return -g;
}

// Child blockIdx.x of `c` from LP job.src of `p` (RG: the parent is ragged,
// and then the child is; a parent of one shape has a ragged child where the
// cut counts differ). The prologue marks the source's basic columns in an LDS
// byte map and computes (f0, rho) of every cut; then grow_copy by the job's k
// cut rows, cut t made from row sRow[t].
template <bool RG>
__global__ __launch_bounds__(kBlock) void k_batch_cut(BatchGeo p, BatchGeo c, const CutJob *jobs, const int32_t *rows,
                                                      const uint8_t *mask, int64_t nmask, int64_t ld_mask) {
    __shared__ double sF0[LPG_BATCH_MAX_CUTS], sRho[LPG_BATCH_MAX_CUTS];
    __shared__ int32_t sRow[LPG_BATCH_MAX_CUTS];
    __shared__ uint32_t sBasicWords[LPG_BATCH_MAX_DIM / 4];
    uint8_t *sBasic = (uint8_t *)sBasicWords;

    const CutJob job = jobs[blockIdx.x];
    const LpGeo ps = lp_geo<RG>(p, job.src, 1, 0), cs = lp_geo_any(c, blockIdx.x);
    const double *pT = p.T + ps.t_off;
    const int64_t *pB = p.basis + ps.b_off;
    const uint8_t *mk = mask + (int64_t)job.src * ld_mask;
    const int64_t m = ps.m, nc = ps.ncols, nact = ps.nact, k = job.k;
    const int tid = threadIdx.x;

    for (int64_t w = tid; w < (nc + 3) >> 2; w += kBlock) sBasicWords[w] = 0;
    for (int64_t t = tid; t < k; t += kBlock) {
        const int32_t r = rows[job.first + t];
        const double f0 = cut_frac(pT[r * ps.ld]);
        sRow[t] = r;
        sF0[t] = f0;
        sRho[t] = __ddiv_rn(f0, 1.0 - f0);
    }
    __syncthreads();
    for (int64_t i = tid; i < m; i += kBlock) {
        const int64_t bj = pB[i];
        if (bj >= 0 && bj < nc) sBasic[bj] = 1;
    }
    __syncthreads();

    grow_copy(p, ps, c, cs, k, [&](int64_t t) { return sRow[t]; }, [&](int64_t t) {
        const double f0 = sF0[t], rho = sRho[t];
        return [=](double a, int64_t j) { return cut_entry(a, j, nact, sBasic, mk, nmask, f0, rho); };
    });
}

// ------------------------------------------------------------------------
// scenarios (include/lpg.h, "scenarios"): the same LP under another
// right-hand side. The columns that were the identity when the LP was stated
// (`ident`) hold B^-1 now, so column 0 of every row r, the objective row
// included, is
//     acc = 0.0; for i = 0..m-1: acc = acc + T[r][ident[i]] * rhs[i]
// in that order, every operation one rounding (the product spelled
// __dmul_rn, as the cut's), so tests/scenario_cases.py reproduces every bit.
// ------------------------------------------------------------------------

struct ScenarioJob {          // child c of lpg_batch_scenario: validated on the host
    int32_t src, pad;
    int64_t rhs_off;          // its right-hand side at rhs[rhs_off .. rhs_off + m_src)
};

constexpr int WALK_TILE = 0, WALK_ROWS = 1;   // how scenario_column walks the tableau
constexpr int kScnRows = 64, kScnCols = 32;   // WALK_TILE: rows and ident columns of a tile

// LP's m ident columns and right-hand side into the launch's dynamic LDS: [rhs: m doubles][ident: m int32]
__device__ __forceinline__ void scenario_stage(const int64_t *ident, const double *rhs, int64_t m, double *&sR, int32_t *&sI) {
    extern __shared__ double smem[];
    sR = smem;
    sI = (int32_t *)(smem + m);
    for (int64_t i = threadIdx.x; i < m; i += kBlock) {
        sR[i] = rhs[i];
        sI[i] = (int32_t)ident[i];
    }
    __syncthreads();
}

// out[r * old] = sum_i T[r][sI[i]] * sR[i] for the rows r = 0..m of the tableau T (pitch ld), the additions of
// a row in ascending i. T's column 0 is not read, so out may be it. WALK_ROWS: a lane owns a row and gathers
// its m entries from device memory, lanes a pitch apart. WALK_TILE: the workgroup reads kScnRows x kScnCols
// entries at a time along the rows (ident columns are mostly neighbours: slacks, artificials) into an LDS
// tile of odd pitch; then lane = row adds its kScnCols products in order, the sum kept in its register from
// tile to tile of the row block.
__device__ __forceinline__ void scenario_column(const double *T, int64_t ld, int64_t m, const int32_t *sI, const double *sR,
                                                double *out, int64_t old, int walk) {
    const int tid = threadIdx.x;
    if (walk == WALK_ROWS) {
        for (int64_t r = tid; r <= m; r += kBlock) {
            const double *row = T + r * ld;
            double acc = 0.0;
#pragma unroll 4
            for (int64_t i = 0; i < m; i++) acc = acc + __dmul_rn(row[sI[i]], sR[i]);
            out[r * old] = acc;
        }
        return;
    }
    __shared__ double tile[kScnRows][kScnCols + 1];
    const int ti = tid & (kScnCols - 1), tr0 = tid / kScnCols;     // a lane's column of the tile, its first row
    for (int64_t r0 = 0; r0 <= m; r0 += kScnRows) {
        double acc = 0.0;
        for (int64_t i0 = 0; i0 < m; i0 += kScnCols) {
            const int64_t nc = m - i0 < kScnCols ? m - i0 : kScnCols;
            if (ti < nc) {
                const int64_t col = sI[i0 + ti];
                for (int tr = tr0; tr < kScnRows && r0 + tr <= m; tr += kBlock / kScnCols)
                    tile[tr][ti] = T[(r0 + tr) * ld + col];
            }
            __syncthreads();
            if (tid < kScnRows && r0 + tid <= m)
                for (int64_t i = 0; i < nc; i++) acc = acc + __dmul_rn(tile[tid][i], sR[i0 + i]);
            __syncthreads();
        }
        if (tid < kScnRows && r0 + tid <= m) out[(r0 + tid) * old] = acc;
    }
}

// Child blockIdx.x of `c` from LP job.src of `p` (RG: both ragged, as the parent is): grow_copy by no row, so
// the child is the parent moved as 16-byte pairs, inert artificial columns included; then column 0 from the
// parent's tableau. The copy writes the child's column 0 as well, from other lanes: the barrier puts
// scenario_column's stores behind it.
template <bool RG>
__global__ __launch_bounds__(kBlock) void k_batch_scenario(BatchGeo p, BatchGeo c, const ScenarioJob *jobs, const int64_t *ident,
                                                           const double *rhs, int walk) {
    const ScenarioJob job = jobs[blockIdx.x];
    const LpGeo ps = lp_geo<RG>(p, job.src, 1, 0), cs = lp_geo<RG>(c, blockIdx.x, 1, 0);
    double *sR;
    int32_t *sI;
    scenario_stage(ident + ps.b_off, rhs + job.rhs_off, ps.m, sR, sI);
    grow_copy(p, ps, c, cs, 0, [](int64_t) { return 0; }, [](int64_t) { return [](double x, int64_t) { return x; }; });
    __syncthreads();
    scenario_column(p.T + ps.t_off, ps.ld, ps.m, sI, sR, c.T + cs.t_off, cs.ld, walk);
}

// LP blockIdx.x of `g` restated in place: column 0 is only written, the columns from 1 on only read
__global__ __launch_bounds__(kBlock) void k_batch_set_rhs(BatchGeo g, const int64_t *ident, const double *rhs, int walk) {
    const LpGeo s = lp_geo_any(g, blockIdx.x);
    double *sR;
    int32_t *sI;
    scenario_stage(ident + s.b_off, rhs + s.b_off, s.m, sR, sI);
    double *T = g.T + s.t_off;
    scenario_column(T, s.ld, s.m, sI, sR, T, s.ld, walk);
}

// ------------------------------------------------------------------------
// ranging (include/lpg.h, "ranging"): dual values, and how far every cost and
// every right-hand side of a solved LP can move before its basis changes.
// Every bound is the largest (lower) or smallest (upper) q = (-x) / a over
// candidates (x, a, index); a candidate for the lower bound iff a > eps_piv,
// for the upper iff a < -eps_piv, never one whose q is NaN; equal q: the
// smallest index. That order is total (indices are unique, NaNs are out), so
// a lane's stride, the butterfly of a wave and any other grouping keep the
// same winner, and tests/ranging_cases.py states it in numpy bit for bit.
// ------------------------------------------------------------------------

struct RangingOut {           // device arrays in the layouts of include/lpg.h; a group that is not wanted is null
    double  *dual;
    double  *cost_lo, *cost_hi;
    int64_t *cost_lo_at, *cost_hi_at;
    double  *rhs_lo, *rhs_hi;
    int64_t *rhs_lo_at, *rhs_hi_at;
};

struct RangeRec {             // one running bound: its ratio and the candidate's index, -1 = no candidate yet
    double  q;
    int32_t at;
};

// candidate `a` takes the place of `b`; UP: the upper bound (smallest q), else the lower (largest q).
// Branch-free, and the take is one select per field (lpg_device.h, the miscompile note).
template <bool UP>
__device__ __forceinline__ bool range_better(const RangeRec &a, const RangeRec &b) {
    const bool ord = (UP ? a.q < b.q : a.q > b.q) | ((a.q == b.q) & (a.at < b.at));
    return (a.at >= 0) & ((b.at < 0) | ord);
}
__device__ __forceinline__ void range_take(RangeRec &best, const RangeRec &c, bool t) {
    best.q = t ? c.q : best.q;
    best.at = t ? c.at : best.at;
}

// the candidate (x, a, at) offered to both running bounds
__device__ __forceinline__ void range_offer(RangeRec &lo, RangeRec &hi, double x, double a, int32_t at, double eps) {
    const double q = __ddiv_rn(-x, a);
    const bool num = q == q;
    const RangeRec cl{q, ((a > eps) & num) ? at : -1}, ch{q, ((a < -eps) & num) ? at : -1};
    range_take(lo, cl, range_better<false>(cl, lo));
    range_take(hi, ch, range_better<true>(ch, hi));
}

// the best record of the wave in every lane; the whole wave is active
template <bool UP>
__device__ __forceinline__ RangeRec range_wave(RangeRec c) {
#pragma unroll
    for (int mask = 32; mask > 0; mask >>= 1) {
        RangeRec o;
        o.q = __shfl_xor(c.q, mask, 64);
        o.at = __shfl_xor(c.at, mask, 64);
        range_take(c, o, range_better<UP>(o, c));
    }
    return c;
}

__device__ __forceinline__ double range_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// LP blockIdx.x of `g`. Dynamic LDS, the two phases one after the other in the same bytes:
//   costs:             [objective row: ncols doubles][column -> the row it is basic in, or -1: ncols int32]
//   right-hand sides:  [column 0: m doubles][ident: m int32]
// Costs: wave w takes the basic rows w, w + 4, ..., its lanes stride the columns, one butterfly per bound and
// row, no block barrier in the row loop; nonbasic and inert columns are filled lane = column. Right-hand sides:
// a lane owns frame row i and walks the rows r of column ident[i] (neighbouring lanes read neighbouring
// columns: slacks, artificials), so no cross-lane step.
template <bool RG>
__global__ __launch_bounds__(kBlock) void k_batch_ranging(BatchGeo g, const int64_t *ident, RangingOut o) {
    extern __shared__ double smem[];
    const LpGeo s = lp_geo<RG>(g, blockIdx.x, 1, 0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = s.m, N = s.ncols - 1, nact = s.nact, ld = s.ld;
    const double *T = g.T + s.t_off, *obj = T + m * ld;
    const int64_t *basis = g.basis + s.b_off;
    const double eps = g.eps_piv, inf = __longlong_as_double(0x7ff0000000000000ll);
    ident += s.b_off;

    if (g.lp[s.lp].status != OPTIMAL) {        // not ranged: NaN and "none" (column 0, row -1)
        for (int64_t i = tid; i < m; i += kBlock) {
            if (o.dual) o.dual[s.b_off + i] = range_nan();
            if (o.rhs_lo) {
                o.rhs_lo[s.b_off + i] = o.rhs_hi[s.b_off + i] = range_nan();
                o.rhs_lo_at[s.b_off + i] = o.rhs_hi_at[s.b_off + i] = -1;
            }
        }
        if (o.cost_lo)
            for (int64_t j = tid; j < N; j += kBlock) {
                o.cost_lo[s.c_off + j] = o.cost_hi[s.c_off + j] = range_nan();
                o.cost_lo_at[s.c_off + j] = o.cost_hi_at[s.c_off + j] = 0;
            }
        return;
    }

    if (o.dual)
        for (int64_t i = tid; i < m; i += kBlock) o.dual[s.b_off + i] = obj[ident[i]];

    if (o.cost_lo) {
        double *sObj = smem;
        int32_t *sRow = (int32_t *)(smem + s.ncols);
        for (int64_t j = tid; j <= N; j += kBlock) {
            sObj[j] = obj[j];
            sRow[j] = -1;
        }
        __syncthreads();
        for (int64_t i = tid; i < m; i += kBlock) {
            const int64_t bj = basis[i];
            if (bj >= 1 && bj <= N) sRow[bj] = (int32_t)i;
        }
        __syncthreads();
        double *lo = o.cost_lo + s.c_off, *hi = o.cost_hi + s.c_off;               // column j at [j - 1]
        int64_t *lo_at = o.cost_lo_at + s.c_off, *hi_at = o.cost_hi_at + s.c_off;
        for (int64_t j = 1 + tid; j <= N; j += kBlock) {
            const bool inert = j > nact;
            if (!inert && sRow[j] >= 0) continue;                 // basic: its row's wave stores it
            lo[j - 1] = -inf;
            lo_at[j - 1] = 0;
            hi[j - 1] = inert ? inf : sObj[j];
            hi_at[j - 1] = inert ? 0 : j;
        }
        for (int64_t r = wave; r < m; r += kBlock / 64) {         // wave-uniform
            const int64_t j = basis[r];
            if (j < 1 || j > nact || sRow[j] != (int32_t)r) continue;   // a kept artificial; a column listed twice: one row's
            const double *row = T + r * ld;
            RangeRec rl{0.0, -1}, rh{0.0, -1};
            for (int64_t k = 1 + lane; k <= nact; k += 64)
                if (sRow[k] < 0) range_offer(rl, rh, sObj[k], row[k], (int32_t)k, eps);
            rl = range_wave<false>(rl);
            rh = range_wave<true>(rh);
            if (lane == 0) {
                lo[j - 1] = rl.at < 0 ? -inf : rl.q;
                lo_at[j - 1] = rl.at < 0 ? 0 : rl.at;
                hi[j - 1] = rh.at < 0 ? inf : rh.q;
                hi_at[j - 1] = rh.at < 0 ? 0 : rh.at;
            }
        }
    }

    if (o.rhs_lo) {
        __syncthreads();                                          // the cost phase is done with the bytes
        double *sB = smem;
        int32_t *sI = (int32_t *)(smem + m);
        for (int64_t i = tid; i < m; i += kBlock) {
            sB[i] = T[i * ld];
            sI[i] = (int32_t)ident[i];
        }
        __syncthreads();
        for (int64_t i = tid; i < m; i += kBlock) {
            const double *col = T + sI[i];
            RangeRec rl{0.0, -1}, rh{0.0, -1};
#pragma unroll 4
            for (int64_t r = 0; r < m; r++) range_offer(rl, rh, sB[r], col[r * ld], (int32_t)r, eps);
            o.rhs_lo[s.b_off + i] = rl.at < 0 ? -inf : rl.q;
            o.rhs_lo_at[s.b_off + i] = rl.at;
            o.rhs_hi[s.b_off + i] = rh.at < 0 ? inf : rh.q;
            o.rhs_hi_at[s.b_off + i] = rh.at;
        }
    }
}

}  // namespace lpg

// ---------------------------------------------------------------------------
// host: the batch object and the extern "C" entry points
// ---------------------------------------------------------------------------
using namespace lpg;

struct lpg_batch {
    int device = 0;
    int64_t count = 0, m = 0, ncols = 0, ld = 0, nact = 0;
    int nobj = 1;                 // 2: a Big-M batch (lpg_batch_create_big_m), tableaus of m + 2 rows
    bool goal = false;            // a goal batch (lpg_batch_create_goal): nobj = K priority levels, tableaus of m + K rows
    uint32_t flags = 0;
    double eps_piv = 1e-9, eps_opt = 1e-9;
    int tier = TIER_LDS;
    int64_t lds = 0;
    int chunk = kBatchChunk;
    int pitch = 0, txs = 0;
    int64_t logcap = 0;
    bool pivoted = false;         // a solve call has run since the last load / generate of the whole batch
    double *T = nullptr;
    int64_t *basis = nullptr;
    BatchLP *lp = nullptr;
    int32_t *logk = nullptr, *logr = nullptr;
    int32_t *running = nullptr;
    unsigned long long *bad = nullptr;
    double *cost = nullptr;       // count x N real costs of two-phase and Big-M calls / set_objective (allocated on first use)
    double *attain = nullptr;     // goal batch: count x K attained levels (its cost is count x K x N; both allocated on first use)
    hipStream_t stream = nullptr;
    char err[512] = {0};
    // A round of a solve call is one launch per group: LPs order[first .. first + count)
    // with `lds` bytes of dynamic LDS on `tier`, its count of running LPs in running[slot].
    // A uniform batch is one group of all its LPs.
    struct Group {
        int64_t first, count, lds;
        int tier, slot;
    };
    std::vector<Group> groups;
    // a ragged batch (lpg_batch_create_ragged): m, ncols, ld and lds above are the
    // largest of any LP, tier is TIER_GLOBAL if any LP is on it
    bool ragged = false;
    std::vector<BatchShape> shape;            // the records, as in dshape
    std::vector<lpg_batch_shape_t> pub;       // what lpg_batch_shape reports, packed offsets included
    int64_t t_total = 0, b_total = 0, c_total = 0;   // doubles of T, entries of basis, doubles of cost
    BatchShape *dshape = nullptr;
    int32_t *dorder = nullptr;
};

constexpr int kBatchSlots = 2;                // ints behind lpg_batch::running: group 0 (global tier) and group 1 (LDS tier)

namespace {

BatchGeo bgeo(const lpg_batch *b) {
    BatchGeo g{};
    g.T = b->T;
    g.basis = b->basis;
    g.lp = b->lp;
    g.logk = b->logk;
    g.logr = b->logr;
    g.running = b->running;
    g.ld = b->ld;
    g.m = b->m;
    g.ncols = b->ncols;
    g.nact = b->nact;
    g.logcap = b->logcap;
    g.eps_piv = b->eps_piv;
    g.eps_opt = b->eps_opt;
    g.chunk = b->chunk;
    g.pitch = b->pitch;
    g.txs = b->txs;
    g.nobj = b->nobj;
    g.shape = b->dshape;
    g.order = b->dorder;
    return g;
}

// the geometry a launch of group `gr` sees: its slice of the order, its counter
BatchGeo bgeo(const lpg_batch *b, const lpg_batch::Group &gr) {
    BatchGeo g = bgeo(b);
    if (g.order) g.order += gr.first;
    g.running += gr.slot;
    return g;
}

// dynamic LDS of one workgroup: [tableau of m + nobj rows at an odd pitch] P C [int32 basis]
int64_t lds_bytes(int tier, int64_t m, int64_t ncols, int nobj) {
    const int64_t rows = m + nobj, pitch = ncols | 1;
    int64_t d = ncols + rows;
    if (tier == TIER_LDS) d += rows * pitch + (m + 1) / 2;
    return d * (int64_t)sizeof(double);
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int range_ok(lpg_batch *b, const char *what, int64_t first, int64_t n) {
    if (first < 0 || n < 0 || first > b->count || n > b->count - first)
        return fail(b, LPG_ERR_ARG, "%s: LPs [%lld, %lld) outside the batch of %lld", what, (long long)first,
                    (long long)(first + n), (long long)b->count);
    return 0;
}

int alloc_log(lpg_batch *b, int64_t cap) {
    if (b->logk) (void)hipFree(b->logk);
    if (b->logr) (void)hipFree(b->logr);
    b->logk = b->logr = nullptr;
    b->logcap = 0;
    if ((b->flags & LPG_FLAG_NO_LOG) || cap == 0) return 0;
    const size_t bytes = (size_t)b->count * (size_t)cap * sizeof(int32_t);
    if (hipMalloc(&b->logk, bytes) != hipSuccess || hipMalloc(&b->logr, bytes) != hipSuccess) {
        (void)hipGetLastError();
        if (b->logk) (void)hipFree(b->logk);
        b->logk = b->logr = nullptr;
        return fail(b, LPG_ERR_OOM, "hipMalloc(pivot log, 2 x %zu bytes) failed", bytes);
    }
    b->logcap = cap;
    return 0;
}

// which solver a call runs
enum Method { M_PRIMAL, M_DUAL, M_TWO_PHASE, M_BIG_M, M_GOAL };

// the dynamic LDS limit of kernel K (`name` for the error message) raised to `bytes`, once per device
template <auto K>
int raise_lds(lpg_batch *b, const char *name, int bytes = kBatchMaxLds) {
    static std::atomic<unsigned long long> attr{0};
    const int dev = b->device & 63;
    if (!((attr.load(std::memory_order_acquire) >> dev) & 1ull)) {
        if (hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(b, LPG_ERR_DEVICE, "hipFuncSetAttribute(%s, %d bytes of LDS) failed", name, bytes);
        }
        attr.fetch_or(1ull << dev, std::memory_order_acq_rel);
    }
    return 0;
}

// one launch of solve kernel K (`name` for the error message) on group `gr`,
// one workgroup per LP; its dynamic LDS limit is raised once per device
template <auto K, class... Args>
int launch_lp(lpg_batch *b, const lpg_batch::Group &gr, const char *name, const Args &...args) {
    if (int rc = raise_lds<K>(b, name)) return rc;
    hipLaunchKernelGGL(K, dim3((unsigned)gr.count), dim3(kBlock), (size_t)gr.lds, b->stream, bgeo(b, gr), args...);
    return 0;
}

template <int TIER, bool RG>
int launch_tier(lpg_batch *b, const lpg_batch::Group &gr, Method method, int rule, const TwoPhase &t) {
    const bool bland = rule == RULE_BLAND;
    switch (method) {
    case M_DUAL: return launch_lp<k_batch_solve<MODE_DUAL, TIER, RG>>(b, gr, "k_batch_solve");
    case M_PRIMAL:
        return bland ? launch_lp<k_batch_solve<RULE_BLAND, TIER, RG>>(b, gr, "k_batch_solve")
                     : launch_lp<k_batch_solve<RULE_DANTZIG, TIER, RG>>(b, gr, "k_batch_solve");
    case M_TWO_PHASE:
        return bland ? launch_lp<k_batch_two_phase<RULE_BLAND, TIER, RG>>(b, gr, "k_batch_two_phase", t)
                     : launch_lp<k_batch_two_phase<RULE_DANTZIG, TIER, RG>>(b, gr, "k_batch_two_phase", t);
    default:
        return bland ? launch_lp<k_batch_big_m<RULE_BLAND, TIER, RG>>(b, gr, "k_batch_big_m", t)
                     : launch_lp<k_batch_big_m<RULE_DANTZIG, TIER, RG>>(b, gr, "k_batch_big_m", t);
    }
}

template <int TIER>
int launch_goal(lpg_batch *b, const lpg_batch::Group &gr, int rule, const GoalArgs &a) {
    return rule == RULE_BLAND ? launch_lp<k_batch_goal<RULE_BLAND, TIER>>(b, gr, "k_batch_goal", a)
                              : launch_lp<k_batch_goal<RULE_DANTZIG, TIER>>(b, gr, "k_batch_goal", a);
}

int launch_solve(lpg_batch *b, const lpg_batch::Group &gr, Method method, int rule, const TwoPhase &t) {
    if (method == M_GOAL) {
        const GoalArgs a{b->cost, b->attain};
        return gr.tier == TIER_LDS ? launch_goal<TIER_LDS>(b, gr, rule, a) : launch_goal<TIER_GLOBAL>(b, gr, rule, a);
    }
    if (b->ragged)
        return gr.tier == TIER_LDS ? launch_tier<TIER_LDS, true>(b, gr, method, rule, t)
                                   : launch_tier<TIER_GLOBAL, true>(b, gr, method, rule, t);
    return gr.tier == TIER_LDS ? launch_tier<TIER_LDS, false>(b, gr, method, rule, t)
                               : launch_tier<TIER_GLOBAL, false>(b, gr, method, rule, t);
}

// what the calls of the other layout answer: a uniform-layout call on a ragged
// batch, or a packed / _ragged call on a batch of one shape
int wrong_layout(lpg_batch *b, const char *call, const char *other) {
    if (b->ragged)
        return fail(b, LPG_ERR_STATE, "%s: this is a ragged batch (lpg_batch_create_ragged), whose LPs have no common "
                                      "shape; use %s; nothing has moved or pivoted", call, other);
    return fail(b, LPG_ERR_STATE, "%s: this batch has one shape (lpg_batch_create, lpg_batch_create_big_m); use %s; "
                                  "nothing has moved or pivoted", call, other);
}

// a plain batch: neither Big-M nor goal
bool plain(const lpg_batch *b) { return b->nobj == 1 && !b->goal; }

// what a Big-M batch and a goal batch refuse (and a plain batch, for lpg_batch_solve_big_m)
int wrong_kind(lpg_batch *b, const char *call) {
    if (b->goal)
        return fail(b, LPG_ERR_STATE, "%s: this is a goal batch (lpg_batch_create_goal, %d objective rows); only "
                                      "lpg_batch_solve_goal pivots it, and lpg_batch_load, _get_rows, _get_basis, _get_log, "
                                      "_info and _set_tolerances serve it; nothing has moved or pivoted", call, b->nobj);
    if (b->nobj == 2)
        return fail(b, LPG_ERR_STATE, "%s: this is a Big-M batch (lpg_batch_create_big_m, two objective rows); only "
                                      "lpg_batch_solve_big_m pivots it; nothing has pivoted", call);
    return fail(b, LPG_ERR_STATE, "%s: the batch has one objective row (lpg_batch_create); Big-M needs a batch from "
                                  "lpg_batch_create_big_m; nothing has pivoted", call);
}

// the batch's count x N cost buffer, filled from the host's (pitch ld_cost) when given;
// ragged: the packed costs, ncols - 1 per LP, the same on both sides
int stage_costs(lpg_batch *b, const double *cost, int64_t ld_cost) {
    const int64_t N = b->ncols - 1;
    const size_t total = b->ragged ? (size_t)b->c_total : (size_t)b->count * (size_t)N;
    if (!b->cost && hipMalloc(&b->cost, total * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        b->cost = nullptr;
        return fail(b, LPG_ERR_OOM, "hipMalloc(costs of %lld LPs) failed", (long long)b->count);
    }
    if (cost && b->ragged)
        LPG_HIPCHK(b, hipMemcpyAsync(b->cost, cost, total * sizeof(double), hipMemcpyHostToDevice, b->stream));
    else if (cost)
        LPG_HIPCHK(b, hipMemcpy2DAsync(b->cost, (size_t)N * sizeof(double), cost, (size_t)ld_cost * sizeof(double),
                                    (size_t)N * sizeof(double), (size_t)b->count, hipMemcpyHostToDevice, b->stream));
    if (cost) LPG_HIPCHK(b, hipStreamSynchronize(b->stream));        // the caller's array is free again
    return 0;
}

// one solve call: `method` with `rule` (M_DUAL: RULE_DANTZIG); `t` for M_TWO_PHASE and M_BIG_M
int batch_run(lpg_batch *b, int64_t max_pivots, Method method, int rule, lpg_result *out, const TwoPhase &t = {}) {
    if (!b) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "batch is NULL");
    if (max_pivots < 0) return fail(b, LPG_ERR_ARG, "max_pivots < 0");
    LPG_HIPCHK(b, hipSetDevice(b->device));
    if (method == M_DUAL) {
        const unsigned long long none = ~0ull;
        unsigned long long bad = none;
        LPG_HIPCHK(b, hipMemcpyAsync(b->bad, &none, sizeof none, hipMemcpyHostToDevice, b->stream));
        hipLaunchKernelGGL(k_batch_dual_check, dim3((unsigned)b->count), dim3(kBlock), 0, b->stream, bgeo(b), b->bad);
        LPG_HIPCHK(b, hipGetLastError());
        LPG_HIPCHK(b, hipMemcpyAsync(&bad, b->bad, sizeof bad, hipMemcpyDeviceToHost, b->stream));
        LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
        if (bad != none)
            return fail(b, LPG_ERR_STATE, "lpg_batch_solve_dual: LP %llu is not dual feasible (a d_j < -eps_opt); "
                                          "nothing has pivoted", bad);
    }
    // every launch spends `chunk` of each running LP's budget (or ends the LP)
    int64_t max_launches = max_pivots / b->chunk + 2;
    if (method == M_TWO_PHASE) {
        // both phases have a budget of up to max_pivots, and the drive-out
        // pivots (at most m) and the two objectives are work as well
        max_launches = 2 * std::min<int64_t>(max_pivots / b->chunk, (int64_t)1 << 60) + (b->m + 2) / b->chunk + 4;
    } else if (method == M_BIG_M || method == M_GOAL) {
        max_launches = max_pivots / b->chunk + 4;                 // the pivots and one objective unit
    }
    if (method == M_TWO_PHASE || method == M_BIG_M || method == M_GOAL)
        hipLaunchKernelGGL(k_batch_begin_two_phase, dim3(blocks_for(b->count)), dim3(kBlock), 0, b->stream, b->lp,
                           b->count, max_pivots);
    else
        hipLaunchKernelGGL(k_batch_begin, dim3(blocks_for(b->count)), dim3(kBlock), 0, b->stream, b->lp, b->count,
                           max_pivots, method == M_DUAL ? 1 : 0);
    LPG_HIPCHK(b, hipGetLastError());
    b->pivoted = true;
    // a round: one launch per group that still has running LPs; the counters are
    // reset once before it and read once after it
    int32_t live[kBatchSlots];
    const size_t nslots = (size_t)b->groups.back().slot + 1;
    for (int64_t it = 0;; it++) {
        LPG_HIPCHK(b, hipMemsetAsync(b->running, 0, nslots * sizeof(int32_t), b->stream));
        for (const lpg_batch::Group &gr : b->groups) {
            if (it > 0 && live[gr.slot] == 0) continue;
            if (int rc = launch_solve(b, gr, method, rule, t)) return rc;
            LPG_HIPCHK(b, hipGetLastError());
        }
        LPG_HIPCHK(b, hipMemcpyAsync(live, b->running, nslots * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
        LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
        int64_t running = 0;
        for (size_t q = 0; q < nslots; q++) running += live[q];
        if (running == 0) break;
        if (it + 1 >= max_launches)
            return fail(b, LPG_ERR_DEVICE, "lpg_batch: %lld LPs still running after %lld rounds of %d pivots",
                        (long long)running, (long long)(it + 1), b->chunk);
    }
    if (out) {
        std::vector<BatchLP> h((size_t)b->count);
        LPG_HIPCHK(b, hipMemcpy(h.data(), b->lp, h.size() * sizeof(BatchLP), hipMemcpyDeviceToHost));
        for (int64_t q = 0; q < b->count; q++) {
            out[q].status = h[q].status;
            out[q].rule = rule == RULE_BLAND ? LPG_RULE_BLAND : LPG_RULE_DANTZIG;
            out[q].pivots = h[q].pivots;
            out[q].objective = h[q].objective;
            out[q].entering = h[q].last_k;
            out[q].leaving = h[q].last_r;
        }
    }
    return 0;
}

// the records of a ragged batch to the device (after nact or art_first changed)
int push_shapes(lpg_batch *b) {
    LPG_HIPCHK(b, hipMemcpy(b->dshape, b->shape.data(), b->shape.size() * sizeof(BatchShape), hipMemcpyHostToDevice));
    return 0;
}

// lpg_batch_solve_two_phase and lpg_batch_solve_big_m (M_TWO_PHASE, M_BIG_M; art_first points to the one
// value, cost has pitch ld_cost) and their _ragged forms (`packed`: one art_first per LP, packed costs);
// `call` names the entry point
int solve_artificial(lpg_batch *b, Method method, const char *call, bool packed, const int64_t *art_first,
                     const double *cost, int64_t ld_cost, int64_t max_pivots, int rule, lpg_result *out) {
    if (!b) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "batch is NULL");
    if (b->goal || (b->nobj == 2) != (method == M_BIG_M)) return wrong_kind(b, call);
    if (b->ragged != packed) {
        if (packed) return wrong_layout(b, call, method == M_BIG_M ? "lpg_batch_solve_big_m" : "lpg_batch_solve_two_phase");
        return wrong_layout(b, call, method == M_BIG_M ? "lpg_batch_solve_big_m_ragged" : "lpg_batch_solve_two_phase_ragged");
    }
    const int64_t N = b->ncols - 1;
    if (packed) {
        if (!art_first) return fail(b, LPG_ERR_ARG, "%s: art_first is NULL", call);
        for (int64_t q = 0; q < b->count; q++)
            if (art_first[q] < 2 || art_first[q] > b->shape[(size_t)q].ncols - 1)
                return fail(b, LPG_ERR_ARG, "%s: art_first %lld of LP %lld outside 2..%lld", call, (long long)art_first[q],
                            (long long)q, (long long)(b->shape[(size_t)q].ncols - 1));
    } else if (*art_first < 2 || *art_first > N) {
        return fail(b, LPG_ERR_ARG, "%s: art_first %lld outside 2..%lld", call, (long long)*art_first, (long long)N);
    }
    if (rule != LPG_RULE_DANTZIG && rule != LPG_RULE_BLAND) return fail(b, LPG_ERR_ARG, "%s: rule %d", call, rule);
    if (!packed && cost && ld_cost < N)
        return fail(b, LPG_ERR_ARG, "%s: ld_cost %lld < N = %lld", call, (long long)ld_cost, (long long)N);
    if (max_pivots < 0) return fail(b, LPG_ERR_ARG, "%s: max_pivots < 0", call);
    LPG_HIPCHK(b, hipSetDevice(b->device));
    if (int rc = stage_costs(b, cost, ld_cost)) return rc;
    TwoPhase t{};
    t.cost = b->cost;
    t.max_pivots = max_pivots;
    t.save_cost = cost ? 0 : 1;
    // two-phase: nact is what phase II prices, and what a later lpg_batch_solve goes on with; Big-M prices all of 1..N
    if (packed) {
        for (int64_t q = 0; q < b->count; q++) {
            b->shape[(size_t)q].art_first = (int32_t)art_first[q];
            if (method == M_TWO_PHASE) b->shape[(size_t)q].nact = (int32_t)art_first[q] - 1;
        }
        if (int rc = push_shapes(b)) return rc;
    } else {
        t.art_first = *art_first;
        if (method == M_TWO_PHASE) b->nact = *art_first - 1;
    }
    return batch_run(b, max_pivots, method, rule, out, t);
}

// lpg_batch_generate and lpg_batch_generate_artificial once the arguments are checked
int generate(lpg_batch *b, int64_t n, uint64_t seed, int kind) {
    LPG_HIPCHK(b, hipSetDevice(b->device));
    hipLaunchKernelGGL(k_batch_generate, dim3((unsigned)(b->count * (b->m + b->nobj))), dim3(kBlock), 0, b->stream, bgeo(b),
                       n, seed, kind);
    hipLaunchKernelGGL(k_batch_reset, dim3(blocks_for(b->count)), dim3(kBlock), 0, b->stream, b->lp, (int64_t)0, b->count);
    LPG_HIPCHK(b, hipGetLastError());
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    b->pivoted = false;
    return 0;
}

// env LPG_BATCH_CHUNK into *chunk (0: not set)
int env_chunk(int *chunk) {
    *chunk = 0;
    if (const char *ce = getenv("LPG_BATCH_CHUNK")) {
        const long long v = atoll(ce);
        if (v < 1 || v > (1 << 20))
            return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "LPG_BATCH_CHUNK=%s out of range [1, %d]", ce, 1 << 20);
        *chunk = (int)v;
    }
    return 0;
}

// a launch stays bounded in time as well as in pivots: the LDS tier spends
// microseconds per pivot; a global-tier workgroup streams its tableau twice
// per pivot at some tens of GB/s, so large tableaus get fewer pivots per
// launch (about 0.1 s at 50 GB/s). rows x ncols: the largest global-tier LP.
int default_chunk(bool any_global, int64_t rows, int64_t ncols) {
    if (!any_global) return kBatchChunk;
    const double per_pivot = 16.0 * (double)rows * (double)ncols / 50e9;
    return (int)std::min<double>(kBatchChunk, std::max(16.0, 0.1 / per_pivot));
}

int txs_of(int64_t ncols) {
    int txs = 0;
    while ((1 << txs) < ncols && txs < 8) txs++;
    return txs;
}

// The device side of a batch whose host fields are set (t_total, b_total, the
// log capacity `logcap`, for a ragged batch shape and `order`): allocations,
// stream, zero tableaus (the padding columns stay zero for good), slack-less
// bases, fresh states. On failure the batch is destroyed.
int batch_alloc(lpg_batch **out, lpg_batch *b, int64_t logcap, const std::vector<int32_t> &order) {
    auto die = [&](int code) {
        snprintf(thread_err<lpg_batch>(), kErrLen, "%s", b->err);
        lpg_batch_destroy(b);
        return code;
    };
    const int64_t count = b->count;
    hipError_t e = hipSetDevice(b->device);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fail(b, LPG_ERR_DEVICE, "hipSetDevice(%d): %s", b->device, hipGetErrorString(e));
        return die(LPG_ERR_DEVICE);
    }
    const size_t tbytes = (size_t)b->t_total * sizeof(double), bbytes = (size_t)b->b_total * sizeof(int64_t);
    if (hipMalloc(&b->T, tbytes) != hipSuccess || hipMalloc(&b->basis, bbytes) != hipSuccess ||
        hipMalloc(&b->lp, (size_t)count * sizeof(BatchLP)) != hipSuccess ||
        hipMalloc(&b->running, kBatchSlots * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&b->bad, sizeof(unsigned long long)) != hipSuccess ||
        (b->ragged && (hipMalloc(&b->dshape, (size_t)count * sizeof(BatchShape)) != hipSuccess ||
                       hipMalloc(&b->dorder, (size_t)count * sizeof(int32_t)) != hipSuccess))) {
        (void)hipGetLastError();
        fail(b, LPG_ERR_OOM, "hipMalloc(batch of %lld tableaus, %zu bytes) failed", (long long)count, tbytes);
        return die(LPG_ERR_OOM);
    }
    if (int rc = alloc_log(b, logcap)) return die(rc);
    if ((e = hipStreamCreate(&b->stream)) != hipSuccess) {
        (void)hipGetLastError();
        fail(b, LPG_ERR_DEVICE, "hipStreamCreate: %s", hipGetErrorString(e));
        return die(LPG_ERR_DEVICE);
    }
    if (hipMemsetAsync(b->T, 0, tbytes, b->stream) != hipSuccess ||
        hipMemsetAsync(b->basis, 0, bbytes, b->stream) != hipSuccess) {
        (void)hipGetLastError();
        fail(b, LPG_ERR_DEVICE, "hipMemset failed");
        return die(LPG_ERR_DEVICE);
    }
    if (b->ragged &&
        (hipMemcpyAsync(b->dshape, b->shape.data(), (size_t)count * sizeof(BatchShape), hipMemcpyHostToDevice, b->stream) !=
             hipSuccess ||
         hipMemcpyAsync(b->dorder, order.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, b->stream) !=
             hipSuccess)) {
        (void)hipGetLastError();
        fail(b, LPG_ERR_DEVICE, "hipMemcpy(shapes of %lld LPs) failed", (long long)count);
        return die(LPG_ERR_DEVICE);
    }
    hipLaunchKernelGGL(k_batch_reset, dim3(blocks_for(count)), dim3(kBlock), 0, b->stream, b->lp, (int64_t)0, count);
    if ((e = hipStreamSynchronize(b->stream)) != hipSuccess || (e = hipGetLastError()) != hipSuccess) {
        fail(b, LPG_ERR_DEVICE, "batch setup: %s", hipGetErrorString(e));
        return die(LPG_ERR_DEVICE);
    }
    *out = b;
    return 0;
}

// lpg_batch_create (nobj = 1), lpg_batch_create_big_m (nobj = 2) and lpg_batch_create_goal (`goal`, nobj = K);
// `call` names the entry point
int batch_create(lpg_batch **out, int device, int64_t count, int64_t m, int64_t ncols, uint32_t flags, int nobj,
                 const char *call, bool goal = false) {
    if (!out) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (count < 1 || m < 1 || ncols < 2)
        return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: bad shape count=%lld m=%lld ncols=%lld (need count >= 1, "
                                                     "m >= 1, ncols >= 2)", call, (long long)count, (long long)m, (long long)ncols);
    if (flags & ~(uint32_t)LPG_FLAG_NO_LOG)
        return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: flags 0x%x not supported (LPG_FLAG_NO_LOG only: a Big-M batch comes from "
                                                     "lpg_batch_create_big_m; no eager or no-skip batches)", call, flags);
    if (m + nobj > LPG_BATCH_MAX_DIM || ncols > LPG_BATCH_MAX_DIM)
        return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: m + %d = %lld, ncols = %lld exceed %d; a tableau this large "
                                                     "belongs to lpg_create", call, nobj, (long long)(m + nobj), (long long)ncols,
                               LPG_BATCH_MAX_DIM);
    if (device < 0) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: device %d", call, device);
    const int64_t rows = m + nobj, ld = (ncols + 63) & ~(int64_t)63;   // the engine's padded pitch (512-byte rows)
    if (count > (int64_t)0x7fffffff / rows)
        return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: count * (m + %d) = %lld x %lld exceeds 2^31 - 1", call, nobj,
                               (long long)count, (long long)rows);
    int chunk = 0;
    if (int rc = env_chunk(&chunk)) return rc;
    lpg_batch *b = new lpg_batch();
    b->device = device;
    b->count = count;
    b->m = m;
    b->ncols = ncols;
    b->ld = ld;
    b->nact = ncols - 1;
    b->nobj = nobj;
    b->goal = goal;
    b->flags = flags;
    const bool force_global = env_is("LPG_BATCH_TIER", "global");
    b->tier = (!force_global && lds_bytes(TIER_LDS, m, ncols, nobj) <= kBatchMaxLds) ? TIER_LDS : TIER_GLOBAL;
    b->lds = lds_bytes(b->tier, m, ncols, nobj);
    b->pitch = (int)(ncols | 1);
    b->txs = txs_of(ncols);
    b->chunk = chunk ? chunk : default_chunk(b->tier == TIER_GLOBAL, rows, ncols);
    b->groups.push_back({0, count, b->lds, b->tier, 0});
    b->t_total = count * rows * ld;
    b->b_total = count * m;
    return batch_alloc(out, b, 2 * (m + ncols), {});
}

int ragged_create(lpg_batch **out, int device, int64_t count, const int64_t *m, const int64_t *ncols, int nobj,
                  uint32_t flags) {
    const char *call = "lpg_batch_create_ragged";
    if (!out) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!m || !ncols) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: %s is NULL", call, !m ? "m" : "ncols");
    if (count < 1) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: count = %lld (need count >= 1)", call, (long long)count);
    if (nobj != 1 && nobj != 2)
        return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: nobj = %d (1: a plain batch, 2: a Big-M batch)", call, nobj);
    if (flags & ~(uint32_t)LPG_FLAG_NO_LOG)
        return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: flags 0x%x not supported (LPG_FLAG_NO_LOG only: nobj = 2 makes a Big-M "
                                                     "batch; no eager or no-skip batches)", call, flags);
    if (device < 0) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: device %d", call, device);
    int64_t sum_rows = 0;
    for (int64_t q = 0; q < count; q++) {
        if (m[q] < 1)
            return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: LP %lld: m = %lld (need m >= 1)", call, (long long)q,
                                   (long long)m[q]);
        if (ncols[q] < 2)
            return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: LP %lld: ncols = %lld (need ncols >= 2)", call, (long long)q,
                                   (long long)ncols[q]);
        if (m[q] + nobj > LPG_BATCH_MAX_DIM)
            return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: LP %lld: m + %d = %lld exceeds %d; a tableau this large belongs to "
                                                         "lpg_create", call, (long long)q, nobj, (long long)(m[q] + nobj),
                                   LPG_BATCH_MAX_DIM);
        if (ncols[q] > LPG_BATCH_MAX_DIM)
            return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: LP %lld: ncols = %lld exceeds %d; a tableau this large belongs to "
                                                         "lpg_create", call, (long long)q, (long long)ncols[q], LPG_BATCH_MAX_DIM);
        sum_rows += m[q] + nobj;
        if (sum_rows > (int64_t)0x7fffffff)
            return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: LP %lld: the rows of LPs 0..%lld (m + %d each) exceed 2^31 - 1", call,
                                   (long long)q, (long long)q, nobj);
    }
    int chunk = 0;
    if (int rc = env_chunk(&chunk)) return rc;
    const bool force_global = env_is("LPG_BATCH_TIER", "global");

    lpg_batch *b = new lpg_batch();
    b->device = device;
    b->count = count;
    b->nobj = nobj;
    b->flags = flags;
    b->ragged = true;
    b->tier = TIER_LDS;
    b->shape.resize((size_t)count);
    b->pub.resize((size_t)count);
    int64_t big_global = 0, grows = 0, gncols = 0, pt = 0;
    for (int64_t q = 0; q < count; q++) {
        BatchShape &s = b->shape[(size_t)q];
        lpg_batch_shape_t &p = b->pub[(size_t)q];
        const int64_t rows = m[q] + nobj, ld = (ncols[q] + 63) & ~(int64_t)63;
        s = BatchShape{};
        s.t_off = b->t_total;
        s.b_off = b->b_total;
        s.c_off = b->c_total;
        s.m = (int32_t)m[q];
        s.ncols = (int32_t)ncols[q];
        s.ld = (int32_t)ld;
        s.pitch = (int32_t)(ncols[q] | 1);
        s.txs = txs_of(ncols[q]);
        s.nact = (int32_t)ncols[q] - 1;
        s.art_first = (int32_t)ncols[q];           // no artificial column until a call names one
        p.m = m[q];
        p.ncols = ncols[q];
        p.ld = ld;
        p.tier = (!force_global && lds_bytes(TIER_LDS, m[q], ncols[q], nobj) <= kBatchMaxLds) ? TIER_LDS : TIER_GLOBAL;
        p.lds_bytes = lds_bytes(p.tier, m[q], ncols[q], nobj);
        p.group = p.tier == TIER_GLOBAL ? 0 : 1;
        p.tableau_offset = pt;
        p.basis_offset = b->b_total;
        p.cost_offset = b->c_total;
        pt += rows * ncols[q];
        b->t_total += rows * ld;
        b->b_total += m[q];
        b->c_total += ncols[q] - 1;
        b->m = std::max(b->m, m[q]);
        b->ncols = std::max(b->ncols, ncols[q]);
        b->ld = std::max(b->ld, ld);
        b->lds = std::max(b->lds, p.lds_bytes);
        if (p.tier == TIER_GLOBAL) {
            b->tier = TIER_GLOBAL;
            if (rows * ncols[q] > big_global) big_global = rows * ncols[q], grows = rows, gncols = ncols[q];
        }
    }
    b->nact = b->ncols - 1;
    b->chunk = chunk ? chunk : default_chunk(b->tier == TIER_GLOBAL, grows, gncols);
    // the order of the workgroups: the global-tier group, then the LDS-tier group
    // (launched with the LDS of its largest LP; one group per occupancy class was
    // measured and not kept), in a group the LPs with the most
    // update work first, so that the round's tail is short
    std::vector<int32_t> order((size_t)count);
    for (int64_t q = 0; q < count; q++) order[(size_t)q] = (int32_t)q;
    std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        const lpg_batch_shape_t &px = b->pub[(size_t)x], &py = b->pub[(size_t)y];
        if (px.group != py.group) return px.group < py.group;
        const int64_t wx = (px.m + nobj) * px.ncols, wy = (py.m + nobj) * py.ncols;
        return wx != wy ? wx > wy : x < y;
    });
    for (int64_t w = 0; w < count; w++) {
        const lpg_batch_shape_t &p = b->pub[(size_t)order[(size_t)w]];
        if (b->groups.empty() || b->groups.back().slot != p.group) b->groups.push_back({w, 0, 0, p.tier, p.group});
        b->groups.back().count++;
        b->groups.back().lds = std::max(b->groups.back().lds, p.lds_bytes);
    }
    return batch_alloc(out, b, 2 * (b->m + b->ncols), order);
}

// m, ncols and active columns of LP q, whatever the layout
int64_t lp_m(const lpg_batch *b, int64_t q) { return b->ragged ? b->shape[(size_t)q].m : b->m; }
int64_t lp_ncols(const lpg_batch *b, int64_t q) { return b->ragged ? b->shape[(size_t)q].ncols : b->ncols; }
int64_t lp_nact(const lpg_batch *b, int64_t q) { return b->ragged ? b->shape[(size_t)q].nact : b->nact; }

// a device buffer of a branching call: freed when the call returns
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

// the mask checks of the calls that take one, once the batch is known
int mask_ok(lpg_batch *b, const char *call, int64_t nmask, int64_t ld_mask) {
    if (nmask < 1 || nmask > b->ncols - 1)
        return fail(b, LPG_ERR_ARG, "%s: nmask %lld outside 1..%lld (the columns of the %s)", call, (long long)nmask,
                    (long long)(b->ncols - 1), b->ragged ? "widest LP" : "batch");
    if (ld_mask != 0 && ld_mask < nmask)
        return fail(b, LPG_ERR_ARG, "%s: ld_mask %lld < nmask %lld (0: one mask for every LP)", call, (long long)ld_mask,
                    (long long)nmask);
    return 0;
}

// The masks of a call on the device, for the kernels that read mask[q * pitch + j - 1] for j <= nmask only:
// `count` masks packed at pitch nmask, or the one for all at pitch 0 (ld_mask = 0), uploaded on `stream`.
// hipErrorOutOfMemory: the allocation failed (the caller's message names what it allocates beside it).
hipError_t stage_mask(DevBuf &dmask, int64_t &pitch, const uint8_t *mask, int64_t nmask, int64_t ld_mask, int64_t count,
                      hipStream_t stream) {
    const int64_t nrows = ld_mask ? count : 1;
    pitch = ld_mask ? nmask : 0;
    if (hipMalloc(&dmask.p, (size_t)(nrows * nmask)) != hipSuccess) return hipErrorOutOfMemory;
    return hipMemcpy2DAsync(dmask.p, (size_t)nmask, mask, (size_t)(ld_mask ? ld_mask : nmask), (size_t)nmask, (size_t)nrows,
                            hipMemcpyHostToDevice, stream);
}

// src[c] of lpg_batch_branch and lpg_batch_cut names an LP of the parent
int src_ok(lpg_batch *p, const char *call, int64_t c, int64_t src) {
    if (src < 0 || src >= p->count)
        return fail(p, LPG_ERR_ARG, "%s: src[%lld] = %lld outside the parent's LPs 0..%lld", call, (long long)c, (long long)src,
                    (long long)(p->count - 1));
    return 0;
}

// a child batch that will not be returned: its message to the parent and the thread, and away with it
int child_die(lpg_batch *p, lpg_batch *ch, int code) {
    snprintf(thread_err<lpg_batch>(), kErrLen, "%s", ch->err);
    snprintf(p->err, sizeof p->err, "%s", ch->err);
    lpg_batch_destroy(ch);
    return code;
}

// The child batch of lpg_batch_branch and lpg_batch_cut (`call`), its tableaus still zero: child c is LP src[c]
// of `p` (checked) with k[c] more rows, columns and active columns, in a batch of the parent's flags and
// tolerances; ragged when the parent is or the k[c] differ
int grow_create(lpg_batch **out, lpg_batch *p, const char *call, int64_t n, const int64_t *src, const int64_t *k) {
    const bool ragged = p->ragged || !std::all_of(k, k + n, [&](int64_t x) { return x == k[0]; });
    lpg_batch *ch = nullptr;
    int rc;
    if (ragged) {
        std::vector<int64_t> ms((size_t)n), ncs((size_t)n);
        for (int64_t c = 0; c < n; c++) ms[(size_t)c] = lp_m(p, src[c]) + k[c], ncs[(size_t)c] = lp_ncols(p, src[c]) + k[c];
        rc = ragged_create(&ch, p->device, n, ms.data(), ncs.data(), 1, p->flags);
    } else {
        rc = batch_create(&ch, p->device, n, p->m + k[0], p->ncols + k[0], p->flags, 1, call);
    }
    if (rc) return fail(p, rc, "%s: the child batch: %s", call, thread_err<lpg_batch>());
    ch->eps_piv = p->eps_piv;
    ch->eps_opt = p->eps_opt;
    if (ragged) {
        // a parent of one shape records no art_first (lpg_batch_active_columns: ncols), and neither does its child
        for (int64_t c = 0; c < n; c++) {
            ch->shape[(size_t)c].nact = (int32_t)(lp_nact(p, src[c]) + k[c]);
            if (p->ragged) ch->shape[(size_t)c].art_first = p->shape[(size_t)src[c]].art_first + (int32_t)k[c];
        }
        if ((rc = push_shapes(ch))) return child_die(p, ch, rc);
    } else {
        ch->nact = p->nact + k[0];
    }
    *out = ch;
    return 0;
}

// The end of lpg_batch_branch and lpg_batch_cut: the jobs to `djobs`, kernel KU (a parent of one shape) or KR
// (a ragged one) with one workgroup per child and `lds` bytes of dynamic LDS, the wait for it. `e`: what the
// caller's own uploads on the child's stream returned. The child goes to *out, or on an error away.
template <auto KU, auto KR, class Job, class... Args>
int grow_finish(lpg_batch **out, lpg_batch *p, lpg_batch *ch, const char *call, hipError_t e, const std::vector<Job> &jobs,
                const DevBuf &djobs, size_t lds, const Args &...args) {
    // the parent's stream is idle (every call on it ends with a synchronisation); the copy runs on the child's
    if (e == hipSuccess)
        e = hipMemcpyAsync(djobs.p, jobs.data(), jobs.size() * sizeof(Job), hipMemcpyHostToDevice, ch->stream);
    if (e == hipSuccess) {
        const dim3 grid((unsigned)jobs.size()), block(kBlock);
        if (p->ragged) hipLaunchKernelGGL(KR, grid, block, lds, ch->stream, bgeo(p), bgeo(ch), (const Job *)djobs.p, args...);
        else hipLaunchKernelGGL(KU, grid, block, lds, ch->stream, bgeo(p), bgeo(ch), (const Job *)djobs.p, args...);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ch->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fail(ch, LPG_ERR_DEVICE, "%s: %s", call, hipGetErrorString(e));
        return child_die(p, ch, LPG_ERR_DEVICE);
    }
    *out = ch;
    return 0;
}

// how scenario_column walks the tableau: a lane per row, the faster of the two where measured (DESIGN.md §3.7,
// "Scenarios"); LPG_SCENARIO_WALK=tile: the tiled walk
int scenario_walk() { return env_is("LPG_SCENARIO_WALK", "tile") ? WALK_TILE : WALK_ROWS; }

// dynamic LDS of a scenario workgroup: the right-hand side and the ident columns of an LP of m rows
// (scenario_stage), and the most of it (beside the static tile of scenario_column it stays under the CU's LDS)
size_t scenario_lds(int64_t m) { return (size_t)m * (sizeof(double) + sizeof(int32_t)); }
constexpr int kScenarioMaxLds = LPG_BATCH_MAX_DIM * (int)(sizeof(double) + sizeof(int32_t));

// dynamic LDS of a ranging workgroup: a double and an int32 per column in the cost phase, per row in the
// right-hand-side phase, in the same bytes (k_batch_ranging); `dim` the larger of the batch's m and ncols
size_t ranging_lds(int64_t dim) { return (size_t)dim * (sizeof(double) + sizeof(int32_t)); }
constexpr int kRangingMaxLds = LPG_BATCH_MAX_DIM * (int)(sizeof(double) + sizeof(int32_t));

// every ident entry of every LP of `b` names one of its columns 1..N
int ident_ok(lpg_batch *b, const char *call, const int64_t *ident) {
    for (int64_t q = 0, at = 0; q < b->count; q++)
        for (int64_t i = 0, m = lp_m(b, q), N = lp_ncols(b, q) - 1; i < m; i++, at++)
            if (ident[at] < 1 || ident[at] > N)
                return fail(b, LPG_ERR_ARG, "%s: ident[%lld] = %lld (row %lld of LP %lld) outside the columns 1..%lld", call,
                            (long long)at, (long long)ident[at], (long long)i, (long long)q, (long long)N);
    return 0;
}

// rhs[at .. at + m) is finite; `whose` names the LP or child it belongs to
int rhs_ok(lpg_batch *b, const char *call, const double *rhs, int64_t at, int64_t m, const char *whose, int64_t q) {
    for (int64_t i = 0; i < m; i++)
        if (!std::isfinite(rhs[at + i]))
            return fail(b, LPG_ERR_ARG, "%s: rhs[%lld] = %g (row %lld of %s %lld) is not finite", call, (long long)(at + i),
                        rhs[at + i], (long long)i, whose, (long long)q);
    return 0;
}

}  // namespace

extern "C" {

int lpg_batch_scenario(lpg_batch **out, lpg_batch *p, int64_t n, const int64_t *src, const int64_t *ident, const double *rhs) {
    const char *call = "lpg_batch_scenario";
    if (!out) return fail(p, LPG_ERR_ARG, "%s: child is NULL", call);
    *out = nullptr;
    // what does not depend on the parent first
    if (n < 1) return fail(p, LPG_ERR_ARG, "%s: n = %lld (need n >= 1)", call, (long long)n);
    if (!src || !ident || !rhs)
        return fail(p, LPG_ERR_ARG, "%s: %s is NULL", call, !src ? "src" : !ident ? "ident" : "rhs");
    if (!p) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: parent is NULL", call);
    if (!plain(p)) return wrong_kind(p, call);
    for (int64_t c = 0; c < n; c++)
        if (int rc = src_ok(p, call, c, src[c])) return rc;
    if (int rc = ident_ok(p, call, ident)) return rc;
    std::vector<ScenarioJob> jobs((size_t)n);
    int64_t at = 0;
    for (int64_t c = 0; c < n; c++) {
        const int64_t m = lp_m(p, src[c]);
        if (int rc = rhs_ok(p, call, rhs, at, m, "child", c)) return rc;
        jobs[(size_t)c] = ScenarioJob{(int32_t)src[c], 0, at};
        at += m;
    }
    lpg_batch *ch = nullptr;
    if (int rc = grow_create(&ch, p, call, n, src, std::vector<int64_t>((size_t)n, 0).data())) return rc;
    if (int rc = p->ragged ? raise_lds<k_batch_scenario<true>>(ch, "k_batch_scenario", kScenarioMaxLds)
                           : raise_lds<k_batch_scenario<false>>(ch, "k_batch_scenario", kScenarioMaxLds))
        return child_die(p, ch, rc);
    DevBuf djobs, dident, drhs;
    const size_t ibytes = (size_t)p->b_total * sizeof(int64_t), rbytes = (size_t)at * sizeof(double);
    if (hipMalloc(&djobs.p, jobs.size() * sizeof(ScenarioJob)) != hipSuccess || hipMalloc(&dident.p, ibytes) != hipSuccess ||
        hipMalloc(&drhs.p, rbytes) != hipSuccess) {
        (void)hipGetLastError();
        fail(ch, LPG_ERR_OOM, "%s: hipMalloc(%lld jobs, ident, %lld right-hand sides) failed", call, (long long)n, (long long)at);
        return child_die(p, ch, LPG_ERR_OOM);
    }
    hipError_t e = hipMemcpyAsync(dident.p, ident, ibytes, hipMemcpyHostToDevice, ch->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(drhs.p, rhs, rbytes, hipMemcpyHostToDevice, ch->stream);
    return grow_finish<k_batch_scenario<false>, k_batch_scenario<true>>(out, p, ch, call, e, jobs, djobs, scenario_lds(p->m),
                                                                        (const int64_t *)dident.p, (const double *)drhs.p,
                                                                        scenario_walk());
}

int lpg_batch_set_rhs(lpg_batch *b, const int64_t *ident, const double *rhs) {
    const char *call = "lpg_batch_set_rhs";
    if (!b) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: batch is NULL", call);
    if (!ident || !rhs) return fail(b, LPG_ERR_ARG, "%s: %s is NULL", call, !ident ? "ident" : "rhs");
    if (!plain(b)) return wrong_kind(b, call);
    if (int rc = ident_ok(b, call, ident)) return rc;
    for (int64_t q = 0, at = 0; q < b->count; at += lp_m(b, q), q++)
        if (int rc = rhs_ok(b, call, rhs, at, lp_m(b, q), "LP", q)) return rc;
    LPG_HIPCHK(b, hipSetDevice(b->device));
    if (int rc = raise_lds<k_batch_set_rhs>(b, "k_batch_set_rhs", kScenarioMaxLds)) return rc;
    DevBuf dident, drhs;
    if (hipMalloc(&dident.p, (size_t)b->b_total * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&drhs.p, (size_t)b->b_total * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(b, LPG_ERR_OOM, "%s: hipMalloc(ident and right-hand sides of %lld LPs) failed", call, (long long)b->count);
    }
    LPG_HIPCHK(b, hipMemcpyAsync(dident.p, ident, (size_t)b->b_total * sizeof(int64_t), hipMemcpyHostToDevice, b->stream));
    LPG_HIPCHK(b, hipMemcpyAsync(drhs.p, rhs, (size_t)b->b_total * sizeof(double), hipMemcpyHostToDevice, b->stream));
    hipLaunchKernelGGL(k_batch_set_rhs, dim3((unsigned)b->count), dim3(kBlock), scenario_lds(b->m), b->stream, bgeo(b),
                       (const int64_t *)dident.p, (const double *)drhs.p, scenario_walk());
    hipLaunchKernelGGL(k_batch_reset, dim3(blocks_for(b->count)), dim3(kBlock), 0, b->stream, b->lp, (int64_t)0, b->count);
    LPG_HIPCHK(b, hipGetLastError());
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    b->pivoted = false;
    return 0;
}

int lpg_batch_ranging(lpg_batch *b, const int64_t *ident, const lpg_ranging_t *out) {
    const char *call = "lpg_batch_ranging";
    // what does not depend on the batch first
    if (!out) return fail(b, LPG_ERR_ARG, "%s: out is NULL", call);
    if (!ident) return fail(b, LPG_ERR_ARG, "%s: ident is NULL", call);
    if (!b) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: batch is NULL", call);
    const int ncost = !!out->cost_lo + !!out->cost_hi + !!out->cost_lo_at + !!out->cost_hi_at;
    const int nrhs = !!out->rhs_lo + !!out->rhs_hi + !!out->rhs_lo_at + !!out->rhs_hi_at;
    if (ncost % 4)
        return fail(b, LPG_ERR_ARG, "%s: out: %d of cost_lo, cost_hi, cost_lo_at, cost_hi_at given (all four or none)", call,
                    ncost);
    if (nrhs % 4)
        return fail(b, LPG_ERR_ARG, "%s: out: %d of rhs_lo, rhs_hi, rhs_lo_at, rhs_hi_at given (all four or none)", call, nrhs);
    if (!out->dual && !ncost && !nrhs)
        return fail(b, LPG_ERR_ARG, "%s: out: none of dual, cost_*, rhs_* given (nothing to compute)", call);
    if (!plain(b)) return wrong_kind(b, call);
    if (int rc = ident_ok(b, call, ident)) return rc;
    LPG_HIPCHK(b, hipSetDevice(b->device));
    if (int rc = b->ragged ? raise_lds<k_batch_ranging<true>>(b, "k_batch_ranging", kRangingMaxLds)
                           : raise_lds<k_batch_ranging<false>>(b, "k_batch_ranging", kRangingMaxLds))
        return rc;
    // one allocation of 8-byte entries: ident, then the arrays of the wanted groups
    const size_t nb = (size_t)b->b_total, nc = b->ragged ? (size_t)b->c_total : (size_t)b->count * (size_t)(b->ncols - 1);
    const size_t total = nb + (out->dual ? nb : 0) + (ncost ? 4 * nc : 0) + (nrhs ? 4 * nb : 0);
    DevBuf buf;
    if (hipMalloc(&buf.p, total * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(b, LPG_ERR_OOM, "%s: hipMalloc(ident and the outputs of %lld LPs) failed", call, (long long)b->count);
    }
    double *at = (double *)buf.p + nb;
    auto take = [&at](bool want, size_t n) { double *p = want ? at : nullptr; if (want) at += n; return p; };
    RangingOut o{};
    o.dual = take(out->dual, nb);
    o.cost_lo = take(ncost, nc);
    o.cost_hi = take(ncost, nc);
    o.cost_lo_at = (int64_t *)take(ncost, nc);
    o.cost_hi_at = (int64_t *)take(ncost, nc);
    o.rhs_lo = take(nrhs, nb);
    o.rhs_hi = take(nrhs, nb);
    o.rhs_lo_at = (int64_t *)take(nrhs, nb);
    o.rhs_hi_at = (int64_t *)take(nrhs, nb);
    LPG_HIPCHK(b, hipMemcpyAsync(buf.p, ident, nb * sizeof(int64_t), hipMemcpyHostToDevice, b->stream));
    const size_t lds = ranging_lds(std::max(b->m, b->ncols));
    if (b->ragged)
        hipLaunchKernelGGL(k_batch_ranging<true>, dim3((unsigned)b->count), dim3(kBlock), lds, b->stream, bgeo(b),
                           (const int64_t *)buf.p, o);
    else
        hipLaunchKernelGGL(k_batch_ranging<false>, dim3((unsigned)b->count), dim3(kBlock), lds, b->stream, bgeo(b),
                           (const int64_t *)buf.p, o);
    LPG_HIPCHK(b, hipGetLastError());
    const struct { void *dst; const void *src; size_t n; } back[] = {
        {out->dual, o.dual, nb},           {out->cost_lo, o.cost_lo, nc},       {out->cost_hi, o.cost_hi, nc},
        {out->cost_lo_at, o.cost_lo_at, nc}, {out->cost_hi_at, o.cost_hi_at, nc}, {out->rhs_lo, o.rhs_lo, nb},
        {out->rhs_hi, o.rhs_hi, nb},       {out->rhs_lo_at, o.rhs_lo_at, nb},   {out->rhs_hi_at, o.rhs_hi_at, nb}};
    for (const auto &c : back)
        if (c.dst) LPG_HIPCHK(b, hipMemcpyAsync(c.dst, c.src, c.n * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

int lpg_batch_branch_select(lpg_batch *b, const uint8_t *mask, int64_t nmask, int64_t ld_mask, double int_tol, int rule,
                            lpg_branch_t *out) {
    const char *call = "lpg_batch_branch_select";
    if (!b) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: batch is NULL", call);
    if (!mask || !out) return fail(b, LPG_ERR_ARG, "%s: %s is NULL", call, !mask ? "mask" : "out");
    if (!plain(b)) return wrong_kind(b, call);
    if (int rc = mask_ok(b, call, nmask, ld_mask)) return rc;
    if (!(int_tol >= 0.0 && int_tol < 0.5)) return fail(b, LPG_ERR_ARG, "%s: int_tol %g outside [0, 0.5)", call, int_tol);
    if (rule != LPG_BRANCH_MOST_FRACTIONAL && rule != LPG_BRANCH_FIRST) return fail(b, LPG_ERR_ARG, "%s: rule %d", call, rule);
    LPG_HIPCHK(b, hipSetDevice(b->device));
    DevBuf dmask, dout;
    int64_t pitch;
    const hipError_t e = hipMalloc(&dout.p, (size_t)b->count * sizeof(BranchPick)) == hipSuccess
                             ? stage_mask(dmask, pitch, mask, nmask, ld_mask, b->count, b->stream)
                             : hipErrorOutOfMemory;
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(b, LPG_ERR_OOM, "%s: hipMalloc(masks and picks of %lld LPs) failed", call, (long long)b->count);
    }
    LPG_HIPCHK(b, e);
    if (rule == LPG_BRANCH_FIRST)
        hipLaunchKernelGGL(k_batch_branch_select<RULE_BLAND>, dim3((unsigned)b->count), dim3(kBlock), 0, b->stream, bgeo(b),
                           (const uint8_t *)dmask.p, nmask, pitch, int_tol, (BranchPick *)dout.p);
    else
        hipLaunchKernelGGL(k_batch_branch_select<RULE_DANTZIG>, dim3((unsigned)b->count), dim3(kBlock), 0, b->stream, bgeo(b),
                           (const uint8_t *)dmask.p, nmask, pitch, int_tol, (BranchPick *)dout.p);
    LPG_HIPCHK(b, hipGetLastError());
    LPG_HIPCHK(b, hipMemcpyAsync(out, dout.p, (size_t)b->count * sizeof(BranchPick), hipMemcpyDeviceToHost, b->stream));
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

int lpg_batch_branch(lpg_batch **out, lpg_batch *p, int64_t n, const int64_t *src, const int64_t *row, const int8_t *dir) {
    const char *call = "lpg_batch_branch";
    if (!out) return fail(p, LPG_ERR_ARG, "%s: child is NULL", call);
    *out = nullptr;
    // what does not depend on the parent first
    if (n < 1) return fail(p, LPG_ERR_ARG, "%s: n = %lld (need n >= 1)", call, (long long)n);
    if (!src || !row || !dir) return fail(p, LPG_ERR_ARG, "%s: %s is NULL", call, !src ? "src" : !row ? "row" : "dir");
    for (int64_t c = 0; c < n; c++)
        if (dir[c] != -1 && dir[c] != 1)
            return fail(p, LPG_ERR_ARG, "%s: dir[%lld] = %d (-1: x <= floor(v), +1: x >= ceil(v))", call, (long long)c,
                        (int)dir[c]);
    if (!p) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: parent is NULL", call);
    if (!plain(p)) return wrong_kind(p, call);
    for (int64_t c = 0; c < n; c++) {
        if (int rc = src_ok(p, call, c, src[c])) return rc;
        const int64_t m = lp_m(p, src[c]), ncols = lp_ncols(p, src[c]);
        if (row[c] < 0 || row[c] >= m)
            return fail(p, LPG_ERR_ARG, "%s: row[%lld] = %lld outside the rows 0..%lld of LP %lld", call, (long long)c,
                        (long long)row[c], (long long)(m - 1), (long long)src[c]);
        if (m + 2 > LPG_BATCH_MAX_DIM || ncols + 1 > LPG_BATCH_MAX_DIM)
            return fail(p, LPG_ERR_ARG, "%s: child %lld of LP %lld: m + 2 = %lld, ncols + 1 = %lld exceed %d", call,
                        (long long)c, (long long)src[c], (long long)(m + 2), (long long)(ncols + 1), LPG_BATCH_MAX_DIM);
    }
    lpg_batch *ch = nullptr;
    if (int rc = grow_create(&ch, p, call, n, src, std::vector<int64_t>((size_t)n, 1).data())) return rc;
    std::vector<BranchJob> jobs((size_t)n);
    for (int64_t c = 0; c < n; c++) jobs[(size_t)c] = BranchJob{(int32_t)src[c], (int32_t)row[c], (int32_t)dir[c], 0};
    DevBuf djobs;
    if (hipMalloc(&djobs.p, jobs.size() * sizeof(BranchJob)) != hipSuccess) {
        (void)hipGetLastError();
        fail(ch, LPG_ERR_OOM, "%s: hipMalloc(%lld jobs) failed", call, (long long)n);
        return child_die(p, ch, LPG_ERR_OOM);
    }
    return grow_finish<k_batch_branch<false>, k_batch_branch<true>>(out, p, ch, call, hipSuccess, jobs, djobs, 0);
}

int lpg_batch_cut_select(lpg_batch *b, const uint8_t *mask, int64_t nmask, int64_t ld_mask, double int_tol, int64_t max_cuts,
                         int64_t *ncut, int64_t *rows) {
    const char *call = "lpg_batch_cut_select";
    // what does not depend on the batch first
    if (!mask || !ncut || !rows)
        return fail(b, LPG_ERR_ARG, "%s: %s is NULL", call, !mask ? "mask" : !ncut ? "ncut" : "rows");
    if (max_cuts < 1 || max_cuts > LPG_BATCH_MAX_CUTS)
        return fail(b, LPG_ERR_ARG, "%s: max_cuts = %lld outside 1..%d", call, (long long)max_cuts, LPG_BATCH_MAX_CUTS);
    if (!(int_tol >= 0.0 && int_tol < 0.5)) return fail(b, LPG_ERR_ARG, "%s: int_tol %g outside [0, 0.5)", call, int_tol);
    if (!b) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: batch is NULL", call);
    if (!plain(b)) return wrong_kind(b, call);
    if (int rc = mask_ok(b, call, nmask, ld_mask)) return rc;
    LPG_HIPCHK(b, hipSetDevice(b->device));
    const size_t nbytes = (size_t)b->count * sizeof(int64_t), rbytes = nbytes * (size_t)max_cuts;
    DevBuf dmask, dncut, drows;
    int64_t pitch;
    const hipError_t e = (hipMalloc(&dncut.p, nbytes) == hipSuccess && hipMalloc(&drows.p, rbytes) == hipSuccess)
                             ? stage_mask(dmask, pitch, mask, nmask, ld_mask, b->count, b->stream)
                             : hipErrorOutOfMemory;
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(b, LPG_ERR_OOM, "%s: hipMalloc(masks and rows of %lld LPs) failed", call, (long long)b->count);
    }
    LPG_HIPCHK(b, e);
    hipLaunchKernelGGL(k_batch_cut_select, dim3((unsigned)b->count), dim3(kBlock), 0, b->stream, bgeo(b),
                       (const uint8_t *)dmask.p, nmask, pitch, int_tol, max_cuts, (int64_t *)dncut.p, (int64_t *)drows.p);
    LPG_HIPCHK(b, hipGetLastError());
    LPG_HIPCHK(b, hipMemcpyAsync(ncut, dncut.p, nbytes, hipMemcpyDeviceToHost, b->stream));
    LPG_HIPCHK(b, hipMemcpyAsync(rows, drows.p, rbytes, hipMemcpyDeviceToHost, b->stream));
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

int lpg_batch_cut(lpg_batch **out, lpg_batch *p, int64_t n, const int64_t *src, const int64_t *first, const int64_t *rows,
                  const uint8_t *mask, int64_t nmask, int64_t ld_mask) {
    const char *call = "lpg_batch_cut";
    if (!out) return fail(p, LPG_ERR_ARG, "%s: child is NULL", call);
    *out = nullptr;
    // what does not depend on the parent first
    if (n < 1) return fail(p, LPG_ERR_ARG, "%s: n = %lld (need n >= 1)", call, (long long)n);
    if (!src || !first || !rows || !mask)
        return fail(p, LPG_ERR_ARG, "%s: %s is NULL", call, !src ? "src" : !first ? "first" : !rows ? "rows" : "mask");
    if (first[0] != 0) return fail(p, LPG_ERR_ARG, "%s: first[0] = %lld (the offsets start at 0)", call, (long long)first[0]);
    for (int64_t c = 0; c < n; c++)
        if (first[c + 1] <= first[c])
            return fail(p, LPG_ERR_ARG, "%s: first[%lld] = %lld is not above first[%lld] = %lld (every child has at least "
                                        "one cut)", call, (long long)(c + 1), (long long)first[c + 1], (long long)c,
                        (long long)first[c]);
    if (!p) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "%s: parent is NULL", call);
    if (!plain(p)) return wrong_kind(p, call);
    if (int rc = mask_ok(p, call, nmask, ld_mask)) return rc;
    std::vector<int64_t> ks((size_t)n);
    std::vector<char> seen;
    for (int64_t c = 0; c < n; c++) {
        const int64_t k = ks[(size_t)c] = first[c + 1] - first[c];
        if (int rc = src_ok(p, call, c, src[c])) return rc;
        if (k > LPG_BATCH_MAX_CUTS)
            return fail(p, LPG_ERR_ARG, "%s: child %lld has %lld cuts, more than LPG_BATCH_MAX_CUTS = %d", call, (long long)c,
                        (long long)k, LPG_BATCH_MAX_CUTS);
        const int64_t m = lp_m(p, src[c]), ncols = lp_ncols(p, src[c]);
        seen.assign((size_t)m, 0);
        for (int64_t t = first[c]; t < first[c + 1]; t++) {
            if (rows[t] < 0 || rows[t] >= m)
                return fail(p, LPG_ERR_ARG, "%s: rows[%lld] = %lld (child %lld) outside the rows 0..%lld of LP %lld", call,
                            (long long)t, (long long)rows[t], (long long)c, (long long)(m - 1), (long long)src[c]);
            if (seen[(size_t)rows[t]])
                return fail(p, LPG_ERR_ARG, "%s: rows[%lld] = %lld appears twice in child %lld", call, (long long)t,
                            (long long)rows[t], (long long)c);
            seen[(size_t)rows[t]] = 1;
        }
        if (m + k + 1 > LPG_BATCH_MAX_DIM || ncols + k > LPG_BATCH_MAX_DIM)
            return fail(p, LPG_ERR_ARG, "%s: child %lld of LP %lld: m + %lld + 1 = %lld, ncols + %lld = %lld exceed %d", call,
                        (long long)c, (long long)src[c], (long long)k, (long long)(m + k + 1), (long long)k,
                        (long long)(ncols + k), LPG_BATCH_MAX_DIM);
    }
    lpg_batch *ch = nullptr;
    if (int rc = grow_create(&ch, p, call, n, src, ks.data())) return rc;
    std::vector<CutJob> jobs((size_t)n);
    std::vector<int32_t> rows32((size_t)first[n]);
    for (int64_t c = 0; c < n; c++) jobs[(size_t)c] = CutJob{(int32_t)src[c], (int32_t)first[c], (int32_t)ks[(size_t)c], 0};
    for (int64_t t = 0; t < first[n]; t++) rows32[(size_t)t] = (int32_t)rows[t];
    DevBuf djobs, drows, dmask;
    int64_t pitch;
    hipError_t e = (hipMalloc(&djobs.p, jobs.size() * sizeof(CutJob)) == hipSuccess &&
                    hipMalloc(&drows.p, rows32.size() * sizeof(int32_t)) == hipSuccess)
                       ? stage_mask(dmask, pitch, mask, nmask, ld_mask, p->count, ch->stream)
                       : hipErrorOutOfMemory;
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        fail(ch, LPG_ERR_OOM, "%s: hipMalloc(%lld jobs, %lld rows, masks) failed", call, (long long)n, (long long)first[n]);
        return child_die(p, ch, LPG_ERR_OOM);
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(drows.p, rows32.data(), rows32.size() * sizeof(int32_t), hipMemcpyHostToDevice, ch->stream);
    return grow_finish<k_batch_cut<false>, k_batch_cut<true>>(out, p, ch, call, e, jobs, djobs, 0, (const int32_t *)drows.p,
                                                              (const uint8_t *)dmask.p, nmask, pitch);
}

const char *lpg_batch_last_error(const lpg_batch *b) { return b ? b->err : thread_err<lpg_batch>(); }

int lpg_batch_create(lpg_batch **out, int device, int64_t count, int64_t m, int64_t ncols, uint32_t flags) {
    return batch_create(out, device, count, m, ncols, flags, 1, "lpg_batch_create");
}

int lpg_batch_create_big_m(lpg_batch **out, int device, int64_t count, int64_t m, int64_t ncols, uint32_t flags) {
    return batch_create(out, device, count, m, ncols, flags, 2, "lpg_batch_create_big_m");
}

int lpg_batch_create_goal(lpg_batch **out, int device, int64_t count, int64_t m, int64_t ncols, int nlevels, uint32_t flags) {
    if (!out) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (nlevels < 1 || nlevels > LPG_GOAL_MAX_LEVELS)
        return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "lpg_batch_create_goal: nlevels = %d outside 1..%d (LPG_GOAL_MAX_LEVELS)",
                               nlevels, LPG_GOAL_MAX_LEVELS);
    return batch_create(out, device, count, m, ncols, flags, nlevels, "lpg_batch_create_goal", true);
}

int lpg_batch_solve_goal(lpg_batch *b, const double *cost, int64_t ld_lp, int64_t ld_level, int64_t max_pivots, int rule,
                         lpg_result *res, double *attain) {
    const char *call = "lpg_batch_solve_goal";
    if (!b) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "batch is NULL");
    if (!b->goal) {
        if (b->nobj == 2) return wrong_kind(b, call);
        return fail(b, LPG_ERR_STATE, "%s: the batch has one objective row (lpg_batch_create); a goal programme needs a "
                                      "batch from lpg_batch_create_goal; nothing has pivoted", call);
    }
    const int64_t N = b->ncols - 1, K = b->nobj;
    if (!cost) return fail(b, LPG_ERR_ARG, "%s: cost is NULL (a goal batch keeps no costs of its own)", call);
    if (rule != LPG_RULE_DANTZIG && rule != LPG_RULE_BLAND) return fail(b, LPG_ERR_ARG, "%s: rule %d", call, rule);
    if (ld_level < N) return fail(b, LPG_ERR_ARG, "%s: ld_level %lld < N = %lld", call, (long long)ld_level, (long long)N);
    if (ld_lp / K < ld_level)
        return fail(b, LPG_ERR_ARG, "%s: ld_lp %lld < nlevels * ld_level = %lld x %lld", call, (long long)ld_lp, (long long)K,
                    (long long)ld_level);
    if (max_pivots < 0) return fail(b, LPG_ERR_ARG, "%s: max_pivots < 0", call);
    LPG_HIPCHK(b, hipSetDevice(b->device));
    // the costs packed (the caller's padding is never read), and the attained levels beside them
    const size_t total = (size_t)b->count * (size_t)K * (size_t)N;
    if (!b->cost && hipMalloc(&b->cost, total * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        b->cost = nullptr;
        return fail(b, LPG_ERR_OOM, "hipMalloc(%d levels of costs of %lld LPs) failed", b->nobj, (long long)b->count);
    }
    if (!b->attain && hipMalloc(&b->attain, (size_t)b->count * (size_t)K * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        b->attain = nullptr;
        return fail(b, LPG_ERR_OOM, "hipMalloc(%d attained levels of %lld LPs) failed", b->nobj, (long long)b->count);
    }
    if (ld_level == N && ld_lp == K * N) {                        // no padding: the caller's array is the packed one
        LPG_HIPCHK(b, hipMemcpy(b->cost, cost, total * sizeof(double), hipMemcpyHostToDevice));
    } else {
        double *packed = (double *)malloc(total * sizeof(double));
        if (!packed) return fail(b, LPG_ERR_OOM, "%s: malloc(%zu bytes to pack the costs) failed", call, total * sizeof(double));
        for (int64_t q = 0; q < b->count; q++)
            for (int64_t k = 0; k < K; k++)
                memcpy(packed + (size_t)((q * K + k) * N), cost + q * ld_lp + k * ld_level, (size_t)N * sizeof(double));
        const hipError_t e = hipMemcpy(b->cost, packed, total * sizeof(double), hipMemcpyHostToDevice);
        free(packed);
        LPG_HIPCHK(b, e);
    }
    if (int rc = batch_run(b, max_pivots, M_GOAL, rule, res)) return rc;
    if (attain) LPG_HIPCHK(b, hipMemcpy(attain, b->attain, (size_t)b->count * (size_t)K * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

void lpg_batch_destroy(lpg_batch *b) {
    if (!b) return;
    if (b->T || b->stream) (void)hipSetDevice(b->device);
    if (b->stream) {
        (void)hipStreamSynchronize(b->stream);
        (void)hipStreamDestroy(b->stream);
    }
    if (b->T) (void)hipFree(b->T);
    if (b->basis) (void)hipFree(b->basis);
    if (b->lp) (void)hipFree(b->lp);
    if (b->logk) (void)hipFree(b->logk);
    if (b->logr) (void)hipFree(b->logr);
    if (b->running) (void)hipFree(b->running);
    if (b->bad) (void)hipFree(b->bad);
    if (b->cost) (void)hipFree(b->cost);
    if (b->attain) (void)hipFree(b->attain);
    if (b->dshape) (void)hipFree(b->dshape);
    if (b->dorder) (void)hipFree(b->dorder);
    delete b;
}

int lpg_batch_info(const lpg_batch *b, lpg_batch_info_t *o) {
    if (!b || !o) return fail(const_cast<lpg_batch *>(b), LPG_ERR_ARG, "NULL argument");
    o->count = b->count;
    o->m = b->m;
    o->ncols = b->ncols;
    o->ld = b->ld;
    o->tier = b->tier;
    o->chunk = b->chunk;
    o->lds_bytes = b->lds;
    o->log_capacity = b->logcap;
    o->nobj = b->nobj;
    o->pad = b->ragged ? 1 : 0;
    return 0;
}

int lpg_batch_create_ragged(lpg_batch **out, int device, int64_t count, const int64_t *m, const int64_t *ncols, int nobj,
                            uint32_t flags) {
    return ragged_create(out, device, count, m, ncols, nobj, flags);
}

int lpg_batch_shape(const lpg_batch *cb, int64_t lp, lpg_batch_shape_t *o) {
    lpg_batch *b = const_cast<lpg_batch *>(cb);
    if (!b || !o) return fail(b, LPG_ERR_ARG, "lpg_batch_shape: NULL argument");
    if (!b->ragged) return wrong_layout(b, "lpg_batch_shape", "lpg_batch_info");
    if (lp < 0 || lp >= b->count)
        return fail(b, LPG_ERR_ARG, "lpg_batch_shape: LP %lld outside the batch of %lld", (long long)lp, (long long)b->count);
    *o = b->pub[(size_t)lp];
    return 0;
}

int lpg_batch_load_packed(lpg_batch *b, int64_t first, int64_t n, const double *tableaus, const int64_t *basis) {
    if (!b || !tableaus) return fail(b, LPG_ERR_ARG, "lpg_batch_load_packed: NULL argument");
    if (b->goal) return wrong_kind(b, "lpg_batch_load_packed");
    if (!b->ragged) return wrong_layout(b, "lpg_batch_load_packed", "lpg_batch_load");
    if (int rc = range_ok(b, "lpg_batch_load_packed", first, n)) return rc;
    if (n == 0) return 0;
    const BatchShape &s0 = b->shape[(size_t)first], &s1 = b->shape[(size_t)(first + n - 1)];
    if (basis)
        for (int64_t q = first; q < first + n; q++) {
            const BatchShape &s = b->shape[(size_t)q];
            for (int64_t i = 0; i < s.m; i++) {
                const int64_t k = basis[s.b_off - s0.b_off + i];
                if (k < 1 || k >= s.ncols)
                    return fail(b, LPG_ERR_ARG, "lpg_batch_load_packed: basis[%lld] of LP %lld out of range 1..%lld",
                                (long long)i, (long long)q, (long long)(s.ncols - 1));
            }
        }
    LPG_HIPCHK(b, hipSetDevice(b->device));
    // the LPs' device images are back to back: build them on the host (rows at
    // pitch ld, zero padding) and move them in one copy
    const int64_t doubles = s1.t_off + (int64_t)(s1.m + b->nobj) * s1.ld - s0.t_off;
    std::vector<double> img((size_t)doubles, 0.0);
    const double *src = tableaus;
    for (int64_t q = first; q < first + n; q++) {
        const BatchShape &s = b->shape[(size_t)q];
        double *dst = img.data() + (s.t_off - s0.t_off);
        for (int64_t i = 0; i < s.m + b->nobj; i++, src += s.ncols, dst += s.ld) memcpy(dst, src, (size_t)s.ncols * sizeof(double));
    }
    LPG_HIPCHK(b, hipMemcpyAsync(b->T + s0.t_off, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (basis)
        LPG_HIPCHK(b, hipMemcpyAsync(b->basis + s0.b_off, basis, (size_t)(s1.b_off + s1.m - s0.b_off) * sizeof(int64_t),
                                  hipMemcpyHostToDevice, b->stream));
    hipLaunchKernelGGL(k_batch_reset, dim3(blocks_for(n)), dim3(kBlock), 0, b->stream, b->lp, first, n);
    LPG_HIPCHK(b, hipGetLastError());
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    if (first == 0 && n == b->count) b->pivoted = false;
    return 0;
}

int lpg_batch_get_rows_packed(lpg_batch *b, int64_t first, int64_t n, double *out) {
    if (!b || !out) return fail(b, LPG_ERR_ARG, "lpg_batch_get_rows_packed: NULL argument");
    if (b->goal) return wrong_kind(b, "lpg_batch_get_rows_packed");
    if (!b->ragged) return wrong_layout(b, "lpg_batch_get_rows_packed", "lpg_batch_get_rows");
    if (int rc = range_ok(b, "lpg_batch_get_rows_packed", first, n)) return rc;
    if (n == 0) return 0;
    LPG_HIPCHK(b, hipSetDevice(b->device));
    const BatchShape &s0 = b->shape[(size_t)first], &s1 = b->shape[(size_t)(first + n - 1)];
    std::vector<double> img((size_t)(s1.t_off + (int64_t)(s1.m + b->nobj) * s1.ld - s0.t_off));
    LPG_HIPCHK(b, hipMemcpyAsync(img.data(), b->T + s0.t_off, img.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    for (int64_t q = first; q < first + n; q++) {
        const BatchShape &s = b->shape[(size_t)q];
        const double *src = img.data() + (s.t_off - s0.t_off);
        for (int64_t i = 0; i < s.m + b->nobj; i++, src += s.ld, out += s.ncols) memcpy(out, src, (size_t)s.ncols * sizeof(double));
    }
    return 0;
}

int lpg_batch_get_basis_packed(lpg_batch *b, int64_t first, int64_t n, int64_t *basis) {
    if (!b || !basis) return fail(b, LPG_ERR_ARG, "lpg_batch_get_basis_packed: NULL argument");
    if (b->goal) return wrong_kind(b, "lpg_batch_get_basis_packed");
    if (!b->ragged) return wrong_layout(b, "lpg_batch_get_basis_packed", "lpg_batch_get_basis");
    if (int rc = range_ok(b, "lpg_batch_get_basis_packed", first, n)) return rc;
    if (n == 0) return 0;
    LPG_HIPCHK(b, hipSetDevice(b->device));
    const BatchShape &s0 = b->shape[(size_t)first], &s1 = b->shape[(size_t)(first + n - 1)];
    LPG_HIPCHK(b, hipMemcpy(basis, b->basis + s0.b_off, (size_t)(s1.b_off + s1.m - s0.b_off) * sizeof(int64_t),
                         hipMemcpyDeviceToHost));
    return 0;
}

int lpg_batch_set_objective_packed(lpg_batch *b, const double *cost) {
    if (!b || !cost) return fail(b, LPG_ERR_ARG, "lpg_batch_set_objective_packed: NULL argument");
    if (!plain(b)) return wrong_kind(b, "lpg_batch_set_objective_packed");
    if (!b->ragged) return wrong_layout(b, "lpg_batch_set_objective_packed", "lpg_batch_set_objective");
    LPG_HIPCHK(b, hipSetDevice(b->device));
    if (int rc = stage_costs(b, cost, 0)) return rc;
    hipLaunchKernelGGL(k_batch_set_objective, dim3((unsigned)b->count), dim3(kBlock), 0, b->stream, bgeo(b), b->cost);
    LPG_HIPCHK(b, hipGetLastError());
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

int lpg_batch_solve_two_phase_ragged(lpg_batch *b, const int64_t *art_first, const double *cost, int64_t max_pivots,
                                     int rule, lpg_result *out) {
    return solve_artificial(b, M_TWO_PHASE, "lpg_batch_solve_two_phase_ragged", true, art_first, cost, 0, max_pivots, rule, out);
}

int lpg_batch_solve_big_m_ragged(lpg_batch *b, const int64_t *art_first, const double *cost, int64_t max_pivots, int rule,
                                 lpg_result *out) {
    return solve_artificial(b, M_BIG_M, "lpg_batch_solve_big_m_ragged", true, art_first, cost, 0, max_pivots, rule, out);
}

int lpg_batch_load(lpg_batch *b, int64_t first, int64_t n, const double *tableaus, int64_t ld, const int64_t *basis) {
    if (!b || !tableaus) return fail(b, LPG_ERR_ARG, "lpg_batch_load: NULL argument");
    if (b->ragged) return wrong_layout(b, "lpg_batch_load", "lpg_batch_load_packed");
    if (int rc = range_ok(b, "lpg_batch_load", first, n)) return rc;
    if (ld < b->ncols) return fail(b, LPG_ERR_ARG, "lpg_batch_load: ld %lld < ncols %lld", (long long)ld, (long long)b->ncols);
    if (basis)
        for (int64_t q = 0; q < n * b->m; q++)
            if (basis[q] < 1 || basis[q] >= b->ncols)
                return fail(b, LPG_ERR_ARG, "lpg_batch_load: basis[%lld] of LP %lld out of range 1..%lld",
                            (long long)(q % b->m), (long long)(first + q / b->m), (long long)(b->ncols - 1));
    if (n == 0) return 0;
    LPG_HIPCHK(b, hipSetDevice(b->device));
    const int64_t rows = b->m + b->nobj;
    // rows are back to back on both sides: one strided copy of n * (m + nobj) rows
    LPG_HIPCHK(b, hipMemcpy2DAsync(b->T + first * rows * b->ld, (size_t)b->ld * sizeof(double), tableaus,
                                (size_t)ld * sizeof(double), (size_t)b->ncols * sizeof(double), (size_t)(n * rows),
                                hipMemcpyHostToDevice, b->stream));
    if (basis)
        LPG_HIPCHK(b, hipMemcpyAsync(b->basis + first * b->m, basis, (size_t)(n * b->m) * sizeof(int64_t),
                                  hipMemcpyHostToDevice, b->stream));
    hipLaunchKernelGGL(k_batch_reset, dim3(blocks_for(n)), dim3(kBlock), 0, b->stream, b->lp, first, n);
    LPG_HIPCHK(b, hipGetLastError());
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    if (first == 0 && n == b->count) b->pivoted = false;
    return 0;
}

int lpg_batch_generate(lpg_batch *b, int64_t n, uint64_t seed, int kind) {
    if (!b) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "batch is NULL");
    if (!plain(b)) return wrong_kind(b, "lpg_batch_generate");
    if (b->ragged) return wrong_layout(b, "lpg_batch_generate", "lpg_batch_load_packed (a ragged batch has no generator)");
    if (n < 1 || b->ncols != n + b->m + 1)
        return fail(b, LPG_ERR_ARG, "lpg_batch_generate: ncols %lld != n + m + 1 = %lld", (long long)b->ncols,
                    (long long)(n + b->m + 1));
    if (kind != LPG_GEN_DENSE && kind != LPG_GEN_DEGENERATE && kind != LPG_GEN_DUAL)
        return fail(b, LPG_ERR_ARG, "lpg_batch_generate: kind %d (dense, degenerate or dual only)", kind);
    return generate(b, n, seed, kind);
}

int lpg_batch_set_tolerances(lpg_batch *b, double eps_piv, double eps_opt) {
    if (!b || !(eps_piv >= 0) || !(eps_opt >= 0)) return fail(b, LPG_ERR_ARG, "lpg_batch_set_tolerances: bad tolerances");
    b->eps_piv = eps_piv;
    b->eps_opt = eps_opt;
    return 0;
}

int lpg_batch_set_active_columns(lpg_batch *b, int64_t nact) {
    if (b && !plain(b)) return wrong_kind(b, "lpg_batch_set_active_columns");
    if (b && b->ragged)
        return wrong_layout(b, "lpg_batch_set_active_columns", "lpg_batch_solve_two_phase_ragged, which sets them per LP");
    if (!b || nact < 1 || nact > b->ncols - 1)
        return fail(b, LPG_ERR_ARG, "lpg_batch_set_active_columns: nact out of range 1..N");
    b->nact = nact;
    return 0;
}

int lpg_batch_reserve_log(lpg_batch *b, int64_t npivots) {
    if (!b || npivots < 0) return fail(b, LPG_ERR_ARG, "lpg_batch_reserve_log: bad arguments");
    if (b->pivoted) return fail(b, LPG_ERR_STATE, "lpg_batch_reserve_log: set the log capacity before the first solve");
    if (npivots > (int64_t)0x7fffffff || (double)npivots * (double)b->count > 4e9)
        return fail(b, LPG_ERR_ARG, "lpg_batch_reserve_log: %lld pivots x %lld LPs is too large", (long long)npivots,
                    (long long)b->count);
    LPG_HIPCHK(b, hipSetDevice(b->device));
    return alloc_log(b, npivots);
}

int lpg_batch_solve(lpg_batch *b, int64_t max_pivots, int rule, lpg_result *out) {
    if (b && !plain(b)) return wrong_kind(b, "lpg_batch_solve");
    if (b && rule != LPG_RULE_DANTZIG && rule != LPG_RULE_BLAND) return fail(b, LPG_ERR_ARG, "lpg_batch_solve: rule %d", rule);
    return batch_run(b, max_pivots, M_PRIMAL, rule, out);
}

int lpg_batch_solve_dual(lpg_batch *b, int64_t max_pivots, lpg_result *out) {
    if (b && !plain(b)) return wrong_kind(b, "lpg_batch_solve_dual");
    return batch_run(b, max_pivots, M_DUAL, RULE_DANTZIG, out);
}

int lpg_batch_solve_two_phase(lpg_batch *b, int64_t art_first, const double *cost, int64_t ld_cost, int64_t max_pivots,
                              int rule, lpg_result *out) {
    return solve_artificial(b, M_TWO_PHASE, "lpg_batch_solve_two_phase", false, &art_first, cost, ld_cost, max_pivots, rule, out);
}

int lpg_batch_solve_big_m(lpg_batch *b, int64_t art_first, const double *cost, int64_t ld_cost, int64_t max_pivots,
                          int rule, lpg_result *out) {
    return solve_artificial(b, M_BIG_M, "lpg_batch_solve_big_m", false, &art_first, cost, ld_cost, max_pivots, rule, out);
}

int lpg_batch_set_objective(lpg_batch *b, const double *cost, int64_t ld_cost) {
    if (!b || !cost) return fail(b, LPG_ERR_ARG, "lpg_batch_set_objective: NULL argument");
    if (!plain(b)) return wrong_kind(b, "lpg_batch_set_objective");
    if (b->ragged) return wrong_layout(b, "lpg_batch_set_objective", "lpg_batch_set_objective_packed");
    if (ld_cost < b->ncols - 1)
        return fail(b, LPG_ERR_ARG, "lpg_batch_set_objective: ld_cost %lld < N = %lld", (long long)ld_cost,
                    (long long)(b->ncols - 1));
    LPG_HIPCHK(b, hipSetDevice(b->device));
    if (int rc = stage_costs(b, cost, ld_cost)) return rc;
    hipLaunchKernelGGL(k_batch_set_objective, dim3((unsigned)b->count), dim3(kBlock), 0, b->stream, bgeo(b), b->cost);
    LPG_HIPCHK(b, hipGetLastError());
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

int lpg_batch_generate_artificial(lpg_batch *b, int64_t n, uint64_t seed, int64_t *art_first) {
    if (!b) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "batch is NULL");
    if (b->goal) return wrong_kind(b, "lpg_batch_generate_artificial");
    if (b->ragged)
        return wrong_layout(b, "lpg_batch_generate_artificial", "lpg_batch_load_packed (a ragged batch has no generator)");
    if (n < 1 || b->ncols != n + b->m + 1)
        return fail(b, LPG_ERR_ARG, "lpg_batch_generate_artificial: ncols %lld != n + m + 1 = %lld", (long long)b->ncols,
                    (long long)(n + b->m + 1));
    if (int rc = generate(b, n, seed, (int)LPG_GEN_ARTIFICIAL)) return rc;
    if (art_first) *art_first = 1 + n + (b->m + 1) / 2;
    return 0;
}

int lpg_batch_get_rows(lpg_batch *b, int64_t first, int64_t n, double *out, int64_t ld) {
    if (!b || !out) return fail(b, LPG_ERR_ARG, "lpg_batch_get_rows: NULL argument");
    if (b->ragged) return wrong_layout(b, "lpg_batch_get_rows", "lpg_batch_get_rows_packed");
    if (int rc = range_ok(b, "lpg_batch_get_rows", first, n)) return rc;
    if (ld < b->ncols) return fail(b, LPG_ERR_ARG, "lpg_batch_get_rows: ld %lld < ncols %lld", (long long)ld, (long long)b->ncols);
    if (n == 0) return 0;
    LPG_HIPCHK(b, hipSetDevice(b->device));
    const int64_t rows = b->m + b->nobj;
    LPG_HIPCHK(b, hipMemcpy2DAsync(out, (size_t)ld * sizeof(double), b->T + first * rows * b->ld, (size_t)b->ld * sizeof(double),
                                (size_t)b->ncols * sizeof(double), (size_t)(n * rows), hipMemcpyDeviceToHost, b->stream));
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    return 0;
}

int lpg_batch_get_basis(lpg_batch *b, int64_t first, int64_t n, int64_t *basis) {
    if (!b || !basis) return fail(b, LPG_ERR_ARG, "lpg_batch_get_basis: NULL argument");
    if (b->ragged) return wrong_layout(b, "lpg_batch_get_basis", "lpg_batch_get_basis_packed");
    if (int rc = range_ok(b, "lpg_batch_get_basis", first, n)) return rc;
    if (n == 0) return 0;
    LPG_HIPCHK(b, hipSetDevice(b->device));
    LPG_HIPCHK(b, hipMemcpy(basis, b->basis + first * b->m, (size_t)(n * b->m) * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

int64_t lpg_batch_get_log(lpg_batch *b, int64_t lp, int64_t *k, int64_t *r, int64_t max) {
    if (!b) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "batch is NULL");
    if (lp < 0 || lp >= b->count)
        return fail(b, LPG_ERR_ARG, "lpg_batch_get_log: LP %lld outside the batch of %lld", (long long)lp, (long long)b->count);
    if (!b->logk) return 0;
    LPG_HIPCHK(b, hipSetDevice(b->device));
    BatchLP h;
    LPG_HIPCHK(b, hipMemcpy(&h, b->lp + lp, sizeof h, hipMemcpyDeviceToHost));
    const int64_t rec = std::min(h.pivots, b->logcap);
    const int64_t n = std::max<int64_t>(0, std::min(rec, max));
    if (n > 0 && (k || r)) {
        std::vector<int32_t> t((size_t)n);
        for (int w = 0; w < 2; w++) {
            int64_t *dst = w ? r : k;
            if (!dst) continue;
            LPG_HIPCHK(b, hipMemcpy(t.data(), (w ? b->logr : b->logk) + lp * b->logcap, (size_t)n * sizeof(int32_t),
                                 hipMemcpyDeviceToHost));
            for (int64_t q = 0; q < n; q++) dst[q] = t[(size_t)q];
        }
    }
    return rec;
}

int lpg_batch_active_columns(const lpg_batch *cb, int64_t lp, int64_t *nact, int64_t *art_first) {
    lpg_batch *b = const_cast<lpg_batch *>(cb);
    if (!b) return fail<lpg_batch>(nullptr, LPG_ERR_ARG, "lpg_batch_active_columns: batch is NULL");
    if (lp < 0 || lp >= b->count)
        return fail(b, LPG_ERR_ARG, "lpg_batch_active_columns: LP %lld outside the batch of %lld", (long long)lp,
                    (long long)b->count);
    if (nact) *nact = lp_nact(b, lp);
    if (art_first) *art_first = b->ragged ? b->shape[(size_t)lp].art_first : b->ncols;
    return 0;
}

}  // extern "C"
