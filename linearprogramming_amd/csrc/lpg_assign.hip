// lpg_assign.hip — batches of assignment problems (include/lpg.h, "assignment"):
// the primal-dual (shortest augmenting path) Hungarian method, one launch per
// batch, one problem per wave (nc <= 64) or per workgroup, no communication
// between problems. Host code and launches live in this file like the other
// translation units'.
//
// The arithmetic is the header's, operation for operation: the reduced cost is
// (C - u) - v in two roundings, the updates one rounding each, nothing is
// contracted (-ffp-contract=off), and the argmin compares VALUES: the key of a
// minv is its bits mapped to a total order with -0 folded onto +0 for the key
// only, because a reduced cost can be slightly negative or -0 here (the packed
// key of block_argmin_cand, "the bits of theta >= 0", would put every negative
// number above +inf). delta is the winner's own bits, read back from the
// winner, never rebuilt from the key: -0 + -0 and -0 + +0 differ.
//
// Every compare-and-keep is a per-field select on one predicate (see the
// comment above the reductions in lpg_device.h: hipcc has miscompiled the
// early-return form).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/lpg.h"
#include "lpg_internal.h"
#include "lpg_device.h"
#include "lpg_host.h"

namespace lpg {

constexpr int kAssignMaxLds = 150 * 1024;      // dynamic LDS cap, as lpg_batch.hip's kBatchMaxLds
constexpr int kWaveProblems = kBlock / 64;     // wave form: problems per workgroup
constexpr int kNone = -1;
constexpr uint64_t kKeyInf = 0xfff0000000000000ull;   // order_key(+inf): no key of a finite minv reaches it

struct AssignGeo {
    const double *C;       // count x nr x nc, dense; negated for a maximisation (+inf kept)
    double *u, *v;         // count x nr, count x nc
    int32_t *col;          // count x nr
    lpg_assign_result *res;
    char *scratch;         // workgroup form, column state that does not fit the LDS: scratch_stride bytes per problem
    int64_t scratch_stride;
    int64_t count;
    int32_t nr, nc;
    int32_t maximize;
    int32_t state_lds;     // workgroup form with nc > kBlock: 1 the column state is in LDS, 0 in `scratch`
};

// order_key (lpg_device.h): no NaN occurs here, see the cap in lpg.h.
__device__ __forceinline__ int rdl_int(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

__device__ __forceinline__ double sense(double x, int maximize) { return maximize ? -x : x; }

__global__ __launch_bounds__(kBlock) void k_assign_generate(double *C, int64_t count, int64_t per, uint64_t seed,
                                                            double range, int maximize) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= count * per) return;
    const int64_t q = e / per;
    const double c = floor(uniform01(seed + (uint64_t)q, (uint64_t)(e - q * per)) * range);
    C[e] = sense(c, maximize);
}

// ---- wave form: one wave per problem, one column per lane (nc <= 64) ------
// minv, v, way, used and rowof are registers, C and u the wave's slice of the
// LDS, the argmin six DPP steps with no LDS. The four waves of a workgroup run
// four problems with four step counts and any of them may end infeasible
// early, so nothing here is a workgroup barrier: the load is per wave as well.
// The DPP helpers need the whole wave active; the lanes behind nc carry the
// neutral key and never leave the control flow.
__global__ __launch_bounds__(kBlock) void k_assign_wave(AssignGeo g) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * kWaveProblems + w;
    if (q >= g.count) return;                  // an idle wave of the last workgroup: before any memory access
    const int nr = g.nr, nc = g.nc, mx = g.maximize;
    double *Cw = lds + (size_t)w * (size_t)(nr * nc + nr);
    double *uw = Cw + nr * nc;
    const double *Cg = g.C + q * (int64_t)(nr * nc);
    for (int e = lane; e < nr * nc; e += 64) Cw[e] = Cg[e];
    if (lane < nr) uw[lane] = 0.0;
    wave_fence();

    const bool iscol = lane < nc;
    double v = 0.0;
    int rowof = kNone;
    int64_t steps = 0;
    int status = OPTIMAL;
    for (int i = 0; i < nr; i++) {
        double minv = INFINITY;
        int way = kNone;
        bool used = false;
        int i0 = i, j0 = kNone;
        for (;;) {
            steps++;
            used = used | (lane == j0);
            const double ui0 = uw[i0];
            const double c = iscol ? Cw[i0 * nc + lane] : INFINITY;
            const double cur = (c - ui0) - v;
            const bool cand = iscol & !used;
            const bool take = cand & (cur < minv);
            minv = take ? cur : minv;
            way = take ? j0 : way;
            uint64_t h = cand ? order_key(minv) : ~0ull;
            uint32_t l = cand ? (uint32_t)lane : ~0u;
            wave_min_key(h, l);
            if (h >= kKeyInf) {                // wave-uniform: no unused column with minv < +inf
                status = INFEASIBLE;
                break;
            }
            const int j1 = (int)l;
            const double delta = __longlong_as_double((long long)rdl64((uint64_t)__double_as_longlong(minv), j1));
            if (lane == 0) uw[i] = uw[i] + delta;
            if (used) uw[rowof] = uw[rowof] + delta;     // rows of used columns are distinct, and none is row i
            v = used ? v - delta : v;
            minv = cand ? minv - delta : minv;
            wave_fence();
            j0 = j1;
            const int r = rdl_int(rowof, j0);
            if (r < 0) break;
            i0 = r;
        }
        if (status != OPTIMAL) break;
        while (j0 >= 0) {                      // augment: wave-uniform walk, at most i + 1 columns
            const int jn = rdl_int(way, j0);
            const int r = jn >= 0 ? rdl_int(rowof, jn) : i;
            rowof = lane == j0 ? r : rowof;
            j0 = jn;
        }
    }

    double *uo = g.u + q * nr, *vo = g.v + q * nc;
    int32_t *co = g.col + q * nr;
    if (iscol) vo[lane] = sense(v, mx);
    if (lane < nr) uo[lane] = sense(uw[lane], mx);
    double obj = NAN;
    if (status == OPTIMAL) {
        wave_fence();
        if (iscol & (rowof >= 0)) {
            co[rowof] = lane;
            uw[rowof] = sense(Cw[rowof * nc + lane], mx);     // the caller's cost of the pair
        }
        wave_fence();
        if (lane == 0) {
            obj = 0.0;
            for (int r = 0; r < nr; r++) obj = obj + uw[r];
        }
    } else if (lane < nr) {
        co[lane] = -1;
    }
    if (lane == 0) {
        lpg_assign_result o;
        o.status = status;
        o.pad = 0;
        o.steps = steps;
        o.objective = obj;
        g.res[q] = o;
    }
}

// ---- workgroup form: one workgroup per problem ----------------------------
// Columns are strided over the 256 threads. REG (nc <= 256): a thread owns one
// column and keeps its minv, v and used in registers; else they are arrays, in
// LDS where they fit and in device memory beyond (g.state_lds). way and rowof
// are arrays in both, because the augmenting walk is one thread's. TIER: C in
// LDS, or in device memory with one coalesced row read per step.
// A step has ONE barrier, inside the argmin: the waves' keys alternate between
// two LDS slots, u[i0] was last written before the previous step's barrier
// (the column that leads to row i0 was unused then, and row i's own u is read
// only in the search's first step, before anything adds to it), and rowof
// changes only in the walk, which has a barrier on either side.
template <int TIER, bool REG>
__global__ __launch_bounds__(kBlock) void k_assign_wg(AssignGeo g) {
    extern __shared__ double lds[];
    __shared__ int s_way[REG ? kBlock : 1], s_rowof[REG ? kBlock : 1];
    __shared__ uint64_t sh[2][kBlock / 64], sv[2][kBlock / 64];
    __shared__ uint32_t sl[2][kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t q = blockIdx.x;
    const int nr = g.nr, nc = g.nc, mx = g.maximize;
    double *u = lds;
    const double *C = g.C + q * ((int64_t)nr * nc);
    if (TIER == LPG_BATCH_TIER_LDS) {
        double *Cl = lds + nr;
        for (int e = tid; e < nr * nc; e += kBlock) Cl[e] = C[e];
        C = Cl;
    }
    double *minv_a = nullptr, *v_a = nullptr;
    int *way_a = s_way, *rowof_a = s_rowof, *used_a = nullptr;
    if (!REG) {
        double *base = g.state_lds ? lds + nr + (TIER == LPG_BATCH_TIER_LDS ? (size_t)nr * nc : 0)
                                   : (double *)(g.scratch + q * g.scratch_stride);
        minv_a = base;
        v_a = base + nc;
        way_a = (int *)(base + 2 * (size_t)nc);
        rowof_a = way_a + nc;
        used_a = rowof_a + nc;
    }
    double r_minv = INFINITY, r_v = 0.0;
    int r_used = 0;
    auto MINV = [&](int j) -> double & { if constexpr (REG) return r_minv; else return minv_a[j]; };
    auto V = [&](int j) -> double & { if constexpr (REG) return r_v; else return v_a[j]; };
    auto USED = [&](int j) -> int & { if constexpr (REG) return r_used; else return used_a[j]; };
    // f(j, valid) for this thread's columns; REG: its one column, valid iff it exists
    auto for_cols = [&](auto f) {
        if constexpr (REG) f(tid, tid < nc);
        else for (int j = tid; j < nc; j += kBlock) f(j, true);
    };

    for (int r = tid; r < nr; r += kBlock) u[r] = 0.0;
    for_cols([&](int j, bool valid) {
        V(j) = 0.0;
        if (valid) rowof_a[j] = kNone;
    });
    __syncthreads();

    int64_t steps = 0;
    int status = OPTIMAL, par = 0;
    for (int i = 0; i < nr; i++) {
        for_cols([&](int j, bool valid) {
            MINV(j) = INFINITY;
            USED(j) = 0;
            if (valid) way_a[j] = kNone;
        });
        int i0 = i, j0 = kNone;
        for (;;) {
            steps++;
            const double ui0 = u[i0];
            uint64_t bh = ~0ull, bv = 0;
            uint32_t bl = ~0u;
            for_cols([&](int j, bool valid) {
                int &usd = USED(j);
                usd = usd | (j == j0);
                const double c = valid ? C[(size_t)i0 * nc + j] : INFINITY;
                const double cur = (c - ui0) - V(j);
                double &mv = MINV(j);
                const bool cand = valid & !usd;
                const bool take = cand & (cur < mv);
                mv = take ? cur : mv;
                if (take) way_a[j] = j0;
                const uint64_t h = cand ? order_key(mv) : ~0ull;
                const uint32_t l = cand ? (uint32_t)j : ~0u;
                const bool better = (h < bh) | ((h == bh) & (l < bl));
                bh = better ? h : bh;
                bl = better ? l : bl;
                bv = better ? (uint64_t)__double_as_longlong(mv) : bv;
            });
            uint64_t h = bh;
            uint32_t l = bl;
            wave_min_key(h, l);
            const int src = winner_lane((bh == h) & (bl == l));
            const uint64_t val = rdl64(bv, src < 0 ? 0 : src);
            if (lane == 0) {
                sh[par][w] = h;
                sl[par][w] = l;
                sv[par][w] = val;
            }
            __syncthreads();
            uint64_t fh = sh[par][0], fv = sv[par][0];
            uint32_t fl = sl[par][0];
#pragma unroll
            for (int k = 1; k < kBlock / 64; k++) {
                const uint64_t kh = sh[par][k], kv = sv[par][k];
                const uint32_t kl = sl[par][k];
                const bool better = (kh < fh) | ((kh == fh) & (kl < fl));
                fh = better ? kh : fh;
                fl = better ? kl : fl;
                fv = better ? kv : fv;
            }
            par ^= 1;
            if (fh >= kKeyInf) {               // uniform: no unused column with minv < +inf
                status = INFEASIBLE;
                break;
            }
            const int j1 = (int)fl;
            const double delta = __longlong_as_double((long long)fv);
            if (tid == 0) u[i] = u[i] + delta;
            for_cols([&](int j, bool valid) {
                const bool usd = USED(j) != 0;
                if (usd) {
                    const int r = rowof_a[j];
                    u[r] = u[r] + delta;
                }
                double &vj = V(j);
                vj = usd ? vj - delta : vj;
                double &mv = MINV(j);
                mv = (valid & !usd) ? mv - delta : mv;
            });
            j0 = j1;
            const int r = rowof_a[j0];
            if (r < 0) break;
            i0 = r;
        }
        if (status != OPTIMAL) break;
        __syncthreads();
        if (tid == 0) {                        // augment: at most i + 1 columns
            int j = j0;
            while (j >= 0) {
                const int jn = way_a[j];
                rowof_a[j] = jn >= 0 ? rowof_a[jn] : i;
                j = jn;
            }
        }
        __syncthreads();
    }

    __syncthreads();
    double *uo = g.u + q * nr, *vo = g.v + q * nc;
    int32_t *co = g.col + q * nr;
    for_cols([&](int j, bool valid) {
        if (valid) vo[j] = sense(V(j), mx);
    });
    for (int r = tid; r < nr; r += kBlock) uo[r] = sense(u[r], mx);
    double obj = NAN;
    if (status == OPTIMAL) {                   // uniform
        __syncthreads();
        for_cols([&](int j, bool valid) {
            const int r = valid ? rowof_a[j] : kNone;
            if (r >= 0) {
                co[r] = j;
                u[r] = sense(C[(size_t)r * nc + j], mx);      // the caller's cost of the pair
            }
        });
        __syncthreads();
        if (tid == 0) {
            obj = 0.0;
            for (int r = 0; r < nr; r++) obj = obj + u[r];
        }
    } else {
        for (int r = tid; r < nr; r += kBlock) co[r] = -1;
    }
    if (tid == 0) {
        lpg_assign_result o;
        o.status = status;
        o.pad = 0;
        o.steps = steps;
        o.objective = obj;
        g.res[q] = o;
    }
}

}  // namespace lpg

using namespace lpg;

struct lpg_assign : BatchHost {
    int64_t nr = 0, nc = 0;
    uint32_t flags = 0;
    int tier = LPG_BATCH_TIER_LDS, form = LPG_ASSIGN_FORM_WAVE;
    bool state_lds = true;
    int64_t scratch_stride = 0;
    double *C = nullptr, *u = nullptr, *v = nullptr;
    int32_t *col = nullptr;
    lpg_assign_result *res = nullptr;
    char *scratch = nullptr;
};

namespace {

// bytes of the column state of the workgroup form beyond kBlock columns: minv, v, then way, rowof, used
int64_t state_bytes(int64_t nc) { return nc > kBlock ? ((2 * 8 + 3 * 4) * nc + 7) / 8 * 8 : 0; }

const void *solve_kernel(const lpg_assign *a) {
    const bool reg = a->nc <= kBlock;
    if (a->form == LPG_ASSIGN_FORM_WAVE) return (const void *)k_assign_wave;
    if (a->tier == LPG_BATCH_TIER_LDS)
        return reg ? (const void *)k_assign_wg<LPG_BATCH_TIER_LDS, true> : (const void *)k_assign_wg<LPG_BATCH_TIER_LDS, false>;
    return reg ? (const void *)k_assign_wg<LPG_BATCH_TIER_GLOBAL, true> : (const void *)k_assign_wg<LPG_BATCH_TIER_GLOBAL, false>;
}

}  // namespace

extern "C" {

const char *lpg_assign_last_error(const lpg_assign *a) { return a ? a->err : thread_err<lpg_assign>(); }

int lpg_assign_create(lpg_assign **out, int device, int64_t count, int64_t nr, int64_t nc, uint32_t flags) {
    const char *call = "lpg_assign_create";
    lpg_assign *a = nullptr;           // not made yet: the refusals below go to the thread's buffer only
    if (!out) return fail(a, LPG_ERR_ARG, "%s: out is NULL", call);
    *out = nullptr;
    if (count < 1 || nr < 1 || nr > nc)
        return fail(a, LPG_ERR_ARG, "%s: bad shape count=%lld nr=%lld nc=%lld (need count >= 1 and "
                                    "1 <= nr <= nc; a matrix with more rows than columns is solved transposed)", call,
                    (long long)count, (long long)nr, (long long)nc);
    if (nc > LPG_BATCH_MAX_DIM)
        return fail(a, LPG_ERR_ARG, "%s: nc = %lld exceeds LPG_BATCH_MAX_DIM = %d", call, (long long)nc,
                    LPG_BATCH_MAX_DIM);
    if (flags & ~(uint32_t)LPG_ASSIGN_MAXIMIZE)
        return fail(a, LPG_ERR_ARG, "%s: flags 0x%x not supported (LPG_ASSIGN_MAXIMIZE only)", call, flags);
    if (device < 0) return fail(a, LPG_ERR_ARG, "%s: device %d", call, device);
    if (count > (int64_t)0x7fffffff / nr)
        return fail(a, LPG_ERR_ARG, "%s: count * nr = %lld x %lld exceeds 2^31 - 1", call, (long long)count,
                    (long long)nr);
    a = new lpg_assign();
    a->device = device;
    a->count = count;
    a->nr = nr;
    a->nc = nc;
    a->flags = flags;
    a->have.assign((size_t)count, 0);
    const int64_t cbytes = 8 * nr * nc, ubytes = 8 * nr;
    // only the workgroup form has a global tier, so forcing that tier picks the form as well
    const bool force_global = env_is("LPG_ASSIGN_TIER", "global");
    if (nc <= 64 && !force_global && !env_is("LPG_ASSIGN_FORM", "workgroup")) {
        // four problems' C and u; 64 x 64 is 4 x 33,280 bytes, inside the cap
        a->form = LPG_ASSIGN_FORM_WAVE;
        a->tier = LPG_BATCH_TIER_LDS;
        a->lds = kWaveProblems * (cbytes + ubytes);
    } else {
        a->form = LPG_ASSIGN_FORM_WORKGROUP;
        const int64_t sbytes = state_bytes(nc);
        if (!force_global && ubytes + cbytes + sbytes <= kAssignMaxLds) {
            a->tier = LPG_BATCH_TIER_LDS;
            a->lds = ubytes + cbytes + sbytes;
        } else {
            a->tier = LPG_BATCH_TIER_GLOBAL;
            a->state_lds = ubytes + sbytes <= kAssignMaxLds;
            a->lds = ubytes + (a->state_lds ? sbytes : 0);
            a->scratch_stride = a->state_lds ? 0 : sbytes;
        }
    }
    const int64_t cb = count * nr * nc * (int64_t)sizeof(double);
    a->allocs = {dev_array(a->C, count * nr * nc), dev_array(a->u, count * nr), dev_array(a->v, count * nc),
                 dev_array(a->col, count * nr), dev_array(a->res, count),
                 dev_array(a->scratch, a->state_lds ? 0 : count * a->scratch_stride)};
    snprintf(a->oom_what, sizeof a->oom_what, "batch of %lld cost matrices, %zu bytes", (long long)count, (size_t)cb);
    *out = a;
    return 0;
}

void lpg_assign_destroy(lpg_assign *a) { destroy(a); }

int lpg_assign_info(const lpg_assign *a, lpg_assign_info_t *out) {
    if (!a) return fail<lpg_assign>(nullptr, LPG_ERR_ARG, "lpg_assign_info: the batch is NULL");
    if (!out) return fail(const_cast<lpg_assign *>(a), LPG_ERR_ARG, "lpg_assign_info: out is NULL");
    out->count = a->count;
    out->nr = a->nr;
    out->nc = a->nc;
    out->tier = a->tier;
    out->form = a->form;
    out->lds_bytes = a->lds;
    out->kernel_ms = a->kernel_ms;
    return 0;
}

int lpg_assign_load(lpg_assign *a, int64_t first, int64_t n, const double *costs, int64_t ld) {
    const char *call = "lpg_assign_load";
    if (!a) return fail(a, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (!costs) return fail(a, LPG_ERR_ARG, "%s: costs is NULL", call);
    if (int rc = range_ok(a, call, first, n)) return rc;
    if (ld < a->nc) return fail(a, LPG_ERR_ARG, "%s: ld %lld < nc = %lld", call, (long long)ld, (long long)a->nc);
    const int64_t nr = a->nr, nc = a->nc;
    const bool mx = (a->flags & LPG_ASSIGN_MAXIMIZE) != 0;
    std::vector<double> stage((size_t)(n * nr * nc));
    for (int64_t p = 0; p < n; p++)
        for (int64_t i = 0; i < nr; i++)
            for (int64_t j = 0; j < nc; j++) {
                const double c = costs[(p * nr + i) * ld + j];
                // +inf passes (a forbidden pair); NaN, -inf and |c| > the cap do not
                if (!(c == INFINITY) && !(fabs(c) <= LPG_ASSIGN_COST_CAP))
                    return fail(a, LPG_ERR_ARG, "%s: problem %lld, entry (%lld, %lld) is %s; costs are +inf (a forbidden "
                                                "pair) or finite with |c| <= 2^1000; nothing was loaded", call,
                                (long long)(first + p), (long long)i, (long long)j,
                                c != c ? "NaN" : c == -INFINITY ? "-inf" : "above the cap 2^1000 in magnitude");
                stage[(size_t)((p * nr + i) * nc + j)] = (mx && c != INFINITY) ? -c : c;
            }
    if (int rc = ensure_device(a, call)) return rc;
    LPG_HIPCHK(a, hipMemcpy(a->C + first * nr * nc, stage.data(), stage.size() * sizeof(double), hipMemcpyHostToDevice));
    mark_loaded(a, first, n);
    a->solved = false;
    return 0;
}

int lpg_assign_generate(lpg_assign *a, uint64_t seed, int64_t range) {
    const char *call = "lpg_assign_generate";
    if (!a) return fail(a, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (range < 1 || range > ((int64_t)1 << 53))
        return fail(a, LPG_ERR_ARG, "%s: range %lld outside 1..2^53", call, (long long)range);
    if (int rc = ensure_device(a, call)) return rc;
    const int64_t per = a->nr * a->nc, total = a->count * per;
    hipLaunchKernelGGL(k_assign_generate, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, a->stream, a->C,
                       a->count, per, seed, (double)range, (a->flags & LPG_ASSIGN_MAXIMIZE) ? 1 : 0);
    LPG_HIPCHK(a, hipGetLastError());
    LPG_HIPCHK(a, hipStreamSynchronize(a->stream));
    mark_all_loaded(a);
    a->solved = false;
    return 0;
}

int lpg_assign_solve(lpg_assign *a, lpg_assign_result *out) {
    const char *call = "lpg_assign_solve";
    if (!a) return fail(a, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (!a->loaded)
        return fail(a, LPG_ERR_STATE, "%s: problem %lld has no costs yet (lpg_assign_load or lpg_assign_generate first)",
                    call, (long long)first_unloaded(a));
    if (int rc = ensure_device(a, call)) return rc;
    AssignGeo g{};
    g.C = a->C;
    g.u = a->u;
    g.v = a->v;
    g.col = a->col;
    g.res = a->res;
    g.scratch = a->scratch;
    g.scratch_stride = a->scratch_stride;
    g.count = a->count;
    g.nr = (int32_t)a->nr;
    g.nc = (int32_t)a->nc;
    g.maximize = (a->flags & LPG_ASSIGN_MAXIMIZE) ? 1 : 0;
    g.state_lds = a->state_lds ? 1 : 0;
    // One launch, no chunk / relaunch scheme: row i's search marks a new column
    // used in every step and ends at the first free one, so it takes at most
    // i + 1 steps whatever the arithmetic does, nr (nr + 1) / 2 per problem.
    const void *kern = solve_kernel(a);
    const unsigned grid = (unsigned)(a->form == LPG_ASSIGN_FORM_WAVE ? (a->count + kWaveProblems - 1) / kWaveProblems : a->count);
    if (int rc = raise_lds_once(a, kern, kAssignMaxLds, call)) return rc;
    LPG_HIPCHK(a, timed_launch(a, kern, grid, g));
    LPG_HIPCHK(a, hipStreamSynchronize(a->stream));
    a->solved = true;
    float ms = 0.0f;
    LPG_HIPCHK(a, hipEventElapsedTime(&ms, a->ev0, a->ev1));
    a->kernel_ms = ms;
    if (out) LPG_HIPCHK(a, hipMemcpy(out, a->res, (size_t)a->count * sizeof(lpg_assign_result), hipMemcpyDeviceToHost));
    return 0;
}

int lpg_assign_get(lpg_assign *a, int64_t first, int64_t n, int64_t *col, double *u, double *v) {
    const char *call = "lpg_assign_get";
    if (!a) return fail(a, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (!col && !u && !v) return fail(a, LPG_ERR_ARG, "%s: col, u and v are all NULL", call);
    if (int rc = range_ok(a, call, first, n)) return rc;
    if (!a->solved) return fail(a, LPG_ERR_STATE, "%s: no solve since the last load or generate", call);
    LPG_HIPCHK(a, hipSetDevice(a->device));
    if (col) {
        std::vector<int32_t> c32((size_t)(n * a->nr));
        LPG_HIPCHK(a, hipMemcpy(c32.data(), a->col + first * a->nr, c32.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < c32.size(); e++) col[e] = c32[e];
    }
    if (u) LPG_HIPCHK(a, hipMemcpy(u, a->u + first * a->nr, (size_t)(n * a->nr) * sizeof(double), hipMemcpyDeviceToHost));
    if (v) LPG_HIPCHK(a, hipMemcpy(v, a->v + first * a->nc, (size_t)(n * a->nc) * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
