// lpg_transport.hip — batches of balanced transportation problems (include/lpg.h,
// "transportation"): a northwest-corner or least-cost start, then potentials
// (MODI), pricing and the closed-loop adjustment, one problem per wave (nr + nc
// <= 64, four problems per workgroup) or per workgroup, no communication
// between problems. Host code and launches live in this file like the other
// translation units'.
//
// All data are integers held in fp64 inside the caps of lpg.h, so every
// subtraction, addition, product and comparison below is exact: no order of
// evaluation, no form and no tier can change a bit. What the header fixes are
// the choices: the start's cell order, the entering cell (argmin over the
// total-order key of the reduced cost, ties to the smallest cell index), the
// leaving cell (the smallest flow on a minus cell, ties to the smallest cell
// index). The tree of basic cells is rebuilt from the cell list in every
// iteration (levels from row 0), so the state that crosses a launch is the
// cell list, the flows, the iteration count and the status and nothing else.
//
// One kernel body serves both forms: NT = 64 threads of a problem (the wave
// form: the only synchronisation is the wave's own, a finished or idle wave
// leaves at once) or NT = 256 (the workgroup form, workgroup barriers). Every
// compare-and-keep is a per-field select on one predicate (lpg_device.h).
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

constexpr int kTransportMaxLds = 150 * 1024;   // dynamic LDS cap, as lpg_batch.hip's kBatchMaxLds
constexpr int kTransportWaves = kBlock / 64;   // wave form: problems per workgroup
constexpr int kNodeBytes = 32;                 // LDS per node: pot, flow (fp64); cell, pred, depth, sgn (int32)

struct TransportGeo {
    const double *C;       // count x nr x nc, internal (0.0 - c for a maximisation)
    const double *S, *D;   // count x nr, count x nc
    int32_t *cell;         // state: count x (nr + nc - 1) basic cells, (i << 16) | j, in slot order
    double *flow;          // state: their flows
    lpg_transport_result *res;
    double *x, *u, *v;     // outputs
    int32_t *basis;        // count x (nr + nc - 1) cell indices i * nc + j, ascending
    int32_t *running;      // problems this launch left unfinished with budget to come
    int64_t count;
    int32_t nr, nc;
    int32_t maximize, northwest, rule;
    int32_t budget;        // iterations this launch may apply per problem
    int32_t final;         // the call's last launch: a problem out of budget is LPG_ITER_LIMIT
};

__global__ __launch_bounds__(kBlock) void k_transport_gen_costs(double *C, int64_t count, int64_t per, uint64_t seed,
                                                                double range, int maximize) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= count * per) return;
    const int64_t q = e / per;
    const double c = floor(uniform01(seed + (uint64_t)q, (uint64_t)(e - q * per)) * range);
    C[e] = maximize ? 0.0 - c : c;
}

// one thread per problem: the supplies, the demands, and the difference onto the smaller side's last entry
__global__ __launch_bounds__(kBlock) void k_transport_gen_amounts(double *S, double *D, int64_t count, int nr, int nc,
                                                                  uint64_t seed, double qmax) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= count) return;
    const uint64_t key = seed + (uint64_t)q, base = (uint64_t)nr * (uint64_t)nc;
    double *s = S + q * nr, *d = D + q * nc;
    double ss = 0.0, sd = 0.0;
    for (int i = 0; i < nr; i++) {
        s[i] = 1.0 + floor(uniform01(key, base + (uint64_t)i) * qmax);
        ss = ss + s[i];
    }
    for (int j = 0; j < nc; j++) {
        d[j] = 1.0 + floor(uniform01(key, base + (uint64_t)nr + (uint64_t)j) * qmax);
        sd = sd + d[j];
    }
    if (ss > sd) d[nc - 1] = d[nc - 1] + (ss - sd);
    else s[nr - 1] = s[nr - 1] + (sd - ss);
}

// the threads of one problem meet: the wave's own order (NT == 64) or the workgroup barrier
template <int NT>
__device__ __forceinline__ void tsync() {
    if constexpr (NT == 64) wave_fence();
    else __syncthreads();
}

// tsync, and whether any thread of the problem holds p
template <int NT>
__device__ __forceinline__ bool tsync_any(bool p) {
    if constexpr (NT == 64) {
        wave_fence();
        const bool any = __ballot(p) != 0ull;
        wave_fence();
        return any;
    } else {
        return __syncthreads_count(p) != 0;
    }
}

// The smallest key (h, l) over the threads of one problem, in every thread.
// NT == 256: the waves' keys alternate between two LDS slots, so one barrier
// serves a call (a wave still reading slot `par` has passed the barrier of the
// call that wrote it, and the next write to that slot is two barriers later).
template <int NT>
__device__ __forceinline__ void problem_min_key(uint64_t &h, uint32_t &l, uint64_t (*sh)[kBlock / 64],
                                                uint32_t (*sl)[kBlock / 64], int &par) {
    wave_min_key(h, l);
    if constexpr (NT > 64) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        if (lane == 0) {
            sh[par][w] = h;
            sl[par][w] = l;
        }
        __syncthreads();
        uint64_t fh = sh[par][0];
        uint32_t fl = sl[par][0];
#pragma unroll
        for (int k = 1; k < kBlock / 64; k++) {
            const uint64_t kh = sh[par][k];
            const uint32_t kl = sl[par][k];
            const bool better = (kh < fh) | ((kh == fh) & (kl < fl));
            fh = better ? kh : fh;
            fl = better ? kl : fl;
        }
        par ^= 1;
        h = fh;
        l = fl;
    }
}

// NT threads per problem; TIER: C in the problem's LDS, or in device memory
// with coalesced row reads. Per problem in LDS, 32 bytes a node: pot (the
// potentials, rows then columns; the remaining amounts during the start), flow
// and cell (the basis by slot), pred (a node's slot towards row 0), depth (its
// level; the open flags during the start), sgn (a slot's sign on the loop).
template <int NT, int TIER>
__global__ __launch_bounds__(kBlock) void k_transport(TransportGeo g) {
    extern __shared__ double lds[];
    __shared__ uint64_t sh[2][kBlock / 64];
    __shared__ uint32_t sl[2][kBlock / 64];
    __shared__ double s_theta[kBlock / 64], s_obj[kBlock / 64];
    __shared__ int s_leave[kBlock / 64];
    const int tid = NT == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int w = NT == 64 ? (int)(threadIdx.x >> 6) : 0;
    const int64_t q = NT == 64 ? (int64_t)blockIdx.x * kTransportWaves + w : (int64_t)blockIdx.x;
    if (q >= g.count) return;                  // an idle wave of the last workgroup: before any memory access
    lpg_transport_result r = g.res[q];
    if (r.status == OPTIMAL || r.status == NUMERIC) return;      // uniform over the problem's threads

    const int nr = g.nr, nc = g.nc, nn = nr + nc, nb = nn - 1, ncell = nr * nc;
    const size_t per = (size_t)4 * nn + (TIER == LPG_BATCH_TIER_LDS ? (size_t)ncell : 0);
    double *pot = lds + (size_t)w * per, *flow = pot + nn;
    int *cell = (int *)(pot + 2 * (size_t)nn), *pred = cell + nn, *depth = pred + nn, *sgn = depth + nn;
    const double *C = g.C + q * (int64_t)ncell;
    if (TIER == LPG_BATCH_TIER_LDS) {
        double *Cl = pot + 4 * (size_t)nn;
        for (int e = tid; e < ncell; e += NT) Cl[e] = C[e];
        C = Cl;
    }
    int32_t *cell_g = g.cell + q * nb;
    double *flow_g = g.flow + q * nb;
    int par = 0;
    // this thread's first cell and its stride, as (row, column)
    const int i_first = tid / nc, j_first = tid - i_first * nc;
    const int i_step = NT / nc, j_step = NT - i_step * nc;

    for (int k = tid; k < nn; k += NT) sgn[k] = 0;
    if (!r.started) {
        const double *S = g.S + q * nr, *D = g.D + q * nc;
        for (int k = tid; k < nn; k += NT) {
            pot[k] = k < nr ? S[k] : D[k - nr];
            depth[k] = 1;
        }
        tsync<NT>();
        if (g.northwest) {
            if (tid == 0) {
                int i = 0, j = 0;
                double rs = pot[0], rd = pot[nr];
                for (int k = 0; k < nb; k++) {
                    const double x = rd < rs ? rd : rs;
                    cell[k] = (i << 16) | j;
                    flow[k] = x;
                    rs = rs - x;
                    rd = rd - x;
                    if (k == nb - 1) break;
                    if (rs == 0.0 && i < nr - 1) rs = pot[++i];
                    else rd = pot[nr + ++j];
                }
            }
        } else {
            int rows_open = nr;
            for (int k = 0; k < nb; k++) {
                uint64_t bh = ~0ull;
                uint32_t bl = ~0u;
                for (int e = tid, i = i_first, j = j_first; e < ncell; e += NT) {
                    const bool cand = (depth[i] & depth[nr + j]) != 0;
                    const uint64_t h = cand ? order_key(C[e]) : ~0ull;
                    const uint32_t l = cand ? (uint32_t)e : ~0u;
                    const bool better = (h < bh) | ((h == bh) & (l < bl));
                    bh = better ? h : bh;
                    bl = better ? l : bl;
                    i += i_step;
                    j += j_step;
                    const bool wrap = j >= nc;
                    j = wrap ? j - nc : j;
                    i = wrap ? i + 1 : i;
                }
                problem_min_key<NT>(bh, bl, sh, sl, par);
                // an open cell always exists (balance, lpg.h); a guard against reading past the arrays all the same
                const int e = bl < (uint32_t)ncell ? (int)bl : 0;
                const int i = e / nc, j = e - i * nc;
                const double rs = pot[i], rd = pot[nr + j];
                const double x = rd < rs ? rd : rs;
                const bool close_row = (rs - x == 0.0) & ((rd - x != 0.0) | (rows_open > 1));
                tsync<NT>();                   // every thread has read the amounts
                if (tid == 0) {
                    cell[k] = (i << 16) | j;
                    flow[k] = x;
                    pot[i] = rs - x;
                    pot[nr + j] = rd - x;
                    if (k < nb - 1) depth[close_row ? i : nr + j] = 0;
                }
                rows_open -= close_row ? 1 : 0;
                tsync<NT>();
            }
        }
        r.started = 1;
        r.iterations = 0;
    } else {
        for (int k = tid; k < nb; k += NT) {
            cell[k] = cell_g[k];
            flow[k] = flow_g[k];
        }
    }
    tsync<NT>();

    int done = 0, status = RUNNING;
    for (;;) {
        // 1. potentials, predecessors and depths by levels from row 0
        for (int k = tid; k < nn; k += NT) depth[k] = k ? -1 : 0;
        if (tid == 0) {
            pot[0] = 0.0;
            pred[0] = -1;
        }
        tsync<NT>();
        for (int level = 1; level <= nn; level++) {
            bool found = false;
            for (int k = tid; k < nb; k += NT) {
                const int pc = cell[k], i = pc >> 16, jn = nr + (pc & 0xffff);
                const int di = depth[i], dj = depth[jn];
                // known before this level; a node found in this level reads as -1 or as `level`
                const bool kr = (di >= 0) & (di < level), kc = (dj >= 0) & (dj < level);
                if (kr != kc) {
                    const int src = kr ? i : jn, dst = kr ? jn : i;
                    pot[dst] = C[i * nc + (pc & 0xffff)] - pot[src];
                    pred[dst] = k;
                    depth[dst] = level;
                    found = true;
                }
            }
            if (!tsync_any<NT>(found)) break;
        }

        // 2. pricing
        uint64_t bh = ~0ull;
        uint32_t bl = ~0u;
        const bool bland = g.rule == RULE_BLAND;
        for (int e = tid, i = i_first, j = j_first; e < ncell; e += NT) {
            const double dl = (C[e] - pot[i]) - pot[nr + j];
            const bool neg = dl < 0.0;
            const uint64_t h = neg ? (bland ? 0ull : order_key(dl)) : ~0ull;
            const uint32_t l = neg ? (uint32_t)e : ~0u;
            const bool better = (h < bh) | ((h == bh) & (l < bl));
            bh = better ? h : bh;
            bl = better ? l : bl;
            i += i_step;
            j += j_step;
            const bool wrap = j >= nc;
            j = wrap ? j - nc : j;
            i = wrap ? i + 1 : i;
        }
        problem_min_key<NT>(bh, bl, sh, sl, par);
        if (bh == ~0ull) {                     // uniform: no negative reduced cost
            status = OPTIMAL;
            break;
        }
        if (done == g.budget) {
            status = g.final ? ITER_LIMIT : RUNNING;
            break;
        }

        // 3. the closed loop: from the entering cell's column up and from its row up until the two meet
        const int ie = (int)bl / nc, je = (int)bl - ie * nc;
        if (tid == 0) {
            int a = nr + je, b = ie, ka = 0, kb = 0, leave = -1, leave_cell = 0x7fffffff;
            double theta = INFINITY;
            for (int step = 0; a != b && step < nn; step++) {
                const bool ua = depth[a] >= depth[b];
                const int n = ua ? a : b, s = ua ? ka : kb;
                const int slot = pred[n];
                if (slot < 0) break;           // not a tree (cannot happen): reported as LPG_NUMERIC below
                const int pc = cell[slot];
                const int parent = n < nr ? nr + (pc & 0xffff) : (pc >> 16);
                const bool minus = (s & 1) == 0;
                sgn[slot] = minus ? -1 : 1;
                const double f = flow[slot];
                const bool better = minus & ((f < theta) | ((f == theta) & (pc < leave_cell)));
                theta = better ? f : theta;
                leave = better ? slot : leave;
                leave_cell = better ? pc : leave_cell;
                a = ua ? parent : a;
                b = ua ? b : parent;
                ka += ua ? 1 : 0;
                kb += ua ? 0 : 1;
            }
            s_theta[w] = theta;
            s_leave[w] = a == b ? leave : -1;
        }
        tsync<NT>();
        const double theta = s_theta[w];
        const int leave = s_leave[w];
        if (leave < 0) {                       // uniform
            status = NUMERIC;
            break;
        }
        for (int k = tid; k < nb; k += NT) {
            const int sg = sgn[k];
            const double f = flow[k];
            flow[k] = k == leave ? theta : sg < 0 ? f - theta : sg > 0 ? f + theta : f;
            if (k == leave) cell[k] = (ie << 16) | je;
            sgn[k] = 0;
        }
        r.iterations++;
        done++;
        tsync<NT>();
    }

    for (int k = tid; k < nb; k += NT) {
        cell_g[k] = cell[k];
        flow_g[k] = flow[k];
    }
    double obj = NAN;
    if (status == OPTIMAL || status == ITER_LIMIT) {             // uniform: the outputs of the basis as it stands
        const int mx = g.maximize;
        double *uo = g.u + q * nr, *vo = g.v + q * nc, *xo = g.x + q * (int64_t)ncell;
        int32_t *bo = g.basis + q * nb;
        for (int k = tid; k < nn; k += NT) {
            const double p = mx ? 0.0 - pot[k] : pot[k];
            if (k < nr) uo[k] = p;
            else vo[k - nr] = p;
        }
        for (int e = tid; e < ncell; e += NT) xo[e] = 0.0;
        if (tid == 0) s_obj[w] = 0.0;
        __threadfence_block();                 // the zeros are in place before a flow lands on one of them
        tsync<NT>();
        double part = 0.0;
        for (int k = tid; k < nb; k += NT) {
            const int pc = cell[k], e = (pc >> 16) * nc + (pc & 0xffff);
            const double f = flow[k];
            xo[e] = f;
            part = part + C[e] * f;            // exact integers: any order
            int rank = 0;
            for (int m = 0; m < nb; m++) rank += cell[m] < pc ? 1 : 0;
            bo[rank] = e;
        }
        atomicAdd(&s_obj[w], part);
        tsync<NT>();
        obj = mx ? 0.0 - s_obj[w] : s_obj[w];
    }
    if (tid == 0) {
        r.status = status;
        r.objective = obj;
        g.res[q] = r;
        if (status == RUNNING) atomicAdd(g.running, 1);
    }
}

}  // namespace lpg

using namespace lpg;

struct lpg_transport : BatchHost {
    int64_t nr = 0, nc = 0;
    uint32_t flags = 0;
    int tier = LPG_BATCH_TIER_LDS, form = LPG_TRANSPORT_FORM_WAVE;
    int chunk = LPG_TRANSPORT_DEFAULT_CHUNK;
    double *C = nullptr, *S = nullptr, *D = nullptr, *flow = nullptr, *x = nullptr, *u = nullptr, *v = nullptr;
    int32_t *cell = nullptr, *basis = nullptr, *running = nullptr;
    lpg_transport_result *res = nullptr;
};

namespace {

constexpr double kTwo53 = 0x1p53;
typedef unsigned __int128 u128;

// a u128 below 2^80 in decimal
const char *dec(u128 x, char *buf, size_t n) {
    char tmp[48];
    int k = 0;
    do {
        tmp[k++] = (char)('0' + (int)(x % 10));
        x /= 10;
    } while (x && k < 47);
    size_t o = 0;
    while (k && o + 1 < n) buf[o++] = tmp[--k];
    buf[o] = '\0';
    return buf;
}

// The shared device side, and with it every problem's result "not started". A
// setup that fails here is taken down like one that fails in the shared part.
int device_ready(lpg_transport *t, const char *call) {
    const bool made = !t->on_device;
    if (int rc = ensure_device(t, call)) return rc;
    if (!made) return 0;
    const hipError_t e = hipMemset(t->res, 0, (size_t)t->count * sizeof(lpg_transport_result));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        release_device(t);
        return fail(t, LPG_ERR_DEVICE, "%s: stream and events: %s", call, hipGetErrorString(e));
    }
    return 0;
}

const void *solve_kernel(const lpg_transport *t) {
    if (t->form == LPG_TRANSPORT_FORM_WAVE) return (const void *)k_transport<64, LPG_BATCH_TIER_LDS>;
    return t->tier == LPG_BATCH_TIER_LDS ? (const void *)k_transport<kBlock, LPG_BATCH_TIER_LDS>
                                         : (const void *)k_transport<kBlock, LPG_BATCH_TIER_GLOBAL>;
}

const char *why_not_amount(double a) {
    return a != a ? "NaN" : (a == INFINITY || a == -INFINITY) ? "infinite" : a < 0.0 ? "negative" : a != floor(a) ? "not an integer"
           : a > kTwo53 ? "above 2^53" : nullptr;
}

}  // namespace

extern "C" {

const char *lpg_transport_last_error(const lpg_transport *t) { return t ? t->err : thread_err<lpg_transport>(); }

int lpg_transport_create(lpg_transport **out, int device, int64_t count, int64_t nr, int64_t nc, uint32_t flags) {
    const char *call = "lpg_transport_create";
    lpg_transport *t = nullptr;           // not made yet: the refusals below go to the thread's buffer only
    if (!out) return fail(t, LPG_ERR_ARG, "%s: out is NULL", call);
    *out = nullptr;
    if (count < 1 || nr < 1 || nc < 1)
        return fail(t, LPG_ERR_ARG, "%s: bad shape count=%lld nr=%lld nc=%lld (need count >= 1, nr >= 1, nc >= 1)", call,
                    (long long)count, (long long)nr, (long long)nc);
    if (nr > LPG_TRANSPORT_MAX_NODES || nc > LPG_TRANSPORT_MAX_NODES || nr + nc > LPG_TRANSPORT_MAX_NODES)
        return fail(t, LPG_ERR_ARG, "%s: nr + nc = %lld + %lld exceeds LPG_TRANSPORT_MAX_NODES = %d", call,
                    (long long)nr, (long long)nc, LPG_TRANSPORT_MAX_NODES);
    if (flags & ~(uint32_t)(LPG_TRANSPORT_MAXIMIZE | LPG_TRANSPORT_START_NORTHWEST))
        return fail(t, LPG_ERR_ARG, "%s: flags 0x%x not supported (LPG_TRANSPORT_MAXIMIZE, "
                                    "LPG_TRANSPORT_START_NORTHWEST)", call, flags);
    if (device < 0) return fail(t, LPG_ERR_ARG, "%s: device %d", call, device);
    if (count > (int64_t)0x7fffffff / (nr * nc) || count > (int64_t)0x7fffffff / (nr + nc))
        return fail(t, LPG_ERR_ARG, "%s: count * nr * nc = %lld x %lld x %lld exceeds 2^31 - 1", call, (long long)count,
                    (long long)nr, (long long)nc);
    int chunk = LPG_TRANSPORT_DEFAULT_CHUNK;
    if (const char *e = getenv("LPG_TRANSPORT_CHUNK")) {
        char *end = nullptr;
        const long c = strtol(e, &end, 10);
        if (end == e || *end || c < 1 || c > (1 << 30))
            return fail(t, LPG_ERR_ARG, "%s: LPG_TRANSPORT_CHUNK=\"%s\" is not an integer in 1..2^30", call, e);
        chunk = (int)c;
    }
    t = new lpg_transport();
    t->device = device;
    t->count = count;
    t->nr = nr;
    t->nc = nc;
    t->flags = flags;
    t->chunk = chunk;
    t->have.assign((size_t)count, 0);
    const int64_t nbytes = kNodeBytes * (nr + nc), cbytes = 8 * nr * nc;
    // only the workgroup form has a global tier, so forcing that tier picks the form as well
    const bool force_global = env_is("LPG_TRANSPORT_TIER", "global");
    if (nr + nc <= 64 && !force_global && !env_is("LPG_TRANSPORT_FORM", "workgroup")) {
        // four problems' nodes and C; 32 x 32 is 4 x 10,240 bytes, inside the cap
        t->form = LPG_TRANSPORT_FORM_WAVE;
        t->tier = LPG_BATCH_TIER_LDS;
        t->lds = kTransportWaves * (nbytes + cbytes);
    } else {
        t->form = LPG_TRANSPORT_FORM_WORKGROUP;
        if (!force_global && nbytes + cbytes <= kTransportMaxLds) {
            t->tier = LPG_BATCH_TIER_LDS;
            t->lds = nbytes + cbytes;
        } else {
            t->tier = LPG_BATCH_TIER_GLOBAL;
            t->lds = nbytes;                   // 4096 nodes: 128 KiB
        }
    }
    const int64_t cells = count * nr * nc, nb = count * (nr + nc - 1);
    t->allocs = {dev_array(t->C, cells), dev_array(t->x, cells), dev_array(t->S, count * nr), dev_array(t->u, count * nr),
                 dev_array(t->D, count * nc), dev_array(t->v, count * nc), dev_array(t->flow, nb), dev_array(t->cell, nb),
                 dev_array(t->basis, nb), dev_array(t->running, 1), dev_array(t->res, count)};
    snprintf(t->oom_what, sizeof t->oom_what, "batch of %lld problems, %zu bytes of costs", (long long)count,
             (size_t)cells * 8);
    *out = t;
    return 0;
}

void lpg_transport_destroy(lpg_transport *t) { destroy(t); }

int lpg_transport_info(const lpg_transport *t, lpg_transport_info_t *out) {
    if (!t) return fail<lpg_transport>(nullptr, LPG_ERR_ARG, "lpg_transport_info: the batch is NULL");
    if (!out) return fail(const_cast<lpg_transport *>(t), LPG_ERR_ARG, "lpg_transport_info: out is NULL");
    out->count = t->count;
    out->nr = t->nr;
    out->nc = t->nc;
    out->tier = t->tier;
    out->form = t->form;
    out->start = (t->flags & LPG_TRANSPORT_START_NORTHWEST) ? LPG_TRANSPORT_START_NORTHWEST : LPG_TRANSPORT_START_LEAST_COST;
    out->chunk = t->chunk;
    out->lds_bytes = t->lds;
    out->launches = t->launches;
    out->kernel_ms = t->kernel_ms;
    return 0;
}

int lpg_transport_load(lpg_transport *t, int64_t first, int64_t n, const double *costs, int64_t ld, const double *supply,
                       const double *demand) {
    const char *call = "lpg_transport_load";
    if (!t) return fail(t, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (!costs) return fail(t, LPG_ERR_ARG, "%s: costs is NULL", call);
    if (!supply) return fail(t, LPG_ERR_ARG, "%s: supply is NULL", call);
    if (!demand) return fail(t, LPG_ERR_ARG, "%s: demand is NULL", call);
    if (int rc = range_ok(t, call, first, n)) return rc;
    if (ld < t->nc) return fail(t, LPG_ERR_ARG, "%s: ld %lld < nc = %lld", call, (long long)ld, (long long)t->nc);
    const int64_t nr = t->nr, nc = t->nc;
    const bool mx = (t->flags & LPG_TRANSPORT_MAXIMIZE) != 0;
    std::vector<double> stage((size_t)(n * nr * nc));
    char b1[48], b2[48];
    for (int64_t p = 0; p < n; p++) {
        const long long P = (long long)(first + p);
        double cmax = 0.0;
        for (int64_t i = 0; i < nr; i++)
            for (int64_t j = 0; j < nc; j++) {
                const double c = costs[(p * nr + i) * ld + j];
                const char *why = c != c ? "NaN" : (c == INFINITY || c == -INFINITY) ? "infinite" : c != floor(c) ? "not an integer"
                                  : fabs(c) > LPG_TRANSPORT_COST_CAP ? "above the cap 2^40 in magnitude" : nullptr;
                if (why)
                    return fail(t, LPG_ERR_ARG, "%s: problem %lld, cost (%lld, %lld) is %s; costs are integers with |c| <= "
                                                "2^40; nothing was loaded", call, P, (long long)i, (long long)j, why);
                cmax = fabs(c) > cmax ? fabs(c) : cmax;
                stage[(size_t)((p * nr + i) * nc + j)] = mx ? 0.0 - c : c + 0.0;
            }
        u128 ss = 0, sd = 0;
        for (int64_t i = 0; i < nr; i++) {
            const double a = supply[p * nr + i];
            if (const char *why = why_not_amount(a))
                return fail(t, LPG_ERR_ARG, "%s: problem %lld, supply %lld is %s; supplies are integers in 0..2^53; nothing "
                                            "was loaded", call, P, (long long)i, why);
            ss += (u128)(uint64_t)a;
        }
        for (int64_t j = 0; j < nc; j++) {
            const double a = demand[p * nc + j];
            if (const char *why = why_not_amount(a))
                return fail(t, LPG_ERR_ARG, "%s: problem %lld, demand %lld is %s; demands are integers in 0..2^53; nothing "
                                            "was loaded", call, P, (long long)j, why);
            sd += (u128)(uint64_t)a;
        }
        if (ss != sd)
            return fail(t, LPG_ERR_ARG, "%s: problem %lld is not balanced: the supplies sum to %s, the demands to %s; nothing "
                                        "was loaded", call, P, dec(ss, b1, sizeof b1), dec(sd, b2, sizeof b2));
        if (ss > ((u128)1 << 53))
            return fail(t, LPG_ERR_ARG, "%s: problem %lld: the supplies sum to %s, above 2^53; nothing was loaded", call, P,
                        dec(ss, b1, sizeof b1));
        if ((u128)(uint64_t)cmax * ss > ((u128)1 << 53))
            return fail(t, LPG_ERR_ARG, "%s: problem %lld: max |c| x sum of supplies = %s x %s exceeds 2^53; nothing was "
                                        "loaded", call, P, dec((u128)(uint64_t)cmax, b1, sizeof b1), dec(ss, b2, sizeof b2));
    }
    if (int rc = device_ready(t, call)) return rc;
    LPG_HIPCHK(t, hipMemcpy(t->C + first * nr * nc, stage.data(), stage.size() * sizeof(double), hipMemcpyHostToDevice));
    LPG_HIPCHK(t, hipMemcpy(t->S + first * nr, supply, (size_t)(n * nr) * sizeof(double), hipMemcpyHostToDevice));
    LPG_HIPCHK(t, hipMemcpy(t->D + first * nc, demand, (size_t)(n * nc) * sizeof(double), hipMemcpyHostToDevice));
    LPG_HIPCHK(t, hipMemset(t->res + first, 0, (size_t)n * sizeof(lpg_transport_result)));    // not started
    mark_loaded(t, first, n);
    t->solved = false;
    return 0;
}

int lpg_transport_generate(lpg_transport *t, uint64_t seed, int64_t range, int64_t qmax) {
    const char *call = "lpg_transport_generate";
    if (!t) return fail(t, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (range < 1 || range > ((int64_t)1 << 40) + 1)
        return fail(t, LPG_ERR_ARG, "%s: range %lld outside 1..2^40 + 1", call, (long long)range);
    if (qmax < 1 || qmax > ((int64_t)1 << 53))
        return fail(t, LPG_ERR_ARG, "%s: qmax %lld outside 1..2^53", call, (long long)qmax);
    const int64_t side = t->nr > t->nc ? t->nr : t->nc;
    // the larger sum is at most side * qmax; costs reach range - 1
    if ((u128)side * (u128)qmax > ((u128)1 << 53) || (u128)(range - 1) * (u128)side * (u128)qmax > ((u128)1 << 53))
        return fail(t, LPG_ERR_ARG, "%s: (range - 1) x max(nr, nc) x qmax = %lld x %lld x %lld may exceed 2^53", call,
                    (long long)(range - 1), (long long)side, (long long)qmax);
    if (int rc = device_ready(t, call)) return rc;
    const int64_t per = t->nr * t->nc, total = t->count * per;
    hipLaunchKernelGGL(k_transport_gen_costs, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, t->stream,
                       t->C, t->count, per, seed, (double)range, (t->flags & LPG_TRANSPORT_MAXIMIZE) ? 1 : 0);
    hipLaunchKernelGGL(k_transport_gen_amounts, dim3((unsigned)((t->count + kBlock - 1) / kBlock)), dim3(kBlock), 0, t->stream,
                       t->S, t->D, t->count, (int)t->nr, (int)t->nc, seed, (double)qmax);
    LPG_HIPCHK(t, hipGetLastError());
    LPG_HIPCHK(t, hipMemsetAsync(t->res, 0, (size_t)t->count * sizeof(lpg_transport_result), t->stream));
    LPG_HIPCHK(t, hipStreamSynchronize(t->stream));
    mark_all_loaded(t);
    t->solved = false;
    return 0;
}

int lpg_transport_solve(lpg_transport *t, int64_t max_iters, int rule, lpg_transport_result *out) {
    const char *call = "lpg_transport_solve";
    if (!t) return fail(t, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (max_iters < 1)
        return fail(t, LPG_ERR_ARG, "%s: max_iters = %lld (need >= 1: the rules do not exclude cycling, so there is no "
                                    "unbounded form)", call, (long long)max_iters);
    if (rule != LPG_RULE_DANTZIG && rule != LPG_RULE_BLAND)
        return fail(t, LPG_ERR_ARG, "%s: rule %d (LPG_RULE_DANTZIG or LPG_RULE_BLAND)", call, rule);
    if (!t->loaded)
        return fail(t, LPG_ERR_STATE, "%s: problem %lld has no data yet (lpg_transport_load or lpg_transport_generate first)",
                    call, (long long)first_unloaded(t));
    if (int rc = device_ready(t, call)) return rc;
    TransportGeo g{};
    g.C = t->C;
    g.S = t->S;
    g.D = t->D;
    g.cell = t->cell;
    g.flow = t->flow;
    g.res = t->res;
    g.x = t->x;
    g.u = t->u;
    g.v = t->v;
    g.basis = t->basis;
    g.running = t->running;
    g.count = t->count;
    g.nr = (int32_t)t->nr;
    g.nc = (int32_t)t->nc;
    g.maximize = (t->flags & LPG_TRANSPORT_MAXIMIZE) ? 1 : 0;
    g.northwest = (t->flags & LPG_TRANSPORT_START_NORTHWEST) ? 1 : 0;
    g.rule = rule;
    t->kernel_ms = 0.0;
    t->launches = 0;
    const void *kern = solve_kernel(t);
    const unsigned grid =
        (unsigned)(t->form == LPG_TRANSPORT_FORM_WAVE ? (t->count + kTransportWaves - 1) / kTransportWaves : t->count);
    // At most `chunk` iterations per problem and launch; the host relaunches while a problem is unfinished and the
    // call has budget left. The last launch of the call turns "out of budget" into LPG_ITER_LIMIT.
    for (int64_t remaining = max_iters;;) {
        g.budget = (int32_t)(remaining < t->chunk ? remaining : t->chunk);
        g.final = g.budget == remaining;
        LPG_HIPCHK(t, hipMemsetAsync(t->running, 0, sizeof(int32_t), t->stream));
        if (int rc = raise_lds_once(t, kern, kTransportMaxLds, call)) return rc;
        LPG_HIPCHK(t, timed_launch(t, kern, grid, g));
        LPG_HIPCHK(t, hipStreamSynchronize(t->stream));
        float ms = 0.0f;
        LPG_HIPCHK(t, hipEventElapsedTime(&ms, t->ev0, t->ev1));
        t->kernel_ms += ms;
        t->launches++;
        remaining -= g.budget;
        if (g.final) break;
        int32_t running = 0;
        LPG_HIPCHK(t, hipMemcpy(&running, t->running, sizeof running, hipMemcpyDeviceToHost));
        if (!running) break;
    }
    t->solved = true;
    if (out) LPG_HIPCHK(t, hipMemcpy(out, t->res, (size_t)t->count * sizeof(lpg_transport_result), hipMemcpyDeviceToHost));
    return 0;
}

int lpg_transport_get(lpg_transport *t, int64_t first, int64_t n, double *x, double *u, double *v, int64_t *basis) {
    const char *call = "lpg_transport_get";
    if (!t) return fail(t, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (!x && !u && !v && !basis) return fail(t, LPG_ERR_ARG, "%s: x, u, v and basis are all NULL", call);
    if (int rc = range_ok(t, call, first, n)) return rc;
    if (!t->solved) return fail(t, LPG_ERR_STATE, "%s: no solve since the last load or generate", call);
    LPG_HIPCHK(t, hipSetDevice(t->device));
    const int64_t nr = t->nr, nc = t->nc, nb = nr + nc - 1;
    if (x) LPG_HIPCHK(t, hipMemcpy(x, t->x + first * nr * nc, (size_t)(n * nr * nc) * sizeof(double), hipMemcpyDeviceToHost));
    if (u) LPG_HIPCHK(t, hipMemcpy(u, t->u + first * nr, (size_t)(n * nr) * sizeof(double), hipMemcpyDeviceToHost));
    if (v) LPG_HIPCHK(t, hipMemcpy(v, t->v + first * nc, (size_t)(n * nc) * sizeof(double), hipMemcpyDeviceToHost));
    if (basis) {
        std::vector<int32_t> b32((size_t)(n * nb));
        LPG_HIPCHK(t, hipMemcpy(b32.data(), t->basis + first * nb, b32.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < b32.size(); e++) basis[e] = b32[e];
    }
    return 0;
}

}  // extern "C"
