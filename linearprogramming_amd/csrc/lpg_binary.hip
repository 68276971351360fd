// lpg_binary.hip — batches of 0-1 programs by implicit enumeration
// (include/lpg.h, "0-1 programs"): a depth-first walk over partial assignments
// with interval tests per row and a bound on the objective. One wave per
// sub-search, four waves per workgroup, a constraint row per lane (1, 2 or 4
// rows per lane), a wave-wide vote per node. Host code and launches live in
// this file like the other translation units'.
//
// The arithmetic is the header's, operation for operation. On the integer data
// lpg_binary_load admits every sum stays an integer below 2^53, so every
// addition, subtraction and comparison is exact and unfixing a column (the same
// terms subtracted) restores the bits that stood before: a search keeps one row
// state, not one per level, and the device is held to the numpy statement bit
// for bit (tests/binary_cases.py).
//
// A launch visits at most `budget` nodes per sub-search; d, x, the second-value
// mask, z, the incumbent and the node count (BinSub) and the rows' lo / hi /
// comp round-trip through device memory between launches. Those are
// wave-uniform: the wave index goes through readfirstlane, so they are loaded
// and kept as scalars where the compiler allows. Memory is written with plain
// C++ stores from a lane.
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

constexpr int kBinaryMaxLds = 150 * 1024;      // dynamic LDS cap, as lpg_batch.hip's kBatchMaxLds
constexpr int kWaves = kBlock / 64;            // sub-searches per workgroup

struct BinSub {                                // one sub-search between launches
    uint64_t x, sec, inc_x;                    // fixed values, second-value mask, the incumbent's point
    double z, inc;
    int64_t nodes;
    int32_t d, running;
    int32_t found, pad;
};

struct BinaryGeo {
    double *At;            // count x n x m: A transposed
    double *L, *U;         // count x m
    double *c;             // count x n: the internal, minimising cost
    BinSub *sub;           // count << split
    double *rows;          // per sub-search lo[m], hi[m], comp[m]
    int32_t *running;      // sub-searches still running after this launch
    int64_t count, nsub;
    int32_t m, n, split, budget;
    int32_t maximize;
};

__device__ __forceinline__ uint64_t low_mask(int d) { return d >= 64 ? ~0ull : ((1ull << d) - 1ull); }

// The terms of fixing a column with entry a at value v (lpg.h, step 2); pj the
// column's preferred value. Unfixing subtracts the same three.
__device__ __forceinline__ void fix_terms(double a, int v, int pj, double &tl, double &th, double &tc) {
    tl = v ? fmax(0.0, a) : fmax(0.0, -a);
    th = v ? fmin(0.0, a) : -fmax(0.0, a);
    tc = (v != pj) ? (v ? a : -a) : 0.0;
}

__global__ __launch_bounds__(kBlock) void k_binary_generate(BinaryGeo g, uint64_t seed) {
    const int m = g.m, n = g.n;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= g.count * (int64_t)(m + n)) return;
    const int64_t q = e / (m + n);
    const int r = (int)(e - q * (m + n));
    const uint64_t key = seed + (uint64_t)q;
    if (r >= m) {
        const int j = r - m;
        const double cv = floor(uniform01(key, (uint64_t)(4 * m + n + j)) * 19.0) - 9.0;
        g.c[q * n + j] = g.maximize ? 0.0 - cv : cv + 0.0;
        return;
    }
    const int i = r, w = n < 3 ? n : 3;
    const int s = (m > 1 && n > 3) ? (int)(((int64_t)i * (n - 3)) / (m - 1)) : 0;     // s + w <= n
    double act = 0.0;
    for (int t = 0; t < w; t++) {
        const double a = floor(uniform01(key, (uint64_t)(4 * i + t)) * 9.0) - 4.0;
        const bool xp = uniform01(key, (uint64_t)(4 * m + s + t)) < 0.5;
        g.At[(q * n + (s + t)) * m + i] = a;       // the other entries of the row were zeroed by the caller
        act = xp ? act + a : act;
    }
    const double rr = uniform01(key, (uint64_t)(4 * i + 3));
    double lo = act, hi = act;
    if (rr >= 0.5) {
        if (rr < 0.75) { lo = -INFINITY; hi = act + 1.0; }
        else { lo = act - 1.0; hi = INFINITY; }
    }
    g.L[q * m + i] = lo;
    g.U[q * m + i] = hi;
}

// The root of every sub-search: the root sums of lpg.h, then the prefix columns
// t < split fixed at their first (bit t of k clear) or second value.
__global__ __launch_bounds__(kBlock) void k_binary_init(BinaryGeo g) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t s = (int64_t)blockIdx.x * kWaves + w;
    if (s >= g.nsub) return;
    const int m = g.m, n = g.n, split = g.split;
    const int64_t q = s >> split;
    const uint64_t k = (uint64_t)s & low_mask(split);
    const double *At = g.At + q * (int64_t)(n * m), *c = g.c + q * n;
    double z = 0.0;
    uint64_t x = 0;
    for (int j = 0; j < n; j++) z = z + fmin(0.0, c[j]);
    for (int t = 0; t < split; t++) {
        const int p = c[t] < 0.0, v = ((k >> t) & 1) ? !p : p;
        z = (v != p) ? z + fabs(c[t]) : z;
        x |= (uint64_t)v << t;
    }
    double *rs = g.rows + s * (int64_t)(3 * m);
    for (int r = lane; r < m; r += 64) {
        double lo = 0.0, hi = 0.0, cp = 0.0;
        for (int j = 0; j < n; j++) {
            const double a = At[j * m + r];
            lo = lo + fmin(0.0, a);
            hi = hi + fmax(0.0, a);
            cp = (c[j] < 0.0) ? cp + a : cp;
        }
        for (int t = 0; t < split; t++) {
            const int p = c[t] < 0.0, v = ((k >> t) & 1) ? !p : p;
            double tl, th, tc;
            fix_terms(At[t * m + r], v, p, tl, th, tc);
            lo = lo + tl;
            hi = hi + th;
            cp = cp + tc;
        }
        rs[r] = lo;
        rs[m + r] = hi;
        rs[2 * m + r] = cp;
    }
    if (lane == 0) {
        BinSub o;
        o.x = x;
        o.sec = k;
        o.inc_x = 0;
        o.z = z;
        o.inc = INFINITY;
        o.nodes = 0;
        o.d = split;
        o.running = 1;
        o.found = 0;
        o.pad = 0;
        g.sub[s] = o;
    }
}

// RPL rows per lane: row r = lane + 64 k, k < RPL. A lane without a row holds
// L = -inf, U = +inf and zeros, so it votes neutrally in all three tests and
// never leaves the control flow: every vote is over the whole wave.
template <int RPL, int TIER>
__global__ __launch_bounds__(kBlock) void k_binary_solve(BinaryGeo g) {
    extern __shared__ double lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = g.m, n = g.n, split = g.split;
    const int64_t s0 = (int64_t)blockIdx.x * kWaves;
    bool any = false;                          // workgroup-uniform: nothing to do, nothing to load
    for (int k = 0; k < kWaves; k++)
        if (s0 + k < g.nsub && g.sub[s0 + k].running) any = true;
    if (!any) return;
    const int64_t q0 = s0 >> split;
    const int per = n * m + n;                 // A^T and c of one problem
    if (TIER == LPG_BATCH_TIER_LDS) {
        // the workgroup's problems (four, two, or one shared by its sub-searches), loaded by all four waves
        const int64_t slast = s0 + kWaves - 1 < g.nsub ? s0 + kWaves - 1 : g.nsub - 1;
        const int npb = (int)((slast >> split) - q0) + 1;
        for (int p = 0; p < npb; p++) {
            const double *Ag = g.At + (q0 + p) * (int64_t)(n * m), *cg = g.c + (q0 + p) * n;
            double *dst = lds + (size_t)p * per;
            for (int e = tid; e < n * m; e += kBlock) dst[e] = Ag[e];
            for (int e = tid; e < n; e += kBlock) dst[n * m + e] = cg[e];
        }
        __syncthreads();                       // the only workgroup barrier: the waves part here
    }
    const int64_t s = s0 + w;
    if (s >= g.nsub) return;
    const BinSub st = g.sub[s];
    if (!st.running) return;
    const int64_t q = s >> split;
    const double *At, *cc;
    if (TIER == LPG_BATCH_TIER_LDS) {
        At = lds + (size_t)(q - q0) * per;
        cc = At + n * m;
    } else {
        At = g.At + q * (int64_t)(n * m);
        cc = g.c + q * n;
    }
    const uint64_t pmask = __builtin_amdgcn_ballot_w64((lane < n ? cc[lane < n ? lane : 0] : 0.0) < 0.0);

    int d = st.d, found = st.found;
    uint64_t x = st.x, sec = st.sec, incx = st.inc_x;
    double z = st.z, inc = st.inc;
    int64_t nodes = st.nodes;

    double lo[RPL], hi[RPL], cp[RPL], L[RPL], U[RPL];
    bool has[RPL];
    double *rs = g.rows + s * (int64_t)(3 * m);
#pragma unroll
    for (int k = 0; k < RPL; k++) {
        const int r = lane + 64 * k;
        has[k] = r < m;
        lo[k] = has[k] ? rs[r] : 0.0;
        hi[k] = has[k] ? rs[m + r] : 0.0;
        cp[k] = has[k] ? rs[2 * m + r] : 0.0;
        L[k] = has[k] ? g.L[q * m + r] : -INFINITY;
        U[k] = has[k] ? g.U[q * m + r] : INFINITY;
    }
    // column j's entries of this lane's rows; j < n is the caller's to keep
    auto column = [&](int j, double (&a)[RPL]) {
#pragma unroll
        for (int k = 0; k < RPL; k++) a[k] = has[k] ? At[j * m + lane + 64 * k] : 0.0;
    };
    auto apply = [&](const double (&a)[RPL], int j, int v, bool add) {
        const int pj = (int)((pmask >> j) & 1);
#pragma unroll
        for (int k = 0; k < RPL; k++) {
            double tl, th, tc;
            fix_terms(a[k], v, pj, tl, th, tc);
            lo[k] = add ? lo[k] + tl : lo[k] - tl;
            hi[k] = add ? hi[k] + th : hi[k] - th;
            cp[k] = add ? cp[k] + tc : cp[k] - tc;
        }
        const double tz = (v != pj) ? fabs(cc[j]) : 0.0;
        z = add ? z + tz : z - tz;
    };

    bool running = true;
    for (int left = g.budget; left > 0; left--) {
        nodes++;
        bool prune = z >= inc;
        if (!prune) {
            bool bad = false, ok = true;
#pragma unroll
            for (int k = 0; k < RPL; k++) {
                bad = bad | (lo[k] > U[k]) | (hi[k] < L[k]);
                ok = ok & (L[k] <= cp[k]) & (cp[k] <= U[k]);
            }
            if (__builtin_amdgcn_ballot_w64(bad) != 0) {
                prune = true;
            } else if (__builtin_amdgcn_ballot_w64(!ok) == 0) {
                inc = z;
                incx = (x & low_mask(d)) | (pmask & ~low_mask(d));
                found = 1;
                prune = true;
            }
        }
        double a[RPL];
        if (!prune && d < n) {                 // descend (at d = n one of the two votes above has pruned)
            const int v = (int)((pmask >> d) & 1);
            column(d, a);
            apply(a, d, v, true);
            x = (x & ~(1ull << d)) | ((uint64_t)v << d);
            sec &= ~(1ull << d);
            d++;
            continue;
        }
        while (d > split && ((sec >> (d - 1)) & 1)) {      // backtrack over levels on their second value
            d--;
            column(d, a);
            apply(a, d, (int)((x >> d) & 1), false);
            x &= ~(1ull << d);
            sec &= ~(1ull << d);
        }
        if (d == split) {
            running = false;
            break;
        }
        d--;                                   // the deepest level on its first value: its other value
        const int v = (int)((x >> d) & 1);
        column(d, a);
        apply(a, d, v, false);
        apply(a, d, v ^ 1, true);
        x ^= 1ull << d;
        sec |= 1ull << d;
        d++;
    }

    if (running) {
#pragma unroll
        for (int k = 0; k < RPL; k++) {
            const int r = lane + 64 * k;
            if (has[k]) {
                rs[r] = lo[k];
                rs[m + r] = hi[k];
                rs[2 * m + r] = cp[k];
            }
        }
    }
    if (lane == 0) {
        BinSub o;
        o.x = x;
        o.sec = sec;
        o.inc_x = incx;
        o.z = z;
        o.inc = inc;
        o.nodes = nodes;
        o.d = d;
        o.running = running ? 1 : 0;
        o.found = found;
        o.pad = 0;
        g.sub[s] = o;
        if (running) atomicAdd(g.running, 1);
    }
}

}  // namespace lpg

using namespace lpg;

struct lpg_binary : BatchHost {
    int64_t m = 0, n = 0, nsub = 0;
    int split = 0;
    uint32_t flags = 0;
    int tier = LPG_BATCH_TIER_LDS, rpl = 1, chunk = LPG_BINARY_DEFAULT_CHUNK;
    bool fresh = true;            // the searches stand before their roots' init
    bool any_running = true;
    double *At = nullptr, *L = nullptr, *U = nullptr, *c = nullptr, *rows = nullptr;
    BinSub *sub = nullptr;
    int32_t *running = nullptr;
    std::vector<lpg_binary_result> res;      // of the last solve, reduced over the sub-searches
    std::vector<int8_t> x;
};

namespace {

const void *solve_kernel(int rpl, int tier) {
    if (tier == LPG_BATCH_TIER_LDS)
        return rpl == 1   ? (const void *)k_binary_solve<1, LPG_BATCH_TIER_LDS>
               : rpl == 2 ? (const void *)k_binary_solve<2, LPG_BATCH_TIER_LDS>
                          : (const void *)k_binary_solve<4, LPG_BATCH_TIER_LDS>;
    return rpl == 1   ? (const void *)k_binary_solve<1, LPG_BATCH_TIER_GLOBAL>
           : rpl == 2 ? (const void *)k_binary_solve<2, LPG_BATCH_TIER_GLOBAL>
                      : (const void *)k_binary_solve<4, LPG_BATCH_TIER_GLOBAL>;
}

BinaryGeo geo_of(const lpg_binary *b) {
    BinaryGeo g{};
    g.At = b->At;
    g.L = b->L;
    g.U = b->U;
    g.c = b->c;
    g.sub = b->sub;
    g.rows = b->rows;
    g.running = b->running;
    g.count = b->count;
    g.nsub = b->nsub;
    g.m = (int32_t)b->m;
    g.n = (int32_t)b->n;
    g.split = b->split;
    g.budget = 0;
    g.maximize = (b->flags & LPG_BINARY_MAXIMIZE) ? 1 : 0;
    return g;
}

void reset_searches(lpg_binary *b) {
    b->fresh = true;
    b->any_running = true;
    b->solved = false;
}

// the position of sub-search k in the search order: bit 0 of k is the outermost column
uint32_t order_of(uint32_t k, int split) {
    uint32_t r = 0;
    for (int t = 0; t < split; t++) r |= ((k >> t) & 1u) << (split - 1 - t);
    return r;
}

const char *what_is(double v) { return v != v ? "NaN" : (v == INFINITY || v == -INFINITY) ? "infinite" : "not an integer"; }

}  // namespace

extern "C" {

const char *lpg_binary_last_error(const lpg_binary *b) { return b ? b->err : thread_err<lpg_binary>(); }

int lpg_binary_create(lpg_binary **out, int device, int64_t count, int64_t m, int64_t n, int32_t split, uint32_t flags) {
    const char *call = "lpg_binary_create";
    lpg_binary *b = nullptr;           // not made yet: the refusals below go to the thread's buffer only
    if (!out) return fail(b, LPG_ERR_ARG, "%s: out is NULL", call);
    *out = nullptr;
    if (count < 1 || m < 1 || m > LPG_BINARY_MAX_M || n < 1 || n > LPG_BINARY_MAX_N)
        return fail(b, LPG_ERR_ARG, "%s: bad shape count=%lld m=%lld n=%lld (need count >= 1, 1 <= m <= %d, "
                                    "1 <= n <= %d)", call, (long long)count, (long long)m, (long long)n,
                    LPG_BINARY_MAX_M, LPG_BINARY_MAX_N);
    const int64_t smax = n < LPG_BINARY_MAX_SPLIT ? n : LPG_BINARY_MAX_SPLIT;
    if (split < 0 || split > smax)
        return fail(b, LPG_ERR_ARG, "%s: split %d outside 0..min(n, %d) = %lld", call, split, LPG_BINARY_MAX_SPLIT,
                    (long long)smax);
    if (flags & ~(uint32_t)LPG_BINARY_MAXIMIZE)
        return fail(b, LPG_ERR_ARG, "%s: flags 0x%x not supported (LPG_BINARY_MAXIMIZE only)", call, flags);
    if (device < 0) return fail(b, LPG_ERR_ARG, "%s: device %d", call, device);
    if (count > ((int64_t)0x7fffffff >> split))
        return fail(b, LPG_ERR_ARG, "%s: count * 2^split = %lld x %d exceeds 2^31 - 1", call, (long long)count,
                    1 << split);
    int chunk = LPG_BINARY_DEFAULT_CHUNK;
    if (const char *ce = getenv("LPG_BINARY_CHUNK")) {
        const long long v = atoll(ce);
        if (v < 1 || v > (1 << 24))
            return fail(b, LPG_ERR_ARG, "%s: LPG_BINARY_CHUNK=%s out of range [1, %d]", call, ce, 1 << 24);
        chunk = (int)v;
    }
    b = new lpg_binary();
    b->device = device;
    b->count = count;
    b->m = m;
    b->n = n;
    b->split = split;
    b->nsub = count << split;
    b->flags = flags;
    b->chunk = chunk;
    b->rpl = m <= 64 ? 1 : m <= 128 ? 2 : 4;
    b->have.assign((size_t)count, 0);
    // a workgroup's four sub-searches belong to four, two or one problem
    const int64_t ppw = split >= 2 ? 1 : (kWaves >> split);
    const int64_t need = ppw * 8 * (n * m + n);
    if (need <= kBinaryMaxLds && !env_is("LPG_BINARY_TIER", "global")) {
        b->tier = LPG_BATCH_TIER_LDS;
        b->lds = need;
    } else {
        b->tier = LPG_BATCH_TIER_GLOBAL;
        b->lds = 0;
    }
    b->allocs = {dev_array(b->At, count * n * m), dev_array(b->L, count * m), dev_array(b->U, count * m),
                 dev_array(b->c, count * n), dev_array(b->rows, b->nsub * 3 * m), dev_array(b->sub, b->nsub),
                 dev_array(b->running, 1)};
    snprintf(b->oom_what, sizeof b->oom_what, "batch of %lld problems, %lld sub-searches", (long long)count,
             (long long)b->nsub);
    *out = b;
    return 0;
}

void lpg_binary_destroy(lpg_binary *b) { destroy(b); }

int lpg_binary_info(const lpg_binary *b, lpg_binary_info_t *out) {
    if (!b) return fail<lpg_binary>(nullptr, LPG_ERR_ARG, "lpg_binary_info: the batch is NULL");
    if (!out) return fail(const_cast<lpg_binary *>(b), LPG_ERR_ARG, "lpg_binary_info: out is NULL");
    out->count = b->count;
    out->m = b->m;
    out->n = b->n;
    out->split = b->split;
    out->rows_per_lane = b->rpl;
    out->tier = b->tier;
    out->chunk = b->chunk;
    out->lds_bytes = b->lds;
    out->launches = b->launches;
    out->kernel_ms = b->kernel_ms;
    return 0;
}

int lpg_binary_load(lpg_binary *b, int64_t first, int64_t np, const double *A, int64_t ldA, const int32_t *sense,
                    const double *rhs, const double *c) {
    const char *call = "lpg_binary_load";
    if (!b) return fail(b, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (!A) return fail(b, LPG_ERR_ARG, "%s: A is NULL", call);
    if (!sense) return fail(b, LPG_ERR_ARG, "%s: sense is NULL", call);
    if (!rhs) return fail(b, LPG_ERR_ARG, "%s: rhs is NULL", call);
    if (!c) return fail(b, LPG_ERR_ARG, "%s: c is NULL", call);
    if (int rc = range_ok(b, call, first, np)) return rc;
    if (ldA < b->n) return fail(b, LPG_ERR_ARG, "%s: ldA %lld < n = %lld", call, (long long)ldA, (long long)b->n);
    const int64_t m = b->m, n = b->n;
    const bool mx = (b->flags & LPG_BINARY_MAXIMIZE) != 0;
    const uint64_t cap = (uint64_t)1 << 52;
    std::vector<double> At((size_t)(np * n * m)), L((size_t)(np * m)), U((size_t)(np * m)), cs((size_t)(np * n));
    for (int64_t p = 0; p < np; p++) {
        const long long q = (long long)(first + p);
        for (int64_t i = 0; i < m; i++) {
            uint64_t sum = 0;
            for (int64_t j = 0; j < n; j++) {
                const double a = A[(p * m + i) * ldA + j];
                if (!(fabs(a) < INFINITY) || a != floor(a))
                    return fail(b, LPG_ERR_ARG, "%s: problem %lld, row %lld, entry %lld is %s; entries are finite "
                                                "integers; nothing was loaded", call, q, (long long)i, (long long)j,
                                what_is(a));
                if (fabs(a) > LPG_BINARY_SUM_CAP || (sum += (uint64_t)fabs(a)) > cap)
                    return fail(b, LPG_ERR_ARG, "%s: problem %lld, row %lld, entry %lld: the row's sum of |a| exceeds "
                                                "the cap LPG_BINARY_SUM_CAP = 2^52; nothing was loaded", call, q,
                                (long long)i, (long long)j);
                At[(size_t)((p * n + j) * m + i)] = a + 0.0;
            }
            const int32_t sn = sense[p * m + i];
            if (sn < -1 || sn > 1)
                return fail(b, LPG_ERR_ARG, "%s: problem %lld, row %lld: sense %d outside {-1, 0, 1}; nothing was "
                                            "loaded", call, q, (long long)i, (int)sn);
            const double r = rhs[p * m + i];
            if (!(fabs(r) < INFINITY) || r != floor(r))
                return fail(b, LPG_ERR_ARG, "%s: problem %lld, row %lld: the right-hand side is %s; nothing was loaded",
                            call, q, (long long)i, what_is(r));
            if (fabs(r) > LPG_BINARY_RHS_CAP)
                return fail(b, LPG_ERR_ARG, "%s: problem %lld, row %lld: the right-hand side exceeds the cap "
                                            "LPG_BINARY_RHS_CAP = 2^53 in magnitude; nothing was loaded", call, q,
                            (long long)i);
            L[(size_t)(p * m + i)] = sn < 0 ? -INFINITY : r + 0.0;
            U[(size_t)(p * m + i)] = sn > 0 ? INFINITY : r + 0.0;
        }
        uint64_t sum = 0;
        for (int64_t j = 0; j < n; j++) {
            const double v = c[p * n + j];
            if (!(fabs(v) < INFINITY) || v != floor(v))
                return fail(b, LPG_ERR_ARG, "%s: problem %lld, cost %lld is %s; costs are finite integers; nothing was "
                                            "loaded", call, q, (long long)j, what_is(v));
            if (fabs(v) > LPG_BINARY_SUM_CAP || (sum += (uint64_t)fabs(v)) > cap)
                return fail(b, LPG_ERR_ARG, "%s: problem %lld, cost %lld: the sum of |c| exceeds the cap "
                                            "LPG_BINARY_SUM_CAP = 2^52; nothing was loaded", call, q, (long long)j);
            cs[(size_t)(p * n + j)] = mx ? 0.0 - v : v + 0.0;
        }
    }
    if (int rc = ensure_device(b, call)) return rc;
    LPG_HIPCHK(b, hipMemcpy(b->At + first * n * m, At.data(), At.size() * sizeof(double), hipMemcpyHostToDevice));
    LPG_HIPCHK(b, hipMemcpy(b->L + first * m, L.data(), L.size() * sizeof(double), hipMemcpyHostToDevice));
    LPG_HIPCHK(b, hipMemcpy(b->U + first * m, U.data(), U.size() * sizeof(double), hipMemcpyHostToDevice));
    LPG_HIPCHK(b, hipMemcpy(b->c + first * n, cs.data(), cs.size() * sizeof(double), hipMemcpyHostToDevice));
    mark_loaded(b, first, np);
    reset_searches(b);
    return 0;
}

int lpg_binary_generate(lpg_binary *b, uint64_t seed, int kind) {
    const char *call = "lpg_binary_generate";
    if (!b) return fail(b, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (kind != LPG_BINARY_GEN_BANDED)
        return fail(b, LPG_ERR_ARG, "%s: kind %d unknown (LPG_BINARY_GEN_BANDED = 0 only)", call, kind);
    if (int rc = ensure_device(b, call)) return rc;
    const int64_t total = b->count * (b->m + b->n);
    LPG_HIPCHK(b, hipMemsetAsync(b->At, 0, (size_t)(b->count * b->n * b->m) * sizeof(double), b->stream));
    hipLaunchKernelGGL(k_binary_generate, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, b->stream,
                       geo_of(b), seed);
    LPG_HIPCHK(b, hipGetLastError());
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    mark_all_loaded(b);
    reset_searches(b);
    return 0;
}

int lpg_binary_occupancy(lpg_binary *b, int64_t *resident_waves) {
    const char *call = "lpg_binary_occupancy";
    if (!b) return fail(b, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (!resident_waves) return fail(b, LPG_ERR_ARG, "%s: resident_waves is NULL", call);
    LPG_HIPCHK(b, hipSetDevice(b->device));
    if (int rc = raise_lds_once(b, solve_kernel(b->rpl, b->tier), kBinaryMaxLds, call)) return rc;
    int blocks = 0, cus = 0;
    LPG_HIPCHK(b, hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, solve_kernel(b->rpl, b->tier), kBlock, (size_t)b->lds));
    LPG_HIPCHK(b, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device));
    *resident_waves = (int64_t)blocks * cus * kWaves;
    return 0;
}

int lpg_binary_solve(lpg_binary *b, int64_t max_nodes, lpg_binary_result *out) {
    const char *call = "lpg_binary_solve";
    if (!b) return fail(b, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (!b->loaded)
        return fail(b, LPG_ERR_STATE, "%s: problem %lld has no data yet (lpg_binary_load or lpg_binary_generate first)",
                    call, (long long)first_unloaded(b));
    if (int rc = ensure_device(b, call)) return rc;
    if (int rc = raise_lds_once(b, solve_kernel(b->rpl, b->tier), kBinaryMaxLds, call)) return rc;
    BinaryGeo g = geo_of(b);
    const unsigned grid = (unsigned)((b->nsub + kWaves - 1) / kWaves);
    if (b->fresh) {
        hipLaunchKernelGGL(k_binary_init, dim3(grid), dim3(kBlock), 0, b->stream, g);
        LPG_HIPCHK(b, hipGetLastError());
        b->fresh = false;
        b->any_running = true;
    }
    b->launches = 0;
    b->kernel_ms = 0.0;
    const void *kern = solve_kernel(b->rpl, b->tier);
    int64_t used = 0;
    while (b->any_running && !(max_nodes > 0 && used >= max_nodes)) {
        g.budget = (max_nodes > 0 && max_nodes - used < b->chunk) ? (int32_t)(max_nodes - used) : b->chunk;
        int32_t left = 0;
        LPG_HIPCHK(b, hipMemsetAsync(b->running, 0, sizeof(int32_t), b->stream));
        LPG_HIPCHK(b, timed_launch(b, kern, grid, g));
        LPG_HIPCHK(b, hipMemcpyAsync(&left, b->running, sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
        LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
        float ms = 0.0f;
        LPG_HIPCHK(b, hipEventElapsedTime(&ms, b->ev0, b->ev1));
        b->kernel_ms += ms;
        b->launches++;
        used += g.budget;
        b->any_running = left > 0;
    }
    // the split reduction, over the records copied back (lpg.h, "Split")
    std::vector<BinSub> sub((size_t)b->nsub);
    LPG_HIPCHK(b, hipMemcpyAsync(sub.data(), b->sub, sub.size() * sizeof(BinSub), hipMemcpyDeviceToHost, b->stream));
    LPG_HIPCHK(b, hipStreamSynchronize(b->stream));
    const int64_t S = (int64_t)1 << b->split, n = b->n;
    const bool mx = (b->flags & LPG_BINARY_MAXIMIZE) != 0;
    b->res.assign((size_t)b->count, lpg_binary_result{});
    b->x.assign((size_t)(b->count * n), (int8_t)-1);
    for (int64_t q = 0; q < b->count; q++) {
        const BinSub *best = nullptr;
        uint32_t best_at = 0;
        int64_t nodes = 0;
        bool running = false;
        for (int64_t k = 0; k < S; k++) {
            const BinSub &s = sub[(size_t)(q * S + k)];
            nodes += s.nodes;
            running = running || s.running;
            if (!s.found) continue;
            const uint32_t at = order_of((uint32_t)k, b->split);
            if (!best || s.inc < best->inc || (s.inc == best->inc && at < best_at)) {
                best = &s;
                best_at = at;
            }
        }
        lpg_binary_result &r = b->res[(size_t)q];
        r.status = running ? LPG_ITER_LIMIT : best ? LPG_OPTIMAL : LPG_INFEASIBLE;
        r.found = best ? 1 : 0;
        r.nodes = nodes;
        r.objective = best ? (mx ? 0.0 - best->inc : best->inc) : NAN;
        if (best)
            for (int64_t j = 0; j < n; j++) b->x[(size_t)(q * n + j)] = (int8_t)((best->inc_x >> j) & 1);
    }
    b->solved = true;
    if (out) memcpy(out, b->res.data(), (size_t)b->count * sizeof(lpg_binary_result));
    return 0;
}

int lpg_binary_get(lpg_binary *b, int64_t first, int64_t np, int8_t *x) {
    const char *call = "lpg_binary_get";
    if (!b) return fail(b, LPG_ERR_ARG, "%s: the batch is NULL", call);
    if (!x) return fail(b, LPG_ERR_ARG, "%s: x is NULL", call);
    if (int rc = range_ok(b, call, first, np)) return rc;
    if (!b->solved) return fail(b, LPG_ERR_STATE, "%s: no solve since the last load or generate", call);
    memcpy(x, b->x.data() + first * b->n, (size_t)(np * b->n));
    return 0;
}

}  // extern "C"
