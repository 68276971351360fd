// flushw_probe.hip -- the block pass k_flushw<96,2,1,8> (the product's form at
// config 3) and two timing probes of the SAME body (lpg_flushw.h, MODE; lab
// only, the product never links this file):
//   MODE 0  the product kernel (checked bitwise against the plain fma chain
//           x = fma(-C_q[i], P_q[j], x), q = 0 .. K-1, first)
//   MODE 1  no MFMA: the memory path alone (loads, ring, barrier, stores; the
//           A operands still read from LDS)
//   MODE 2  no tableau traffic: the matrix path alone (multiplier ring, LDS,
//           barrier, MFMAs; stores only under a never-true condition)
// over config 3's shape (16384 rows, 49153 columns, pitch 49216, the 32769
// first columns live, P zero beyond), random data, 96 pending slots, the
// product's XCD item map (flushx_plan). Run the probes under rocprofv3 --pmc
// too (LAB_MODE=m selects one). The 32- / 64-row bands and the first buffer
// form (MODE 3) that this file once carried are recorded in DESIGN.md 3.4.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o tools/flushw_probe tools/flushw_probe.hip
//   tools/flushw_probe [reps]
#include "../linearprogramming_amd/csrc/lpg_kernels.hip"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#define CHK(x)                                                                      \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                     \
            printf("%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                \
        }                                                                           \
    } while (0)

namespace lpg {

// the eager chain of one element, in pending order (what K eager updates compute)
__global__ void k_chain_ref(double *T, int64_t m, int64_t ncols, int64_t ld, const double *P, const double *C,
                            int64_t cs, int K) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ncols) return;
    for (int64_t i = blockIdx.y; i < m; i += gridDim.y) {
        double x = T[i * ld + j];
        for (int q = 0; q < K; q++) x = fma(-C[(int64_t)q * cs + i], P[(int64_t)q * ld + j], x);
        T[i * ld + j] = x;
    }
}

__global__ void k_fillr(double *p, int64_t n, uint64_t seed) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t z = (seed + (uint64_t)i) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        p[i] = (double)(z >> 11) * (1.0 / 9007199254740992.0) - 0.5;
    }
}
__global__ void k_zero_cols_from(double *P, int64_t ld, int64_t c0, int K) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)K * ld; i += (int64_t)gridDim.x * blockDim.x)
        if (i % ld >= c0) P[i] = 0.0;
}
__global__ void k_diff(const double *a, const double *b, int64_t n, unsigned long long *bad) {
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        c += __double_as_longlong(a[i]) != __double_as_longlong(b[i]);
    if (c) atomicAdd(bad, c);
}

}  // namespace lpg

using namespace lpg;

int main(int argc, char **argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 5;
    const int64_t m = 16384, nstruct = 32768, ncols = nstruct + m + 1, ld = (ncols + 63) / 64 * 64, cs = m;
    const int K = 96;
    const int64_t n = m * ld;
    double *T, *T0, *Tr, *Pbuf, *Cbuf;
    DevState *st;
    unsigned long long *bad;
    CHK(hipMalloc(&T, n * 8));
    CHK(hipMalloc(&T0, n * 8));
    CHK(hipMalloc(&Tr, n * 8));
    CHK(hipMalloc(&Pbuf, (size_t)K * ld * 8));
    CHK(hipMalloc(&Cbuf, (size_t)K * cs * 8));
    CHK(hipMalloc(&st, sizeof(DevState)));
    CHK(hipMalloc(&bad, 8));
    hipLaunchKernelGGL(k_fillr, dim3(8192), dim3(256), 0, 0, T0, n, 1ull);
    hipLaunchKernelGGL(k_fillr, dim3(1024), dim3(256), 0, 0, Pbuf, (int64_t)K * ld, 2ull);
    hipLaunchKernelGGL(k_fillr, dim3(1024), dim3(256), 0, 0, Cbuf, (int64_t)K * cs, 3ull);
    hipLaunchKernelGGL(k_zero_cols_from, dim3(1024), dim3(256), 0, 0, Pbuf, ld, nstruct + 1, K);
    CHK(hipDeviceSynchronize());
    Geo g{};
    g.T = T;
    g.ld = ld;
    g.nloc = m;
    g.nobj = 1;
    g.ncols = ncols;
    g.nact = ncols - 1;
    g.m = m;
    const int64_t ntiles = (ncols + 255) / 256;
    const int64_t rows = 2048, nitems = flush_nitems(ntiles, rows, m);
    const FlushX X = flushx_plan(ntiles, m, K, 256, -1);
    const unsigned grid = 256;
    auto reset = [&]() {
        DevState h{};
        h.npend = K;
        CHK(hipMemcpy(st, &h, sizeof h, hipMemcpyHostToDevice));
    };
    auto launch = [&](int which) {
        reset();
#define LPG_FW(M)                                                                                                     \
        hipLaunchKernelGGL((k_flushw<96, 2, 1, 8, M>), dim3(grid), dim3(512), 0, 0, T, g, st, Pbuf, Cbuf, cs, ntiles,   \
                           nitems, rows, 1, X, (const int32_t *)nullptr, (const int64_t *)nullptr,                    \
                           (const int32_t *)nullptr)
        if (which == 0) LPG_FW(0);
        else if (which == 1) LPG_FW(1);
        else LPG_FW(2);
#undef LPG_FW
    };
    // bitwise: the product kernel (MODE 0) against the plain chain
    CHK(hipMemcpy(Tr, T0, n * 8, hipMemcpyDeviceToDevice));
    hipLaunchKernelGGL(k_chain_ref, dim3((unsigned)((ncols + 255) / 256), 1024), dim3(256), 0, 0, Tr, m, ncols, ld, Pbuf,
                       Cbuf, cs, K);
    CHK(hipMemcpy(T, T0, n * 8, hipMemcpyDeviceToDevice));
    launch(0);
    CHK(hipMemset(bad, 0, 8));
    hipLaunchKernelGGL(k_diff, dim3(4096), dim3(256), 0, 0, T, Tr, n, bad);
    unsigned long long hb = 0;
    CHK(hipMemcpy(&hb, bad, 8, hipMemcpyDeviceToHost));
    const double bytes = 16.0 * m * (nstruct + 2), flops = bytes / 16.0 * 2.0 * K;
    printf("# flushw probe: %lld x %lld (ld %lld), K = %d, live columns 0..%lld, XCD map H = %d rb %d rs %d; "
           "lpg::k_flushw<96,2,1,8> (MODE 0) vs the fma chain: %llu doubles differ\n", (long long)m, (long long)ncols,
           (long long)ld, K, (long long)nstruct, X.H, X.rb, X.rs, hb);
    if (hb) return 1;
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0));
    CHK(hipEventCreate(&e1));
    const char *names[] = {"MODE 0 lpg::k_flushw<96,2,1,8> (product)", "MODE 1 (no MFMA: memory path)",
                           "MODE 2 (no T traffic: matrix path)"};
    const int only = getenv("LAB_MODE") ? atoi(getenv("LAB_MODE")) : -1;
    for (int round = 0; round < 2; round++)
        for (int w = 0; w < 3; w++) {
            if (only >= 0 && w != only) continue;
            std::vector<float> t;
            for (int r = 0; r <= reps; r++) {
                CHK(hipMemcpy(T, T0, n * 8, hipMemcpyDeviceToDevice));
                CHK(hipEventRecord(e0));
                launch(w);
                CHK(hipEventRecord(e1));
                CHK(hipEventSynchronize(e1));
                float ms = 0;
                CHK(hipEventElapsedTime(&ms, e0, e1));
                if (r) t.push_back(ms);
            }
            std::sort(t.begin(), t.end());
            printf("%-42s best %.3f ms  median %.3f ms  %6.0f GB/s  %5.1f TFLOP/s\n", names[w], t[0], t[t.size() / 2],
                   bytes / (t[0] * 1e-3) / 1e9, flops / (t[0] * 1e-3) / 1e12);
            fflush(stdout);
        }
    return 0;
}
