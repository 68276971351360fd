// lpg_flushw.h -- k_flushw, the banded block pass, in one body for the product
// (lpg_kernels.hip, MODE 0 only) and the timing probe (tools/flushw_probe.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lpg_internal.h"
#include "lpg_device.h"

namespace lpg {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));

// a wave-uniform 64-bit value the compiler can keep in scalar registers
// (anything that went through LDS or threadIdx is divergent to it)
__device__ inline int64_t flushw_uniform(int64_t v) {
    return ((int64_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// k_flushw: k_flushm's wave tile (16 rows x 32 columns, 16-byte accesses,
// even/odd-column MFMA chains, B fragments in VGPRs) on TALL items, which is
// what keeps 64-pivot blocks memory-bound. A block's 4 waves sweep `rows`
// rows (runtime, multiple of 16) of a 128-column tile in 16-row bands, in
// step: the multipliers of band s (-C_q[i] in A-fragment order [q][row],
// 8 KB at KMAX = 64) sit in an NB-deep LDS ring, loaded into registers one
// band ahead and written one barrier later, and tableau band s+1 is loaded
// while band s is on the matrix cores. k_flushm instead stages the C of a
// whole 64-128-row strip per item (the LDS tile caps the strip at 64 rows
// for 64 slots) and restarts its pipeline per item: 2.36 ms vs 1.64 ms for
// this kernel at config 3, K = 64 (tools/flush_lab.hip,
// profiles/r01_flush_lab_k64.log). Same chain, same MFMA, bitwise identical.
// WPB waves per block: a tile is 32 * WPB columns wide, and every column
// tile reads all of C once (WPB = 8 halves that on-chip traffic: C is
// 8.4 MB at config 3, read by every tile from the Infinity Cache).
//
// Addressing. The item (tile, rows [i0, i1)) is held in scalar registers.
// Band s of the tile is a raw buffer: base T + (i0 + 16 s) ld + the tile's
// first column, advanced with scalar arithmetic, and as many bytes as the band
// has rows inside the item (16 ld 8 for a full band, fewer for the ragged last
// one, none past the item's end, where the last bands' look-aheads run and
// touch nothing). A lane adds
// one 32-bit byte offset, ((lk + 4 r) ld + its column pair in the tile) * 8,
// fixed for the item; the hardware's range check against
// the band's size is the row predicate, and a lane that is not `ok` sits at
// kNoLane, beyond every band: its loads return zero and its stores are
// dropped without touching memory. The multipliers are one buffer over the np
// live slots of Cbuf (piece offset (q cs + row pair) * 8 per thread, fixed for
// the launch; the band's first row in the scalar offset). No integer multiply
// and no 64-bit compare is left between two barriers; flushw_fits
// (lpg_internal.h) is the bound on ld and cs that this needs.
//
// MODE (tools/flushw_probe.hip; the product instantiates 0 only):
//   0  the pass
//   1  no MFMA: the memory path alone (loads, ring, barrier, stores; the A
//      operands still read from LDS)
//   2  no tableau traffic: the matrix path alone (multiplier ring, LDS,
//      barrier, MFMAs; stores only under a never-true condition)
template <int KMAX, int NB, int LB, int WPB = 4, int MODE = 0>
__global__ __launch_bounds__(64 * WPB, LB) void k_flushw(double *__restrict__ T, Geo g, DevState *__restrict__ st,
                                                         const double *__restrict__ Pbuf,
                                                         const double *__restrict__ Cbuf, int64_t cs, int64_t ntiles,
                                                         int64_t nitems, int64_t rows, int skip, FlushX X,
                                                         const int32_t *__restrict__ tlive,
                                                         const int64_t *__restrict__ lv,
                                                         const int32_t *__restrict__ inv) {
    constexpr int NTH = 64 * WPB;
    constexpr int G = KMAX / 4;
    constexpr int BAND = KMAX * 16;                 // doubles per band
    constexpr int NPC = BAND / 2;                   // 16-byte multiplier pieces per band
    constexpr int PER = (NPC + NTH - 1) / NTH;      // ... per thread (the last round partial when NTH does not divide)
    static_assert(PER >= 1 && NB >= 1, "band staging");
    __shared__ __attribute__((aligned(16))) double sC[NB][BAND];
    __shared__ int64_t next_item;
    __shared__ int next_grp;
    __shared__ int wsum[WPB];
    const int np = (int)st->npend;
    if (np <= 0) return;
    const int64_t ld = g.ld;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    unsigned long long touched = 0;
    const int g0 = (int)(blockIdx.x & 7);   // blocks with the same b % 8 share an XCD
    int gd = 0;                             // X.on: queue g0 + gd (mod 8) is being drained
    // A lane at kNoLane is out of every buffer's range (flushw_fits keeps the
    // buffers below 2 GB)
    constexpr unsigned kNoLane = 0x80000000u;
    constexpr int kRsrc = 0x00020000;       // raw buffer, 32-bit offsets
    const int bandrow = (int)(ld * 8);      // bytes of a tableau row
    const unsigned rstep = 4u * (unsigned)bandrow;   // ... to the lane's next row
    // multiplier piece e = threadIdx.x + u NTH: slot q = e / 8, band rows 2 (e % 8) .. +1;
    // slots >= np are out of crs' range
    const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc((void *)Cbuf, 0, (int)((int64_t)np * cs * 8), kRsrc);
    unsigned coff[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int e = threadIdx.x + u * NTH;
        const int q = e >> 3, rr = 2 * (e & 7);
        coff[u] = (NPC % NTH == 0 || e < NPC) ? (unsigned)(((int64_t)q * cs + rr) * 8) : kNoLane;
    }
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) {
            if (X.on) {
                int64_t it = -1;
                int grp = 0;
                for (; gd < 8; gd++) {
                    grp = (g0 + gd) & 7;
                    const int64_t cnt = flushx_group(X, grp).count;
                    if (cnt == 0) continue;
                    it = (int64_t)atomicAdd(&st->gwork[grp], 1ull);
                    if (it < cnt) break;
                    it = -1;
                }
                next_item = it;
                next_grp = grp;
            } else {
                next_item = (int64_t)atomicAdd(&st->fwork, 1ull);
            }
        }
        __syncthreads();
        const int64_t item = next_item;
        int64_t tile_, i0_, i1_;
        if (X.on) {
            if (item < 0) break;
            const int grp = next_grp;
            flushx_item(X, flushx_group(X, grp), grp, item, tile_, i0_, i1_);
        } else {
            if (item >= nitems) break;
            flush_item(item, ntiles, rows, g.nloc, tile_, i0_, i1_);
        }
        // the item in scalar registers (the same for the whole block)
        const int64_t tile = flushw_uniform(tile_), i0 = flushw_uniform(i0_), i1 = flushw_uniform(i1_);
        // region mode (launch_flush_main): a tile without block-start nonbasic
        // columns holds live entries only in a leaving column of the block, if
        // any (one whose trade did not move it); otherwise it is skipped
        // without reading its pending P entries
        if (tlive) {
            constexpr int NCH = 32 * WPB / 64;
            const int64_t ch = tile * NCH + threadIdx.x;
            const bool maybe = threadIdx.x < NCH && ch < ld / 64 && tlive[ch] != 0;
            if (!__syncthreads_or(maybe)) {
                bool hit = false;
                if ((int)threadIdx.x < np) {
                    const int64_t L = lv[threadIdx.x];
                    if (L > 0) {
                        const int64_t p = inv[L];
                        hit = p >= tile * (32 * WPB) && p < (tile + 1) * (32 * WPB);
                    }
                }
                if (!__syncthreads_or(hit)) continue;
            }
        }
        const int64_t cl = tile * (32 * WPB) + wave * 32 + 2 * lc;   // this lane's column pair
        const bool in = cl < g.ncols;                                // cl even, ld even: cl + 1 < ld
        double be[G], bo[G];
        bool live = false;
#pragma unroll
        for (int gq = 0; gq < G; gq++) {
            const int q = 4 * gq + lk;
            d2 v = d2{0.0, 0.0};
            if (in && q < np) v = *(const d2 *)(Pbuf + (int64_t)q * ld + cl);
            be[gq] = v.x;
            bo[gq] = v.y;
            live = live || v.x != 0.0 || v.y != 0.0;
        }
        // a column pair is live if any of its P entries over all slots is
        // non-zero: OR over the 4 lanes holding its k-slices
        live = (__shfl_xor((int)live, 16, 64) | (int)live) != 0;
        live = (__shfl_xor((int)live, 32, 64) | (int)live) != 0;
        const bool ok = in && (!skip || live);
        int mine = (lk == 0 && ok) ? (cl + 1 < g.ncols ? 2 : 1) : 0;   // live doubles per row, pairs counted once
        for (int mask = 32; mask > 0; mask >>= 1) mine += __shfl_xor(mine, mask, 64);
        const bool wlive = mine > 0;                                   // wave-uniform
        if (lane == 0) wsum[wave] = mine;
        if (__syncthreads_count(wlive && lane == 0) == 0) continue;    // the whole tile is skipped
        // (read again as a scalar: a value merged after a divergent branch sits in a VGPR)
        const int nrows = __builtin_amdgcn_readfirstlane((int)(i1 - i0)), nb = (nrows + 15) / 16;
        if (threadIdx.x == 0) {
            int sum = 0;
#pragma unroll
            for (int w = 0; w < WPB; w++) sum += wsum[w];
            touched += (unsigned long long)sum * (unsigned long long)nrows;
        }
        // band s of this tile as a buffer: its rows inside the item (none past its end)
        char *const tb = (char *)(T + i0 * ld + tile * (32 * WPB));
        auto brows = [&](int s) {
            const int nr = nrows - 16 * s;   // (not a clamp: the compiler would take that to the vector ALU)
            return s >= nb ? 0 : nr > 16 ? 16 : nr;
        };
        auto trs = [&](int s) {
            return __builtin_amdgcn_make_buffer_rsrc((void *)(tb + (int64_t)s * 16 * ld * 8), 0, brows(s) * bandrow, kRsrc);
        };
        // this lane's row lk of the band and column pair of the tile
        const unsigned tv = ok ? (unsigned)(((int64_t)lk * ld + wave * 32 + 2 * lc) * 8) : kNoLane;
        // the multipliers of band s (zeros past np and past i1: A = -0 there, x + -0 == x)
        auto cload = [&](d2 (&cr)[PER], int s) {
            const int so = (int)((i0 + 16 * (int64_t)s) * 8);
            const bool rin = 2 * (int)(threadIdx.x & 7) < brows(s);   // the piece's first row is in the item; row + 1 < cs
#pragma unroll
            for (int u = 0; u < PER; u++)
                cr[u] = -__builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(crs, (int)(rin ? coff[u] : kNoLane), so, 0));
        };
        auto cstore = [&](const d2 (&cr)[PER], int s) {
#pragma unroll
            for (int u = 0; u < PER; u++)
                if (NPC % NTH == 0 || threadIdx.x + u * NTH < NPC) *(d2 *)(&sC[s % NB][2 * (threadIdx.x + u * NTH)]) = cr[u];
        };
        for (int s = 0; s < NB - 1; s++) {   // prologue: bands 0 .. NB-2 into the ring
            d2 cr[PER];
            cload(cr, s);
            cstore(cr, s);
        }
        d2 cn[PER];
        cload(cn, NB - 1);
        auto tload = [&](d2 (&x)[4], int s) {
            const __amdgpu_buffer_rsrc_t rs = trs(s);
#pragma unroll
            for (int r = 0; r < 4; r++)       // aux 2: nontemporal
                x[r] = __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(MODE != 2 ? tv + r * rstep : kNoLane), 0, 2));
        };
        d2 t[4];
        tload(t, 0);
        for (int s = 0; s < nb; s++) {
            d2 tn[4];                         // one band ahead (two ahead measured no faster)
            // The look-aheads are unconditional: past the item's end they meet an
            // empty buffer and touch nothing. Behind a branch on s they cost the
            // pass a quarter (2.57 vs 1.93 ms at config 3, profiles/flushw_lean.md).
            tload(tn, s + 1);
            __syncthreads();                  // band s is staged; ring slot (s - 1) % NB is free
            cstore(cn, s + NB - 1);
            cload(cn, s + NB);
            if (wlive) {
                d4 ae = d4{t[0].x, t[1].x, t[2].x, t[3].x};
                d4 ao = d4{t[0].y, t[1].y, t[2].y, t[3].y};
                const double *sa = &sC[s % NB][lk * 16 + lc];
                // the next pair of A operands is read while this pair's four
                // MFMAs run: left to the scheduler, every ds_read sat behind
                // the MFMAs of the pair before and the chain waited an LDS
                // round trip per four MFMAs (config 3, K = 96: 29.7-29.8k vs
                // 28.6-28.8k pivots/s, profiles/r05_ab_flushw_aprefetch.log)
                double a0 = sa[0], a1 = sa[64];
#pragma unroll
                for (int gq = 0; gq < G; gq += 2) {
                    double n0 = 0.0, n1 = 0.0;
                    if (gq + 2 < G) {
                        n0 = sa[(gq + 2) * 64];
                        n1 = sa[(gq + 3) * 64];
                    }
                    __builtin_amdgcn_sched_barrier(0);   // the reads stay in front of the MFMAs
                    if (MODE != 1) {
                        ae = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, be[gq], ae, 0, 0, 0);
                        ao = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bo[gq], ao, 0, 0, 0);
                        ae = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, be[gq + 1], ae, 0, 0, 0);
                        ao = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bo[gq + 1], ao, 0, 0, 0);
                    } else {
                        ae[0] += a0 * 0.0;               // keep the A reads (and their LDS traffic) live
                        ao[0] += a1 * 0.0;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    a0 = n0;
                    a1 = n1;
                }
                const __amdgpu_buffer_rsrc_t rs = trs(s);
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (MODE != 2 || ae[r] == 12345.0)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, d2{ae[r], ao[r]}), rs, (int)(tv + r * rstep), 0, 2);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) t[r] = tn[r];
        }
    }
    if (threadIdx.x == 0 && touched) atomicAdd(&st->touched, touched);
}

}  // namespace lpg
