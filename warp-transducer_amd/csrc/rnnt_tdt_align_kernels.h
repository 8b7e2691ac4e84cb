// rnnt_tdt_align_kernels.h -- the gfx950 kernels of the TDT best-path alignment (include/rnnt_tdt_align.h).  Three stages:
//   1 tdt_stats_kernel             rnnt_tdt_kernels.h's, unchanged: the cell record [lp_blank, lp_label, logZ_tok, logZ_dur,
//                                  lp_dur_0 ..] of every in-lattice row and the poison flag
//   2 tdt_align_lattice_kernel     one block per sample: the max-plus form of tdt_lattice_kernel's forward half -- a thread
//                                  per cell of the anti-diagonal, one barrier pair per diagonal, values relative to the fp64
//                                  per-diagonal offset (the previous diagonal's maximum), the 128-entry LDS ring of offsets.
//                                  Per cell the best value and one back-pointer byte; the block closes the sample (the best
//                                  final blank into the terminal node, the score in fp64)               [latency-bound, O(T+U)]
//   3 tdt_align_traceback_kernel   a thread per sample walks the back-pointer bytes from the final edge to (0, 0): at most
//                                  T_b + L_b dependent one-byte loads; writes frames, durs and the score       [O(T+U) serial]
//
// Back-pointer of cell (t, u): 2 * duration_index + is_label of its best in-edge, kTdtAlignNone for the start node and for
// cells no path reaches.  Ties: in-edges in the order duration index 0 .. D-1, blank before label; a candidate replaces the
// best so far only if strictly greater (a NaN or -inf candidate never does).
#pragma once

#include "rnnt_tdt_kernels.h"

namespace rnnt {

constexpr unsigned char kTdtAlignNone = 0xFF;

// The duration value of index j without indexing the by-value argument dynamically (that would put it into scratch)
__device__ __forceinline__ int tdt_align_duration(const TdtDurations& dur, int j) {
    int d = 0;
#pragma unroll
    for (int k = 0; k < kTdtMaxDurations; ++k) d = (k == j) ? dur.d[k] : d;
    return d;
}

// ------------------------------------------------------------------------------------------
// Stage 2.  grid = N slice, block = any multiple of 64 up to 1024.  val: the cell values (the loss's alpha array), bp: the
// back-pointer bytes (N * maxT * maxU of them, in the loss's beta array), best[b]: the base-2 absolute weight of the best
// path (-inf: none; NaN: lengths that do not fit the tensor), fin[b]: the duration index of the final blank (-1: none).
// The 2 D predecessor loads of a cell -- value, edge weight and duration weight each -- are issued together: invalid edges
// read the sample's cell (0, 0) (always inside the lattice) and are masked afterwards, so no load waits behind a branch.
// The fp32 lattice issues all 8 duration slots at once; the fp64 lattice in two batches of 4 (48 values of 8 bytes in flight
// do not fit the 128 registers of a 1024-thread block), the second skipped when D <= 4.
template <typename L>
__global__ __launch_bounds__(1024) void tdt_align_lattice_kernel(
        const L* __restrict__ tab, L* __restrict__ val, unsigned char* __restrict__ bp, double* __restrict__ best,
        int* __restrict__ fin, const int* __restrict__ xlen, const int* __restrict__ ylen, TdtDurations dur,
        int maxT, int maxU, int b0) {
    constexpr int JB = sizeof(L) == 8 ? 4 : kTdtMaxDurations;        // duration slots whose loads are in flight together
    __shared__ double ring[kTdtRing];
    __shared__ L wmax[2][16];
    const int b = b0 + blockIdx.x;
    const int D = dur.n, RS = tdt_rec_stride(D);
    int T, Lb;
    if (!tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb)) {
        if (threadIdx.x == 0) { best[b] = __builtin_nan(""); fin[b] = -1; }
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const size_t c00 = tdt_cell(b, 0, 0, maxT, maxU);
    const int last = T - 1 + Lb;                                     // last diagonal of the grid; the terminal node: last + 1
    double base = 0.0;                                               // off[n] of the diagonal being computed
    for (int n = 0; n <= last; ++n) {
        if (tid == 0) ring[n & (kTdtRing - 1)] = base;
        __syncthreads();                                             // ring[n] and (n > 0) the previous diagonals' values
        const int ulo = n - (T - 1) > 0 ? n - (T - 1) : 0, uhi = n < Lb ? n : Lb;
        L tmax = neg_inf<L>();
        for (int u = ulo + tid; u <= uhi; u += blockDim.x) {
            const int t = n - u;
            L v = n == 0 ? L(0) : neg_inf<L>();
            int arg = kTdtAlignNone;
#pragma unroll
            for (int j0 = 0; j0 < kTdtMaxDurations; j0 += JB) {
                if (j0 >= D) break;                                                  // (uniform: the fp64 form's second batch)
                L vb[JB], wb[JB], db[JB], ob[JB];                                    // blank (t - d, u) -> (t, u)
                L vl[JB], wl[JB], dl[JB], ol[JB];                                    // label (t - d, u - 1) -> (t, u)
                bool okb[JB], okl[JB];
#pragma unroll
                for (int i = 0; i < JB; ++i) {                                       // every load of the batch first ...
                    const int j = j0 + i, d = dur.d[j], ts = t - d;
                    okb[i] = j < D && ts >= 0 && d > 0;
                    okl[i] = j < D && ts >= 0 && u >= 1;
                    const size_t cb = okb[i] ? tdt_cell(b, ts, u, maxT, maxU) : c00;
                    const size_t cl = okl[i] ? tdt_cell(b, ts, u - 1, maxT, maxU) : c00;
                    const int jj = j < D ? j : 0;
                    vb[i] = val[cb]; wb[i] = tab[cb * RS]; db[i] = tab[cb * RS + 4 + jj];
                    vl[i] = val[cl]; wl[i] = tab[cl * RS + 1]; dl[i] = tab[cl * RS + 4 + jj];
                    ob[i] = static_cast<L>(ring[(n - d) & (kTdtRing - 1)] - base);
                    ol[i] = static_cast<L>(ring[(n - d - 1) & (kTdtRing - 1)] - base);
                }
#pragma unroll
                for (int i = 0; i < JB; ++i) {                                       // ... then the compares, in tie order
                    const L candb = okb[i] ? vb[i] + ob[i] + wb[i] + db[i] : neg_inf<L>();
                    if (candb > v) { v = candb; arg = 2 * (j0 + i); }
                    const L candl = okl[i] ? vl[i] + ol[i] + wl[i] + dl[i] : neg_inf<L>();
                    if (candl > v) { v = candl; arg = 2 * (j0 + i) + 1; }
                }
            }
            const size_t c = tdt_cell(b, t, u, maxT, maxU);
            val[c] = v;
            bp[c] = static_cast<unsigned char>(arg);
            tmax = vmax(tmax, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tmax = vmax(tmax, __shfl_xor(tmax, o, kWave));
        if (lane == 0) wmax[n & 1][wave] = tmax;
        __syncthreads();
        L M = wmax[n & 1][0];
        for (int w = 1; w < nw; ++w) M = vmax(M, wmax[n & 1][w]);
        if (M - M == L(0)) base += static_cast<double>(M);           // (a diagonal without a finite value keeps the offset)
    }
    if (tid != 0) return;
    // the final blanks (T_b - d, L_b) -> terminal, read behind the last barrier, in tie order
    double m = -__builtin_huge_val();
    int arg = -1;
    for (int j = 0; j < D; ++j) {
        const int d = tdt_align_duration(dur, j), ts = T - d;
        if (d <= 0 || ts < 0) continue;
        const size_t c = tdt_cell(b, ts, Lb, maxT, maxU);
        const double v = static_cast<double>(val[c]) + ring[(ts + Lb) & (kTdtRing - 1)] +
                         static_cast<double>(tab[c * RS]) + static_cast<double>(tab[c * RS + 4 + j]);
        if (v > m) { m = v; arg = j; }
    }
    best[b] = m;
    fin[b] = arg;
}

// ------------------------------------------------------------------------------------------
// Stage 3.  A thread per sample: grid = ceil(N / 64), block = 64.  score[b] = best[b] in natural log; NaN for a poisoned
// sample and for lengths that do not fit, -inf without a path -- those samples get -1 in every entry of frames and durs.
// `L` only names the code object's lattice type (the kernel reads no lattice value).
template <typename L>
__global__ __launch_bounds__(64) void tdt_align_traceback_kernel(
        const unsigned char* __restrict__ bp, const double* __restrict__ best, const int* __restrict__ fin,
        const int* __restrict__ poison, const int* __restrict__ xlen, const int* __restrict__ ylen,
        double* __restrict__ score, int* __restrict__ frames, int* __restrict__ durs, TdtDurations dur, int maxT, int maxU,
        int N) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= N) return;
    int T, Lb;
    const bool fits = tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb);
    const double lp = best[b];
    const int jf = fin[b];
    const bool nan = !fits || poison[b] != 0 || lp != lp;
    const bool walk = !nan && lp - lp == 0.0 && jf >= 0;             // a finite best path
    score[b] = nan ? __builtin_nan("") : lp * kLn2;                  // (-inf stays -inf)
    const int L1 = maxU - 1;
    int* fr = frames + static_cast<size_t>(b) * L1;
    int* du = durs + static_cast<size_t>(b) * L1;
    for (int i = walk ? Lb : 0; i < L1; ++i) { fr[i] = -1; du[i] = -1; }
    if (!walk) return;
    int u = Lb, t = T - tdt_align_duration(dur, jf);                 // the source node of the final blank
    for (int step = T + Lb; step > 0 && (t > 0 || u > 0); --step) {
        const int e = bp[tdt_cell(b, t, u, maxT, maxU)];
        const int d = tdt_align_duration(dur, e >> 1);
        if (e == kTdtAlignNone || t - d < 0 || ((e & 1) && u == 0)) break;      // (no finite path reaches such a cell)
        t -= d;
        if (e & 1) { --u; fr[u] = t; du[u] = d; }
    }
    for (int i = 0; i < u; ++i) { fr[i] = -1; du[i] = -1; }          // (only behind a break: never with a finite score)
}

}  // namespace rnnt
