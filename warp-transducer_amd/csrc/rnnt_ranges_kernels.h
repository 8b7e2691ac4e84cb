// rnnt_ranges_kernels.h -- the gfx950 kernels of the prune ranges from edge occupations (include/rnnt_ranges.h).
//
// px_grad / py_grad are contiguous along t and a window runs along u: a wavefront per column would gather at a stride of
// T + 1 elements.  So a block takes a TILE of TF consecutive frames of one sample, loads the rows u = 0 .. S_b of the tile
// along t (lane-consecutive frames: runs of TF elements per row), forms g = double(py) + double(px) -- the one IEEE addition
// of the definition -- and keeps it in LDS TRANSPOSED, column f of the tile at g[f * Us + u], Us = (S + 1) | 1 (odd: the
// writes of the lanes of a row spread over the banks, the reads of consecutive u are conflict-free).
//
//   1 ranges_window_kernel    after the stage a WAVEFRONT per column: lane l sums the windows of the starts s = l, l + 64, ...
//                             each from 0.0 in ascending u, keeps its largest sum (the first among equals: the smallest s),
//                             and a butterfly over the 64 lanes keeps the larger sum, then the smaller s -- the scheme of
//                             pruned_window_kernel with a "has a sum" flag in place of its -1 (occupations of a lattice
//                             someone else built need not be positive; a NaN sum never sets the flag).  The raw start goes
//                             to ranges[b, t]; frames t >= T_b are left to the repair.
//   2 ranges_repair_kernel    a BLOCK per sample.  Both passes are integer maxima -- after the forward pass s_t is the running
//                             maximum of the clamped starts, after the backward pass max over j >= t of s_j - (j - t) step --
//                             so a thread takes a contiguous run of frames, the runs' maxima meet in a scan through the lanes
//                             (rg_scan_max), and the result is the serial passes' exactly (a thread per sample,
//                             pruned_ranges_kernel's form, spends T dependent round trips to memory per pass: 1500 of them at
//                             the c4-like shape).
//   3 ranges_coverage_kernel  the same stage, then a THREAD per column: w of the given start and c over the whole column, both
//                             from 0.0 in ascending u, one division.  Lane f reads g[f * Us + u]: with Us odd the 32 columns
//                             of a tile sit on 32 different banks.
//
// THE TILE (rg_tile).  The whole column, S + 1 rows, is staged -- a single-tile form for every S the library takes, so every
// w(s) is added in the defined order with no halo.  TF is the largest power of two <= kRgMaxTile whose tile fits
// kRgLdsDoubles (48 KiB, three blocks a CU):
//     S + 1 <=  191   TF = 32        <=  383   TF = 16        <=  767   TF = 8
//           <= 1535   TF = 4         <= 3071   TF = 2         <= 4096   TF = 1
// A block has 256 threads (four columns at a time) down to TF = 4, 128 at TF = 2 and 64 at TF = 1.  Walking u in chunks with
// an R - 1 halo at a wide tile -- coalesced loads for S + 1 > 383 too -- was designed and is not built.
#pragma once

#include "rnnt_kernels.h"              // through rnnt_device.h the tags and load1

namespace rnnt {

constexpr int kRgLdsDoubles = 6144;     // staged occupancies of a block at most: 48 KiB
constexpr int kRgMaxTile = 32;          // frames of a tile at most
constexpr int kRgRepairBlock = 256;     // threads of a repair block

__host__ __device__ inline int rg_stride(int U) { return U | 1; }
__host__ __device__ inline int rg_tile(int U) {
    int tf = kRgMaxTile;
    while (tf > 1 && tf * rg_stride(U) > kRgLdsDoubles) tf >>= 1;
    return tf;
}

// S_b and T_b of sample b: columns 2 and 3 of the boundary clamped into [0, S] and [0, T]; no boundary: S and T.
struct RgLen { int Sb, Tb; };
__device__ __forceinline__ RgLen rg_len(const long long* __restrict__ boundary, int b, int S, int T) {
    long long s = S, t = T;
    if (boundary != nullptr) {
        s = boundary[static_cast<size_t>(b) * 4 + 2];
        t = boundary[static_cast<size_t>(b) * 4 + 3];
    }
    s = s < 0 ? 0 : (s > S ? S : s);
    t = t < 0 ? 0 : (t > T ? T : t);
    return {static_cast<int>(s), static_cast<int>(t)};
}

// The tile's columns f < nf (frames t0 + f < T_b), rows u <= Sb, into g[f * Us + u].  TF = 1 << lg.  Consecutive threads take
// consecutive frames of a row.  Nothing outside the sample's rows and frames is read.  (A branch-free form with the loads of
// eight cells in flight together was measured and not kept: EXPERIMENTS.md section 27.)
template <typename Tag, bool MOD>
__device__ __forceinline__ void rg_stage(double* __restrict__ g, const typename Tag::store* __restrict__ px,
                                         const typename Tag::store* __restrict__ py, int b, int S, int T, int Sb, int t0,
                                         int nf, int lg, int Us) {
    using St = typename Tag::store;
    const int TX = MOD ? T : T + 1;
    const St* by = py + static_cast<size_t>(b) * (S + 1) * T + t0;
    const size_t ox = static_cast<size_t>(b) * S * TX + t0;            // (S == 0: px is not looked at)
    const int cells = (Sb + 1) << lg, mask = (1 << lg) - 1, nthreads = static_cast<int>(blockDim.x);
#pragma unroll 8
    for (int i = threadIdx.x; i < cells; i += nthreads) {
        const int u = i >> lg, f = i & mask;
        if (f < nf) {
            const double y = static_cast<double>(load1<Tag>(by + static_cast<size_t>(u) * T + f));
            const double x = u < Sb ? static_cast<double>(load1<Tag>(px + ox + static_cast<size_t>(u) * TX + f)) : 0.0;
            g[f * Us + u] = y + x;
        }
    }
}

// grid = (ceil(T / TF), samples of the slice), block = 64 * min(4, TF), TF * Us doubles of LDS; b0: the slice's first sample.
template <typename Tag, bool MOD>
__global__ __launch_bounds__(256) void ranges_window_kernel(
        const typename Tag::store* __restrict__ px, const typename Tag::store* __restrict__ py,
        const long long* __restrict__ boundary, int* __restrict__ ranges, int S, int T, int R, int lg, int b0) {
    extern __shared__ double rg_lds[];
    const int b = b0 + blockIdx.y, t0 = static_cast<int>(blockIdx.x) << lg;
    const RgLen len = rg_len(boundary, b, S, T);
    const int Sb = len.Sb, Tb = len.Tb;
    if (t0 >= Tb) return;                                              // (block-uniform; the repair writes these frames)
    const int nf = Tb - t0 < (1 << lg) ? Tb - t0 : (1 << lg), Us = rg_stride(S + 1);
    rg_stage<Tag, MOD>(rg_lds, px, py, b, S, T, Sb, t0, nf, lg, Us);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = static_cast<int>(blockDim.x) >> 6;
    const int smax = Sb + 1 - R > 0 ? Sb + 1 - R : 0;
    for (int f = wave; f < nf; f += nwaves) {
        const double* g = rg_lds + f * Us;
        double best = 0.0;
        int bs = 0, have = 0;
        for (int s = lane; s <= smax; s += 64) {
            const int e = s + R < Sb + 1 ? s + R : Sb + 1;
            double sum = 0.0;
#pragma unroll 4
            for (int u = s; u < e; ++u) sum += g[u];                   // (the LDS reads go ahead, the additions keep their order)
            if (sum == sum && (!have || sum > best)) { best = sum; bs = s; have = 1; }      // (a NaN sum never wins)
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ob = __shfl_xor(best, off, 64);
            const int os = __shfl_xor(bs, off, 64), oh = __shfl_xor(have, off, 64);
            if (oh && (!have || ob > best || (ob == best && os < bs))) { best = ob; bs = os; have = 1; }
        }
        if (lane == 0) ranges[static_cast<size_t>(b) * T + t0 + f] = have ? bs : 0;
    }
}

// The maximum of v over the threads BEFORE this one (UP) or AFTER it (!UP) in the block, `none` where there is none: a scan
// through the lanes, the wavefronts' totals through `part` (one word per wavefront).  Every thread of the block calls it.
template <bool UP>
__device__ __forceinline__ long long rg_scan_max(long long v, long long none, long long* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long o = UP ? __shfl_up(inc, off, 64) : __shfl_down(inc, off, 64);
        if (UP ? lane >= off : lane + off < 64) inc = o > inc ? o : inc;
    }
    if (lane == (UP ? 63 : 0)) part[wave] = inc;
    long long ex = UP ? __shfl_up(inc, 1, 64) : __shfl_down(inc, 1, 64);
    if (lane == (UP ? 0 : 63)) ex = none;
    __syncthreads();
    for (int w = 0; w < kRgRepairBlock / 64; ++w)
        if ((UP ? w < wave : w > wave) && part[w] > ex) ex = part[w];
    __syncthreads();                                                   // (part is free again)
    return ex;
}

// grid = samples of the slice, block = kRgRepairBlock.  Thread i owns the frames [i chunk, (i + 1) chunk) of its sample.
template <int UNUSED = 0>                 // (a template: only the translation units that launch it hold it)
__global__ __launch_bounds__(kRgRepairBlock) void ranges_repair_kernel(const long long* __restrict__ boundary,
                                                                       int* __restrict__ ranges, int S, int T, int R, int step,
                                                                       int b0) {
    __shared__ long long part[kRgRepairBlock / 64];
    const int b = b0 + blockIdx.x, tid = threadIdx.x;
    const RgLen len = rg_len(boundary, b, S, T);
    const int Sb = len.Sb, Tb = len.Tb;
    int* s = ranges + static_cast<size_t>(b) * T;
    const int smax = Sb + 1 - R > 0 ? Sb + 1 - R : 0;
    const long long st = step, NONE = -(1ll << 62);
    if (Tb > 0 && smax > (Tb - 1) * st) {                              // no chain of windows reaches smax
        for (int t = tid; t < Tb; t += kRgRepairBlock) {
            const long long v = t * st;
            s[t] = v < smax ? static_cast<int>(v) : smax;
        }
    } else if (Tb > 0) {                                               // (block-uniform: every thread meets the barriers)
        const int chunk = (Tb + kRgRepairBlock - 1) / kRgRepairBlock;
        const long long lo_l = static_cast<long long>(tid) * chunk;
        const int lo = lo_l < Tb ? static_cast<int>(lo_l) : Tb, hi = Tb - lo < chunk ? Tb : lo + chunk;
        // the clamp and the running maximum inside the run
        long long m = NONE;
        for (int t = lo; t < hi; ++t) {
            const long long cl_l = smax - (Tb - 1 - t) * st, ch_l = t * st;
            const int cl = cl_l > 0 ? static_cast<int>(cl_l) : 0, ch = ch_l < smax ? static_cast<int>(ch_l) : smax;
            int v = s[t];
            v = v < cl ? cl : (v > ch ? ch : v);
            m = v > m ? v : m;
            s[t] = static_cast<int>(m);
        }
        const long long pre = rg_scan_max<true>(m, NONE, part);       // the running maximum of the runs before this one
        // s_t = max over j >= t of a_j - (j - t) step, a the forward pass's result
        long long q = NONE;
        for (int t = lo; t < hi; ++t) {
            const long long a = s[t] > pre ? s[t] : pre;
            q = a - t * st > q ? a - t * st : q;
        }
        q = rg_scan_max<false>(q, NONE, part);                        // ... of the runs behind this one
        for (int t = hi - 1; t >= lo; --t) {
            const long long a = s[t] > pre ? s[t] : pre;
            q = a - t * st > q ? a - t * st : q;
            s[t] = static_cast<int>(q + t * st);
        }
    }
    for (int t = Tb + tid; t < T; t += kRgRepairBlock) s[t] = 0;
}

// grid and LDS as ranges_window_kernel.  Thread f of the block takes column f of the tile.
template <typename Tag, bool MOD>
__global__ __launch_bounds__(256) void ranges_coverage_kernel(
        const typename Tag::store* __restrict__ px, const typename Tag::store* __restrict__ py,
        const long long* __restrict__ boundary, const int* __restrict__ ranges, double* __restrict__ kept, int S, int T,
        int R, int lg, int b0) {
    extern __shared__ double rg_lds[];
    const int b = b0 + blockIdx.y, TF = 1 << lg, t0 = static_cast<int>(blockIdx.x) << lg;
    const int nthreads = static_cast<int>(blockDim.x);
    const RgLen len = rg_len(boundary, b, S, T);
    const int Sb = len.Sb, Tb = len.Tb;
    const int nf = Tb - t0 < TF ? (Tb - t0 > 0 ? Tb - t0 : 0) : TF, Us = rg_stride(S + 1);
    if (nf > 0) {                                                      // (block-uniform)
        rg_stage<Tag, MOD>(rg_lds, px, py, b, S, T, Sb, t0, nf, lg, Us);
        __syncthreads();
    }
    for (int f = threadIdx.x; f < TF && t0 + f < T; f += nthreads) {
        double out = 0.0;
        if (f < nf) {
            const double* g = rg_lds + f * Us;
            int s = ranges[static_cast<size_t>(b) * T + t0 + f];
            s = s < 0 ? 0 : (s > Sb ? Sb : s);
            const int e = Sb + 1 - s < R ? Sb + 1 : s + R;
            double w = 0.0, c = 0.0;
#pragma unroll 4
            for (int u = s; u < e; ++u) w += g[u];
#pragma unroll 8
            for (int u = 0; u <= Sb; ++u) c += g[u];
            out = c == 0.0 ? 0.0 : w / c;
        }
        kept[static_cast<size_t>(b) * T + t0 + f] = out;
    }
}

}  // namespace rnnt
