// rnnt_align_kernels.h -- best-path (Viterbi) alignment on the lattice the loss sums over (compute_rnnt_align*, include/rnnt.h).
//
//   1 (the statistics stage of the loss, unchanged: lp2 = {log2 p(blank|t,u), log2 p(y_u|t,u)} in the skewed layout)
//   2 align_lattice_kernel    max-plus recursion over the anti-diagonals: one block per sample, one lane per u, the left
//                             neighbour through a DPP wave shift (and one LDS word per wavefront boundary and diagonal when
//                             maxU > 64); fp64 accumulation of the base-2 terms (c4 paths add ~1800 of them); ONE decision
//                             bit per cell -- "the label predecessor (t, u-1) is strictly better than the blank one (t-1, u)",
//                             so a tie keeps the blank predecessor and labels are emitted as early as possible -- packed by
//                             a ballot into one 64-bit word per (diagonal, wavefront), stored in the sample's beta array
//                             (free in an align call: no beta sweep, no coefficient table)               [latency-bound, O(T+U)]
//   3 align_traceback_kernel  one block per sample walks back from (T_b-1, U_b) over the decision bits, staged into LDS a
//                             chunk of diagonals at a time, so that the serial walk reads LDS and never waits on a
//                             dependent HBM load; writes frames[b, u] and the natural-log score          [O(T+U) serial]
//
// Host side: launch_align() below, the one entry the materialised driver (run_gpu_align, rnnt_gpu_impl.h) and the
// additive-joint driver (run_gpu_joint) call behind their statistics stages.  The kernels are instantiated in ONE translation
// unit, rnnt_joint.hip (rnnt_align.h says why).
#pragma once

#include "rnnt_align.h"
#include "rnnt_kernels.h"

namespace rnnt {

constexpr int kAlignMaxWaves = 16;                  // maxU <= 1024 (make_plan): at most 16 wavefronts of one column per lane
template <typename L> struct AlignChunk { static constexpr int C = sizeof(L) == 4 ? 16 : 8; };   // lp2 rows per chunk: the next chunk loads while this one computes
constexpr int kAlignLdsWords = 4096;                // traceback staging: 32 KB of decision words per chunk of diagonals

__device__ __forceinline__ double align_neg_inf() { return -__builtin_huge_val(); }

// Decision words of sample b: word n * W + w holds the bits of wavefront w on anti-diagonal n (bit = lane).  Dp rows of W words
// take Dp * W * 8 <= Dp * Up * sizeof(L) bytes (Up >= 8, W = ceil(Up / 64)): the sample's beta array holds them.
template <typename L>
__host__ __device__ inline unsigned long long* align_bits(L* beta, int b, int maxT, int maxU, int Up) {
    return reinterpret_cast<unsigned long long*>(beta + lat_sample(b, maxT, maxU, Up));
}

// grid = N, block = 64 W (W = ceil(Up / 64)).  best[b] = base-2 log-probability of the best path, or -inf (no path of
// non-zero probability), NaN (a non-finite row inside the sample: the poison hint of the statistics kernels), the
// cost_invalid marker (device-side lengths that do not fit the tensor).
template <typename L>
static __global__ __launch_bounds__(kAlignMaxWaves * 64) void align_lattice_kernel(
        const LogPair<L>* __restrict__ lp2, const L* __restrict__ logz, L* __restrict__ beta, double* __restrict__ best,
        int* __restrict__ poison, const int* __restrict__ xlen, const int* __restrict__ ylen, int maxT, int maxU, int Up) {
    constexpr int C = AlignChunk<L>::C;
    __shared__ double edge[2][kAlignMaxWaves];      // lane 63's label candidate of each wavefront, per diagonal parity
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6), W = static_cast<int>(blockDim.x >> 6);
    const int Tb_raw = xlen[b], Ub_raw = ylen[b] + 1;
    const bool bad_len = Tb_raw < 1 || Ub_raw < 1 || Tb_raw > maxT || Ub_raw > maxU;
    const int Tb = Tb_raw < 1 ? 1 : (Tb_raw > maxT ? maxT : Tb_raw);
    const int Ub = Ub_raw < 1 ? 1 : (Ub_raw > maxU ? maxU : Ub_raw);
    const int Db = Tb + Ub - 1;
    const int u = tid;
    const bool in_row = u < Up;
    const LogPair<L>* row0 = lp2 + lat_sample_pair(b, maxT, maxU, Up) + static_cast<size_t>(kLatPad) * Up + (in_row ? u : 0);
    unsigned long long* bits = align_bits(beta, b, maxT, maxU, Up) + wave;
    const double NEG = align_neg_inf();
    // a = best base-2 score of the path prefix ending in cell (n - u, u) of the current diagonal; -inf off the lattice
    double a = (u == 0) ? 0.0 : NEG;
    auto load = [&](int n) -> LogPair<L> {       // row n of the sample (clamped: the last chunk re-reads row Db - 1)
        const int r = n < Db ? n : Db - 1;
        return in_row ? row0[static_cast<size_t>(r) * Up] : LogPair<L>{L(0), L(0)};
    };
    LogPair<L> bufA[C], bufB[C];
#pragma unroll
    for (int k = 0; k < C; ++k) bufA[k] = load(k);
    double keep = NEG;                           // lane 0's left neighbour inside one wavefront: never a cell (u = -1)
    // chunk n0: step n = n0 + k + 1 reads row n - 1 = cur[k] (the predecessors' terms) and decides the cells of diagonal n,
    // while the next chunk's rows are in flight in `nxt`.  The two buffers keep FIXED roles per call site (the loop is
    // unrolled by two chunks): a register copy between them would wait for the loads still in flight.
    auto chunk = [&](int n0, LogPair<L> (&cur)[C], LogPair<L> (&nxt)[C]) {
#pragma unroll
        for (int k = 0; k < C; ++k) nxt[k] = load(n0 + C + k);
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int n = n0 + k + 1;            // target diagonal
            if (n >= Db) break;
            const bool live = a != NEG;
            const double stay = live ? a + static_cast<double>(lat_clamp(cur[k].x)) : NEG;    // (t-1, u) -> (t, u) by a blank
            const double emit = live ? a + static_cast<double>(lat_clamp(cur[k].y)) : NEG;    // (t, u) -> (t, u+1) by label u
            double up = wave_shr1(keep, emit);
            if (W > 1) {
                if (lane == 63) edge[n & 1][wave] = emit;
                lds_barrier();
                if (lane == 0 && wave > 0) up = edge[n & 1][wave - 1];
            }
            const bool take_label = up > stay;   // strict: an exact tie keeps the blank predecessor
            const int t = n - u;
            const bool cell = u < Ub && t >= 0 && t < Tb;
            a = cell ? (take_label ? up : stay) : NEG;
            const unsigned long long word = __ballot(cell && take_label);
            if (lane == 0) bits[static_cast<size_t>(n) * W] = word;
        }
    };
    for (int n0 = 0; n0 < Db; n0 += 2 * C) {
        chunk(n0, bufA, bufB);
        if (n0 + C < Db) chunk(n0 + C, bufB, bufA);
    }
    // the terminal cell (T_b - 1, U_b - 1) of the loss's indexing, then the final blank
    if (u == Ub - 1) {
        const LogPair<L> last = row0[static_cast<size_t>(Db - 1) * Up];
        double s = a + static_cast<double>(lat_clamp(last.x));
        const int hint = poison[b];
        if (hint != 0) {
            poison[b] = 0;
            if (hint_is_poison(hint, logz, lat_sample(b, maxT, maxU, Up), Up, Tb, Ub)) s = __builtin_nan("");
        }
        // every path crosses a cell masked with -inf: the sum ends on the finite "log zero" sentinel of lat_clamp
        if (s < 0.5 * static_cast<double>(log_zero<L>())) s = NEG;
        best[b] = bad_len ? cost_invalid<double>() : s;
    }
}

// grid = N, block = 256.  frames (N, maxU - 1): the frame of label u for u < U_b - 1 (the loss's U_b = labels + 1), -1 behind;
// a sample without a finite best path gets -1 everywhere.  score[b] = best[b] in natural log.
template <typename L>
static __global__ __launch_bounds__(256) void align_traceback_kernel(
        const L* __restrict__ beta, const double* __restrict__ best, double* __restrict__ score, int* __restrict__ frames,
        const int* __restrict__ xlen, const int* __restrict__ ylen, int maxT, int maxU, int Up) {
    __shared__ unsigned long long sbits[kAlignLdsWords];
    __shared__ int walk_n;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int W = (Up + 63) / 64;
    const int Tb_raw = xlen[b], Ub_raw = ylen[b] + 1;
    const bool bad_len = Tb_raw < 1 || Ub_raw < 1 || Tb_raw > maxT || Ub_raw > maxU;
    const double s = best[b];
    const bool ok = !bad_len && s - s == 0.0;    // finite
    const int L1 = maxU - 1;                     // frames per row
    int* fr = frames + static_cast<size_t>(b) * L1;
    if (tid == 0) score[b] = bad_len ? s : s * kLn2;
    const int first_unused = ok ? Ub_raw - 1 : 0;
    for (int i = first_unused + tid; i < L1; i += blockDim.x) fr[i] = -1;
    if (!ok) return;
    const int Tb = Tb_raw, Ub = Ub_raw;
    const unsigned long long* bits = align_bits(const_cast<L*>(beta), b, maxT, maxU, Up);
    const int rows = kAlignLdsWords / W;         // diagonals per staged chunk (>= 256)
    int t = Tb - 1, u = Ub - 1, n = Tb + Ub - 2;    // thread 0's walk
    if (tid == 0) walk_n = n;
    __syncthreads();
    int nn = walk_n;
    while (nn > 0) {
        const int lo = nn - rows + 1 > 1 ? nn - rows + 1 : 1;     // diagonal 0 needs no decision
        const int words = (nn - lo + 1) * W;
        for (int i = tid; i < words; i += blockDim.x) sbits[i] = bits[static_cast<size_t>(lo) * W + i];
        __syncthreads();
        if (tid == 0) {
            for (; n >= lo; --n) {
                bool label;
                if (u == 0) label = false;
                else if (t == 0) label = true;
                else label = (sbits[(n - lo) * W + (u >> 6)] >> (u & 63)) & 1ull;
                if (label) { fr[u - 1] = t; --u; } else { --t; }
            }
            walk_n = n;
        }
        __syncthreads();
        nn = walk_n;
    }
}

// Both stages for the whole batch on `stream`; returns false if a launch failed.
template <typename L>
bool launch_align(const AlignArgs<L>& g) {
    const int W = (g.Up + 63) / 64;
    if (W > kAlignMaxWaves) return false;
    hipLaunchKernelGGL((align_lattice_kernel<L>), dim3(g.N), dim3(64 * W), 0, g.stream, g.lp2, g.logz, g.beta, g.best,
                       g.poison, g.xlen, g.ylen, g.maxT, g.maxU, g.Up);
    if (hipGetLastError() != hipSuccess) return false;
    hipLaunchKernelGGL((align_traceback_kernel<L>), dim3(g.N), dim3(256), 0, g.stream, g.beta, g.best, g.score, g.frames,
                       g.xlen, g.ylen, g.maxT, g.maxU, g.Up);
    return hipGetLastError() == hipSuccess;
}

}  // namespace rnnt
