// rnnt_delay_kernels.h -- the gfx950 kernels of the delay-penalized RNN-T loss and of the expected emission frames
// (include/rnnt_delay.h).
//
// Logits (N, maxT, maxU, A), one softmax per row.  The standard RNN-T lattice -- a label edge stays in its frame,
// (t, u) -> (t, u + 1) -- with the label edge of row (t, u) biased by delay_penalty * ((T_b - 1) / 2 - t).  Five stages:
//   1 delay_stats_kernel       online max / sum-exp of every in-lattice row, gather of the blank and label logits; one cell
//                              record per row, with the penalty's bias on both edges in the gauge described at the kernel
//                              (formed in fp64 per row)
//   2 ar_lattice_wave_kernel / ar_lattice_block_kernel (rnnt_ar_kernels.h): the sweep over anti-diagonals works from the cell
//                              records alone and has no band test, so the bias needs nothing of it; the fp64 offsets per
//                              chunk (wave form) or per diagonal (block form) absorb the level of a diagonal
//   3 delay_coef_kernel        a thread per row: the posteriors of the row's two out-edges -> the gradient record, written
//                              over the cell record of stage 1; kPadded on padding
//   4 delay_emit_kernel        emit_frames[b, u] = sum_t t * cl(t, u) from word 2 of the records, fp64, a fixed order
//   5 mblank_grad_kernel / mblank_grad_elem_kernel (rnnt_mblank_kernels.h) with K = 0: the record is the multi-blank one
//
// Records, offsets and the lattice arrays are those of rnnt_ar_kernels.h (kArRec, ar_offsets).
#pragma once

#include "rnnt_ar_kernels.h"           // stage 2; through it mono_lse2, the record format and stage 5

namespace rnnt {

constexpr int kDelayEmitSlices = 8;     // frame slices of the narrow form of stage 4: 32 lanes across u, 8 slices of t
constexpr int kDelayEmitNarrow = 64;    // the release rule of stage 4: up to 64 label columns -> the sliced form

// ------------------------------------------------------------------------------------------
// Stage 1.  G lanes per row (G = 4, 16, 64), 256 / G rows per block.  grid = (ceil(maxT * maxU * G / 256), N slice).
// row_lse (rnnt_row_lse.h) over every in-lattice row.  After it a cell holds [lp_blank, lp_label, logZ, -] (lp: base
// 2; logZ: natural log; -inf = no edge); the lp carry the row's biases.
//
// THE GAUGE.  With p = delay_penalty and c = (T_b - 1) / 2 the header puts p (c - t) on the label edge of row (t, u).  Taken
// literally, a partial path to (t, u) has collected about p u (c - t / 2) -- 1350 nats at p = 0.01, T_b = 1500, u = 300 --
// so the values of a diagonal lie that far from its offset and fp32 loses the bits (measured: the gradient of T = 1500,
// U = 301 at 1.5e-3 of its terms).  Edge weights may be re-gauged by any node potential phi, w' = w + phi(from) - phi(to):
// every path (0, 0) -> terminal node changes by phi(0, 0) - phi(terminal), the edge posteriors do not change at all.  With
//     phi(t, u) = p u (c - t / 2),   phi(terminal node) = 0        (phi(0, 0) = 0 and phi(T_b - 1, L_b) = 0 as well)
// the label edge of (t, u) carries -p t / 2, the blank edge (t, u) -> (t + 1, u) carries +p u / 2 and the final blank
// nothing: the same cost, the same posteriors, and the two contributions cancel along a path that spreads its labels evenly,
// so lattice values stay where they are at p = 0.  Neither bias depends on T_b.
template <typename Tag, int G>
__global__ __launch_bounds__(256) void delay_stats_kernel(
        const typename Tag::store* __restrict__ acts, const int* __restrict__ labels, const int* __restrict__ xlen,
        const int* __restrict__ ylen, typename Tag::comp* __restrict__ tab, int maxT, int maxU, int A, int blank, float penalty,
        int b0, int* __restrict__ poison) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const int b = b0 + blockIdx.y;
    const int gl = threadIdx.x & (G - 1);
    const int q = blockIdx.x * (256 / G) + static_cast<int>(threadIdx.x) / G;     // row inside the sample
    if (q >= maxT * maxU) return;                                                 // (whole groups leave together)
    int T, Lb;
    if (!tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb)) return;                      // (the lattice marks the cost)
    const int t = q / maxU, u = q - t * maxU;
    if (t >= T || u > Lb) return;                                                 // padding: never read, never written
    C* rec = tab + tdt_cell(b, t, u, maxT, maxU) * kArRec;
    const bool has_lab = u < Lb;
    const int lab = has_lab ? row_label(labels, b, u, maxU, A) : blank;
    const St* row = acts + tdt_cell(b, t, u, maxT, maxU) * A;
    const C xb = load1<Tag>(row + blank);
    const C xl = load1<Tag>(row + lab);
    const C logZ = row_lse<Tag, G>(row, A, gl).log();
    if (gl != 0) return;
    // the row's two biases in the gauge of the note above, base 2: fp64 from the float's value, one rounding to the lattice
    // type.  The final blank (T_b - 1, L_b) -> terminal node carries none: phi is 0 at both its ends
    const double half = 0.5 * static_cast<double>(penalty) * kLog2e;
    const C bias_label = static_cast<C>(-half * t);
    const C bias_blank = t + 1 < T ? static_cast<C>(half * u) : C(0);
    // the blank of the last frame exists only at u == L_b: it leaves the final node
    const bool has_blank = t + 1 < T || u == Lb;
    rec[0] = has_blank ? (xb - logZ) * C(kLog2e) + bias_blank : neg_inf<C>();
    rec[1] = has_lab ? (xl - logZ) * C(kLog2e) + bias_label : neg_inf<C>();
    rec[2] = logZ;
    if (non_finite(logZ)) poison[b] = 1;                                          // (several bad rows race: any store will do)
}

// ------------------------------------------------------------------------------------------
// Stage 3.  A thread per row: grid = (ceil(maxT * maxU / 256), N slice), block = 256.  ar_coef_kernel without the band:
//   cb = 2^(alpha(t, u) + lp_blank + beta(t + 1, u) - log P),   cl = the same with lp_label and beta(t, u + 1) (the biases inside the lp),
// the fp64 offsets summed first; beta(T_b, L_b) = 0 is the terminal node.  The record: [ln(cb + cl) - logZ, cb, cl, label].
// Padding rows and every row of a sample whose lengths do not fit get kPadded (the gradient stream zero-fills them without
// reading their logits); a poisoned sample or one without a path gets NaN records on every in-lattice row.
template <typename L>
__global__ __launch_bounds__(256) void delay_coef_kernel(
        L* tab, const L* __restrict__ alpha, const L* __restrict__ beta, const double* __restrict__ offa,
        const double* __restrict__ offb, const double* __restrict__ ll, const int* __restrict__ xlen,
        const int* __restrict__ ylen, const int* __restrict__ labels, const int* __restrict__ poison, int maxT, int maxU, int A,
        int b0) {
    const int b = b0 + blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= maxT * maxU) return;
    const int t = q / maxU, u = q - t * maxU;
    const size_t c = tdt_cell(b, t, u, maxT, maxU);
    L* r = tab + c * kArRec;
    int T, Lb;
    if (!tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb) || t >= T || u > Lb) {
        r[3] = static_cast<L>(kPadded);
        return;
    }
    const int lab = u < Lb ? row_label(labels, b, u, maxU, A) : -1;
    const double lp = ll[b];
    if (poison[b] != 0 || !(lp - lp == 0.0)) {                       // NaN gradients on every in-lattice row
        const L nan = static_cast<L>(__builtin_nan(""));
        r[0] = r[1] = r[2] = nan;
        r[3] = static_cast<L>(lab);
        return;
    }
    const size_t o0 = static_cast<size_t>(b) * ar_offsets(maxT, maxU);
    const L o = static_cast<L>(offa[o0 + t + u] + offb[o0 + t + u + 1] - lp);
    const L a = alpha[c] + o;
    const L lb = r[0], ltok = r[1], lz = r[2];
    const L bt = t + 1 < T ? beta[c + maxU] : (u == Lb ? L(0) : neg_inf<L>());
    const L bl = u < Lb ? beta[c + 1] : neg_inf<L>();
    const L cb = fast_exp2(a + lb + bt);
    const L cl = u < Lb ? fast_exp2(a + ltok + bl) : L(0);
    r[0] = acc_log(cb + cl) - lz;
    r[1] = cb;
    r[2] = cl;
    r[3] = static_cast<L>(lab);
}

// ------------------------------------------------------------------------------------------
// Stage 4.  emit[b, u] = sum_t t * cl(t, u), cl = word 2 of row (t, u)'s record; block = 256 = W lanes across u by S slices of
// the frames (W = 256 / S), grid = (ceil((maxU - 1) / W), N slice).  The table lies in natural order (row t * maxU + u), so
// the lanes of a slice read neighbouring records.  Slice y sums its frames [y c, (y + 1) c), c = ceil(T_b / S), in fp64 in
// rising t, four records requested ahead of the four additions; the S partial sums of a column then meet in an LDS tree of
// fixed shape (slice y takes slice y + s, s = S / 2 .. 1).  No atomics: the order of every addition is the same in every
// run.  S = 1: one thread per column, no LDS.  Every element of the array is written: 0 for u >= L_b and for a sample whose
// lengths do not fit; a poisoned or pathless sample has NaN records, so its sums are NaN (0 * NaN included: T_b = 1).
template <typename L, int S>
__global__ __launch_bounds__(256) void delay_emit_kernel(const L* __restrict__ tab, const int* __restrict__ xlen,
                                                         const int* __restrict__ ylen, L* __restrict__ emit, int maxT, int maxU,
                                                         int b0) {
    constexpr int W = 256 / S;
    __shared__ double part[S > 1 ? 256 : 1];
    const int b = b0 + blockIdx.y;
    const int x = static_cast<int>(threadIdx.x) % W, y = static_cast<int>(threadIdx.x) / W;
    const int u = blockIdx.x * W + x;
    int T, Lb;
    const bool fits = tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb);
    double acc = 0.0;
    if (fits && u < Lb) {                                            // (u < L_b <= maxU - 1: a column of the table)
        const int c = (T + S - 1) / S;
        const int t0 = y * c, t1 = t0 + c < T ? t0 + c : T;
        const size_t stride = static_cast<size_t>(maxU) * kArRec;
        const L* p = tab + tdt_cell(b, 0, u, maxT, maxU) * kArRec + 2;
        int t = t0;
        for (; t + 4 <= t1; t += 4) {
            L v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = p[(t + k) * stride];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc += static_cast<double>(t + k) * static_cast<double>(v[k]);
        }
        for (; t < t1; ++t) acc += static_cast<double>(t) * static_cast<double>(p[t * stride]);
    }
    if (S > 1) {                                                     // (every thread of the block arrives: no early return above)
        part[y * W + x] = acc;
        __syncthreads();
#pragma unroll
        for (int s = S / 2; s > 0; s >>= 1) {
            if (y < s) part[y * W + x] += part[(y + s) * W + x];
            __syncthreads();
        }
        acc = part[x];
    }
    if (y == 0 && u < maxU - 1) emit[static_cast<size_t>(b) * (maxU - 1) + u] = static_cast<L>(acc);
}

}  // namespace rnnt
