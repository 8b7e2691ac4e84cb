// rnnt_pstream_kernels.h -- the gfx950 kernels of the pruned RNN-T loss with k2's two lattice types and delay_penalty
// (include/rnnt_pstream.h).
//
// Logits (N, maxT, S, A), one softmax per row: row (b, t, k) is the joint output of lattice state u = s_t + k, s_t =
// ranges[b, t].  rnnt_type 0 is the lattice of rnnt_delay_kernels.h (a label edge stays in its frame), 1 the lattice of
// rnnt_mono_kernels.h (a label edge consumes a frame); in both a node has out-edges only inside its frame's window and the
// label edge of row (t, u) is biased by delay_penalty * ((T_b - 1) / 2 - t).  Five stages:
//   0 pstream_prep_kernel      per frame the window word {s_t, rows inside the lattice}, per sample the "bad start" flag, and
//                              a "no edge" record into every in-lattice cell of the natural-order maxT x maxU table that no
//                              READ row of the tensor covers (outside its frame's window; type 1: outside the band too), so
//                              that the unchanged lattice kernels need no window or band test and read no stale word
//   1 pstream_stats_kernel     online max / sum-exp of every row that can lie on a path, gather of the blank and label
//                              logits; the cell record [lp_blank, lp_label, logZ, -] at cell (t, s_t + k), the penalty's bias
//                              on both edges in the gauge described at the kernel (formed in fp64 per row)
//   2 ar_lattice_wave_kernel / ar_lattice_block_kernel (rnnt_ar_kernels.h, type 0) or mono_lattice_wave_kernel /
//     mono_lattice_block_kernel (rnnt_mono_kernels.h, type 1), instantiated in this library's code objects; then
//     pstream_close_kernel, a thread per sample: the bad-start cost marker, and for type 1 the gauge's constant back into
//     the cost in fp64
//   3 pstream_coef_kernel      a thread per row of the TENSOR: alpha / beta at (t, s_t + k) read once, the gradient record
//                              [ln(cb + cl) - logZ, cb, cl, label] written COMPACTLY at (b, t, k) of an (N, maxT, S) table;
//                              kPadded on every row that is never read
//   4 mblank_grad_kernel / mblank_grad_elem_kernel (rnnt_mblank_kernels.h) with K = 0 over the compact table, its "maxU"
//                              being S: one record lookup per packet, no window word
//
// Records, offsets and the lattice arrays are those of rnnt_ar_kernels.h / rnnt_mono_kernels.h (kArRec == kMonoRec == 4).
#pragma once

#include "rnnt_ar_kernels.h"           // stage 2: both lattices; through it mono_lse2, tdt_cell, the record format and stage 4

namespace rnnt {

constexpr int kPsRec = kArRec;          // == kMonoRec: four lattice values per cell
static_assert(kArRec == kMonoRec && kArRec == 4, "one record format for both lattices");
constexpr int kPsPrepFrames = 32;       // frames per block of stage 0

// per sample offsets of either lattice: one per diagonal and the terminal one (type 0), one per frame and the terminal row
// (type 1; maxT + 1 <= maxT + maxU)
__host__ __device__ inline int ps_offsets(int maxT, int maxU) { return ar_offsets(maxT, maxU); }

// The row (t, u) of a sample with T frames and L labels is READ: inside the lattice and, type 1, inside the band.  (The
// window test is the caller's.)
__device__ __forceinline__ bool ps_row_read(bool mod, int t, int u, int T, int L) { return !mod || mono_live(t, u, T, L); }

// [-inf, -inf, 0, 0]: a cell without out-edges, as 16-byte stores
__device__ __forceinline__ void ps_store_none(float* p) {
    *reinterpret_cast<float4*>(p) = make_float4(neg_inf<float>(), neg_inf<float>(), 0.0f, 0.0f);
}
__device__ __forceinline__ void ps_store_none(double* p) {
    reinterpret_cast<double2*>(p)[0] = make_double2(neg_inf<double>(), neg_inf<double>());
    reinterpret_cast<double2*>(p)[1] = make_double2(0.0, 0.0);
}
__device__ __forceinline__ void ps_store_rec(float* p, float a, float b, float c, float d) {
    *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
__device__ __forceinline__ void ps_store_rec(double* p, double a, double b, double c, double d) {
    reinterpret_cast<double2*>(p)[0] = make_double2(a, b);
    reinterpret_cast<double2*>(p)[1] = make_double2(c, d);
}

// ------------------------------------------------------------------------------------------
// Stage 0.  grid = (ceil(maxT / kPsPrepFrames), N slice), block = 256: frames [32 x, 32 x + 32) of sample b.
// win[b, t] = {s_t, n_t}: n_t = rows of the frame inside the lattice (k < n_t <=> t < T_b and s_t + k <= L_b); {0, 0} for a
// frame past T_b and for every frame of a sample with bad lengths or a bad start.
template <typename L>
__global__ __launch_bounds__(256) void pstream_prep_kernel(
        const int* __restrict__ ranges, const int* __restrict__ xlen, const int* __restrict__ ylen, L* __restrict__ tab,
        int2* __restrict__ win, int* __restrict__ bad, int maxT, int maxU, int S, int mod, int b0) {
    const int b = b0 + blockIdx.y;
    int T, Lb;
    const bool lens_ok = tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb);
    // a start outside [0, L_b] in ANY frame of the sample: the whole sample is invalid (the cost marker, zero gradients)
    int my_bad = 0;
    if (lens_ok)
        for (int t = threadIdx.x; t < T; t += 256) {
            const int s = ranges[static_cast<size_t>(b) * maxT + t];
            if (s < 0 || s > Lb) my_bad = 1;
        }
    const bool sample_bad = __syncthreads_or(my_bad) != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) bad[b] = sample_bad ? 1 : 0;
    const bool live = lens_ok && !sample_bad;
    const int t0 = blockIdx.x * kPsPrepFrames;
    if (threadIdx.x < kPsPrepFrames && t0 + static_cast<int>(threadIdx.x) < maxT) {
        const int t = t0 + threadIdx.x;
        int s = 0, n = 0;
        if (live && t < T) {
            s = ranges[static_cast<size_t>(b) * maxT + t];
            n = Lb - s + 1 < S ? Lb - s + 1 : S;
        }
        win[static_cast<size_t>(b) * maxT + t] = make_int2(s, n);
    }
    if (!lens_ok) return;                     // (the lattice marks the cost and reads no record)
    const int Ub = Lb + 1;
    const int t1 = t0 + kPsPrepFrames < T ? t0 + kPsPrepFrames : T;
    for (int i = threadIdx.x; i < (t1 - t0) * Ub; i += 256) {
        const int t = t0 + i / Ub, u = i - (i / Ub) * Ub;
        if (live) {
            const int s = ranges[static_cast<size_t>(b) * maxT + t];
            // a read row covers the cell: the statistics kernel writes it
            if (u >= s && u < s + S && ps_row_read(mod != 0, t, u, T, Lb)) continue;
        }
        ps_store_none(tab + tdt_cell(b, t, u, maxT, maxU) * kPsRec);
    }
}

// ------------------------------------------------------------------------------------------
// Stage 1.  G lanes per row (G = 4, 16, 64), 256 / G rows per block.  grid = (ceil(maxT * S * G / 256), N slice).  The row
// reduction is row_lse (rnnt_row_lse.h).  After it cell (t, s_t + k) holds [lp_blank, lp_label, logZ, 0] (lp: base 2; logZ: natural log; -inf = no edge); the lp carry
// the row's biases.
//
// THE GAUGE.  With p = delay_penalty and c = (T_b - 1) / 2 the header puts p (c - t) on the label edge of row (t, u).  Taken
// literally a partial path to (t, u) has collected about p u (c - t / 2), so the values of one anti-diagonal (type 0) or of
// one frame (type 1) lie far apart and fp32 loses the bits (rnnt_delay_kernels.h has the measurement).  Edge weights may be
// re-gauged by any node potential phi, w' = w + phi(from) - phi(to): every path changes by phi(0, 0) - phi(terminal), the edge
// posteriors do not change at all.  With
//     phi(t, u) = p u (c - t / 2)
//   type 0   label (t, u) -> (t, u + 1):      p (c - t) + phi(t, u) - phi(t, u + 1)     = -p t / 2
//            blank (t, u) -> (t + 1, u):      phi(t, u) - phi(t + 1, u)                 = +p u / 2
//            the final blank out of (T_b - 1, L_b) carries nothing: phi(T_b - 1, L_b) = 0 = phi(0, 0)
//   type 1   label (t, u) -> (t + 1, u + 1):  p (c - t) + phi(t, u) - phi(t + 1, u + 1) = +p (u - t + 1) / 2
//            blank (t, u) -> (t + 1, u):                                                 +p u / 2
//            the terminal node is (T_b, L_b), phi = p L_b (c - T_b / 2) = -p L_b / 2, and the formulas hold for the two
//            edges into it; phi(0, 0) - phi(terminal) = +p L_b / 2 is NOT zero: every path of the gauged lattice weighs
//            p L_b / 2 more, and pstream_close_kernel takes that constant back out of the cost in fp64.
// None of the terms depends on T_b.  Formed in fp64 per row from the float's value, one rounding to the lattice type.
template <typename Tag, int G>
__global__ __launch_bounds__(256) void pstream_stats_kernel(
        const typename Tag::store* __restrict__ acts, const int2* __restrict__ win, const int* __restrict__ labels,
        const int* __restrict__ xlen, const int* __restrict__ ylen, typename Tag::comp* __restrict__ tab, int maxT, int maxU,
        int S, int A, int blank, int mod, float penalty, int b0, int* __restrict__ poison) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const int b = b0 + blockIdx.y;
    const int gl = threadIdx.x & (G - 1);
    const int q = blockIdx.x * (256 / G) + static_cast<int>(threadIdx.x) / G;     // row inside the sample
    if (q >= maxT * S) return;                                                    // (whole groups leave together)
    const int t = q / S, k = q - t * S;
    const int2 w = win[static_cast<size_t>(b) * maxT + t];
    if (k >= w.y) return;                                                         // padding, bad sample: never read
    const int u = w.x + k;
    const int T = xlen[b], Lb = ylen[b];                                          // (w.y > 0: the lengths fit)
    if (!ps_row_read(mod != 0, t, u, T, Lb)) return;                              // outside the band: never read (stage 0 wrote the cell)
    const bool has_lab = u < Lb;
    const int lab = has_lab ? row_label(labels, b, u, maxU, A) : blank;
    const St* row = acts + (static_cast<size_t>(b) * maxT * S + q) * A;
    const C xb = load1<Tag>(row + blank);
    const C xl = load1<Tag>(row + lab);
    const C logZ = row_lse<Tag, G>(row, A, gl).log();
    if (gl != 0) return;
    // the row's two biases in the gauge of the note above, base 2
    const double half = 0.5 * static_cast<double>(penalty) * kLog2e;
    C bias_label, bias_blank;
    bool has_blank;
    if (mod != 0) {
        bias_label = static_cast<C>(half * (u - t + 1));
        bias_blank = static_cast<C>(half * u);
        has_blank = Lb - u < T - t;               // stays inside the band, or enters the terminal node (rnnt_mono_kernels.h)
    } else {
        bias_label = static_cast<C>(-half * t);
        bias_blank = t + 1 < T ? static_cast<C>(half * u) : C(0);
        has_blank = t + 1 < T || u == Lb;         // the blank of the last frame exists only at u == L_b: the final one
    }
    const C r0 = has_blank ? (xb - logZ) * C(kLog2e) + bias_blank : neg_inf<C>();
    const C r1 = has_lab ? (xl - logZ) * C(kLog2e) + bias_label : neg_inf<C>();
    ps_store_rec(tab + tdt_cell(b, t, u, maxT, maxU) * kPsRec, r0, r1, logZ, C(0));
    if (non_finite(logZ)) poison[b] = 1;                                          // (several bad rows race: any store will do)
}

// ------------------------------------------------------------------------------------------
// Behind stage 2.  A thread per sample: grid = ceil(N / 256).  A sample with a start outside [0, L_b] gets the
// invalid-arguments cost marker.  Type 1: the lattice kernel closed the sample with the GAUGED lattice's cost; every path of
// it weighs phi(0, 0) - phi(terminal) = p L_b / 2 more than the header's, so cost = -ln P' + p L_b / 2, from ll (log2 P',
// fp64) with one rounding to the cost's type.  (ll itself stays gauged: the coefficient kernel normalises gauged terms.)
template <typename L>
__global__ __launch_bounds__(256) void pstream_close_kernel(
        const int* __restrict__ bad, const int* __restrict__ xlen, const int* __restrict__ ylen,
        const double* __restrict__ ll, const int* __restrict__ poison, L* __restrict__ costs, int N, int maxT, int maxU,
        int mod, float penalty) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= N) return;
    int T, Lb;
    if (!tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb)) return;         // (the lattice kernel left the marker)
    if (bad[b] != 0) {
        costs[b] = cost_invalid<L>();
        return;
    }
    if (mod == 0) return;
    const double lp = ll[b];
    if (poison[b] != 0 || !(lp - lp == 0.0)) return;                 // NaN or +inf: as the lattice kernel left it
    costs[b] = static_cast<L>(-lp * kLn2 + 0.5 * static_cast<double>(penalty) * Lb);
}

// ------------------------------------------------------------------------------------------
// Stage 3.  A thread per row of the tensor: grid = (ceil(maxT * S / 256), N slice), block = 256.  Row (t, k) of sample b
// is cell (t, u = s_t + k) of the natural-order table:
//   cb = 2^(alpha(t, u) + lp_blank + beta(t + 1, u) - log P)
//   cl = 2^(alpha(t, u) + lp_label + beta(t, u + 1) - log P)       type 0; the successors lie on diagonal t + u + 1
//   cl = 2^(alpha(t, u) + lp_label + beta(t + 1, u + 1) - log P)   type 1; the successors lie in frame t + 1
// (the biases inside the lp), the fp64 offsets summed first, as delay_coef_kernel / mono_coef_kernel; the terminal node has
// beta = 0.  The record [ln(cb + cl) - logZ, cb, cl, label] goes to row (b, t, k) of the compact (N, maxT, S) table `out`.
// kPadded: padding rows (k >= n_t), every row of a sample with bad lengths or a bad start, and -- type 1, a sample with a
// path -- rows outside the band.  A poisoned sample or one without a path: NaN records on every in-lattice row.
template <typename L>
__global__ __launch_bounds__(256) void pstream_coef_kernel(
        const L* __restrict__ tab, L* __restrict__ out, const L* __restrict__ alpha, const L* __restrict__ beta,
        const double* __restrict__ offa, const double* __restrict__ offb, const double* __restrict__ ll,
        const int2* __restrict__ win, const int* __restrict__ xlen, const int* __restrict__ ylen,
        const int* __restrict__ labels, const int* __restrict__ poison, int maxT, int maxU, int S, int A, int mod, int b0) {
    using P = typename MonoPair<L>::type;
    const int b = b0 + blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= maxT * S) return;
    const int t = q / S, k = q - t * S;
    L* r = out + (static_cast<size_t>(b) * maxT * S + q) * kPsRec;
    const int2 w = win[static_cast<size_t>(b) * maxT + t];
    if (k >= w.y) {                                                  // (bad lengths, bad start: n_t = 0 in every frame)
        ps_store_rec(r, L(0), L(0), L(0), static_cast<L>(kPadded));
        return;
    }
    const int u = w.x + k;
    const int T = xlen[b], Lb = ylen[b];
    const int lab = u < Lb ? row_label(labels, b, u, maxU, A) : -1;
    const double lp = ll[b];
    if (poison[b] != 0 || !(lp - lp == 0.0)) {                       // NaN gradients on every in-lattice row
        const L nan = static_cast<L>(__builtin_nan(""));
        ps_store_rec(r, nan, nan, nan, static_cast<L>(lab));
        return;
    }
    if (!ps_row_read(mod != 0, t, u, T, Lb)) {
        ps_store_rec(r, L(0), L(0), L(0), static_cast<L>(kPadded));
        return;
    }
    const size_t c = tdt_cell(b, t, u, maxT, maxU);
    // (each lattice kernel strides the offset arrays by its own count per sample)
    const size_t o0 = static_cast<size_t>(b) * (mod != 0 ? mono_offsets(maxT) : ar_offsets(maxT, maxU));
    const int d = mod != 0 ? t : t + u;
    const L a = alpha[c] + static_cast<L>(offa[o0 + d] + offb[o0 + d + 1] - lp);
    const P e = *reinterpret_cast<const P*>(tab + c * kPsRec);
    const L lz = tab[c * kPsRec + 2];
    L bu, bu1 = neg_inf<L>();                                        // beta behind the blank edge, behind the label edge
    if (mod != 0) {
        if (t + 1 < T) {
            bu = beta[c + maxU];
            if (u < Lb) bu1 = beta[c + maxU + 1];
        } else {
            bu = u == Lb ? L(0) : neg_inf<L>();
            if (u + 1 == Lb) bu1 = L(0);
        }
    } else {
        bu = t + 1 < T ? beta[c + maxU] : (u == Lb ? L(0) : neg_inf<L>());
        if (u < Lb) bu1 = beta[c + 1];
    }
    const L cb = fast_exp2(a + e.x + bu);
    const L cl = u < Lb ? fast_exp2(a + e.y + bu1) : L(0);
    ps_store_rec(r, acc_log(cb + cl) - lz, cb, cl, static_cast<L>(lab));
}

}  // namespace rnnt
