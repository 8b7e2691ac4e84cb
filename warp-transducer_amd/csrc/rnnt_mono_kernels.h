// rnnt_mono_kernels.h -- the gfx950 kernels of the monotonic (one label per frame) transducer loss (include/rnnt_mono.h).
//
// Logits (N, maxT, maxU, A), one softmax per row.  A label edge consumes a frame like a blank edge does,
// (t, u) -> (t + 1, u + 1), so every path has T_b edges and the sweep runs over FRAMES: T_b steps over rows of a
// natural-order table, no skewed layout.  A cell is live only inside the band u <= t, L_b - u <= T_b - t.  Four stages:
//   1 mono_stats_kernel          online max / sum-exp of every BAND row, gather of the blank and label logits; one cell
//                                record per row.  In-lattice rows outside the band get a "no edge" record without their
//                                logits being read, and the blank edge of a band row that would leave the band (L_b - u ==
//                                T_b - t; at t = T_b - 1 that is every blank edge but the one into the terminal node) is no
//                                edge either: no probability mass ever leaves the band, so the lattice needs no band test
//   2 mono_lattice_wave_kernel   maxU <= 64: one wavefront per (sample, direction), a lane per u, alpha / beta in registers,
//                                the neighbour's value through one DPP wave shift per frame; no LDS, no barrier
//     mono_lattice_block_kernel  any maxU: one block per (sample, direction), threads striding over u, predecessors read from
//                                the global arrays the block wrote, one barrier per frame
//   3 mono_coef_kernel           a thread per row: the posteriors of the row's two out-edges -> the gradient record, written
//                                over the cell record of stage 1; kPadded on padding AND on out-of-band rows
//   4 mblank_grad_kernel / mblank_grad_elem_kernel (rnnt_mblank_kernels.h) with K = 0: the record is the multi-blank one
//
// Lattice values are base-2 logs.  The value stored for a cell of frame t is RELATIVE to an fp64 offset off[t] of that
// frame (offa / offb, maxT + 1 per sample: frame T_b is the terminal row), so stored values stay within a few edge weights
// of zero and keep fp32's relative precision however long the utterance.
#pragma once

#include "rnnt_mblank_kernels.h"       // the record format and stage 4; through it tdt_lens, tdt_cell, tdt_log2

namespace rnnt {

constexpr int kMonoRec = 4;             // == mblank_rec_stride(0)
constexpr int kMonoChunk = 8;           // frames per chunk of the wave form (prefetch distance, re-centring period)
constexpr int kMonoWaveMaxU = 64;       // the release rule: maxU <= 64 -> wave form, else block form

// Per cell (b, t, u) of the workspace table, kMonoRec values of the lattice type:
//   after stage 1  [lp_blank, lp_label, logZ, -]      (lp: base 2; logZ: natural log; -inf = no edge)
//   after stage 3  [x, cb, cl, label]                 x = ln(cb + cl) - logZ
// label: the row's label index, -1 without a label edge (u = L_b), kPadded outside the band.
__host__ __device__ inline int mono_offsets(int maxT) { return maxT + 1; }

// (t, u) of a sample with T frames and L labels lies inside the band.  T < L: no cell does.
__device__ __forceinline__ bool mono_live(int t, int u, int T, int L) { return u <= t && L - u <= T - t; }

// log2(2^x + 2^y); -inf is the additive zero
template <typename L> __device__ __forceinline__ L mono_lse2(L x, L y) {
    const L m = vmax(x, y);
    const L r = m + tdt_log2(L(1) + fast_exp2(vmin(x, y) - m));      // (NaN when both are -inf: a select, no branch)
    return m == neg_inf<L>() ? m : r;
}

// ------------------------------------------------------------------------------------------
// Stage 1.  G lanes per row (G = 4, 16, 64), 256 / G rows per block.  grid = (ceil(maxT * maxU * G / 256), N slice).
// row_lse (rnnt_row_lse.h) for band rows only.
template <typename Tag, int G>
__global__ __launch_bounds__(256) void mono_stats_kernel(
        const typename Tag::store* __restrict__ acts, const int* __restrict__ labels, const int* __restrict__ xlen,
        const int* __restrict__ ylen, typename Tag::comp* __restrict__ tab, int maxT, int maxU, int A, int blank, int b0,
        int* __restrict__ poison) {
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
    C* rec = tab + tdt_cell(b, t, u, maxT, maxU) * kMonoRec;
    if (!mono_live(t, u, T, Lb)) {                                                // outside the band: no edge, never read
        if (gl == 0) { rec[0] = neg_inf<C>(); rec[1] = neg_inf<C>(); rec[2] = C(0); }
        return;
    }
    const bool has_lab = u < Lb;
    const int lab = has_lab ? row_label(labels, b, u, maxU, A) : blank;
    const St* row = acts + tdt_cell(b, t, u, maxT, maxU) * A;
    const C xb = load1<Tag>(row + blank);
    const C xl = load1<Tag>(row + lab);
    const C logZ = row_lse<Tag, G>(row, A, gl).log();
    if (gl != 0) return;
    // the blank edge (t, u) -> (t + 1, u) stays inside the band (or enters the terminal node) iff L_b - u < T_b - t
    rec[0] = Lb - u < T - t ? (xb - logZ) * C(kLog2e) : neg_inf<C>();
    rec[1] = has_lab ? (xl - logZ) * C(kLog2e) : neg_inf<C>();
    rec[2] = logZ;
    if (non_finite(logZ)) poison[b] = 1;                                          // (several bad rows race: any store will do)
}

// ------------------------------------------------------------------------------------------
// Stage 2.  Both forms: grid = (N slice, 2), blockIdx.y = 0 alpha, 1 beta.
//   alpha(0, 0) = 0;  alpha(t + 1, u) = lse(alpha(t, u) + lp_blank(t, u), alpha(t, u - 1) + lp_label(t, u - 1))
//   beta(T_b, L_b) = 0;  beta(t, u) = lse(lp_blank(t, u) + beta(t + 1, u), lp_label(t, u) + beta(t + 1, u + 1))
// alpha(t, .) and beta(t, .) are stored for 0 <= t < T_b, u <= L_b, relative to offa[t] / offb[t]; offb[T_b] = 0 is the
// terminal row's.  The forward side closes the sample: log P = alpha(T_b, L_b), one more step of the recurrence (ll, base
// 2, absolute) and the cost -- the invalid-lengths marker, NaN for a poisoned sample, +inf when no path exists.
template <typename L>
__device__ __forceinline__ void mono_close(double lp, int b, const int* __restrict__ poison, double* __restrict__ ll,
                                           L* __restrict__ costs) {
    ll[b] = lp;
    costs[b] = (poison[b] != 0 || lp != lp) ? static_cast<L>(__builtin_nan("")) : static_cast<L>(-lp * kLn2);
}

// The value of the lane below (DOWN: lane u receives lane u - 1's) or above; the lane without a neighbour receives -inf.
template <bool DOWN> __device__ __forceinline__ int mono_shift32(int old, int v) {
    return DOWN ? __builtin_amdgcn_update_dpp(old, v, 0x138, 0xf, 0xf, false)      // wave_shr:1
                : __builtin_amdgcn_update_dpp(old, v, 0x130, 0xf, 0xf, false);     // wave_shl:1
}
template <bool DOWN> __device__ __forceinline__ float mono_shift(float v) {
    return __int_as_float(mono_shift32<DOWN>(__float_as_int(neg_inf<float>()), __float_as_int(v)));
}
template <bool DOWN> __device__ __forceinline__ double mono_shift(double v) {
    const double ninf = neg_inf<double>();
    return __hiloint2double(mono_shift32<DOWN>(__double2hiint(ninf), __double2hiint(v)),
                            mono_shift32<DOWN>(__double2loint(ninf), __double2loint(v)));
}

template <typename L> struct MonoPair { using type = float2; };
template <> struct MonoPair<double> { using type = double2; };

// Wave form: block = 64 = one wavefront, lane u.  Step s = 0 .. T_b - 1 works on frame t = s (alpha) or T_b - 1 - s (beta).
// The rows of edge weights of chunk j + 1 are requested before chunk j's steps (they do not depend on the recurrence); a
// chunk's kMonoChunk results are stored behind its steps.  At a chunk's end the wave re-centres on its maximum and adds the
// shift to the fp64 offset, so values stay O(10) within a chunk's drift however long T_b is.
template <typename L, bool FWD>
__device__ __forceinline__ void mono_wave_sweep(const L* __restrict__ tab, L* __restrict__ val, double* __restrict__ off,
                                                int b, int T, int Lb, int maxT, int maxU, int u, double& base, L& a) {
    using P = typename MonoPair<L>::type;
    constexpr int CH = kMonoChunk;
    const bool in = u <= Lb;                                         // (lanes past L_b hold -inf and touch no memory)
    const int uc = in ? u : Lb;
    const P none = {neg_inf<L>(), neg_inf<L>()};
    const auto frame = [&](int s) { return FWD ? s : T - 1 - s; };
    const auto request = [&](int s0, P (&w)[CH]) {
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int s = s0 + k < T ? s0 + k : T - 1;               // (the tail re-reads the last row: no branch on the load)
            w[k] = *reinterpret_cast<const P*>(tab + tdt_cell(b, frame(s), uc, maxT, maxU) * kMonoRec);
        }
    };
    P cur[CH], nxt[CH];
    request(0, cur);
    for (int s0 = 0; s0 < T; s0 += CH) {
        request(s0 + CH, nxt);                                       // (unconditional -- past the end it re-reads the last row:
                                                                     //  behind a branch the compiler waits for vmcnt(0) at the join)
        L out[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const P w = in ? cur[k] : none;
            if (FWD) {
                out[k] = a;                                          // alpha(t, u)
                if (s0 + k < T) a = mono_lse2<L>(a + w.x, mono_shift<true>(a + w.y));
            } else {
                if (s0 + k < T) a = mono_lse2<L>(a + w.x, mono_shift<false>(a) + w.y);
                out[k] = a;                                          // beta(t, u)
            }
        }
#pragma unroll
        for (int k = 0; k < CH; ++k)
            if (in && s0 + k < T) val[tdt_cell(b, frame(s0 + k), u, maxT, maxU)] = out[k];
        if (u < CH && s0 + u < T) off[frame(s0 + u)] = base;         // the chunk's frames share one offset
        if (s0 + CH < T) {
            L M = a;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) M = vmax(M, __shfl_xor(M, o, kWave));
            if (M - M == L(0)) { a -= M; base += static_cast<double>(M); }     // (no finite value: the offset stays)
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) cur[k] = nxt[k];
    }
}

template <typename L>
__global__ __launch_bounds__(64) void mono_lattice_wave_kernel(
        const L* __restrict__ tab, L* __restrict__ alpha, L* __restrict__ beta, double* __restrict__ offa,
        double* __restrict__ offb, double* __restrict__ ll, const int* __restrict__ xlen, const int* __restrict__ ylen,
        const int* __restrict__ poison, L* __restrict__ costs, int maxT, int maxU, int b0) {
    const int b = b0 + blockIdx.x, u = threadIdx.x;
    const bool fwd = blockIdx.y == 0;
    int T, Lb;
    if (!tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb)) {
        if (fwd && u == 0) costs[b] = cost_invalid<L>();
        return;
    }
    const size_t o0 = static_cast<size_t>(b) * mono_offsets(maxT);
    double base = 0.0;
    if (fwd) {
        L a = u == 0 ? L(0) : neg_inf<L>();
        mono_wave_sweep<L, true>(tab, alpha, offa + o0, b, T, Lb, maxT, maxU, u, base, a);
        if (u == Lb) mono_close<L>(a == neg_inf<L>() ? static_cast<double>(a) : base + static_cast<double>(a), b, poison, ll, costs);
    } else {
        L a = u == Lb ? L(0) : neg_inf<L>();
        if (u == 0) offb[o0 + T] = 0.0;
        mono_wave_sweep<L, false>(tab, beta, offb + o0, b, T, Lb, maxT, maxU, u, base, a);
    }
}

// Block form: block = any multiple of 64 up to 1024.  Per frame every thread takes cells of it, then the block's maximum
// sets the next frame's offset; the partial maxima are double-buffered, so ONE barrier per frame orders both them and the
// frame's values (written to the global arrays, read back by other threads of the block in the next frame).
template <typename L>
__global__ __launch_bounds__(1024) void mono_lattice_block_kernel(
        const L* __restrict__ tab, L* __restrict__ alpha, L* __restrict__ beta, double* __restrict__ offa,
        double* __restrict__ offb, double* __restrict__ ll, const int* __restrict__ xlen, const int* __restrict__ ylen,
        const int* __restrict__ poison, L* __restrict__ costs, int maxT, int maxU, int b0) {
    __shared__ L wmax[2][16];
    const int b = b0 + blockIdx.x;
    const bool fwd = blockIdx.y == 0;
    int T, Lb;
    if (!tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb)) {
        if (fwd && threadIdx.x == 0) costs[b] = cost_invalid<L>();
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    double* off = (fwd ? offa : offb) + static_cast<size_t>(b) * mono_offsets(maxT);
    L* val = fwd ? alpha : beta;
    if (!fwd && tid == 0) off[T] = 0.0;
    double base = 0.0;                                               // off[t] of the frame being computed
    L rel = L(0);                                                    // off[previous frame of the sweep] - base
    for (int k = 0; k < T; ++k) {
        const int t = fwd ? k : T - 1 - k;
        if (tid == 0) off[t] = base;
        L tmax = neg_inf<L>();
        for (int u = tid; u <= Lb; u += blockDim.x) {
            const size_t c = tdt_cell(b, t, u, maxT, maxU);
            L v;
            if (fwd) {
                if (k == 0) {
                    v = u == 0 ? L(0) : neg_inf<L>();
                } else {                                             // blank (t - 1, u), label (t - 1, u - 1) -> (t, u)
                    const size_t p = c - maxU;
                    const L x = val[p] + rel + tab[p * kMonoRec];
                    const L y = u >= 1 ? val[p - 1] + rel + tab[(p - 1) * kMonoRec + 1] : neg_inf<L>();
                    v = mono_lse2<L>(x, y);
                }
            } else {
                L bu, bu1;                                           // beta(t + 1, u), beta(t + 1, u + 1)
                if (k == 0) {
                    bu = u == Lb ? L(0) : neg_inf<L>();
                    bu1 = u + 1 == Lb ? L(0) : neg_inf<L>();
                } else {
                    bu = val[c + maxU] + rel;
                    bu1 = u < Lb ? val[c + maxU + 1] + rel : neg_inf<L>();
                }
                v = mono_lse2<L>(tab[c * kMonoRec] + bu, tab[c * kMonoRec + 1] + bu1);
            }
            val[c] = v;
            tmax = vmax(tmax, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tmax = vmax(tmax, __shfl_xor(tmax, o, kWave));
        if (lane == 0) wmax[k & 1][wave] = tmax;
        __syncthreads();                                             // the frame's values and its partial maxima
        L M = wmax[k & 1][0];
        for (int w = 1; w < nw; ++w) M = vmax(M, wmax[k & 1][w]);
        const double prev = base;
        if (M - M == L(0)) base += static_cast<double>(M);           // (a frame without a finite value keeps the offset)
        rel = static_cast<L>(prev - base);
    }
    if (!fwd || tid != 0) return;
    // log P = alpha(T_b, L_b): the blank out of (T_b - 1, L_b) and the label out of (T_b - 1, L_b - 1), behind the last barrier
    const size_t c = tdt_cell(b, T - 1, Lb, maxT, maxU);
    const L x = val[c] + tab[c * kMonoRec];
    const L y = Lb >= 1 ? val[c - 1] + tab[(c - 1) * kMonoRec + 1] : neg_inf<L>();
    const L v = mono_lse2<L>(x, y);
    mono_close<L>(v == neg_inf<L>() ? static_cast<double>(v) : off[T - 1] + static_cast<double>(v), b, poison, ll, costs);
}

// ------------------------------------------------------------------------------------------
// Stage 3.  A thread per row: grid = (ceil(maxT * maxU / 256), N slice), block = 256.
//   cb = 2^(alpha(t, u) + lp_blank + beta(t + 1, u) - log P),   cl = the same with lp_label and beta(t + 1, u + 1),
// the fp64 offsets summed first; beta(T_b, .) is the terminal row, 0 at L_b and no edge elsewhere.  Padding rows, rows
// outside the band and every row of a sample whose lengths do not fit get kPadded (the gradient stream zero-fills them
// without reading their logits); a poisoned sample or one without a path gets NaN records on every in-lattice row.
template <typename L>
__global__ __launch_bounds__(256) void mono_coef_kernel(
        L* tab, const L* __restrict__ alpha, const L* __restrict__ beta, const double* __restrict__ offa,
        const double* __restrict__ offb, const double* __restrict__ ll, const int* __restrict__ xlen,
        const int* __restrict__ ylen, const int* __restrict__ labels, const int* __restrict__ poison, int maxT, int maxU,
        int A, int b0) {
    const int b = b0 + blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= maxT * maxU) return;
    const int t = q / maxU, u = q - t * maxU;
    const size_t c = tdt_cell(b, t, u, maxT, maxU);
    L* r = tab + c * kMonoRec;
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
    if (!mono_live(t, u, T, Lb)) {
        r[3] = static_cast<L>(kPadded);
        return;
    }
    const size_t o0 = static_cast<size_t>(b) * mono_offsets(maxT);
    const L o = static_cast<L>(offa[o0 + t] + offb[o0 + t + 1] - lp);
    const L a = alpha[c] + o;
    const L lb = r[0], ltok = r[1], lz = r[2];
    L bu, bu1 = neg_inf<L>();
    if (t + 1 < T) {
        bu = beta[c + maxU];
        if (u < Lb) bu1 = beta[c + maxU + 1];
    } else {
        bu = u == Lb ? L(0) : neg_inf<L>();
        if (u + 1 == Lb) bu1 = L(0);
    }
    const L cb = fast_exp2(a + lb + bu);
    const L cl = u < Lb ? fast_exp2(a + ltok + bu1) : L(0);
    r[0] = acc_log(cb + cl) - lz;
    r[1] = cb;
    r[2] = cl;
    r[3] = static_cast<L>(lab);
}

}  // namespace rnnt
