// rnnt_hat_kernels.h -- the gfx950 kernels of the Hybrid Autoregressive Transducer loss (include/rnnt_hat.h).
//
// HAT factorises blank out of the softmax: b = sigmoid(z_blank), labels by a softmax over the A - 1 other columns.  The
// lattice between the row statistics and the gradient is the plain RNN-T lattice, so stages 2 and 3 are rnnt_kernels.h's,
// instantiated in this library under rnnt_host.h's selection rules:
//   1 hat_stats_kernel       every in-lattice row read once as the aligned 16-byte packets that cover it; online
//                            (max, sum exp) with the blank lane masked out of the packet that holds it, the blank logit
//                            taken from that packet -> lp2 = {log2 b, log2 (1 - b) + log2 q_label} and logz = logZ over
//                            the labels, in the skewed layout of the lattice kernels                       [one read]
//   2 lattice_kernel / lattice_lin_kernel                                                          (rnnt_kernels.h)
//   3 coef_kernel / coef_cell_kernel: the record {ln c - logZ_labels, cb, cl, label}, c = cb + cl       (rnnt_kernels.h)
//   4 hat_grad_kernel        the flat non-temporal 16-byte stream over (N, maxT, maxU, A): record first, padding rows
//                            zeroed without their logits being read.  Per row r = cl / c; label column k:
//                            r exp(z_k + ln c - logZ_labels) - cl [k == label] = cl q_k - cl [k == label]; blank column:
//                            c sigmoid(z_blank) - cb, the sigmoid of the logit the packet holds (so the record needs no
//                            fifth word, and stage 3 is the main library's, unchanged)          [one read, one write]
//     hat_grad_elem_kernel   the same element by element, for tensors off 16-byte boundaries
#pragma once

#include "rnnt_row_lse.h"              // row_lse, row_label; through it rnnt_kernels.h

namespace rnnt {

__device__ __forceinline__ float hat_exp(float x) { return expf(x); }
__device__ __forceinline__ double hat_exp(double x) { return exp(x); }
__device__ __forceinline__ float hat_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double hat_log1p(double x) { return log1p(x); }
__device__ __forceinline__ float hat_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double hat_abs(double x) { return fabs(x); }
// softplus(x) = log(1 + exp(x)) in the stable form: log sigmoid(z) = -softplus(-z), log(1 - sigmoid(z)) = -softplus(z)
template <typename C> __device__ __forceinline__ C hat_softplus(C x) {
    return vmax(x, C(0)) + hat_log1p(hat_exp(-hat_abs(x)));
}
// sigmoid with exact limits at +-inf (exp(-z) = 0 or inf)
template <typename C> __device__ __forceinline__ C hat_sigmoid(C z) { return C(1) / (C(1) + hat_exp(-z)); }

// ------------------------------------------------------------------------------------------
// Stage 1.  G lanes per row (G = 4, 16, 64), 256 / G rows per block; grid = (ceil(maxT * maxU * G / 256), N slice).
// The row reduction is row_lse (rnnt_row_lse.h) with its per-element hook: the blank column is masked out of the sum and
// its value kept by the lane that met it; the group reads it from lane (blank's packet) mod G.  The label logit is one
// scalar load issued in front of the packets.
// A NaN blank logit, and a label equal to blank (HAT has no probability for it), make the stored logZ NaN: the lattice
// kernel's poison check (rnnt_kernels.h, note_non_finite) then gives the sample a NaN cost and NaN gradients.
template <typename Tag, int G>
__global__ __launch_bounds__(256) void hat_stats_kernel(
        const typename Tag::store* __restrict__ acts, const int* __restrict__ labels, const int* __restrict__ xlen,
        const int* __restrict__ ylen, LogPair<typename Tag::comp>* __restrict__ lp2, typename Tag::comp* __restrict__ logz,
        int maxT, int maxU, int Up, int A, int blank, int b0, int* __restrict__ poison) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    constexpr int V = Vec<Tag>::N;
    const int b = b0 + blockIdx.y;
    const int gl = threadIdx.x & (G - 1);
    const int q = blockIdx.x * (256 / G) + static_cast<int>(threadIdx.x) / G;     // row inside the sample
    if (q >= maxT * maxU) return;                                                 // (whole groups leave together)
    const int Tb = clamp_len(xlen[b], maxT), Ub = clamp_len(ylen[b] + 1, maxU);
    if (Tb <= 0 || Ub <= 0) return;                                               // (the lattice marks the cost)
    const int t = q / maxU, u = q - t * maxU;
    if (t >= Tb || u >= Ub) return;                                               // padding: never read
    const bool has_lab = u < Ub - 1;
    const int lab = has_lab ? row_label(labels, b, u, maxU, A) : blank;
    const St* row = acts + (static_cast<size_t>(b) * maxT * maxU + q) * A;
    const C xl = load1<Tag>(row + lab);
    __builtin_assume(static_cast<unsigned>(blank) < static_cast<unsigned>(A));    // (make_plan refuses any other: no range test on the hook)
    C zb = 0;                                                                     // kept by the lane whose packet holds the blank
    const RowLse<C> z = row_lse<Tag, G>(row, A, gl, [&](int col, C x) {
        if (col == blank) zb = x;
        return col == blank;
    });
    const int skip = static_cast<int>((reinterpret_cast<uintptr_t>(row) & 15u) / sizeof(St));
    zb = __shfl(zb, ((skip + blank) / V) & (G - 1), G);                           // the blank's packet in the row's packet stream
    if (gl != 0) return;
    C logZ = z.log();                                                             // over the labels only
    if (zb != zb || (has_lab && lab == blank)) logZ = zb + (neg_inf<C>() - neg_inf<C>());   // NaN: poisons the sample
    LogPair<C> rec;                                                               // lattice log-probs are kept in base 2
    rec.x = vmax(-hat_softplus(-zb) * C(kLog2e), log_zero<C>());
    rec.y = has_lab ? vmax((xl - logZ - hat_softplus(zb)) * C(kLog2e), log_zero<C>()) : log_zero<C>();
    lp2[lat_pair_index(b, t + u, u, maxT, maxU, Up)] = rec;
    logz[lat_index(b, t + u, u, maxT, maxU, Up)] = logZ;
    note_non_finite(poison, b, t + u, u, Up, logZ);
}

// ------------------------------------------------------------------------------------------
// Stage 4: one element at column `pos` of a row with record `rec` = {ln c - logZ_labels, cb, cl, label}; z its logit.
template <typename C>
__device__ __forceinline__ C hat_elem(const Cell<C>& rec, int pos, C z, int blank, C gs) {
    const int lab = static_cast<int>(rec.w);
    if (lab == kPadded) return C(0);
    const C c = rec.y + rec.z;
    C g;
    if (pos == blank) {
        g = c * hat_sigmoid(z) - rec.y;
    } else {
        g = fast_exp(z + rec.x) * (c > C(0) ? rec.z / c : rec.z);                 // (c == 0: cl == 0 too; a NaN record stays NaN)
        if (pos == lab) g -= rec.z;
    }
    return g * gs;
}

// Flat form: the tensor as one array of 16-byte packets; a block owns PPT * 256 consecutive packets per iteration and
// grid-strides (grad_flat_kernel's scheme).  Row of the chunk start carried incrementally in 64 bits, row of a packet by a
// 32-bit reciprocal division inside the chunk.  The record is asked for first; with padding in the batch (padflag, left by
// the coefficient kernel) and rows of 128 bytes or more a packet inside a padding row is zero-filled without its logits
// being read.  The per-sample scale is one block-uniform value when the chunk lies inside one sample.  Non-temporal loads
// and stores; a thread reads an element and writes the same element, so gradients == activations is legal.
// Requires acts and grads on 16-byte boundaries and N * maxT * maxU < 2^32 rows (run_hat).
template <typename Tag>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sizeof(typename Tag::comp) == 8 ? 1 : 8))) void hat_grad_kernel(
        const typename Tag::store* acts, typename Tag::store* grads,           // NOT __restrict__: gradients == activations
        const Cell<typename Tag::comp>* __restrict__ rowtab, const typename Tag::comp* __restrict__ grad_scale,
        unsigned long long E, unsigned R, int A, int blank, unsigned TU, float invA, unsigned long long dq, int drem,
        const int* __restrict__ padflag) {
    using C = typename Tag::comp;
    constexpr int V = Vec<Tag>::N;
    constexpr int PPT = 2;
    constexpr int CH = PPT * 256 * V;                                  // elements per chunk
    const bool ps = padflag[0] != 0 && A * static_cast<int>(sizeof(typename Tag::store)) >= 128;
    const unsigned long long npk = E / V;
    const unsigned long long nchunks = (npk + PPT * 256 - 1) / (PPT * 256);
    const u32x4* in = reinterpret_cast<const u32x4*>(acts);
    u32x4* out = reinterpret_cast<u32x4*>(grads);
    unsigned long long c = blockIdx.x;
    unsigned long long r = (c * CH) / static_cast<unsigned>(A);
    int rem = static_cast<int>((c * CH) - r * static_cast<unsigned>(A));
    for (; c < nchunks; c += gridDim.x) {
        const unsigned long long pk0 = c * (PPT * 256);
        // the chunk's scale: block-uniform when all its rows belong to one sample (nearly always), else per packet
        C chunk_scale = C(1);
        bool uni = true;
        if (grad_scale != nullptr) {
            const unsigned long long rl0 = r + static_cast<unsigned>(CH / A + 1);
            const unsigned rl = rl0 < R ? static_cast<unsigned>(rl0) : R - 1;   // last row the chunk can touch
            const unsigned s0 = static_cast<unsigned>(r) / TU;
            uni = s0 == rl / TU;
            chunk_scale = grad_scale[s0];
        }
        auto scale_of = [&](unsigned row) -> C {
            if (grad_scale == nullptr || uni) return chunk_scale;
            return grad_scale[(row < R ? row : R - 1) / TU];
        };
        uint4 raw[PPT];
        Cell<C> rec[PPT], rec2[PPT];                                   // rec2: the next row's record, for packets that straddle
        int v0[PPT];
        unsigned row[PPT];
        bool live[PPT];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int p = k * 256 + threadIdx.x;
            live[k] = pk0 + p < npk;
            const unsigned idx = static_cast<unsigned>(rem) + static_cast<unsigned>(p) * V;
            unsigned q = static_cast<unsigned>(static_cast<float>(idx) * invA);
            int rr = static_cast<int>(idx - q * static_cast<unsigned>(A));
            if (rr < 0) { rr += A; --q; } else if (rr >= A) { rr -= A; ++q; }
            v0[k] = rr;
            row[k] = static_cast<unsigned>(r + q);                     // (< 2^32 rows: run_hat)
            if (live[k]) {
                rec[k] = rowtab[row[k]];
                if (!ps) raw[k] = load_packet<true>(in + pk0 + p);
                if (rr + V > A) rec2[k] = rowtab[row[k] + 1 < R ? row[k] + 1 : R - 1];
            }
        }
        if (ps) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const int p = k * 256 + threadIdx.x;
                const bool skip = (v0[k] + V <= A) && static_cast<int>(rec[k].w) == kPadded;
                raw[k] = make_uint4(0, 0, 0, 0);
                if (live[k] && !skip) raw[k] = load_packet<true>(in + pk0 + p);
            }
        }
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            if (!live[k]) continue;
            const int p = k * 256 + threadIdx.x;
            C v[V];
            unpack<Tag>(raw[k], v);
            if (v0[k] + V <= A) {
                // whole packet inside one row (the common case)
                const int lab = static_cast<int>(rec[k].w);
                if (lab == kPadded) {
#pragma unroll
                    for (int j = 0; j < V; ++j) v[j] = 0;
                } else {
                    const C cb = rec[k].y, cl = rec[k].z, cc = rec[k].x, cs = cb + cl;
                    const C ratio = cs > C(0) ? cl / cs : cl;
                    C zb = 0;
                    const bool special = static_cast<unsigned>(blank - v0[k]) < static_cast<unsigned>(V) ||
                                         static_cast<unsigned>(lab - v0[k]) < static_cast<unsigned>(V);
                    if (special) {
#pragma unroll
                        for (int j = 0; j < V; ++j)
                            if (v0[k] + j == blank) zb = v[j];
                    }
#pragma unroll
                    for (int j = 0; j < V; ++j) v[j] = fast_exp(v[j] + cc) * ratio;
                    if (special) {
#pragma unroll
                        for (int j = 0; j < V; ++j) {
                            if (v0[k] + j == lab) v[j] -= cl;
                            if (v0[k] + j == blank) v[j] = cs * hat_sigmoid(zb) - cb;
                        }
                    }
                    if (grad_scale != nullptr) {
                        const C gs = scale_of(row[k]);
#pragma unroll
                        for (int j = 0; j < V; ++j) v[j] *= gs;
                    }
                }
            } else if (A >= V) {
                // two rows at most: elements j < split belong to row[k], the rest to the next row
                const int split = A - v0[k];
                const C gs1 = scale_of(row[k]), gs2 = scale_of(row[k] + 1);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const bool first = j < split;
                    v[j] = hat_elem<C>(first ? rec[k] : rec2[k], first ? v0[k] + j : j - split, v[j], blank, first ? gs1 : gs2);
                }
            } else {
                unsigned rw = row[k];
                int pos = v0[k];
                Cell<C> cur = rec[k];
                C gs = scale_of(rw);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    while (pos >= A) {
                        pos -= A;
                        ++rw;
                        if (rw < R) cur = rowtab[rw];
                        gs = scale_of(rw);
                    }
                    v[j] = hat_elem<C>(cur, pos, v[j], blank, gs);
                    ++pos;
                }
            }
            store_packet<true>(out + pk0 + p, pack<Tag>(v));
        }
        r += dq;
        rem += drem;
        if (rem >= A) { rem -= A; ++r; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)                            // the E % V elements behind the last whole packet
        for (unsigned long long e = npk * V; e < E; ++e) {
            const unsigned rw = static_cast<unsigned>(e / static_cast<unsigned>(A));
            const C gs = grad_scale != nullptr ? grad_scale[rw / TU] : C(1);
            store1<Tag>(grads + e, hat_elem<C>(rowtab[rw], static_cast<int>(e - static_cast<unsigned long long>(rw) * A),
                                               load1<Tag>(acts + e), blank, gs));
        }
}

// Element-wise form (tensors not on 16-byte boundaries).  grid-stride, block = 256.  The record's label word is looked at
// before the logit is read: padding rows are never read here either.
template <typename Tag>
__global__ __launch_bounds__(256) void hat_grad_elem_kernel(
        const typename Tag::store* acts, typename Tag::store* grads, const Cell<typename Tag::comp>* __restrict__ rowtab,
        const typename Tag::comp* __restrict__ grad_scale, unsigned long long E, int A, int blank, unsigned TU) {
    using C = typename Tag::comp;
    for (unsigned long long e = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x; e < E;
         e += static_cast<unsigned long long>(gridDim.x) * 256) {
        const unsigned rw = static_cast<unsigned>(e / static_cast<unsigned>(A));
        const Cell<C> rec = rowtab[rw];
        C g = C(0);
        if (static_cast<int>(rec.w) != kPadded)
            g = hat_elem<C>(rec, static_cast<int>(e - static_cast<unsigned long long>(rw) * A), load1<Tag>(acts + e), blank,
                            grad_scale != nullptr ? grad_scale[rw / TU] : C(1));
        store1<Tag>(grads + e, g);
    }
}

}  // namespace rnnt
