// rnnt_pruned_kernels.h -- the gfx950 kernels of the pruned RNN-T loss and of the prune ranges (include/rnnt_pruned.h).
//
// The pruned loss reads logits of shape (N, maxT, S, A): row (b, t, k) is the joint output of lattice state
// u = s_t + k, s_t = ranges[b, t].  It runs the four stages of the materialised path, two of them unchanged:
//   0 pruned_prep_kernel         per frame the window {s, rows inside the lattice} (`win`), the log-zero sentinel into every
//                                in-lattice cell OUTSIDE its frame's window (no edges: the unchanged lattice reads no
//                                uninitialised word), the per-sample "bad start" flag                          [O(T U)]
//   1 pruned_stats_kernel        online max / sum-exp of every in-window row, gather of the blank and label logits,
//                                lp2 / log Z into the skewed layout at cell (t, s_t + k); G lanes per row (G = 64: a
//                                wavefront per row; 16 / 4 for short rows)                     [HBM-bound, one read]
//   2 lattice_kernel / lattice_lin_kernel (rnnt_kernels.h, unchanged) + pruned_fix_kernel (bad starts: the cost marker)
//   3 coef_cell_kernel / coef_kernel (rnnt_kernels.h, unchanged): the natural-order record table over ALL maxT x maxU cells
//   4 pruned_grad_kernel         one flat read+write stream of 16-byte packets over (N, maxT, S, A), the record of a row
//                                taken at (b, t, s_t + k); rows outside the lattice written as zeros without being read
//     pruned_grad_elem_kernel    the same element by element, for tensors not on 16-byte boundaries
// The prune ranges run behind the additive joint's partition stage and the two-direction lattice:
//   pruned_window_kernel         a wavefront per (b, t): the occupancy gamma(t, u) = exp(alpha + beta - log P) of the row,
//                                the smallest start of a best window of S states
//   pruned_ranges_kernel         per sample the clamp to reachable windows, the monotone pass and the overlap pass
#pragma once

#include "rnnt_row_lse.h"              // row_lse, row_label; through it rnnt_kernels.h

namespace rnnt {

// Per frame of the pruned loss: x = window start s_t (clamped into [0, L_b] for addressing), y = rows of the frame inside the
// lattice (k < y <=> t < T_b and s_t + k <= L_b; 0 for a sample with bad lengths or a bad start).
// Lives behind the lattice layout in the workspace (pruned_layout): the record table never overlays it.

// ------------------------------------------------------------------------------------------
// Stage 0.  grid = (ceil(maxT / 32), N slice), block = 256: frames [32 x, 32 x + 32) of sample b.
template <typename L>
static __global__ __launch_bounds__(256) void pruned_prep_kernel(
        const int* __restrict__ ranges, const int* __restrict__ xlen, const int* __restrict__ ylen,
        LogPair<L>* __restrict__ lp2, L* __restrict__ logz, int2* __restrict__ win, int* __restrict__ bad,
        int maxT, int maxU, int Up, int S, int b0) {
    const int b = b0 + blockIdx.y;
    const int T = xlen[b], Lb = ylen[b];
    const bool lens_ok = T >= 1 && T <= maxT && Lb >= 0 && Lb + 1 <= maxU;
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
    const int t0 = blockIdx.x * 32;
    if (threadIdx.x < 32 && t0 + static_cast<int>(threadIdx.x) < maxT) {
        const int t = t0 + threadIdx.x;
        int s = 0, n = 0;
        if (live && t < T) {
            s = ranges[static_cast<size_t>(b) * maxT + t];
            n = Lb - s + 1 < S ? Lb - s + 1 : S;
        }
        win[static_cast<size_t>(b) * maxT + t] = make_int2(s, n);
    }
    if (!lens_ok) return;                     // (the lattice marks the cost; every record is padding)
    const int Ub = Lb + 1;
    const int t1 = t0 + 32 < T ? t0 + 32 : T;
    LogPair<L> zero;
    zero.x = log_zero<L>(); zero.y = log_zero<L>();
    for (int i = threadIdx.x; i < (t1 - t0) * Ub; i += 256) {
        const int t = t0 + i / Ub, u = i - (i / Ub) * Ub;
        int s = -1;
        if (!sample_bad) s = ranges[static_cast<size_t>(b) * maxT + t];
        if (s >= 0 && u >= s && u < s + S) continue;          // inside the window: the statistics kernel writes it
        lp2[lat_pair_index(b, t + u, u, maxT, maxU, Up)] = zero;
        logz[lat_index(b, t + u, u, maxT, maxU, Up)] = L(0);  // finite: a stale poison hint on this cell is no poison
    }
}

// ------------------------------------------------------------------------------------------
// Stage 1.  G lanes per row (G = 4, 16, 64), 256 / G rows per block.  grid = (ceil(maxT * S * G / 256), N slice).
// The row reduction is row_lse (rnnt_row_lse.h).
template <typename Tag, int G>
__global__ __launch_bounds__(256) void pruned_stats_kernel(
        const typename Tag::store* __restrict__ acts, const int2* __restrict__ win, const int* __restrict__ labels,
        const int* __restrict__ ylen, LogPair<typename Tag::comp>* __restrict__ lp2, typename Tag::comp* __restrict__ logz,
        int maxT, int maxU, int Up, int S, int A, int blank, int b0, int* __restrict__ poison) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const int b = b0 + blockIdx.y;
    const int gl = threadIdx.x & (G - 1);
    const int q = blockIdx.x * (256 / G) + static_cast<int>(threadIdx.x) / G;     // row inside the sample
    if (q >= maxT * S) return;                                                    // (whole groups leave together)
    const int t = q / S, k = q - t * S;
    const int2 w = win[static_cast<size_t>(b) * maxT + t];
    if (k >= w.y) return;                                                         // padding: never read
    const int u = w.x + k;
    const bool has_lab = u < ylen[b];
    const int lab = has_lab ? row_label(labels, b, u, maxU, A) : blank;
    const St* row = acts + (static_cast<size_t>(b) * maxT * S + q) * A;
    const C xb = load1<Tag>(row + blank);
    const C xl = load1<Tag>(row + lab);
    const C logZ = row_lse<Tag, G>(row, A, gl).log();
    if (gl == 0) {
        LogPair<C> rec;                                                           // base-2 log-probs, as the lattice keeps them
        rec.x = vmax((xb - logZ) * C(kLog2e), log_zero<C>());
        rec.y = has_lab ? vmax((xl - logZ) * C(kLog2e), log_zero<C>()) : log_zero<C>();
        lp2[lat_pair_index(b, t + u, u, maxT, maxU, Up)] = rec;
        logz[lat_index(b, t + u, u, maxT, maxU, Up)] = logZ;
        note_non_finite(poison, b, t + u, u, Up, logZ);
    }
}

// ------------------------------------------------------------------------------------------
// Stage 2 epilogue: a sample with a start outside [0, L_b] gets the invalid-arguments cost marker (the synchronous callers
// turn it into RNNT_STATUS_INVALID_VALUE, as for lengths that do not fit the tensor).  grid = ceil(N / 256), block = 256.
template <typename L>
static __global__ __launch_bounds__(256) void pruned_fix_kernel(const int* __restrict__ bad, L* __restrict__ costs, int N) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < N && bad[b] != 0) costs[b] = cost_invalid<L>();
}

// ------------------------------------------------------------------------------------------
// Stage 4: the gradient of one element at position `pos` of pruned row `row` (slow path: packets that straddle rows, the
// tail, the element-wise kernel).  Rows outside the lattice (k >= win.y) are zero.
template <typename Tag>
__device__ __forceinline__ typename Tag::comp pruned_elem(
        const Cell<typename Tag::comp>* __restrict__ rowtab, const int2* __restrict__ win,
        const typename Tag::comp* __restrict__ grad_scale, unsigned long long row, int pos, const typename Tag::store* src,
        int S, int maxT, int maxU, int blank) {
    using C = typename Tag::comp;
    const unsigned long long bt = row / static_cast<unsigned>(S);
    const int k = static_cast<int>(row - bt * static_cast<unsigned>(S));
    const int2 w = win[bt];
    if (k >= w.y) return C(0);
    const Cell<C> rec = rowtab[bt * maxU + w.x + k];
    const int lab = static_cast<int>(rec.w);
    if (lab == kPadded) return C(0);
    C g = fast_exp(load1<Tag>(src) + rec.x);
    if (pos == blank) g -= rec.y;
    if (pos == lab) g -= rec.z;
    if (grad_scale != nullptr) g *= grad_scale[bt / static_cast<unsigned>(maxT)];
    return g;
}

// Flat form: the tensor as one array of 16-byte packets; a block owns PPT * 256 consecutive packets per iteration and
// grid-strides.  Row of the chunk start carried incrementally (64-bit), row of a packet by a 32-bit reciprocal division
// inside the chunk (as grad_flat_kernel).  A packet inside one row asks for its frame's window word first, then -- rows
// inside the lattice only -- for the record and the logits together.  Non-temporal loads and stores.
// Requires acts and grads on 16-byte boundaries and maxT * maxU * N < 2^32 cells (run_pruned).
template <typename Tag>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sizeof(typename Tag::comp) == 8 ? 1 : 8))) void pruned_grad_kernel(
        const typename Tag::store* acts, typename Tag::store* grads,           // NOT __restrict__: gradients == activations
        const Cell<typename Tag::comp>* __restrict__ rowtab, const int2* __restrict__ win,
        const typename Tag::comp* __restrict__ grad_scale, unsigned long long E, int A, int blank, int S, int maxT,
        int maxU, float invA, unsigned long long dq, int drem) {
    using C = typename Tag::comp;
    constexpr int V = Vec<Tag>::N;
    constexpr int PPT = 2;
    constexpr int CH = PPT * 256 * V;                                  // elements per chunk
    const unsigned long long npk = E / V;
    const unsigned long long nchunks = (npk + PPT * 256 - 1) / (PPT * 256);
    const u32x4* in = reinterpret_cast<const u32x4*>(acts);
    u32x4* out = reinterpret_cast<u32x4*>(grads);
    unsigned long long c = blockIdx.x;
    unsigned long long r = (c * CH) / static_cast<unsigned>(A);
    int rem = static_cast<int>((c * CH) - r * static_cast<unsigned>(A));
    for (; c < nchunks; c += gridDim.x) {
        const unsigned long long pk0 = c * (PPT * 256);
        uint4 raw[PPT];
        Cell<C> rec[PPT];
        int v0[PPT], kk[PPT];
        unsigned bt[PPT];
        int2 w[PPT];
        bool live[PPT];
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int p = j * 256 + threadIdx.x;
            live[j] = pk0 + p < npk;
            const unsigned idx = static_cast<unsigned>(rem) + static_cast<unsigned>(p) * V;
            unsigned q = static_cast<unsigned>(static_cast<float>(idx) * invA);
            int rr = static_cast<int>(idx - q * static_cast<unsigned>(A));
            if (rr < 0) { rr += A; --q; } else if (rr >= A) { rr -= A; ++q; }
            v0[j] = rr;
            const unsigned row = static_cast<unsigned>(r + q);          // (< 2^32 rows: run_pruned)
            bt[j] = row / static_cast<unsigned>(S);
            kk[j] = static_cast<int>(row - bt[j] * static_cast<unsigned>(S));
            w[j] = make_int2(0, 0);
            if (live[j]) w[j] = win[bt[j]];
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int p = j * 256 + threadIdx.x;
            const bool inside = v0[j] + V <= A;
            raw[j] = make_uint4(0, 0, 0, 0);
            rec[j].x = rec[j].y = rec[j].z = C(0);
            rec[j].w = static_cast<C>(kPadded);
            if (live[j] && (!inside || kk[j] < w[j].y)) {
                raw[j] = load_packet<true>(in + pk0 + p);
                if (inside) rec[j] = rowtab[static_cast<size_t>(bt[j]) * maxU + w[j].x + kk[j]];
            }
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            if (!live[j]) continue;
            const int p = j * 256 + threadIdx.x;
            C v[V];
            unpack<Tag>(raw[j], v);
            if (v0[j] + V <= A) {
                const int lab = static_cast<int>(rec[j].w);
                if (kk[j] >= w[j].y || lab == kPadded) {
#pragma unroll
                    for (int e = 0; e < V; ++e) v[e] = 0;
                } else {
                    const C cc = rec[j].x;
#pragma unroll
                    for (int e = 0; e < V; ++e) v[e] = fast_exp(v[e] + cc);
                    if (static_cast<unsigned>(blank - v0[j]) < static_cast<unsigned>(V) ||
                        static_cast<unsigned>(lab - v0[j]) < static_cast<unsigned>(V)) {
#pragma unroll
                        for (int e = 0; e < V; ++e) {
                            if (v0[j] + e == blank) v[e] -= rec[j].y;
                            if (v0[j] + e == lab) v[e] -= rec[j].z;
                        }
                    }
                    if (grad_scale != nullptr) {
                        const C gs = grad_scale[bt[j] / static_cast<unsigned>(maxT)];
#pragma unroll
                        for (int e = 0; e < V; ++e) v[e] *= gs;
                    }
                }
            } else {
                // a packet across a row boundary (A not a multiple of the packet, or A < packet): element by element
                const unsigned long long e0 = (pk0 + p) * V;
                unsigned long long rw = static_cast<unsigned long long>(bt[j]) * S + kk[j];
                int pos = v0[j];
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    while (pos >= A) { pos -= A; ++rw; }
                    const typename Tag::store* src = acts + e0 + e;
                    v[e] = pruned_elem<Tag>(rowtab, win, grad_scale, rw, pos, src, S, maxT, maxU, blank);
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
            const unsigned long long rw = e / static_cast<unsigned>(A);
            store1<Tag>(grads + e, pruned_elem<Tag>(rowtab, win, grad_scale, rw, static_cast<int>(e - rw * A), acts + e, S,
                                                    maxT, maxU, blank));
        }
}

// Element-wise form (tensors not on 16-byte boundaries, or whose 16-byte phases differ).  grid-stride, block = 256.
template <typename Tag>
__global__ __launch_bounds__(256) void pruned_grad_elem_kernel(
        const typename Tag::store* acts, typename Tag::store* grads,
        const Cell<typename Tag::comp>* __restrict__ rowtab, const int2* __restrict__ win,
        const typename Tag::comp* __restrict__ grad_scale, unsigned long long E, int A, int blank, int S, int maxT, int maxU) {
    for (unsigned long long e = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x; e < E;
         e += static_cast<unsigned long long>(gridDim.x) * 256) {
        const unsigned long long rw = e / static_cast<unsigned>(A);
        store1<Tag>(grads + e, pruned_elem<Tag>(rowtab, win, grad_scale, rw, static_cast<int>(e - rw * A), acts + e, S, maxT,
                                                maxU, blank));
    }
}

// ------------------------------------------------------------------------------------------
// Prune ranges, pass 1.  A wavefront per (b, t < T_b): gamma(t, u) = 2^(alpha + beta - log2 P) of the row (alpha / beta
// read as the coefficient kernels read them: base 2, with the per-chunk fp64 offsets) into LDS, then every lane sums the
// windows of its starts s in [0, smax] and the wavefront keeps the largest sum, the smallest s among equals.  The start goes
// to ranges[b, t]; pass 2 repairs it.  grid = (ceil(maxT / 4), N slice), block = 256, 4 * maxU doubles of LDS.
template <int UNUSED = 0>                 // (a template: only the translation units that launch it hold it)
static __global__ __launch_bounds__(256) void pruned_window_kernel(
        const float* __restrict__ alpha, const float* __restrict__ beta, const double* __restrict__ offa,
        const double* __restrict__ offb, const double* __restrict__ ll_fwd, const int* __restrict__ xlen,
        const int* __restrict__ ylen, int* __restrict__ ranges, int maxT, int maxU, int Up, int S, int lw, int lsh, int b0) {
    extern __shared__ double gam[];
    const int b = b0 + blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + wave;
    int T = xlen[b], Lb = ylen[b];
    if (T < 1 || T > maxT || Lb < 0 || Lb + 1 > maxU) { T = 0; Lb = 0; }   // lengths that do not fit the tensor: starts 0
    const bool active = t < T;                                         // (every wavefront reaches the barrier)
    const int Ub = Lb + 1;
    const size_t Dp = lat_rows(maxT, maxU);
    const double ll2 = ll_fwd[b];
    double* g = gam + wave * maxU;
    if (active)
        for (int u = lane; u < Ub; u += 64) {
            const int n = t + u;
            const size_t idx = lat_index(b, n, u, maxT, maxU, Up);
            const int wi = u >> lsh;
            const double oa = offa[(static_cast<size_t>(b) * lw + wi) * Dp + kLatPad + n];
            const double ob = offb[(static_cast<size_t>(b) * lw + wi) * Dp + kLatPad + n];
            const double e = static_cast<double>(alpha[idx]) + oa + static_cast<double>(beta[idx]) + ob - ll2;
            g[u] = exp2(e);
        }
    __syncthreads();
    if (t >= maxT) return;
    if (!active) {
        if (lane == 0) ranges[static_cast<size_t>(b) * maxT + t] = 0;
        return;
    }
    const int smax = Ub - S > 0 ? Ub - S : 0;
    double best = -1.0;
    int bs = 0;
    for (int s = lane; s <= smax; s += 64) {
        const int e = s + S < Ub ? s + S : Ub;
        double sum = 0.0;
        for (int u = s; u < e; ++u) sum += g[u];
        if (sum > best) { best = sum; bs = s; }                         // (NaN never wins: such a frame keeps s = 0)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off, kWave);
        const int os = __shfl_xor(bs, off, kWave);
        if (ob > best || (ob == best && os < bs)) { best = ob; bs = os; }
    }
    if (lane == 0) ranges[static_cast<size_t>(b) * maxT + t] = bs;
}

// Prune ranges, pass 2: per sample, serially over its frames -- clamp to the reachable windows, the monotone forward pass,
// the overlap backward pass; frames t >= T_b get 0.  A sample with L_b > T_b (S - 1) has no path through any windows:
// s_t = min(t (S - 1), smax).  grid = ceil(N / 64), block = 64 (a thread per sample).
template <int UNUSED = 0>
static __global__ __launch_bounds__(64) void pruned_ranges_kernel(const int* __restrict__ xlen, const int* __restrict__ ylen,
                                                                   int* __restrict__ ranges, int N, int maxT, int maxU, int S) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= N) return;
    int T = xlen[b], Lb = ylen[b];
    if (T < 1 || T > maxT || Lb < 0 || Lb + 1 > maxU) T = 0;
    int* s = ranges + static_cast<size_t>(b) * maxT;
    const int step = S - 1;
    const int smax = Lb + 1 - S > 0 ? Lb + 1 - S : 0;
    if (T > 0 && static_cast<long long>(Lb) > static_cast<long long>(T) * step) {
        for (int t = 0; t < T; ++t) {
            const long long v = static_cast<long long>(t) * step;
            s[t] = v < smax ? static_cast<int>(v) : smax;
        }
    } else if (T > 0) {
        int prev = 0;
        for (int t = 0; t < T; ++t) {                                   // steps 2 and 3
            const long long lo_l = static_cast<long long>(smax) - static_cast<long long>(T - 1 - t) * step;
            const long long hi_l = static_cast<long long>(t) * step;
            const int lo = lo_l > 0 ? static_cast<int>(lo_l) : 0;
            const int hi = hi_l < smax ? static_cast<int>(hi_l) : smax;
            int v = s[t];
            v = v < lo ? lo : (v > hi ? hi : v);
            if (t > 0 && v < prev) v = prev;
            s[t] = v;
            prev = v;
        }
        for (int t = T - 2; t >= 0; --t) {                              // step 4
            const int need = s[t + 1] - step;
            if (s[t] < need) s[t] = need;
        }
    }
    for (int t = T; t < maxT; ++t) s[t] = 0;                            // step 5
}

}  // namespace rnnt
