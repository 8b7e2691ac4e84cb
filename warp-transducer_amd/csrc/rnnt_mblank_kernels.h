// rnnt_mblank_kernels.h -- the gfx950 kernels of the multi-blank transducer loss (include/rnnt_mblank.h).
//
// Logits (N, maxT, maxU, A), one softmax per row; K big blanks, each a column of that softmax with a duration of its own.
// Four stages, the structure of rnnt_tdt_kernels.h:
//   1 mblank_stats_kernel      online max / sum-exp of every in-lattice row, gather of the blank, label and K big-blank
//                              logits; one cell record per row                                              [one read]
//   2 mblank_lattice_kernel    one block per (sample, direction): forward alpha and backward beta over anti-diagonals with
//                              K + 2 edge types.  A cell's predecessors lie up to dmax diagonals back (forward) or ahead
//                              (backward); they are read from the global arrays the same block wrote, behind one barrier
//                              per diagonal
//   3 mblank_coef_kernel       a thread per row: the posteriors of the row's out-edges -> the gradient record, written over
//                              the cell record of stage 1 (same stride, read before it is written)
//   4 mblank_grad_kernel       one flat read+write stream of 16-byte packets over (N, maxT, maxU, A); rows outside the
//                              lattice written as zeros without their logits being read
//     mblank_grad_elem_kernel  the same element by element, for tensors not on 16-byte boundaries
//
// Lattice values are base-2 logs.  The value stored for a cell on diagonal n is RELATIVE to an fp64 offset off[n] of that
// diagonal (offa / offb): off[n] is the largest absolute value on the previous diagonal of the sweep, so stored values stay
// within a few edge weights of zero and keep fp32's relative precision however long the utterance.
#pragma once

#include "rnnt_tdt_kernels.h"          // Lse2, tdt_log2, tdt_lens, tdt_cell: the lattice arithmetic is TDT's

namespace rnnt {

constexpr int kMbMaxBig = 8;            // K
constexpr int kMbMaxDuration = 64;      // largest big-blank duration
constexpr int kMbRing = 128;            // offsets kept in LDS by the lattice block (>= kMbMaxDuration + 2)
constexpr int kMbMaxU = 4096;

// The big blanks, by value in the kernel arguments (no device copy: a captured call needs none).  lo .. hi: the span of
// the standard blank's and the big blanks' columns -- the gradient stream's one range test per packet.
struct MbBlanks { int n; int blank; int lo; int hi; int col[kMbMaxBig]; int dur[kMbMaxBig]; };

// Per cell (b, t, u) of the workspace table, stride mblank_rec_stride(K) values of the lattice type:
//   after stage 1  [lp_blank, lp_label, logZ, lp_big_0 .. lp_big_{K-1}, -]      (lp: base 2, sigma included; logZ: natural log)
//   after stage 3  [x, cb, cl, label, gamma_big_0 .. gamma_big_{K-1}]           x = ln(c) - logZ, c = cb + cl + sum gamma_big
// label: the row's label index, -1 without a label edge (u = L_b), kPadded outside the lattice.
__host__ __device__ inline int mblank_rec_stride(int K) { return 4 + K; }

// ------------------------------------------------------------------------------------------
// Stage 1.  G lanes per row (G = 4, 16, 64), 256 / G rows per block.  grid = (ceil(maxT * maxU * G / 256), N slice).
// The row reduction is row_lse (rnnt_row_lse.h).  The blank, label and big-blank logits: scalar loads issued before it.
template <typename Tag, int G>
__global__ __launch_bounds__(256) void mblank_stats_kernel(
        const typename Tag::store* __restrict__ acts, const int* __restrict__ labels, const int* __restrict__ xlen,
        const int* __restrict__ ylen, typename Tag::comp* __restrict__ tab, int maxT, int maxU, int A, MbBlanks bb,
        typename Tag::comp sigma2, int b0, int* __restrict__ poison) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const int b = b0 + blockIdx.y;
    const int gl = threadIdx.x & (G - 1);
    const int q = blockIdx.x * (256 / G) + static_cast<int>(threadIdx.x) / G;     // row inside the sample
    if (q >= maxT * maxU) return;                                                 // (whole groups leave together)
    int T, Lb;
    if (!tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb)) return;                      // (the lattice marks the cost)
    const int t = q / maxU, u = q - t * maxU;
    if (t >= T || u > Lb) return;                                                 // padding: never read
    const int K = bb.n;
    const bool has_lab = u < Lb;
    const int lab = has_lab ? row_label(labels, b, u, maxU, A) : bb.blank;
    const St* row = acts + tdt_cell(b, t, u, maxT, maxU) * A;
    const C xb = load1<Tag>(row + bb.blank);
    const C xl = load1<Tag>(row + lab);
    C bz[kMbMaxBig];                                                              // (issued with the packets: one wait)
#pragma unroll
    for (int j = 0; j < kMbMaxBig; ++j) bz[j] = j < K ? load1<Tag>(row + bb.col[j]) : neg_inf<C>();
    const C logZ = row_lse<Tag, G>(row, A, gl).log();
    if (gl != 0) return;
    C* rec = tab + tdt_cell(b, t, u, maxT, maxU) * mblank_rec_stride(K);
    rec[0] = (xb - logZ) * C(kLog2e) - sigma2;
    rec[1] = has_lab ? (xl - logZ) * C(kLog2e) - sigma2 : neg_inf<C>();
    rec[2] = logZ;
#pragma unroll
    for (int j = 0; j < kMbMaxBig; ++j)
        if (j < K) rec[3 + j] = (bz[j] - logZ) * C(kLog2e) - sigma2;
    if (non_finite(logZ)) poison[b] = 1;                                          // (several bad rows race: any store will do)
}

// ------------------------------------------------------------------------------------------
// Stage 2.  grid = (N slice, 2): blockIdx.y = 0 alpha, 1 beta; block = any multiple of 64 up to 1024.  Per diagonal every
// thread takes cells of it, then the block's maximum sets the next diagonal's offset (one barrier per diagonal: the
// partial maxima are double-buffered).  The forward block closes the sample: log P (ll, base 2, absolute) and the cost --
// the invalid-lengths marker, NaN for a poisoned sample, +inf when no path reaches the terminal node.
template <typename L>
__global__ __launch_bounds__(1024) void mblank_lattice_kernel(
        const L* __restrict__ tab, L* __restrict__ alpha, L* __restrict__ beta, double* __restrict__ offa,
        double* __restrict__ offb, double* __restrict__ ll, const int* __restrict__ xlen, const int* __restrict__ ylen,
        const int* __restrict__ poison, L* __restrict__ costs, MbBlanks bb, int maxT, int maxU, int b0) {
    __shared__ double ring[kMbRing];
    __shared__ L wmax[2][16];
    const int b = b0 + blockIdx.x;
    const bool fwd = blockIdx.y == 0;
    const int K = bb.n, RS = mblank_rec_stride(K), DG = tdt_diags(maxT, maxU);
    int T, Lb;
    if (!tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb)) {
        if (fwd && threadIdx.x == 0) costs[b] = cost_invalid<L>();
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    double* off = (fwd ? offa : offb) + static_cast<size_t>(b) * DG;
    L* val = fwd ? alpha : beta;
    const int last = T - 1 + Lb;                                     // last diagonal of the grid; the terminal node: last + 1
    if (!fwd && tid == 0) { ring[(last + 1) & (kMbRing - 1)] = 0.0; off[last + 1] = 0.0; }
    double base = 0.0;                                               // off[n] of the diagonal being computed
    for (int k = 0; k <= last; ++k) {
        const int n = fwd ? k : last - k;
        if (tid == 0) { ring[n & (kMbRing - 1)] = base; off[n] = base; }
        __syncthreads();                                             // ring[n] and (k > 0) the previous diagonal's values
        const int ulo = n - (T - 1) > 0 ? n - (T - 1) : 0, uhi = n < Lb ? n : Lb;
        L tmax = neg_inf<L>();
        for (int u = ulo + tid; u <= uhi; u += blockDim.x) {
            const int t = n - u;
            Lse2<L> acc;
            if (fwd) {
                if (n == 0) acc.add(L(0));
                if (n >= 1) {
                    const L rel = static_cast<L>(ring[(n - 1) & (kMbRing - 1)] - base);
                    if (u >= 1) {                                    // label (t, u - 1) -> (t, u)
                        const size_t c = tdt_cell(b, t, u - 1, maxT, maxU);
                        acc.add(val[c] + rel + tab[c * RS + 1]);
                    }
                    if (t >= 1) {                                    // standard blank (t - 1, u) -> (t, u)
                        const size_t c = tdt_cell(b, t - 1, u, maxT, maxU);
                        acc.add(val[c] + rel + tab[c * RS]);
                    }
                }
#pragma unroll
                for (int j = 0; j < kMbMaxBig; ++j) {
                    if (j >= K) break;
                    const int d = bb.dur[j];
                    if (t < d) continue;                             // big blank j (t - d, u) -> (t, u)
                    const size_t c = tdt_cell(b, t - d, u, maxT, maxU);
                    acc.add(val[c] + static_cast<L>(ring[(n - d) & (kMbRing - 1)] - base) + tab[c * RS + 3 + j]);
                }
            } else {
                const L* r = tab + tdt_cell(b, t, u, maxT, maxU) * RS;
                if (u < Lb)                                          // label (t, u) -> (t, u + 1)
                    acc.add(val[tdt_cell(b, t, u + 1, maxT, maxU)] + static_cast<L>(ring[(n + 1) & (kMbRing - 1)] - base) +
                            r[1]);
                const auto blank_edge = [&](int d, L w) {
                    const int td = t + d;
                    if (td < T)                                      // blank (t, u) -> (td, u)
                        acc.add(val[tdt_cell(b, td, u, maxT, maxU)] + static_cast<L>(ring[(n + d) & (kMbRing - 1)] - base) + w);
                    else if (td == T && u == Lb)                     // the final blank into the terminal node (beta 0)
                        acc.add(static_cast<L>(ring[(n + d) & (kMbRing - 1)] - base) + w);
                };
                blank_edge(1, r[0]);
#pragma unroll
                for (int j = 0; j < kMbMaxBig; ++j) {
                    if (j >= K) break;
                    blank_edge(bb.dur[j], r[3 + j]);
                }
            }
            const L v = acc.get();
            val[tdt_cell(b, t, u, maxT, maxU)] = v;
            tmax = vmax(tmax, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tmax = vmax(tmax, __shfl_xor(tmax, o, kWave));
        if (lane == 0) wmax[k & 1][wave] = tmax;
        __syncthreads();
        L M = wmax[k & 1][0];
        for (int w = 1; w < nw; ++w) M = vmax(M, wmax[k & 1][w]);
        if (M - M == L(0)) base += static_cast<double>(M);           // (a diagonal without a finite value keeps the offset)
    }
    if (!fwd || tid != 0) return;
    // log P: the final blanks (T_b - d, L_b) -> terminal, read behind the last barrier
    double m = -__builtin_huge_val(), s = 0.0;
    bool nan = false;
    for (int j = -1; j < K; ++j) {
        const int d = j < 0 ? 1 : bb.dur[j < 0 ? 0 : j], ts = T - d;
        if (ts < 0) continue;
        const size_t c = tdt_cell(b, ts, Lb, maxT, maxU);
        const double v = static_cast<double>(val[c]) + ring[(ts + Lb) & (kMbRing - 1)] +
                         static_cast<double>(tab[c * RS + (j < 0 ? 0 : 3 + j)]);
        if (v != v) nan = true;
        if (v == -__builtin_huge_val()) continue;
        if (v > m) { s = s * exp2(m - v) + 1.0; m = v; } else s += exp2(v - m);
    }
    const double lp = nan ? __builtin_nan("") : (m == -__builtin_huge_val() ? m : m + log2(s));
    ll[b] = lp;
    L cost;
    if (poison[b] != 0 || lp != lp) cost = static_cast<L>(__builtin_nan(""));
    else cost = static_cast<L>(-lp * kLn2);                          // (+inf without a path)
    costs[b] = cost;
}

// ------------------------------------------------------------------------------------------
// Stage 3.  A thread per row: grid = (ceil(maxT * maxU / 256), N slice), block = 256.  The edge posteriors
// gamma_e = 2^(alpha(src) + w_e + beta(dst) - log P), the fp64 offsets summed first.  Rows outside the lattice (and every
// row of a sample whose lengths do not fit) get kPadded; a poisoned sample or one without a path gets NaN records.
template <typename L>
__global__ __launch_bounds__(256) void mblank_coef_kernel(
        L* tab, const L* __restrict__ alpha, const L* __restrict__ beta, const double* __restrict__ offa,
        const double* __restrict__ offb, const double* __restrict__ ll, const int* __restrict__ xlen,
        const int* __restrict__ ylen, const int* __restrict__ labels, const int* __restrict__ poison, MbBlanks bb,
        int maxT, int maxU, int A, int b0) {
    const int b = b0 + blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= maxT * maxU) return;
    const int t = q / maxU, u = q - t * maxU;
    const int K = bb.n, RS = mblank_rec_stride(K), DG = tdt_diags(maxT, maxU);
    const size_t c = tdt_cell(b, t, u, maxT, maxU);
    L* r = tab + c * RS;
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
        for (int j = 0; j < K; ++j) r[4 + j] = nan;
        return;
    }
    const int n = t + u;
    const double* ob = offb + static_cast<size_t>(b) * DG;
    const double oa = offa[static_cast<size_t>(b) * DG + n] - lp;
    const L a = alpha[c];
    const L lb = r[0], ltok = r[1], lz = r[2];
    L lbig[kMbMaxBig];
#pragma unroll
    for (int j = 0; j < kMbMaxBig; ++j) lbig[j] = j < K ? r[3 + j] : L(0);
    L cb = 0, cl = 0, gsum = 0, gb[kMbMaxBig];
    if (u < Lb) cl = fast_exp2(static_cast<L>(oa + ob[n + 1]) + a + beta[tdt_cell(b, t, u + 1, maxT, maxU)] + ltok);
    if (t + 1 < T) cb = fast_exp2(static_cast<L>(oa + ob[n + 1]) + a + beta[tdt_cell(b, t + 1, u, maxT, maxU)] + lb);
    else if (u == Lb) cb = fast_exp2(static_cast<L>(oa + ob[n + 1]) + a + lb);           // (t + 1 == T_b: the terminal node)
#pragma unroll
    for (int j = 0; j < kMbMaxBig; ++j) {
        gb[j] = 0;
        if (j >= K) continue;
        const int d = bb.dur[j], td = t + d;
        if (td < T) gb[j] = fast_exp2(static_cast<L>(oa + ob[n + d]) + a + beta[tdt_cell(b, td, u, maxT, maxU)] + lbig[j]);
        else if (td == T && u == Lb) gb[j] = fast_exp2(static_cast<L>(oa + ob[n + d]) + a + lbig[j]);
        gsum += gb[j];
    }
    r[0] = acc_log(cb + cl + gsum) - lz;
    r[1] = cb;
    r[2] = cl;
    r[3] = static_cast<L>(lab);
#pragma unroll
    for (int j = 0; j < kMbMaxBig; ++j)
        if (j < K) r[4 + j] = gb[j];
}

// ------------------------------------------------------------------------------------------
// Stage 4: the gradient of one element at column `pos` of row `row` whose logit is z (slow path: packets that straddle
// rows, the tail, the element-wise kernel).  Every word of the row's record is requested at once, no load waits on
// another.  Rows outside the lattice are zero.
template <typename Tag>
__device__ __forceinline__ typename Tag::comp mblank_elem_z(
        const typename Tag::comp* __restrict__ tab, const typename Tag::comp* __restrict__ grad_scale, unsigned long long row,
        int pos, typename Tag::comp z, int RS, const MbBlanks& bb, unsigned rows_per_sample) {
    using C = typename Tag::comp;
    const C* r = tab + row * RS;
    const C x = r[0], cb = r[1], cl = r[2], lf = r[3];
    C gm = 0;
#pragma unroll
    for (int j = 0; j < kMbMaxBig; ++j)
        if (j < bb.n && pos == bb.col[j]) gm = r[4 + j];
    const C gs = grad_scale != nullptr ? grad_scale[row / rows_per_sample] : C(1);
    const int lab = static_cast<int>(lf);
    if (lab == kPadded) return C(0);
    C g = fast_exp(z + x);
    if (pos == bb.blank) g -= cb;
    if (pos == lab) g -= cl;
    g -= gm;
    return g * gs;
}

// The same for an element still in memory; a row outside the lattice is not read.
template <typename Tag>
__device__ __forceinline__ typename Tag::comp mblank_elem(
        const typename Tag::comp* __restrict__ tab, const typename Tag::comp* __restrict__ grad_scale, unsigned long long row,
        int pos, const typename Tag::store* src, int RS, const MbBlanks& bb, unsigned rows_per_sample) {
    using C = typename Tag::comp;
    if (static_cast<int>(tab[row * RS + 3]) == kPadded) return C(0);
    return mblank_elem_z<Tag>(tab, grad_scale, row, pos, load1<Tag>(src), RS, bb, rows_per_sample);
}

// Flat form: the tensor as one array of 16-byte packets; a block owns PPT * 256 consecutive packets per iteration and
// grid-strides.  Row of the chunk start carried incrementally (64-bit), row of a packet by a 32-bit reciprocal division
// inside the chunk.  A packet inside one row asks for its record's label word first, then -- rows inside the lattice only
// -- for x and the logits together.  A packet pays ONE range test against the span of the blank columns (bb.lo .. bb.hi) and
// one against its label; only a packet that passes either looks at the K + 2 special columns and asks for their
// posteriors.  Non-temporal loads and stores.
// Requires acts and grads on 16-byte boundaries and N * maxT * maxU < 2^32 rows (run_mblank).
template <typename Tag>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sizeof(typename Tag::comp) == 8 ? 1 : 8))) void mblank_grad_kernel(
        const typename Tag::store* acts, typename Tag::store* grads,           // NOT __restrict__: gradients == activations
        const typename Tag::comp* __restrict__ tab, const typename Tag::comp* __restrict__ grad_scale, unsigned long long E,
        int A, int RS, MbBlanks bb, unsigned rows_per_sample, float invA, unsigned long long dq, int drem) {
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
        C x[PPT], cb[PPT], cl[PPT];
        int v0[PPT], lab[PPT];
        unsigned row[PPT];
        bool live[PPT], special[PPT];
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int p = j * 256 + threadIdx.x;
            live[j] = pk0 + p < npk;
            const unsigned idx = static_cast<unsigned>(rem) + static_cast<unsigned>(p) * V;
            unsigned q = static_cast<unsigned>(static_cast<float>(idx) * invA);
            int rr = static_cast<int>(idx - q * static_cast<unsigned>(A));
            if (rr < 0) { rr += A; --q; } else if (rr >= A) { rr -= A; ++q; }
            v0[j] = rr;
            row[j] = static_cast<unsigned>(r + q);                      // (< 2^32 rows: run_mblank)
            lab[j] = kPadded;
            if (live[j] && v0[j] + V <= A) lab[j] = static_cast<int>(tab[static_cast<size_t>(row[j]) * RS + 3]);
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int p = j * 256 + threadIdx.x;
            const bool one = v0[j] + V <= A;                            // the packet lies inside one row
            raw[j] = make_uint4(0, 0, 0, 0);
            x[j] = cb[j] = cl[j] = C(0);
            special[j] = false;
            if (live[j] && (!one || lab[j] != kPadded)) {
                raw[j] = load_packet<true>(in + pk0 + p);
                if (one) {
                    const C* rp = tab + static_cast<size_t>(row[j]) * RS;
                    x[j] = rp[0];
                    special[j] = (v0[j] <= bb.hi && v0[j] + V > bb.lo) ||
                                 static_cast<unsigned>(lab[j] - v0[j]) < static_cast<unsigned>(V);
                    if (special[j]) { cb[j] = rp[1]; cl[j] = rp[2]; }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            if (!live[j]) continue;
            const int p = j * 256 + threadIdx.x;
            C v[V];
            unpack<Tag>(raw[j], v);
            if (v0[j] + V <= A) {
                if (lab[j] == kPadded) {
#pragma unroll
                    for (int e = 0; e < V; ++e) v[e] = 0;
                } else {
#pragma unroll
                    for (int e = 0; e < V; ++e) v[e] = fast_exp(v[e] + x[j]);
                    if (special[j]) {
#pragma unroll
                        for (int e = 0; e < V; ++e) {
                            if (v0[j] + e == bb.blank) v[e] -= cb[j];
                            if (v0[j] + e == lab[j]) v[e] -= cl[j];
                        }
#pragma unroll
                        for (int i = 0; i < kMbMaxBig; ++i) {
                            if (i >= bb.n) break;
                            const int col = bb.col[i];
                            if (static_cast<unsigned>(col - v0[j]) >= static_cast<unsigned>(V)) continue;
                            const C gm = tab[static_cast<size_t>(row[j]) * RS + 4 + i];
#pragma unroll
                            for (int e = 0; e < V; ++e)
                                if (v0[j] + e == col) v[e] -= gm;
                        }
                    }
                    if (grad_scale != nullptr) {
                        const C gs = grad_scale[row[j] / rows_per_sample];
#pragma unroll
                        for (int e = 0; e < V; ++e) v[e] *= gs;
                    }
                }
            } else {
                // a row boundary inside the packet: element by element
                unsigned long long rw = row[j];
                int pos = v0[j];
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    while (pos >= A) { pos -= A; ++rw; }
                    v[e] = mblank_elem_z<Tag>(tab, grad_scale, rw, pos, v[e], RS, bb, rows_per_sample);
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
            store1<Tag>(grads + e, mblank_elem<Tag>(tab, grad_scale, rw, static_cast<int>(e - rw * A), acts + e, RS, bb,
                                                    rows_per_sample));
        }
}

// Element-wise form (tensors not on 16-byte boundaries).  grid-stride, block = 256.
template <typename Tag>
__global__ __launch_bounds__(256) void mblank_grad_elem_kernel(
        const typename Tag::store* acts, typename Tag::store* grads, const typename Tag::comp* __restrict__ tab,
        const typename Tag::comp* __restrict__ grad_scale, unsigned long long E, int A, int RS, MbBlanks bb,
        unsigned rows_per_sample) {
    for (unsigned long long e = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x; e < E;
         e += static_cast<unsigned long long>(gridDim.x) * 256) {
        const unsigned long long rw = e / static_cast<unsigned>(A);
        store1<Tag>(grads + e, mblank_elem<Tag>(tab, grad_scale, rw, static_cast<int>(e - rw * A), acts + e, RS, bb,
                                                rows_per_sample));
    }
}

}  // namespace rnnt
