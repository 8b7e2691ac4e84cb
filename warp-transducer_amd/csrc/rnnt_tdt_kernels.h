// rnnt_tdt_kernels.h -- the gfx950 kernels of the Token-and-Duration Transducer loss (include/rnnt_tdt.h).
//
// Logits (N, maxT, maxU, W), W = A + D: row (b, t, u) holds A token logits and D duration logits.  Four stages:
//   1 tdt_stats_kernel       online max / sum-exp of the A token columns of every in-lattice row, gather of the blank and
//                            label logits, log-softmax of the D duration columns; one cell record per row    [one read]
//   2 tdt_lattice_kernel     one block per (sample, direction): forward alpha and backward beta over anti-diagonals.  A
//                            cell's predecessors lie up to dmax + 1 diagonals back (forward) or ahead (backward); they are
//                            read from the global arrays the same block wrote, behind one barrier per diagonal
//   3 tdt_coef_kernel        a thread per row: the posteriors of the row's out-edges -> the gradient record, written over
//                            the cell record of stage 1 (same stride, read before it is written)
//   4 tdt_grad_kernel        one flat read+write stream of 16-byte packets over (N, maxT, maxU, W); rows outside the
//                            lattice written as zeros without their logits being read
//     tdt_grad_elem_kernel   the same element by element, for tensors not on 16-byte boundaries
//
// Lattice values are base-2 logs.  The value stored for a cell on diagonal n is RELATIVE to an fp64 offset off[n] of that
// diagonal (offa / offb): off[n] is the largest absolute value on the previous diagonal of the sweep, so stored values stay
// within a few edge weights of zero and keep fp32's relative precision however long the utterance.
#pragma once

#include "rnnt_row_lse.h"              // row_lse, row_label; through it rnnt_kernels.h

namespace rnnt {

constexpr int kTdtMaxDurations = 8;     // D
constexpr int kTdtMaxDuration = 64;     // largest duration value
constexpr int kTdtRing = 128;           // offsets kept in LDS by the lattice block (>= kTdtMaxDuration + 2)
constexpr int kTdtMaxU = 4096;

// The duration set, by value in the kernel arguments (no device copy: a captured call needs none)
struct TdtDurations { int n; int d[kTdtMaxDurations]; };

// Per cell (b, t, u) of the workspace table, stride tdt_rec_stride(D) values of the lattice type:
//   after stage 1  [lp_blank, lp_label, logZ_tok, logZ_dur, lp_dur_0 .. lp_dur_{D-1}, -]   (lp: base 2, sigma included;
//                                                                                           logZ: natural log)
//   after stage 3  [x_tok, x_dur, cb, cl, label, gamma_dur_0 .. gamma_dur_{D-1}]          x = ln(cb + cl) - logZ
// label: the row's label index, -1 without a label edge (u = L_b), kPadded outside the lattice.
__host__ __device__ inline int tdt_rec_stride(int D) { return 5 + D; }
__host__ __device__ inline size_t tdt_cell(int b, int t, int u, int maxT, int maxU) {
    return (static_cast<size_t>(b) * maxT + t) * maxU + u;
}
// the per-sample offset arrays hold diagonals 0 .. T_b + L_b (the terminal node's included)
__host__ __device__ inline int tdt_diags(int maxT, int maxU) { return maxT + maxU; }

__device__ __forceinline__ bool tdt_lens(const int* __restrict__ xlen, const int* __restrict__ ylen, int b, int maxT,
                                         int maxU, int& T, int& L) {
    T = xlen[b];
    L = ylen[b];
    return T >= 1 && T <= maxT && L >= 0 && L + 1 <= maxU;
}

__device__ __forceinline__ float tdt_log2(float x) { return log2f(x); }
__device__ __forceinline__ double tdt_log2(double x) { return log2(x); }

// Online base-2 log-sum-exp of a stream of terms; -inf terms are skipped, a NaN term makes the sum NaN.
template <typename L> struct Lse2 {
    L m = neg_inf<L>(), s = L(0);
    __device__ __forceinline__ void add(L v) {
        if (v == neg_inf<L>()) return;
        if (v > m) { s = s * fast_exp2(m - v) + L(1); m = v; }
        else s += fast_exp2(v - m);
    }
    __device__ __forceinline__ L get() const { return m == neg_inf<L>() ? m : m + tdt_log2(s); }
};

// ------------------------------------------------------------------------------------------
// Stage 1.  G lanes per row (G = 4, 16, 64), 256 / G rows per block.  grid = (ceil(maxT * maxU * G / 256), N slice).
// The A token columns are reduced by row_lse (rnnt_row_lse.h; the row's stride is A + D, so its last packet may reach
// into the duration columns: masked like a neighbouring row's).  The D duration logits: scalar loads issued before it.
template <typename Tag, int G>
__global__ __launch_bounds__(256) void tdt_stats_kernel(
        const typename Tag::store* __restrict__ acts, const int* __restrict__ labels, const int* __restrict__ xlen,
        const int* __restrict__ ylen, typename Tag::comp* __restrict__ tab, int maxT, int maxU, int A, int D, int blank,
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
    const int W = A + D;
    const bool has_lab = u < Lb;
    const int lab = has_lab ? row_label(labels, b, u, maxU, A) : blank;
    const St* row = acts + tdt_cell(b, t, u, maxT, maxU) * W;
    const C xb = load1<Tag>(row + blank);
    const C xl = load1<Tag>(row + lab);
    C dz[kTdtMaxDurations];                                                       // (issued with the packets: one wait)
#pragma unroll
    for (int j = 0; j < kTdtMaxDurations; ++j) dz[j] = j < D ? load1<Tag>(row + A + j) : neg_inf<C>();
    const C logZ = row_lse<Tag, G>(row, A, gl).log();
    if (gl != 0) return;
    C dm = neg_inf<C>();
#pragma unroll
    for (int j = 0; j < kTdtMaxDurations; ++j) dm = vmax(dm, dz[j]);
    const C dshift = (dm == neg_inf<C>()) ? C(0) : dm;
    C ds = 0;
#pragma unroll
    for (int j = 0; j < kTdtMaxDurations; ++j)
        if (j < D) ds += fast_exp(dz[j] - dshift);
    const C logZd = dshift + acc_log(ds);
    C* rec = tab + tdt_cell(b, t, u, maxT, maxU) * tdt_rec_stride(D);
    rec[0] = (xb - logZ) * C(kLog2e) - sigma2;
    rec[1] = has_lab ? (xl - logZ) * C(kLog2e) - sigma2 : neg_inf<C>();
    rec[2] = logZ;
    rec[3] = logZd;
#pragma unroll
    for (int j = 0; j < kTdtMaxDurations; ++j)
        if (j < D) rec[4 + j] = (dz[j] - logZd) * C(kLog2e);
    if (non_finite(logZ) || non_finite(logZd)) poison[b] = 1;                   // (several bad rows race: any store will do)
}

// ------------------------------------------------------------------------------------------
// Stage 2.  grid = (N slice, 2): blockIdx.y = 0 alpha, 1 beta; block = any multiple of 64 up to 1024.  Per diagonal every
// thread takes cells of it, then the block's maximum sets the next diagonal's offset (one barrier per diagonal: the
// partial maxima are double-buffered).  The forward block closes the sample: log P (ll, base 2, absolute) and the cost --
// the invalid-lengths marker, NaN for a poisoned sample, +inf when no path reaches the terminal node.
template <typename L>
__global__ __launch_bounds__(1024) void tdt_lattice_kernel(
        const L* __restrict__ tab, L* __restrict__ alpha, L* __restrict__ beta, double* __restrict__ offa,
        double* __restrict__ offb, double* __restrict__ ll, const int* __restrict__ xlen, const int* __restrict__ ylen,
        const int* __restrict__ poison, L* __restrict__ costs, TdtDurations dur, int maxT, int maxU, int b0) {
    __shared__ double ring[kTdtRing];
    __shared__ L wmax[2][16];
    const int b = b0 + blockIdx.x;
    const bool fwd = blockIdx.y == 0;
    const int D = dur.n, RS = tdt_rec_stride(D), DG = tdt_diags(maxT, maxU);
    int T, Lb;
    if (!tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb)) {
        if (fwd && threadIdx.x == 0) costs[b] = cost_invalid<L>();
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    double* off = (fwd ? offa : offb) + static_cast<size_t>(b) * DG;
    L* val = fwd ? alpha : beta;
    const int last = T - 1 + Lb;                                     // last diagonal of the grid; the terminal node: last + 1
    if (!fwd && tid == 0) { ring[(last + 1) & (kTdtRing - 1)] = 0.0; off[last + 1] = 0.0; }
    double base = 0.0;                                               // off[n] of the diagonal being computed
    for (int k = 0; k <= last; ++k) {
        const int n = fwd ? k : last - k;
        if (tid == 0) { ring[n & (kTdtRing - 1)] = base; off[n] = base; }
        __syncthreads();                                             // ring[n] and (k > 0) the previous diagonal's values
        const int ulo = n - (T - 1) > 0 ? n - (T - 1) : 0, uhi = n < Lb ? n : Lb;
        L tmax = neg_inf<L>();
        for (int u = ulo + tid; u <= uhi; u += blockDim.x) {
            const int t = n - u;
            Lse2<L> acc;
            if (fwd) {
                if (n == 0) acc.add(L(0));
#pragma unroll
                for (int j = 0; j < kTdtMaxDurations; ++j) {
                    if (j >= D) break;
                    const int d = dur.d[j], ts = t - d;
                    if (ts < 0) continue;
                    if (d > 0) {                                     // blank (ts, u) -> (t, u)
                        const size_t c = tdt_cell(b, ts, u, maxT, maxU);
                        const L* r = tab + c * RS;
                        acc.add(val[c] + static_cast<L>(ring[(n - d) & (kTdtRing - 1)] - base) + r[0] + r[4 + j]);
                    }
                    if (u >= 1) {                                    // label (ts, u - 1) -> (t, u)
                        const size_t c = tdt_cell(b, ts, u - 1, maxT, maxU);
                        const L* r = tab + c * RS;
                        acc.add(val[c] + static_cast<L>(ring[(n - d - 1) & (kTdtRing - 1)] - base) + r[1] + r[4 + j]);
                    }
                }
            } else {
                const L* r = tab + tdt_cell(b, t, u, maxT, maxU) * RS;
                const L lb = r[0], lab = r[1];
#pragma unroll
                for (int j = 0; j < kTdtMaxDurations; ++j) {
                    if (j >= D) break;
                    const int d = dur.d[j], td = t + d;
                    const L ld = r[4 + j];
                    if (d > 0 && td < T)                             // blank (t, u) -> (td, u)
                        acc.add(val[tdt_cell(b, td, u, maxT, maxU)] + static_cast<L>(ring[(n + d) & (kTdtRing - 1)] - base) +
                                lb + ld);
                    else if (d > 0 && td == T && u == Lb)            // the final blank into the terminal node (beta 0)
                        acc.add(static_cast<L>(ring[(n + d) & (kTdtRing - 1)] - base) + lb + ld);
                    if (u < Lb && td < T)                            // label (t, u) -> (td, u + 1)
                        acc.add(val[tdt_cell(b, td, u + 1, maxT, maxU)] +
                                static_cast<L>(ring[(n + d + 1) & (kTdtRing - 1)] - base) + lab + ld);
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
    for (int j = 0; j < D; ++j) {
        const int d = dur.d[j], ts = T - d;
        if (d <= 0 || ts < 0) continue;
        const size_t c = tdt_cell(b, ts, Lb, maxT, maxU);
        const double v = static_cast<double>(val[c]) + ring[(ts + Lb) & (kTdtRing - 1)] +
                         static_cast<double>(tab[c * RS]) + static_cast<double>(tab[c * RS + 4 + j]);
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
__global__ __launch_bounds__(256) void tdt_coef_kernel(
        L* tab, const L* __restrict__ alpha, const L* __restrict__ beta, const double* __restrict__ offa,
        const double* __restrict__ offb, const double* __restrict__ ll, const int* __restrict__ xlen,
        const int* __restrict__ ylen, const int* __restrict__ labels, const int* __restrict__ poison, TdtDurations dur,
        int maxT, int maxU, int A, int blank, int b0) {
    const int b = b0 + blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= maxT * maxU) return;
    const int t = q / maxU, u = q - t * maxU;
    const int D = dur.n, RS = tdt_rec_stride(D), DG = tdt_diags(maxT, maxU);
    const size_t c = tdt_cell(b, t, u, maxT, maxU);
    L* r = tab + c * RS;
    int T, Lb;
    if (!tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb) || t >= T || u > Lb) {
        r[4] = static_cast<L>(kPadded);
        return;
    }
    const int lab = u < Lb ? row_label(labels, b, u, maxU, A) : -1;
    const double lp = ll[b];
    if (poison[b] != 0 || !(lp - lp == 0.0)) {                       // NaN gradients on every in-lattice row
        const L nan = static_cast<L>(__builtin_nan(""));
        r[0] = r[1] = r[2] = r[3] = nan;
        r[4] = static_cast<L>(lab);
        for (int j = 0; j < D; ++j) r[5 + j] = nan;
        return;
    }
    const int n = t + u;
    const double* ob = offb + static_cast<size_t>(b) * DG;
    const double oa = offa[static_cast<size_t>(b) * DG + n] - lp;
    const L a = alpha[c];
    const L lb = r[0], ltok = r[1], lzt = r[2], lzd = r[3];
    L ldur[kTdtMaxDurations];
#pragma unroll
    for (int j = 0; j < kTdtMaxDurations; ++j) ldur[j] = j < D ? r[4 + j] : L(0);
    L cb = 0, cl = 0, gd[kTdtMaxDurations];
#pragma unroll
    for (int j = 0; j < kTdtMaxDurations; ++j) {
        gd[j] = 0;
        if (j >= D) continue;
        const int d = dur.d[j], td = t + d;
        if (d > 0 && td < T) {
            const L g = fast_exp2(static_cast<L>(oa + ob[n + d]) + a + beta[tdt_cell(b, td, u, maxT, maxU)] + lb + ldur[j]);
            cb += g; gd[j] += g;
        } else if (d > 0 && td == T && u == Lb) {
            const L g = fast_exp2(static_cast<L>(oa + ob[n + d]) + a + lb + ldur[j]);
            cb += g; gd[j] += g;
        }
        if (u < Lb && td < T) {
            const L g = fast_exp2(static_cast<L>(oa + ob[n + d + 1]) + a + beta[tdt_cell(b, td, u + 1, maxT, maxU)] + ltok +
                                  ldur[j]);
            cl += g; gd[j] += g;
        }
    }
    const L lc = acc_log(cb + cl);
    r[0] = lc - lzt;
    r[1] = lc - lzd;
    r[2] = cb;
    r[3] = cl;
    r[4] = static_cast<L>(lab);
#pragma unroll
    for (int j = 0; j < kTdtMaxDurations; ++j)
        if (j < D) r[5 + j] = gd[j];
}

// ------------------------------------------------------------------------------------------
// Stage 4: the gradient of one element at column `pos` of row `row` (slow path: packets that straddle rows or the token /
// duration boundary, duration columns, the tail, the element-wise kernel).  Rows outside the lattice are zero.
template <typename Tag>
__device__ __forceinline__ typename Tag::comp tdt_elem(
        const typename Tag::comp* __restrict__ tab, const typename Tag::comp* __restrict__ grad_scale, unsigned long long row,
        int pos, const typename Tag::store* src, int A, int RS, int blank, unsigned rows_per_sample) {
    using C = typename Tag::comp;
    const C* r = tab + row * RS;
    const int lab = static_cast<int>(r[4]);
    if (lab == kPadded) return C(0);
    C g;
    if (pos < A) {
        g = fast_exp(load1<Tag>(src) + r[0]);
        if (pos == blank) g -= r[2];
        if (pos == lab) g -= r[3];
    } else {
        g = fast_exp(load1<Tag>(src) + r[1]) - r[5 + (pos - A)];
    }
    if (grad_scale != nullptr) g *= grad_scale[row / rows_per_sample];
    return g;
}

// The same for an element whose logit z the caller already holds (a packet it loaded): every word of the row's record is
// requested at once, no load waits on another.
template <typename Tag>
__device__ __forceinline__ typename Tag::comp tdt_elem_z(
        const typename Tag::comp* __restrict__ tab, const typename Tag::comp* __restrict__ grad_scale, unsigned long long row,
        int pos, typename Tag::comp z, int A, int RS, int blank, unsigned rows_per_sample) {
    using C = typename Tag::comp;
    const C* r = tab + row * RS;
    const C x0 = r[0], x1 = r[1], cb = r[2], cl = r[3], lf = r[4], gd = r[5 + (pos >= A ? pos - A : 0)];
    const C gs = grad_scale != nullptr ? grad_scale[row / rows_per_sample] : C(1);
    const int lab = static_cast<int>(lf);
    if (lab == kPadded) return C(0);
    C g;
    if (pos < A) {
        g = fast_exp(z + x0);
        if (pos == blank) g -= cb;
        if (pos == lab) g -= cl;
    } else {
        g = fast_exp(z + x1) - gd;
    }
    return g * gs;
}

// Flat form: the tensor as one array of 16-byte packets; a block owns PPT * 256 consecutive packets per iteration and
// grid-strides.  Row of the chunk start carried incrementally (64-bit), row of a packet by a 32-bit reciprocal division
// inside the chunk.  A packet of token columns inside one row asks for its record's label word first, then -- rows inside
// the lattice only -- for the rest of the record and the logits together.  Non-temporal loads and stores.
// Requires acts and grads on 16-byte boundaries and N * maxT * maxU < 2^32 rows (run_tdt).
template <typename Tag>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sizeof(typename Tag::comp) == 8 ? 1 : 8))) void tdt_grad_kernel(
        const typename Tag::store* acts, typename Tag::store* grads,           // NOT __restrict__: gradients == activations
        const typename Tag::comp* __restrict__ tab, const typename Tag::comp* __restrict__ grad_scale, unsigned long long E,
        int W, int A, int RS, int blank, unsigned rows_per_sample, float invW, unsigned long long dq, int drem) {
    using C = typename Tag::comp;
    constexpr int V = Vec<Tag>::N;
    constexpr int PPT = 2;
    constexpr int CH = PPT * 256 * V;                                  // elements per chunk
    const unsigned long long npk = E / V;
    const unsigned long long nchunks = (npk + PPT * 256 - 1) / (PPT * 256);
    const u32x4* in = reinterpret_cast<const u32x4*>(acts);
    u32x4* out = reinterpret_cast<u32x4*>(grads);
    unsigned long long c = blockIdx.x;
    unsigned long long r = (c * CH) / static_cast<unsigned>(W);
    int rem = static_cast<int>((c * CH) - r * static_cast<unsigned>(W));
    for (; c < nchunks; c += gridDim.x) {
        const unsigned long long pk0 = c * (PPT * 256);
        uint4 raw[PPT];
        C x[PPT], cb[PPT], cl[PPT];
        int v0[PPT], lab[PPT];
        unsigned row[PPT];
        bool live[PPT];
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int p = j * 256 + threadIdx.x;
            live[j] = pk0 + p < npk;
            const unsigned idx = static_cast<unsigned>(rem) + static_cast<unsigned>(p) * V;
            unsigned q = static_cast<unsigned>(static_cast<float>(idx) * invW);
            int rr = static_cast<int>(idx - q * static_cast<unsigned>(W));
            if (rr < 0) { rr += W; --q; } else if (rr >= W) { rr -= W; ++q; }
            v0[j] = rr;
            row[j] = static_cast<unsigned>(r + q);                      // (< 2^32 rows: run_tdt)
            lab[j] = kPadded;
            if (live[j] && v0[j] + V <= A) lab[j] = static_cast<int>(tab[static_cast<size_t>(row[j]) * RS + 4]);
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int p = j * 256 + threadIdx.x;
            const bool tok = v0[j] + V <= A;
            raw[j] = make_uint4(0, 0, 0, 0);
            x[j] = cb[j] = cl[j] = C(0);
            if (live[j] && (!tok || lab[j] != kPadded)) {
                raw[j] = load_packet<true>(in + pk0 + p);
                if (tok) {
                    const C* rp = tab + static_cast<size_t>(row[j]) * RS;
                    x[j] = rp[0]; cb[j] = rp[2]; cl[j] = rp[3];
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
                    if (static_cast<unsigned>(blank - v0[j]) < static_cast<unsigned>(V) ||
                        static_cast<unsigned>(lab[j] - v0[j]) < static_cast<unsigned>(V)) {
#pragma unroll
                        for (int e = 0; e < V; ++e) {
                            if (v0[j] + e == blank) v[e] -= cb[j];
                            if (v0[j] + e == lab[j]) v[e] -= cl[j];
                        }
                    }
                    if (grad_scale != nullptr) {
                        const C gs = grad_scale[row[j] / rows_per_sample];
#pragma unroll
                        for (int e = 0; e < V; ++e) v[e] *= gs;
                    }
                }
            } else {
                // duration columns, the token / duration boundary, a row boundary: element by element
                unsigned long long rw = row[j];
                int pos = v0[j];
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    while (pos >= W) { pos -= W; ++rw; }
                    v[e] = tdt_elem_z<Tag>(tab, grad_scale, rw, pos, v[e], A, RS, blank, rows_per_sample);
                    ++pos;
                }
            }
            store_packet<true>(out + pk0 + p, pack<Tag>(v));
        }
        r += dq;
        rem += drem;
        if (rem >= W) { rem -= W; ++r; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)                            // the E % V elements behind the last whole packet
        for (unsigned long long e = npk * V; e < E; ++e) {
            const unsigned long long rw = e / static_cast<unsigned>(W);
            store1<Tag>(grads + e, tdt_elem<Tag>(tab, grad_scale, rw, static_cast<int>(e - rw * W), acts + e, A, RS, blank,
                                                 rows_per_sample));
        }
}

// Element-wise form (tensors not on 16-byte boundaries).  grid-stride, block = 256.
template <typename Tag>
__global__ __launch_bounds__(256) void tdt_grad_elem_kernel(
        const typename Tag::store* acts, typename Tag::store* grads, const typename Tag::comp* __restrict__ tab,
        const typename Tag::comp* __restrict__ grad_scale, unsigned long long E, int W, int A, int RS, int blank,
        unsigned rows_per_sample) {
    for (unsigned long long e = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x; e < E;
         e += static_cast<unsigned long long>(gridDim.x) * 256) {
        const unsigned long long rw = e / static_cast<unsigned>(W);
        store1<Tag>(grads + e, tdt_elem<Tag>(tab, grad_scale, rw, static_cast<int>(e - rw * W), acts + e, A, RS, blank,
                                             rows_per_sample));
    }
}

}  // namespace rnnt
