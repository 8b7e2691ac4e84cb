// rnnt_kd_kernels.h -- the gfx950 kernels of the transducer lattice distillation loss (include/rnnt_kd.h).
//
// No lattice: the loss is a KL divergence per row, so the work is a row reduction over two tensors and a flat gradient
// stream.  Mode 0 = collapsed (classes blank, label, rest), 1 = full (every column a class).
//   1 kd_stats_kernel        every in-lattice row of the student AND of the teacher read once as the aligned 16-byte
//                            packets that cover it, four in flight per lane and tensor; online (max, sum exp) of the
//                            logits / tau.  Collapsed: the blank and label logits are scalar loads in front of the packets
//                            and are masked out of the stream, which accumulates the rest class over its own columns.
//                            Full: also sum_v q_v (w_v - z_v) / tau, so the row's KL needs no second pass.
//                            -> the row record, the label word, the row's KL                          [two reads]
//   2 kd_cost_kernel         per sample the fp64 sum of its rows' KL in a fixed order (a block per sample, tree in LDS; no
//                            floating-point atomics); the cost, the per-sample gradient multiplier (1, or NaN for a sample
//                            whose cost is not finite) and the batch's "some row is padding" word
//   3 kd_grad_kernel         the flat non-temporal 16-byte stream over (N, maxT, maxU, A): records first, padding rows
//                            zeroed without their logits being read.  Collapsed reads the student only, full both tensors
//                                                                                       [one or two reads, one write]
//     kd_grad_elem_kernel    the same element by element, for tensors off 16-byte boundaries
// The record of a row (Cell + a label word in an array of its own):
//   collapsed   {-logZ_S, d_blank, d_label, d_rest}, d_k = log Q(k) - log P(k) (-inf where Q(k) = 0);
//               label word = y_u, -1 for a row of two classes (no label, or y_u == blank), kPadded for padding
//   full        {-logZ_S, -logZ_T, -, -}; label word 0, kPadded for padding
// logZ = logsumexp of the logits / tau.  A row with a non-finite logZ in either tensor gets a NaN record and a NaN KL.
#pragma once

#include "rnnt_kernels.h"

namespace rnnt {

__device__ __forceinline__ float kd_exp(float x) { return expf(x); }
__device__ __forceinline__ double kd_exp(double x) { return exp(x); }
__device__ __forceinline__ float kd_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double kd_log1p(double x) { return log1p(x); }
template <typename C> __device__ __forceinline__ C kd_nan() { return neg_inf<C>() - neg_inf<C>(); }

// The three classes of one tensor's row from their log-masses a[k] (-inf: an empty class): logZ, and per class the
// probability and its log -- of a class above 1/2 as log1p(-(the others)).
template <typename C> __device__ __forceinline__ void kd_classes(const C (&a)[3], C& logZ, C (&pr)[3], C (&lg)[3]) {
    const C mx = vmax(a[0], vmax(a[1], a[2]));
    const C shift = (mx == neg_inf<C>()) ? C(0) : mx;
    C e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = kd_exp(a[k] - shift);      // (a NaN class mass: NaN, whatever the maximum ignored)
    const C Z = e[0] + e[1] + e[2];
    const C lZ = acc_log(Z);
    logZ = shift + lZ;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pr[k] = e[k] / Z;
        const C others = (e[(k + 1) % 3] + e[(k + 2) % 3]) / Z;
        lg[k] = pr[k] > C(0.5) ? kd_log1p(-others) : (a[k] - shift) - lZ;
    }
}

// One 16-byte packet of a row's teacher values in the STUDENT's packet layout, element by element (full mode, the two rows at
// different offsets from a 16-byte boundary): columns outside the row are left to the caller's mask.
template <typename Tag>
__device__ __forceinline__ void kd_gather(const typename Tag::store* row, int col0, int A, typename Tag::comp* v) {
#pragma unroll
    for (int e = 0; e < Vec<Tag>::N; ++e)
        v[e] = static_cast<unsigned>(col0 + e) < static_cast<unsigned>(A) ? load1<Tag>(row + col0 + e) : typename Tag::comp(0);
}

// ------------------------------------------------------------------------------------------
// Stage 1.  G lanes per row (G = 4, 16, 64), 256 / G rows per block; grid = (ceil(maxT * maxU * G / 256), N slice).
// Lane g of a row's group takes the covering packets g, g + G, ... of both rows, four per tensor in flight.  Elements of
// the first and last packet that belong to the neighbouring rows are masked to -inf.  Padding rows (and every row of a sample
// whose lengths do not fit the tensor) are never read: lane 0 marks the label word and leaves a zero KL.  The first thread of
// the launch clears the batch's "some row is padding" word.
// (row_lse, rnnt_row_lse.h, is the single-tensor form; here two tensors interleave, scaled by `it`, two more columns masked, a third accumulator in mode 1.)
template <typename Tag, int G, int Mode>
__global__ __launch_bounds__(256) void kd_stats_kernel(
        const typename Tag::store* acts, const typename Tag::store* teach,      // (may be the same tensor)
        const int* __restrict__ labels, const int* __restrict__ xlen, const int* __restrict__ ylen,
        Cell<typename Tag::comp>* __restrict__ rowtab, int* __restrict__ labtab, typename Tag::comp* __restrict__ kl,
        int* __restrict__ padflag, int maxT, int maxU, int A, int blank, int b0, typename Tag::comp it) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    constexpr int V = Vec<Tag>::N;
    const int b = b0 + blockIdx.y;
    const int gl = threadIdx.x & (G - 1);
    const int q = blockIdx.x * (256 / G) + static_cast<int>(threadIdx.x) / G;     // row inside the sample
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) padflag[0] = 0;   // (kd_cost_kernel sets it, behind this launch)
    if (q >= maxT * maxU) return;                                                 // (whole groups leave together)
    const size_t r = static_cast<size_t>(b) * maxT * maxU + q;
    const int Tb = xlen[b], Ub = ylen[b] + 1;
    const bool bad = Tb < 1 || Ub < 1 || Tb > maxT || Ub > maxU;
    const int t = q / maxU, u = q - t * maxU;
    if (bad || t >= Tb || u >= Ub) {                                              // padding: never read
        if (gl == 0) { labtab[r] = kPadded; kl[r] = C(0); }
        return;
    }
    int lab = blank;
    if (Mode == 0 && u < Ub - 1) {
        lab = labels[static_cast<size_t>(b) * (maxU - 1) + u];
        lab = lab < 0 ? 0 : (lab >= A ? A - 1 : lab);
    }
    const St* rowS = acts + r * A;
    const St* rowT = teach + r * A;
    C xbS = 0, xlS = 0, xbT = 0, xlT = 0;
    if (Mode == 0) {
        xbS = load1<Tag>(rowS + blank) * it; xlS = load1<Tag>(rowS + lab) * it;
        xbT = load1<Tag>(rowT + blank) * it; xlT = load1<Tag>(rowT + lab) * it;
    }
    const uintptr_t aS = reinterpret_cast<uintptr_t>(rowS), aT = reinterpret_cast<uintptr_t>(rowT);
    const int skipS = static_cast<int>((aS & 15u) / sizeof(St)), skipT = static_cast<int>((aT & 15u) / sizeof(St));
    const u32x4* vS = reinterpret_cast<const u32x4*>(aS & ~static_cast<uintptr_t>(15));
    const u32x4* vT = reinterpret_cast<const u32x4*>(aT & ~static_cast<uintptr_t>(15));
    const int npkS = (skipS + A + V - 1) / V, npkT = (skipT + A + V - 1) / V;
    const int npk = npkS > npkT ? npkS : npkT;
    const bool same = skipS == skipT;                                             // (launch-uniform: the rows' offsets are equal)
    C mS = neg_inf<C>(), sS = 0, mT = neg_inf<C>(), sT = 0, accT = 0;
    for (int base = 0; base < npk; base += 4 * G) {
        uint4 ra[4], rb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                                             // all loads of the round first
            const int i = base + gl + j * G;
            ra[j] = make_uint4(0, 0, 0, 0);
            rb[j] = make_uint4(0, 0, 0, 0);
            if (i < npkS) ra[j] = load_packet<false>(vS + i);                     // (the gradient stream reads the student again)
            if ((Mode == 0 || same) && i < npkT) rb[j] = load_packet<Mode == 0>(vT + i);
        }
        if constexpr (Mode == 0) {
            C v[4 * V];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col0 = (base + gl + j * G) * V - skipS;
                unpack<Tag>(ra[j], v + j * V);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const int col = col0 + e;
                    const bool out = static_cast<unsigned>(col) >= static_cast<unsigned>(A) || col == blank || col == lab;
                    v[j * V + e] = out ? neg_inf<C>() : v[j * V + e] * it;
                }
            }
            absorb<C, 4 * V>(v, mS, sS);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col0 = (base + gl + j * G) * V - skipT;
                unpack<Tag>(rb[j], v + j * V);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const int col = col0 + e;
                    const bool out = static_cast<unsigned>(col) >= static_cast<unsigned>(A) || col == blank || col == lab;
                    v[j * V + e] = out ? neg_inf<C>() : v[j * V + e] * it;
                }
            }
            absorb<C, 4 * V>(v, mT, sT);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {                                         // packet by packet: z_v and w_v side by side
                const int col0 = (base + gl + j * G) * V - skipS;
                C z[V], w[V];
                unpack<Tag>(ra[j], z);
                if (same) unpack<Tag>(rb[j], w); else kd_gather<Tag>(rowT, col0, A, w);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const bool out = static_cast<unsigned>(col0 + e) >= static_cast<unsigned>(A);
                    z[e] = out ? neg_inf<C>() : z[e] * it;
                    w[e] = out ? neg_inf<C>() : w[e] * it;
                }
                absorb<C, V>(z, mS, sS);
                C mx = w[0];
#pragma unroll
                for (int e = 1; e < V; ++e) mx = vmax(mx, w[e]);
                const C mn = vmax(mT, mx);
                const C shift = (mn == neg_inf<C>()) ? C(0) : mn;
                const C f = fast_exp(mT - shift);
                C es = 0, ea = 0;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const C ev = fast_exp(w[e] - shift);
                    es += ev;
                    ea += ev > C(0) ? ev * (w[e] - z[e]) : C(0);                  // (q_v = 0 contributes 0, not 0 * inf)
                }
                sT = sT * f + es;
                accT = (f > C(0) ? accT * f : C(0)) + ea;
                mT = mn;
            }
        }
    }
    C MS = mS, MT = mT;
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        MS = vmax(MS, __shfl_xor(MS, off, kWave));
        MT = vmax(MT, __shfl_xor(MT, off, kWave));
    }
    const C shS = (MS == neg_inf<C>()) ? C(0) : MS, shT = (MT == neg_inf<C>()) ? C(0) : MT;
    const C fT = fast_exp(mT - shT);
    C sumS = sS * fast_exp(mS - shS), sumT = sT * fT, acc = fT > C(0) ? accT * fT : C(0);
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        sumS += __shfl_xor(sumS, off, kWave);
        sumT += __shfl_xor(sumT, off, kWave);
        if (Mode == 1) acc += __shfl_xor(acc, off, kWave);
    }
    if (gl != 0) return;
    Cell<C> rec;
    C cost;
    int word;
    bool poisoned;
    if constexpr (Mode == 0) {
        const bool two = lab == blank;                                            // no label, or a label that is the blank
        // log-mass of the rest class: exactly -inf when it is empty, NaN when a logit of it was
        const C lrS = sumS > C(0) ? shS + acc_log(sumS) : (sumS == C(0) ? neg_inf<C>() : kd_nan<C>());
        const C lrT = sumT > C(0) ? shT + acc_log(sumT) : (sumT == C(0) ? neg_inf<C>() : kd_nan<C>());
        const C a_s[3] = {xbS, two ? neg_inf<C>() : xlS, lrS}, a_t[3] = {xbT, two ? neg_inf<C>() : xlT, lrT};
        C lzS, lzT, P[3], Q[3], lP[3], lQ[3], d[3];
        kd_classes<C>(a_s, lzS, P, lP);
        kd_classes<C>(a_t, lzT, Q, lQ);
        cost = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            d[k] = Q[k] > C(0) ? lQ[k] - lP[k] : neg_inf<C>();
            if (Q[k] > C(0)) cost += Q[k] * d[k];
        }
        poisoned = non_finite(lzS) || non_finite(lzT);
        rec.x = -lzS; rec.y = d[0]; rec.z = d[1]; rec.w = d[2];
        word = two ? -1 : lab;
    } else {
        const C lzS = shS + acc_log(sumS), lzT = shT + acc_log(sumT);
        cost = acc / sumT + (lzS - lzT);
        poisoned = non_finite(lzS) || non_finite(lzT);
        rec.x = -lzS; rec.y = -lzT; rec.z = 0; rec.w = 0;
        word = 0;
    }
    if (poisoned) {
        cost = kd_nan<C>();
        rec.x = rec.y = rec.z = rec.w = cost;
    }
    rowtab[r] = rec;
    labtab[r] = word;
    kl[r] = cost;
}

// ------------------------------------------------------------------------------------------
// Stage 2: one block per sample.  Thread i adds rows i, i + 256, ... of the sample's lattice in fp64, then a tree in LDS: a
// fixed order, no atomics.  A NaN row makes the sum NaN, a +inf row (P(k) = 0 < Q(k)) +inf: smul[b] = NaN then, so that
// every in-lattice gradient of the sample is NaN.  Lengths that do not fit the tensor: the cost marker.  A sample with padding
// sets the batch's word (a plain store of 1 by whoever has some: the statistics kernel cleared it).
template <typename C>
__global__ __launch_bounds__(256) void kd_cost_kernel(const C* __restrict__ kl, const int* __restrict__ xlen,
                                                      const int* __restrict__ ylen, C* __restrict__ costs,
                                                      C* __restrict__ smul, int* __restrict__ padflag, int maxT, int maxU) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = xlen[b], Ub = ylen[b] + 1;
    const bool bad = Tb < 1 || Ub < 1 || Tb > maxT || Ub > maxU;
    const C* rows = kl + static_cast<size_t>(b) * maxT * maxU;
    double acc = 0.0;
    if (!bad)
        for (int q = tid; q < Tb * maxU; q += 256)
            if (q % maxU < Ub) acc += static_cast<double>(rows[q]);
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid != 0) return;
    const C cost = bad ? cost_invalid<C>() : static_cast<C>(red[0]);
    costs[b] = cost;
    smul[b] = (bad || !non_finite(cost)) ? C(1) : kd_nan<C>();
    if (bad || Tb < maxT || Ub < maxU) padflag[0] = 1;
}

// ------------------------------------------------------------------------------------------
// Stage 3: one element at column `pos` of a row with record `rec` and label word `lab`; z, w its two logits (w: full mode),
// it = 1 / tau, gs = the sample's scale with 1 / tau folded in.
template <typename C, int Mode>
__device__ __forceinline__ C kd_elem(const Cell<C> rec, int lab, int pos, C z, C w, int blank, C it, C gs) {
    if (lab == kPadded) return C(0);
    const C lp = z * it + rec.x;
    if constexpr (Mode == 1) {
        return (fast_exp(lp) - fast_exp(w * it + rec.y)) * gs;
    } else {
        C d = rec.w;                                                   // (selects of values, not of the record's addresses)
        d = pos == lab ? rec.z : d;
        d = pos == blank ? rec.y : d;
        return (fast_exp(lp) - fast_exp(lp + d)) * gs;
    }
}

// The scale of sample s: its multiplier (kd_cost_kernel), 1 / tau and the caller's grad_scale.
template <typename C>
__device__ __forceinline__ C kd_sample_scale(const C* __restrict__ smul, const C* __restrict__ grad_scale, C it, unsigned s) {
    const C m = smul[s] * it;
    return grad_scale != nullptr ? m * grad_scale[s] : m;
}

// Flat form: the tensor as one array of 16-byte packets; a block owns PPT * 256 consecutive packets per iteration and
// grid-strides.  Row of the chunk start carried incrementally in 64 bits, row of a packet by a 32-bit reciprocal division
// inside the chunk.  The record and the label word are asked for first; with padding in the batch (kd_cost_kernel's word,
// read once when the block starts) and rows of 128 bytes or more a packet inside a padding row is zero-filled without its
// logits being read.  The per-sample scale -- smul, 1 / tau and the caller's grad_scale -- is one block-uniform value
// when the chunk lies inside one sample.  Non-temporal loads and stores; a thread reads an element and writes the same
// element, so gradients == activations is legal.  Requires the tensors on 16-byte boundaries and N * maxT * maxU < 2^32
// rows (run_kd).
template <typename Tag, int Mode>
__global__ __launch_bounds__(256) void kd_grad_kernel(
        const typename Tag::store* acts, const typename Tag::store* teach, typename Tag::store* grads,   // NOT __restrict__
        const Cell<typename Tag::comp>* __restrict__ rowtab, const int* __restrict__ labtab,
        const typename Tag::comp* __restrict__ smul, const int* __restrict__ padflag,
        const typename Tag::comp* __restrict__ grad_scale, unsigned long long E, unsigned R, int A, int blank, unsigned TU,
        float invA, unsigned long long dq, int drem, typename Tag::comp it) {
    using C = typename Tag::comp;
    constexpr int V = Vec<Tag>::N;
    constexpr int PPT = 2;
    constexpr int CH = PPT * 256 * V;                                  // elements per chunk
    const bool ps = padflag[0] != 0 && A * static_cast<int>(sizeof(typename Tag::store)) >= 128;
    const unsigned long long npk = E / V;
    const unsigned long long nchunks = (npk + PPT * 256 - 1) / (PPT * 256);
    const u32x4* in = reinterpret_cast<const u32x4*>(acts);
    const u32x4* tin = reinterpret_cast<const u32x4*>(teach);
    u32x4* out = reinterpret_cast<u32x4*>(grads);
    unsigned long long c = blockIdx.x;
    unsigned long long r = (c * CH) / static_cast<unsigned>(A);
    int rem = static_cast<int>((c * CH) - r * static_cast<unsigned>(A));
    for (; c < nchunks; c += gridDim.x) {
        const unsigned long long pk0 = c * (PPT * 256);
        // the chunk's scale: block-uniform when all its rows belong to one sample (nearly always), else per packet
        const unsigned long long rl0 = r + static_cast<unsigned>(CH / A + 1);
        const unsigned rl = rl0 < R ? static_cast<unsigned>(rl0) : R - 1;   // last row the chunk can touch
        const unsigned s0 = static_cast<unsigned>(r) / TU;
        const bool uni = s0 == rl / TU;
        const C chunk_scale = kd_sample_scale<C>(smul, grad_scale, it, s0);
        auto scale_of = [&](unsigned row) -> C {
            if (uni) return chunk_scale;
            return kd_sample_scale<C>(smul, grad_scale, it, (row < R ? row : R - 1) / TU);
        };
        uint4 raw[PPT], rawt[PPT];
        Cell<C> rec[PPT], rec2[PPT];                                   // rec2, lab2: the next row's, for packets that straddle
        int lab[PPT], lab2[PPT];
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
            row[k] = static_cast<unsigned>(r + q);                     // (< 2^32 rows: run_kd)
            raw[k] = make_uint4(0, 0, 0, 0);
            rawt[k] = make_uint4(0, 0, 0, 0);
            lab[k] = lab2[k] = kPadded;
            if (live[k]) {
                rec[k] = rowtab[row[k]];
                lab[k] = labtab[row[k]];
                if (!ps) {
                    raw[k] = load_packet<true>(in + pk0 + p);
                    if (Mode == 1) rawt[k] = load_packet<true>(tin + pk0 + p);
                }
                if (rr + V > A) {
                    const unsigned nx = row[k] + 1 < R ? row[k] + 1 : R - 1;
                    rec2[k] = rowtab[nx];
                    lab2[k] = labtab[nx];
                }
            }
        }
        if (ps) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const int p = k * 256 + threadIdx.x;
                const bool skip = (v0[k] + V <= A) && lab[k] == kPadded;
                if (live[k] && !skip) {
                    raw[k] = load_packet<true>(in + pk0 + p);
                    if (Mode == 1) rawt[k] = load_packet<true>(tin + pk0 + p);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            if (!live[k]) continue;
            const int p = k * 256 + threadIdx.x;
            C v[V], w[V];                                              // (w: full mode only)
            unpack<Tag>(raw[k], v);
            if constexpr (Mode == 1) unpack<Tag>(rawt[k], w);
            if (v0[k] + V <= A) {
                // whole packet inside one row (the common case)
                if (lab[k] == kPadded) {
#pragma unroll
                    for (int j = 0; j < V; ++j) v[j] = 0;
                } else {
                    const C gs = scale_of(row[k]);
                    if constexpr (Mode == 1) {
#pragma unroll
                        for (int j = 0; j < V; ++j) v[j] = (fast_exp(v[j] * it + rec[k].x) - fast_exp(w[j] * it + rec[k].y)) * gs;
                    } else {
                        const C cc = rec[k].x, db = rec[k].y, dl = rec[k].z, dr = rec[k].w;
#pragma unroll
                        for (int j = 0; j < V; ++j) {
                            const int pos = v0[k] + j;
                            C d = pos == lab[k] ? dl : dr;
                            d = pos == blank ? db : d;
                            const C lp = v[j] * it + cc;
                            v[j] = (fast_exp(lp) - fast_exp(lp + d)) * gs;
                        }
                    }
                }
            } else if (A >= V) {
                // two rows at most: elements j < split belong to row[k], the rest to the next row
                const int split = A - v0[k];
                const C gs1 = scale_of(row[k]), gs2 = scale_of(row[k] + 1);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const bool first = j < split;
                    Cell<C> sel;                                       // (field by field: values, not a choice of addresses)
                    sel.x = first ? rec[k].x : rec2[k].x; sel.y = first ? rec[k].y : rec2[k].y;
                    sel.z = first ? rec[k].z : rec2[k].z; sel.w = first ? rec[k].w : rec2[k].w;
                    v[j] = kd_elem<C, Mode>(sel, first ? lab[k] : lab2[k], first ? v0[k] + j : j - split,
                                            v[j], Mode == 1 ? w[j] : C(0), blank, it, first ? gs1 : gs2);
                }
            } else {
                unsigned rw = row[k];
                int pos = v0[k];
                Cell<C> cur = rec[k];
                int cl = lab[k];
                C gs = scale_of(rw);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    while (pos >= A) {
                        pos -= A;
                        ++rw;
                        if (rw < R) { cur = rowtab[rw]; cl = labtab[rw]; }
                        gs = scale_of(rw);
                    }
                    v[j] = kd_elem<C, Mode>(cur, cl, pos, v[j], Mode == 1 ? w[j] : C(0), blank, it, gs);
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
            const int cl = labtab[rw];
            C g = C(0);
            if (cl != kPadded)
                g = kd_elem<C, Mode>(rowtab[rw], cl, static_cast<int>(e - static_cast<unsigned long long>(rw) * A),
                                     load1<Tag>(acts + e), Mode == 1 ? load1<Tag>(teach + e) : C(0), blank, it,
                                     kd_sample_scale<C>(smul, grad_scale, it, rw / TU));
            store1<Tag>(grads + e, g);
        }
}

// Element-wise form (a tensor not on a 16-byte boundary).  grid-stride, block = 256.  The label word is looked at before a
// logit is read: padding rows are never read here either.
template <typename Tag, int Mode>
__global__ __launch_bounds__(256) void kd_grad_elem_kernel(
        const typename Tag::store* acts, const typename Tag::store* teach, typename Tag::store* grads,
        const Cell<typename Tag::comp>* __restrict__ rowtab, const int* __restrict__ labtab,
        const typename Tag::comp* __restrict__ smul, const typename Tag::comp* __restrict__ grad_scale, unsigned long long E,
        int A, int blank, unsigned TU, typename Tag::comp it) {
    using C = typename Tag::comp;
    for (unsigned long long e = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x; e < E;
         e += static_cast<unsigned long long>(gridDim.x) * 256) {
        const unsigned rw = static_cast<unsigned>(e / static_cast<unsigned>(A));
        const int cl = labtab[rw];
        C g = C(0);
        if (cl != kPadded) {
            const C gs = kd_sample_scale<C>(smul, grad_scale, it, rw / TU);
            g = kd_elem<C, Mode>(rowtab[rw], cl, static_cast<int>(e - static_cast<unsigned long long>(rw) * A),
                                 load1<Tag>(acts + e), Mode == 1 ? load1<Tag>(teach + e) : C(0), blank, it, gs);
        }
        store1<Tag>(grads + e, g);
    }
}

}  // namespace rnnt
