// rnnt_sample_kernels.h -- the gfx950 kernels of the alignment sampler over edge log-probabilities (include/rnnt_sample.h):
// the log-sum sweep on the px / py lattice, and the walks back from the terminal.
//
//   1 sample_fwd_kernel       pxpy_sweep (rnnt_pxpy.h: a block per sample, a thread per lattice row, chunked prefetch, the
//                             neighbour's hand-over through DPP and LDS words) with ONE double per node, px / py [b, s, :]
//                             kSaChunk steps ahead of use.  The emit candidate is the value handed to the row above.  Per
//                             node one exp and one log1p; a -inf candidate is selected out.  Every node's value goes to
//                             `alpha`; the block then writes -inf outside the rectangle and the score last.
//   2 sample_walk_kernel      a thread per walk (b, k); the walks of one sample sit in the same wavefronts.  A step
//                             issues the loads of alpha[s - 1, t'], px[s - 1, t'], alpha[s, t - 1], py[s, t - 1] and the
//                             uniform together: ONE dependent round trip per step.  Whichever edge is taken, the
//                             predecessor's alpha is one of the two just loaded.  py feeds the weight only.  The loop is
//                             bounded by (s1 - s0) + (t1 - t0) steps.
//   3 path_weights_kernel     a wavefront per (b, k): the lanes check the row of frames and add the symbol edges of their
//                             rows, then the frame edges of every row's interval, then a butterfly over the 64 lanes.
//   4 path_edges_kernel       a block per (sample, slice of rows): the threads first judge the K rows of frames (valid or
//                             not, LDS), then a thread per output element loops over k in ascending order with two
//                             comparisons against the interval read from frames.  No atomics.
#pragma once

#include "rnnt_pxpy.h"                 // PxRect / px_rect, pxpy_sweep; through rnnt_kernels.h cost_invalid, load1 / store1

namespace rnnt {

constexpr int kSaChunk = 8;             // steps per prefetched chunk of the sweep
// 8-byte storage: half of it, the registers of 1024 threads (128 each) without a spill
template <typename Tag> constexpr int sa_chunk() { return sizeof(typename Tag::store) == 8 ? kSaChunk / 2 : kSaChunk; }
constexpr int kSaWaveMaxU = 64;         // S + 1 up to here: one wavefront, no LDS exchange
constexpr int kSaMaxK = 1024;           // walks per sample at most
constexpr int kSaWalkBlock = 256;       // threads of a walk block at most
constexpr int kSaEdgeBlock = 256;       // threads of a path_edges block
constexpr int kSaEdgeSlices = 64;       // row slices of a sample at most (grid.y of path_edges_kernel)

// log(exp x + exp y).  A candidate of -inf is selected out: the result is the other candidate bit for bit.
__device__ __forceinline__ double sa_logaddexp(double x, double y) {
    const double NEG = -__builtin_huge_val();
    const bool xmax = x > y;
    const double hi = xmax ? x : y, lo = xmax ? y : x;
    if (!(hi > NEG)) return hi == hi ? NEG : hi;                     // no candidate (NaN: NaN)
    if (!(lo > NEG) && lo == lo) return hi;                          // one candidate
    return hi + log1p(exp(lo - hi));
}

// A double rounded ONCE to the storage type.  16-bit storage goes through fp32 rounded to odd, so that the second
// rounding (fp32 -> 16 bits, to nearest even) sees every sticky bit.
template <typename Tag> __device__ __forceinline__ typename Tag::comp sa_round(double v) {
    using C = typename Tag::comp;
    if constexpr (sizeof(typename Tag::store) != 2) {
        return static_cast<C>(v);
    } else {
        float f = static_cast<float>(v);
        const double back = static_cast<double>(f);
        if (back != v && v - v == 0.0) {                             // inexact, finite
            unsigned u = __float_as_uint(f);
            if (__builtin_fabs(back) > __builtin_fabs(v)) u -= 1;    // towards zero (inf -> FLT_MAX)
            f = __uint_as_float(u | 1u);                             // odd
        }
        return f;
    }
}

// grid = B, block = 64 (MULTI == false: S + 1 <= kSaWaveMaxU) or 64 * ceil((S + 1) / 64) <= 1024.
template <typename Tag, bool MOD, bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void sample_fwd_kernel(
        const typename Tag::store* __restrict__ px, const typename Tag::store* __restrict__ py,
        const long long* __restrict__ boundary, double* __restrict__ scores, double* __restrict__ alpha, int S, int T) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    constexpr int CH = sa_chunk<Tag>();
    __shared__ double edge[2][16][1];
    __shared__ double sh_score;
    __shared__ int sh_bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nthreads = static_cast<int>(blockDim.x);
    const int TX = MOD ? T : T + 1, U = S + 1, T1 = T + 1;
    const PxRect r = px_rect(boundary, b, S, T);
    const int s0 = r.s0, t0 = r.t0, Sr = r.Sr, Tr = r.Tr;
    const double NEG = -__builtin_huge_val(), INF = __builtin_huge_val();
    double* al = alpha + static_cast<size_t>(b) * U * T1;
    if (tid == 0) { sh_bad = 0; sh_score = NEG; }
    __syncthreads();

    if (r.ok) {
        const int ls = tid;
        const bool hasy = ls <= Sr, hasx = ls < Sr;
        const size_t s = static_cast<size_t>(s0 + (hasy ? ls : 0));
        const size_t ox = (static_cast<size_t>(b) * S + (hasx ? s : 0)) * TX + t0;       // (never dereferenced unless hasx)
        const size_t oy = (static_cast<size_t>(b) * U + s) * T + t0;
        const St* const rx[1] = {px + ox};
        const St* const ry[1] = {py + oy};
        double* rn = al + s * T1 + t0;
        double stay = NEG;                                           // the stay candidate; the emit one is the hand-over
        bool bad = false;
        const double none[1] = {NEG};                                // row -1 is no row
        pxpy_sweep<Tag, MOD, MULTI, false, 1, 1, CH, PxNoX>(
            rx, ry, ls, Sr, Tr, edge, none, [](int, bool) { return PxNoX{}; },
            [&](int j, bool act, bool ex, bool ey, const double (&left)[1], const C (&wxs)[1], const C (&wys)[1], PxNoX,
                double (&emit)[1]) {
                double a = sa_logaddexp(left[0], stay);
                if (ls == 0 && j == 0) a = 0.0;                      // the source (both candidates are -inf there)
                const double wx = static_cast<double>(wxs[0]), wy = static_cast<double>(wys[0]);
                bad = bad || (ex && !(wx < INF)) || (ey && !(wy < INF));           // NaN or +inf on an edge of the rectangle
                emit[0] = ex ? a + wx : NEG;
                stay = ey ? a + wy : NEG;
                if (act) {
                    rn[j] = a;
                    if (ls == Sr && j == Tr) sh_score = a;
                }
            });
        if (bad) sh_bad = 1;                                         // (several bad edges race: any store will do)
    }
    __threadfence_block();
    __syncthreads();

    // ---- the nodes outside the rectangle, then the score
    for (size_t i = tid; i < static_cast<size_t>(U) * T1; i += nthreads) {
        const int s = static_cast<int>(i / T1), t = static_cast<int>(i - static_cast<size_t>(s) * T1);
        if (!(r.ok && s >= s0 && s <= s0 + Sr && t >= t0 && t <= t0 + Tr)) al[i] = NEG;
    }
    if (tid == 0) scores[b] = !r.ok ? cost_invalid<double>() : (sh_bad != 0 ? __builtin_nan("") : sh_score);
}

// grid = (B, ceil(K / block)), block = min(kSaWalkBlock, 64 * ceil(K / 64)): thread (b, k) walks from (s1, t1) to (s0, t0).
template <typename Tag, bool MOD>
__global__ __launch_bounds__(kSaWalkBlock) void sample_walk_kernel(
        const typename Tag::store* __restrict__ px, const typename Tag::store* __restrict__ py,
        const long long* __restrict__ boundary, const double* __restrict__ alpha, const double* __restrict__ scores,
        const float* __restrict__ uniforms, int* __restrict__ frames, double* __restrict__ weights, int S, int T, int K) {
    using St = typename Tag::store;
    const int b = blockIdx.x, k = blockIdx.y * static_cast<int>(blockDim.x) + threadIdx.x;
    if (k >= K) return;
    const int TX = MOD ? T : T + 1, U = S + 1, T1 = T + 1;
    const PxRect r = px_rect(boundary, b, S, T);
    const int s0 = r.s0, t0 = r.t0, s1 = r.s0 + r.Sr, t1 = r.t0 + r.Tr;
    const double NEG = -__builtin_huge_val();
    const double sc = scores[b];
    const bool path = r.ok && sc - sc == 0.0;                        // finite (block-uniform)
    const size_t q = static_cast<size_t>(b) * K + k;
    int* fr = frames + q * S;
    for (int s = 0; s < S; ++s)
        if (!(path && s >= s0 && s < s1)) fr[s] = -1;
    if (!path) {
        weights[q] = (r.ok && sc == NEG) ? NEG : __builtin_nan("");
        return;
    }
    const double* al = alpha + static_cast<size_t>(b) * U * T1;
    const St* bx = px + static_cast<size_t>(b) * S * TX;
    const St* by = py + static_cast<size_t>(b) * U * T;
    const float* un = uniforms + q * (static_cast<size_t>(S) + T);
    int s = s1, t = t1;
    double cur = al[static_cast<size_t>(s) * T1 + t], W = 0.0;
    const int nsteps = r.Sr + r.Tr;
    for (int i = 0; i < nsteps && (s > s0 || t > t0); ++i) {
        const int tp = MOD ? t - 1 : t;
        const bool hasx = s > s0 && tp >= t0, hasy = t > t0;
        if (!hasx && !hasy) break;                                   // (no in-edge: not a node of a path)
        double ax = NEG, wx = NEG, ay = NEG, wy = NEG;
        float u = 0.0f;
        if (hasx) {
            ax = al[static_cast<size_t>(s - 1) * T1 + tp];
            wx = static_cast<double>(load1<Tag>(bx + static_cast<size_t>(s - 1) * TX + tp));
        }
        if (hasy) {
            ay = al[static_cast<size_t>(s) * T1 + t - 1];
            wy = static_cast<double>(load1<Tag>(by + static_cast<size_t>(s) * T + t - 1));
        }
        if (s > s0) u = un[(s - s0) + (t - t0) - 1];
        bool sym = false;
        if (s > s0) sym = static_cast<double>(u) < exp(ax + wx - cur);             // the whole rule
        if (!hasy) sym = true;                                       // (r == 1 there; memory safety with a foreign alpha)
        if (!hasx) sym = false;
        if (sym) {
            fr[s - 1] = tp;
            W += wx;
            s -= 1;
            t = tp;
            cur = ax;
        } else {
            W += wy;
            t -= 1;
            cur = ay;
        }
    }
    weights[q] = W;
}

// Is row `fr` of frames a path of the rectangle?  (thread-serial form, path_edges_kernel's)
template <bool MOD>
__device__ __forceinline__ bool sa_row_ok(const int* __restrict__ fr, int s0, int t0, int s1, int t1) {
    int prev = MOD ? t0 - 1 : t0;
    bool ok = true;
    for (int s = s0; s < s1; ++s) {
        const int f = fr[s];
        ok = ok && f >= t0 && f <= (MOD ? t1 - 1 : t1) && (MOD ? f > prev : f >= prev);
        prev = f;
    }
    return ok;
}

// grid = min(B K, 2^20) blocks of one wavefront, striding over (b, k).  ORDER of the additions: lane l first adds, from 0.0,
// the symbol edges of the rows s0 + l, s0 + l + 64, ... in ascending s, then for s = s0 .. s1 in ascending s the frame
// edges py[s, t], t = lo + l, lo + l + 64, ... < hi of the row's interval [lo, hi); the 64 partial sums are combined by a
// butterfly (lane ^ 32, 16, 8, 4, 2, 1).
template <typename Tag, bool MOD>
__global__ __launch_bounds__(64) void path_weights_kernel(
        const typename Tag::store* __restrict__ px, const typename Tag::store* __restrict__ py,
        const long long* __restrict__ boundary, const int* __restrict__ frames, double* __restrict__ weights, int S, int T,
        int K, long long BK) {
    using St = typename Tag::store;
    const int lane = threadIdx.x;
    const int TX = MOD ? T : T + 1, U = S + 1;
    for (long long q = blockIdx.x; q < BK; q += gridDim.x) {
        const int b = static_cast<int>(q / K);
        const PxRect r = px_rect(boundary, b, S, T);
        const int s0 = r.s0, t0 = r.t0, s1 = r.s0 + r.Sr, t1 = r.t0 + r.Tr;
        const int* fr = frames + static_cast<size_t>(q) * S;
        const St* bx = px + static_cast<size_t>(b) * S * TX;
        const St* by = py + static_cast<size_t>(b) * U * T;
        bool bad = !r.ok;
        double acc = 0.0;
        if (r.ok) {
            for (int s = s0 + lane; s < s1; s += 64) {
                const int f = fr[s], prev = s > s0 ? fr[s - 1] : (MOD ? t0 - 1 : t0);
                const bool ok = f >= t0 && f <= (MOD ? t1 - 1 : t1) && (MOD ? f > prev : f >= prev);
                if (ok) acc += static_cast<double>(load1<Tag>(bx + static_cast<size_t>(s) * TX + f));
                else bad = true;
            }
        }
        bad = __any(bad) != 0;                                       // (wave-uniform from here)
        if (!bad) {
            for (int s = s0; s <= s1; ++s) {
                const int lo = s == s0 ? t0 : fr[s - 1] + (MOD ? 1 : 0), hi = s == s1 ? t1 : fr[s];
                for (int t = lo + lane; t < hi; t += 64) acc += static_cast<double>(load1<Tag>(by + static_cast<size_t>(s) * T + t));
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) weights[q] = bad ? __builtin_nan("") : acc;
    }
}

// grid = (B, min(S + 1, kSaEdgeSlices)), block = kSaEdgeBlock.  Block (b, y) owns the rows s = y, y + gridDim.y, ... of
// px_acc / py_acc [b]; coeff: B K doubles or NULL for 1.
template <typename Tag, bool MOD>
__global__ __launch_bounds__(kSaEdgeBlock) void path_edges_kernel(
        const int* __restrict__ frames, const double* __restrict__ coeff, const long long* __restrict__ boundary,
        typename Tag::store* __restrict__ px_acc, typename Tag::store* __restrict__ py_acc, int S, int T, int K) {
    __shared__ double cf[kSaMaxK];
    __shared__ unsigned char live[kSaMaxK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int TX = MOD ? T : T + 1, U = S + 1;
    const PxRect r = px_rect(boundary, b, S, T);
    const int s0 = r.s0, t0 = r.t0, s1 = r.s0 + r.Sr, t1 = r.t0 + r.Tr;
    const int* fb = frames + static_cast<size_t>(b) * K * S;
    for (int k = tid; k < K; k += kSaEdgeBlock) {
        live[k] = r.ok && sa_row_ok<MOD>(fb + static_cast<size_t>(k) * S, s0, t0, s1, t1);
        cf[k] = coeff != nullptr ? coeff[static_cast<size_t>(b) * K + k] : 1.0;
    }
    __syncthreads();
    const int lastx = MOD ? t1 - 1 : t1;
    for (int s = blockIdx.y; s < U; s += gridDim.y) {
        const bool rowy = r.ok && s >= s0 && s <= s1, rowx = r.ok && s >= s0 && s < s1;
        for (int t = tid; t <= T; t += kSaEdgeBlock) {
            const bool iny = rowy && t >= t0 && t < t1, inx = rowx && t >= t0 && t <= lastx;
            double ay = 0.0, ax = 0.0;
            if (iny || inx) {
                for (int k = 0; k < K; ++k) {
                    if (!live[k]) continue;
                    const int* fr = fb + static_cast<size_t>(k) * S;
                    const int lo = s == s0 ? t0 : fr[s - 1] + (MOD ? 1 : 0), hi = s == s1 ? t1 : fr[s];
                    if (iny && t >= lo && t < hi) ay += cf[k];
                    if (inx && t == hi) ax += cf[k];
                }
            }
            if (t < T) store1<Tag>(py_acc + (static_cast<size_t>(b) * U + s) * T + t, sa_round<Tag>(ay));
            if (s < S && t < TX) store1<Tag>(px_acc + (static_cast<size_t>(b) * S + s) * TX + t, sa_round<Tag>(ax));
        }
    }
}

}  // namespace rnnt
