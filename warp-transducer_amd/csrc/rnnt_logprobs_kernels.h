// rnnt_logprobs_kernels.h -- the gfx950 kernels of libwarprnnt_logprobs.so (include/rnnt_logprobs.h): the edge
// log-probabilities px, py and the normaliser lse from joint (N, T, U, C) or pruned (N, T, K, C) logits, and the logit
// gradient from the three incoming gradients.  All of them address rows through ONE row map (lp_row); the launch rule is
// rnnt_logprobs_impl.h's.
//   logprobs_lse_kernel     one pass over every real row: online max / sum-exp with G lanes per row (G = 4, 16, 64), the
//                           reduction of pstream_stats_kernel (rnnt_pstream_kernels.h); lse in logits order, exact 0 on rows
//                           that are not real, which are never read
//   logprobs_edges_kernel   a thread per (b, u, t) of the OUTPUTS, t fastest: lse and two gathered logits (blank, label) per
//                           real row, px / py written along t -- no store is scattered along a stride of T; in the pruned form
//                           it decides per (u, t) whether u - r lies in [0, K)
//   logprobs_grad_kernel    the backward, elementwise given lse: per row the record (gl - gx - gy, gx, gy, label, lse) is
//                           looked up once by every lane, each element is read once and written once; VEC: 16-byte packets,
//                           else element by element
#pragma once
#include "rnnt_row_lse.h"              // row_lse; through it rnnt_kernels.h (non_finite) and rnnt_device.h

namespace rnnt {

constexpr int kLpNarrowBytes = 256;     // rows up to here: 4 lanes per row
constexpr int kLpWideBytes = 2048;      // up to here: 16 lanes per row; beyond: 64
constexpr long long kLpMaxGrid = 1 << 20;

struct LpArgs {
    const int* symbols;                 // (B, U - 1)
    const int* ranges;                  // (B, T) frame starts; nullptr in the joint form
    const long long* boundary;          // (B, 4) or nullptr: columns 2 and 3 are S_b and T_b
    int K;                              // 0: joint form
    int Kp;                             // the third extent of logits, lse and dlogits: U, or K
    int T, U, C, B, blank, mod;         // mod = rnnt_type
};

struct LpSample { int Tb, Sb; };
__device__ __forceinline__ LpSample lp_sample(const LpArgs& a, int b) {
    LpSample s;
    s.Tb = a.T;
    s.Sb = a.U - 1;
    if (a.boundary != nullptr) {
        const long long sb = a.boundary[static_cast<long long>(b) * 4 + 2], tb = a.boundary[static_cast<long long>(b) * 4 + 3];
        s.Sb = static_cast<int>(sb < 0 ? 0 : (sb > a.U - 1 ? a.U - 1 : sb));
        s.Tb = static_cast<int>(tb < 0 ? 0 : (tb > a.T ? a.T : tb));
    }
    return s;
}

// the clamped start of frame (b, t), t < T_b; 0 in the joint form
__device__ __forceinline__ int lp_start(const LpArgs& a, int b, int t) {
    if (a.K == 0) return 0;
    const int r = a.ranges[static_cast<long long>(b) * a.T + t];
    return min(max(r, 0), a.U - a.K);
}

// The row map.  Row (b, t, k) of the logits is lattice row u; real: t < T_b and u <= S_b.
struct LpRow { bool real; int u; };
__device__ __forceinline__ LpRow lp_row(const LpArgs& a, const LpSample& s, int b, int t, int k) {
    LpRow r;
    r.real = false;
    r.u = 0;
    if (t >= s.Tb) return r;
    r.u = lp_start(a, b, t) + k;
    r.real = r.u <= s.Sb;
    return r;
}

// The slot k of frame (b, t) that covers lattice row u, or -1: no real row covers (t, u).
__device__ __forceinline__ int lp_slot(const LpArgs& a, const LpSample& s, int b, int t, int u) {
    if (t >= s.Tb || u > s.Sb) return -1;
    const int k = u - lp_start(a, b, t);
    return (k >= 0 && k < a.Kp) ? k : -1;
}

// The backward's arithmetic.  Its error bound charges exp(z - lse) with ONE rounding of the exponent, which the native
// v_exp_f32(x * log2(e)) of fast_exp cannot keep (the product and the rounded constant are two more): the library's exp,
// within one ulp of the rounded difference.
__device__ __forceinline__ float lp_exp(float x) { return expf(x); }
__device__ __forceinline__ double lp_exp(double x) { return exp(x); }
// a + b and what the rounding dropped (Knuth's TwoSum; never contracted)
template <typename C> __device__ __forceinline__ C lp_two_sum(C a, C b, C& err) {
#pragma clang fp contract(off)
    const C s = a + b;
    const C bb = s - a;
    err = (a - (s - bb)) + (b - bb);
    return s;
}
// gl - gx - gy to within one rounding of the RESULT: the incoming gradients may cancel
template <typename C> __device__ __forceinline__ C lp_coef(C gl, C gx, C gy) {
    C e1, e2;
    const C s = lp_two_sum(gl, -gx, e1);
    const C r = lp_two_sum(s, -gy, e2);
    return r + (e1 + e2);
}
// gx + gy + coef * ex to within one rounding of the result: the column of a symbol that equals the blank
template <typename C> __device__ __forceinline__ C lp_both(C gx, C gy, C coef, C ex) {
    const C p = coef * ex;
    const C pe = fma(coef, ex, -p);
    C e1, e2;
    const C s1 = lp_two_sum(gx, gy, e1);
    const C s2 = lp_two_sum(s1, p, e2);
    return s2 + ((e1 + e2) + pe);
}

template <typename C> __device__ __forceinline__ C lp_nan();
template <> __device__ __forceinline__ float lp_nan<float>() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ double lp_nan<double>() { return __builtin_nan(""); }

// ------------------------------------------------------------------------------------------
// Forward, stage 1.  G lanes per row, 256 / G rows per block, grid = ceil(rows * G / 256) with rows = B T K'.  The row
// reduction is row_lse (rnnt_row_lse.h).  A row that is all -inf, or holds a NaN or +inf, gets NaN.
template <typename Tag, int G>
__global__ __launch_bounds__(256) void logprobs_lse_kernel(const typename Tag::store* __restrict__ logits,
                                                           typename Tag::comp* __restrict__ lse, LpArgs a, long long rows) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const int gl = threadIdx.x & (G - 1);
    const long long q = static_cast<long long>(blockIdx.x) * (256 / G) + static_cast<int>(threadIdx.x) / G;
    if (q >= rows) return;                                                        // (whole groups leave together)
    const int k = static_cast<int>(q % a.Kp);
    const long long bt = q / a.Kp;
    const int t = static_cast<int>(bt % a.T), b = static_cast<int>(bt / a.T);
    const LpSample sm = lp_sample(a, b);
    if (!lp_row(a, sm, b, t, k).real) {                                           // never read
        if (gl == 0) lse[q] = C(0);
        return;
    }
    const St* row = logits + q * a.C;
    C logZ = row_lse<Tag, G>(row, a.C, gl).log();
    if (non_finite(logZ)) logZ = lp_nan<C>();
    if (gl == 0) lse[q] = logZ;
}

// ------------------------------------------------------------------------------------------
// Forward, stage 2.  Element i of the space (B, U, TX), TX = T + 1 - mod, t fastest; grid-stride, block = 256.  t < T: py[b, u, t];
// u < S: px[b, u, t] (column T of the regular type: -inf).  Every element of px and py is written.
template <typename Tag>
__global__ __launch_bounds__(256) void logprobs_edges_kernel(const typename Tag::store* __restrict__ logits,
                                                             const typename Tag::comp* __restrict__ lse,
                                                             typename Tag::comp* __restrict__ px,
                                                             typename Tag::comp* __restrict__ py, LpArgs a) {
    using C = typename Tag::comp;
    const int S = a.U - 1, TX = a.T + 1 - a.mod;
    const long long total = static_cast<long long>(a.B) * a.U * TX;
    for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < total;
         i += static_cast<long long>(gridDim.x) * 256) {
        const int t = static_cast<int>(i % TX);
        const long long bu = i / TX;
        const int u = static_cast<int>(bu % a.U), b = static_cast<int>(bu / a.U);
        const LpSample sm = lp_sample(a, b);
        const int k = t < a.T ? lp_slot(a, sm, b, t, u) : -1;
        C vy = neg_inf<C>(), vx = neg_inf<C>();
        if (k >= 0) {
            const long long row = (static_cast<long long>(b) * a.T + t) * a.Kp + k;
            const typename Tag::store* z = logits + row * a.C;
            const C l = lse[row];
            vy = load1<Tag>(z + a.blank) - l;
            if (u < sm.Sb) {
                const int y = a.symbols[static_cast<long long>(b) * S + u];
                if (y >= 0 && y < a.C) vx = load1<Tag>(z + y) - l;
            }
        }
        if (t < a.T) py[bu * a.T + t] = vy;
        if (u < S) px[(static_cast<long long>(b) * S + u) * TX + t] = vx;
    }
}

// ------------------------------------------------------------------------------------------
// Backward.  blockDim = (PX, RY): RY rows per block step, PX threads over the P accesses of a row (P = C / V packets, or C
// elements); grid-stride over the B T K' rows.  dz[c] = gx [c == y_u] + gy [c == blank] + (gl - gx - gy) exp(z[c] - lse), in
// the lattice type, one rounding to the logits' type; rows that are not real are written as exact zeros and never read.
// logits and dlogits may be the same tensor (NOT __restrict__): an element is read and written by one thread.
template <typename Tag, bool VEC>
__global__ __launch_bounds__(256) void logprobs_grad_kernel(const typename Tag::store* logits, typename Tag::store* dlogits,
                                                            const typename Tag::comp* __restrict__ lse,
                                                            const typename Tag::comp* __restrict__ px_grad,
                                                            const typename Tag::comp* __restrict__ py_grad,
                                                            const typename Tag::comp* __restrict__ lse_grad, LpArgs a,
                                                            long long rows, int P) {
    using C = typename Tag::comp;
    constexpr int V = VEC ? Vec<Tag>::N : 1;
    const int S = a.U - 1, TX = a.T + 1 - a.mod;
    for (long long q = static_cast<long long>(blockIdx.x) * blockDim.y + threadIdx.y; q < rows;
         q += static_cast<long long>(gridDim.x) * blockDim.y) {
        const int k = static_cast<int>(q % a.Kp);
        const long long bt = q / a.Kp;
        const int t = static_cast<int>(bt % a.T), b = static_cast<int>(bt / a.T);
        const LpSample sm = lp_sample(a, b);
        const LpRow r = lp_row(a, sm, b, t, k);
        const typename Tag::store* z = logits + q * a.C;
        typename Tag::store* d = dlogits + q * a.C;
        C v[V];
        if (!r.real) {
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = C(0);
            for (int p = threadIdx.x; p < P; p += blockDim.x) {
                if constexpr (VEC) store_packet<true>(reinterpret_cast<u32x4*>(d) + p, pack<Tag>(v));
                else store1<Tag>(d + p, v[0]);
            }
            continue;
        }
        // the row's record
        const C l = lse[q];
        const C gy = py_grad[(static_cast<long long>(b) * a.U + r.u) * a.T + t];
        const C gl = lse_grad != nullptr ? lse_grad[q] : C(0);
        C gx = C(0);
        int y = -1;
        if (r.u < sm.Sb) {
            y = a.symbols[static_cast<long long>(b) * S + r.u];
            if (y >= 0 && y < a.C) gx = px_grad[(static_cast<long long>(b) * S + r.u) * TX + t];
            else y = -1;
        }
        const C coef = lp_coef(gl, gx, gy);
        for (int p = threadIdx.x; p < P; p += blockDim.x) {
            const int c0 = p * V;
            if constexpr (VEC) unpack<Tag>(load_packet<true>(reinterpret_cast<const u32x4*>(z) + p), v);
            else v[0] = load1<Tag>(z + p);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const C ex = lp_exp(v[e] - l);
                const bool is_y = c0 + e == y, is_b = c0 + e == a.blank;
                C g = coef * ex;
                if (is_y && is_b) g = lp_both(gx, gy, coef, ex);
                else if (is_y) g += gx;
                else if (is_b) g += gy;
                v[e] = g;
            }
            if constexpr (VEC) store_packet<true>(reinterpret_cast<u32x4*>(d) + p, pack<Tag>(v));
            else store1<Tag>(d + p, v[0]);
        }
    }
}

}  // namespace rnnt
