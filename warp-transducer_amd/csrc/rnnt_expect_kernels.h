// rnnt_expect_kernels.h -- the gfx950 kernels of the expected path cost over edge log-probabilities (include/rnnt_expect.h):
// the expectation semiring on the px / py lattice.  The schedule of kernels 1 and 2 -- a block per sample, a thread per
// lattice row, chunked prefetch, the neighbour's hand-over through DPP and LDS words -- is pxpy_sweep's (rnnt_pxpy.h);
// what is here is each kernel's semiring, its stores and its fills.
//
//   1 expect_fwd_kernel       the sweep over px / py / cx / cy [b, s, :], kExChunk steps ahead of use.  The node's pair
//                             (a, A) and the stay candidate (a + py, A + cy) are fp64 registers; the emit candidate
//                             (a + px, A + cx) is the pair handed to the row above.  Per node: one exp and one log1p --
//                             logaddexp with the share from the same exponential -- and the convex combination, by select
//                             where a candidate is -inf.  Every node's pair goes to `nodes`; the block then writes
//                             (-inf, 0) outside the rectangle.
//   2 expect_bwd_kernel       the sweep in reverse: the thread of row r hands (bt, Bc) of its node to the row below, reads
//                             nodes[u] a chunk (kExChunkBwd steps) ahead with the rows and stores the gradients of u's two
//                             out-edges as it goes: no second table, no element-wise pass over a table.  occ_e =
//                             exp(a[u] + bt[u] - score) times the edge's share of bt[u]: two exponentials and one log1p per
//                             node.  The block then writes the zeros outside the rectangle's edges.
//   3 expect_restore_kernel   the host-scores entry parks (score, expect) of sample b in nodes[b, 0, 0] -- the one array
//                             there is -- and this puts the node's own pair back behind the copies.
//
// DESIGN.md 8p lists the modified type's 16-byte packets as open.
#pragma once

#include "rnnt_pxpy.h"                 // PxRect / px_rect, pxpy_sweep; through rnnt_kernels.h cost_invalid, load1 / store1

namespace rnnt {

constexpr int kExChunk = 4;             // steps per prefetched chunk of the forward sweep
constexpr int kExChunkBwd = 2;          // ... of the backward sweep (it prefetches the node pairs as well)
// 8-byte storage: half of either, the registers of 1024 threads (128 each) without a spill
template <typename Tag> constexpr int ex_chunk(int steps) { return sizeof(typename Tag::store) == 8 ? steps / 2 : steps; }
constexpr int kExWaveMaxU = 64;         // S + 1 up to here: one wavefront, no LDS exchange

// (a, A) of a node from its two in-candidates (forward), or (bt, Bc) from its two out-candidates (backward): the log of
// the sum of the weights, the convex combination of the costs and the share of candidate x.  A candidate of -inf is selected
// out: its cost is never looked at.  Both -inf: (-inf, 0), share 0.
struct ExNode { double w, c, share; };
__device__ __forceinline__ ExNode ex_combine(double x, double xc, double y, double yc) {
    const double NEG = -__builtin_huge_val();
    const bool xmax = x > y;
    const double hi = xmax ? x : y, lo = xmax ? y : x;
    if (!(hi > NEG)) return {hi == hi ? NEG : hi, hi == hi ? 0.0 : hi, 0.0};     // no candidate (NaN weights: NaN)
    if (!(lo > NEG) && lo == lo) return {hi, xmax ? xc : yc, xmax ? 1.0 : 0.0};  // one candidate
    const double e = exp(lo - hi);                                               // in [0, 1]
    const double slo = e / (1.0 + e);                                            // the smaller candidate's share
    const double r = xmax ? 1.0 - slo : slo;
    return {hi + log1p(e), r * xc + (1.0 - r) * yc, r};
}

// grid = B, block = 64 (MULTI == false: S + 1 <= kExWaveMaxU) or 64 * ceil((S + 1) / 64) <= 1024.
// scores[b * stride], expect[b * stride] (the host-scores entry: both inside nodes[b, 0, 0], written LAST).
template <typename Tag, bool MOD, bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void expect_fwd_kernel(
        const typename Tag::store* __restrict__ px, const typename Tag::store* __restrict__ py,
        const typename Tag::store* __restrict__ cx, const typename Tag::store* __restrict__ cy,
        const long long* __restrict__ boundary, double* scores, double* expect, long long stride, double* nodes, int S,
        int T) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    constexpr int CH = ex_chunk<Tag>(kExChunk);
    __shared__ double edge[2][16][2];
    __shared__ double sh_score, sh_expect;
    __shared__ int sh_bad, sh_badc;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nthreads = static_cast<int>(blockDim.x);
    const int TX = MOD ? T : T + 1, U = S + 1, T1 = T + 1;
    const PxRect r = px_rect(boundary, b, S, T);
    const int s0 = r.s0, t0 = r.t0, Sr = r.Sr, Tr = r.Tr;
    const double NEG = -__builtin_huge_val(), INF = __builtin_huge_val();
    double2* nd = reinterpret_cast<double2*>(nodes) + static_cast<size_t>(b) * U * T1;
    if (tid == 0) { sh_bad = 0; sh_badc = 0; sh_score = NEG; sh_expect = 0.0; }
    __syncthreads();

    if (r.ok) {
        const int ls = tid;
        const bool hasy = ls <= Sr, hasx = ls < Sr;
        const size_t s = static_cast<size_t>(s0 + (hasy ? ls : 0));
        const size_t ox = (static_cast<size_t>(b) * S + (hasx ? s : 0)) * TX + t0;       // (never dereferenced unless hasx)
        const size_t oy = (static_cast<size_t>(b) * U + s) * T + t0;
        const St* const rx[2] = {px + ox, cx + ox};
        const St* const ry[2] = {py + oy, cy + oy};
        double2* rn = nd + s * T1 + t0;
        double stay_w = NEG, stay_c = 0.0;                           // the stay candidate; the emit one is the hand-over
        bool bad = false, badc = false;
        const double none[2] = {NEG, 0.0};                           // row -1 is no row
        pxpy_sweep<Tag, MOD, MULTI, false, 2, 2, CH, PxNoX>(
            rx, ry, ls, Sr, Tr, edge, none, [](int, bool) { return PxNoX{}; },
            [&](int j, bool act, bool ex, bool ey, const double (&left)[2], const C (&wxs)[2], const C (&wys)[2], PxNoX,
                double (&emit)[2]) {
                ExNode n = ex_combine(left[0], left[1], stay_w, stay_c);
                if (ls == 0 && j == 0) { n.w = 0.0; n.c = 0.0; }     // the source (both candidates are -inf there)
                const double wx = static_cast<double>(wxs[0]), wy = static_cast<double>(wys[0]);
                const double kx = static_cast<double>(wxs[1]), ky = static_cast<double>(wys[1]);
                bad = bad || (ex && !(wx < INF)) || (ey && !(wy < INF));           // NaN or +inf on an edge of the rectangle
                emit[0] = ex ? n.w + wx : NEG;
                stay_w = ey ? n.w + wy : NEG;
                // a non-finite cost on a reachable edge of finite weight
                badc = badc || (emit[0] > NEG && !(__builtin_fabs(kx) < INF)) || (stay_w > NEG && !(__builtin_fabs(ky) < INF));
                emit[1] = emit[0] > NEG ? n.c + kx : 0.0;
                stay_c = stay_w > NEG ? n.c + ky : 0.0;
                if (act) {
                    rn[j] = make_double2(n.w, n.c);
                    if (ls == Sr && j == Tr) { sh_score = n.w; sh_expect = n.c; }
                }
            });
        if (bad) sh_bad = 1;                                         // (several bad edges race: any store will do)
        if (badc) sh_badc = 1;
    }
    __threadfence_block();
    __syncthreads();

    // ---- the nodes outside the rectangle, then the two scalars (LAST: the host-scores entry parks them in nodes[b, 0, 0])
    for (size_t i = tid; i < static_cast<size_t>(U) * T1; i += nthreads) {
        const int s = static_cast<int>(i / T1), t = static_cast<int>(i - static_cast<size_t>(s) * T1);
        if (!(r.ok && s >= s0 && s <= s0 + Sr && t >= t0 && t <= t0 + Tr)) nd[i] = make_double2(NEG, 0.0);
    }
    __syncthreads();
    if (tid == 0) {
        const double qnan = __builtin_nan("");
        const double sc = !r.ok ? cost_invalid<double>() : (sh_bad != 0 ? qnan : sh_score);
        const double ec = !r.ok ? 0.0 : ((sh_bad != 0 || sh_badc != 0) ? qnan : (sc > NEG ? sh_expect : 0.0));
        scores[static_cast<size_t>(b) * stride] = sc;
        expect[static_cast<size_t>(b) * stride] = ec;
    }
}

// grid = B, block as expect_fwd_kernel's.  g_expect / g_score: B doubles each, or NULL for 1 / 0.  The pair of the
// rectangle's source is (0, 0) by definition and is not read from `nodes` (the host-scores entry parks the scalars in
// nodes[b, 0, 0], which is that source or a node outside the rectangle).
template <typename Tag, bool MOD, bool MULTI, bool WITH_COST_GRADS>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void expect_bwd_kernel(
        const typename Tag::store* __restrict__ px, const typename Tag::store* __restrict__ py,
        const typename Tag::store* __restrict__ cx, const typename Tag::store* __restrict__ cy,
        const long long* __restrict__ boundary, const double* __restrict__ nodes, const double* __restrict__ scores,
        const double* __restrict__ expect, long long stride, const double* __restrict__ g_expect,
        const double* __restrict__ g_score, typename Tag::store* __restrict__ px_grad,
        typename Tag::store* __restrict__ py_grad, typename Tag::store* __restrict__ cx_grad,
        typename Tag::store* __restrict__ cy_grad, int S, int T) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    constexpr int CH = ex_chunk<Tag>(kExChunkBwd);
    __shared__ double edge[2][16][2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nthreads = static_cast<int>(blockDim.x);
    const int TX = MOD ? T : T + 1, U = S + 1, T1 = T + 1;
    const PxRect r = px_rect(boundary, b, S, T);
    const int s0 = r.s0, t0 = r.t0, Sr = r.Sr, Tr = r.Tr;
    const double NEG = -__builtin_huge_val();
    const double sc = scores[static_cast<size_t>(b) * stride], ec = expect[static_cast<size_t>(b) * stride];
    const bool nan = r.ok && sc != sc, path = r.ok && sc - sc == 0.0;          // (block-uniform)
    const double ge = g_expect != nullptr ? g_expect[b] : 1.0, gs = g_score != nullptr ? g_score[b] : 0.0;
    const int lastx = MOD ? Tr - 1 : Tr;
    const size_t bx0 = static_cast<size_t>(b) * S * TX, by0 = static_cast<size_t>(b) * U * T;

    if (path) {
        const int ls = tid;
        const bool hasy = ls <= Sr, hasx = ls < Sr;
        const size_t s = static_cast<size_t>(s0 + (hasy ? ls : 0));
        const size_t ox = bx0 + (hasx ? s : 0) * TX + t0;                      // (never dereferenced unless hasx)
        const size_t oy = by0 + s * T + t0;
        const St* const rx[2] = {px + ox, cx + ox};
        const St* const ry[2] = {py + oy, cy + oy};
        const double2* rn = reinterpret_cast<const double2*>(nodes) + (static_cast<size_t>(b) * U + s) * T1 + t0;
        const double none[2] = {NEG, 0.0};                           // the row past the last is no row
        // the hand-over `own` is (bt, Bc) of the row's node; x: the node's forward pair, read a chunk ahead with the edges
        pxpy_sweep<Tag, MOD, MULTI, true, 2, 2, CH, double2>(
            rx, ry, ls, Sr, Tr, edge, none,
            [&](int j, bool in) { return (in && !(ls == 0 && j == 0)) ? rn[j] : make_double2(0.0, 0.0); },   // the source: (0, 0)
            [&](int j, bool act, bool ex, bool ey, const double (&right)[2], const C (&wxs)[2], const C (&wys)[2],
                const double2& nn, double (&own)[2]) {
                const double kx = static_cast<double>(wxs[1]), ky = static_cast<double>(wys[1]);
                const double x = ex ? static_cast<double>(wxs[0]) + right[0] : NEG;
                const double y = ey ? static_cast<double>(wys[0]) + own[0] : NEG;
                const double xc = x > NEG ? kx + right[1] : 0.0, yc = y > NEG ? ky + own[1] : 0.0;
                ExNode n = ex_combine(x, xc, y, yc);
                if (ls == Sr && j == Tr) { n.w = 0.0; n.c = 0.0; }   // the sink (no out-edge: both candidates are -inf)
                own[0] = act ? n.w : NEG;
                own[1] = act ? n.c : 0.0;
                if (act) {
                    const double a = nn.x, A = nn.y;
                    const double occ = exp(a + n.w - sc);            // the node's occupation; -inf - ... = -inf: 0
                    const double occx = x > NEG ? occ * n.share : 0.0, occy = y > NEG ? occ * (1.0 - n.share) : 0.0;
                    if (ex) {
                        const double g = occx > 0.0 ? ge * occx * (A + xc - ec) + gs * occx : 0.0;
                        store1<Tag>(px_grad + ox + j, static_cast<C>(g));
                        if (WITH_COST_GRADS) store1<Tag>(cx_grad + ox + j, static_cast<C>(occx > 0.0 ? ge * occx : 0.0));
                    }
                    if (ey) {
                        const double g = occy > 0.0 ? ge * occy * (A + yc - ec) + gs * occy : 0.0;
                        store1<Tag>(py_grad + oy + j, static_cast<C>(g));
                        if (WITH_COST_GRADS) store1<Tag>(cy_grad + oy + j, static_cast<C>(occy > 0.0 ? ge * occy : 0.0));
                    }
                }
            });
    }

    // ---- everything the sweep did not write: zeros outside the rectangle's edges; without a path zeros (NaN score: NaN) inside
    const C fill = nan ? static_cast<C>(__builtin_nan("")) : C(0);
    for (size_t i = tid; i < static_cast<size_t>(S) * TX; i += nthreads) {
        const int s = static_cast<int>(i / TX), t = static_cast<int>(i - static_cast<size_t>(s) * TX);
        const bool in = r.ok && s >= s0 && s < s0 + Sr && t >= t0 && t <= t0 + lastx;
        if (in && path) continue;
        store1<Tag>(px_grad + bx0 + i, in ? fill : C(0));
        if (WITH_COST_GRADS) store1<Tag>(cx_grad + bx0 + i, in ? fill : C(0));
    }
    for (size_t i = tid; i < static_cast<size_t>(U) * T; i += nthreads) {
        const int s = static_cast<int>(i / T), t = static_cast<int>(i - static_cast<size_t>(s) * T);
        const bool in = r.ok && s >= s0 && s <= s0 + Sr && t >= t0 && t < t0 + Tr;
        if (in && path) continue;
        store1<Tag>(py_grad + by0 + i, in ? fill : C(0));
        if (WITH_COST_GRADS) store1<Tag>(cy_grad + by0 + i, in ? fill : C(0));
    }
}

// grid = ceil(B / 256), block = 256: nodes[b, 0, 0] back to its own pair behind the host-scores entry's copies.
template <typename Tag>
__global__ __launch_bounds__(256) void expect_restore_kernel(const long long* __restrict__ boundary, double* nodes, int S,
                                                             int T, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const PxRect r = px_rect(boundary, b, S, T);
    double2* nd = reinterpret_cast<double2*>(nodes) + static_cast<size_t>(b) * (S + 1) * (T + 1);
    nd[0] = make_double2((r.ok && r.s0 == 0 && r.t0 == 0) ? 0.0 : -__builtin_huge_val(), 0.0);
}

}  // namespace rnnt
