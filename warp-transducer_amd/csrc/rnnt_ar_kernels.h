// rnnt_ar_kernels.h -- the gfx950 kernels of the alignment-restricted RNN-T loss (include/rnnt_ar.h).
//
// Logits (N, maxT, maxU, A), one softmax per row.  The standard RNN-T lattice -- a label edge stays in its frame,
// (t, u) -> (t, u + 1) -- but label u may be emitted only at frames lo_u <= t <= hi_u.  With e the prefix maximum of lo and l
// the suffix minimum of hi (the header), node (t, u) lies on a path iff e_u <= t <= l_u: the BAND.  Five stages:
//   0 ar_bounds_kernel         a wavefront per sample: e_u, l_u (u <= L_b) and the feasibility flag (e_{u+1} <= l_u for all u)
//   1 ar_stats_kernel          online max / sum-exp of every BAND row, gather of the blank and label logits; one cell record
//                              per row.  In-lattice rows outside the band get a "no edge" record without their logits being
//                              read; inside the band the label edge is no edge before e_{u+1} (that is: outside [lo_u, hi_u])
//                              and the blank edge is no edge when it would leave the band (t + 1 > l_u, but for the final
//                              node): no probability mass ever leaves the band, so the lattice needs no band test
//   2 ar_lattice_wave_kernel   maxU <= 64: one wavefront per (sample, direction), a lane per u, over anti-diagonals: step d
//                              works on t = d - u, alpha / beta in registers, the neighbour's value through one DPP wave
//                              shift per diagonal; no LDS, no barrier
//     ar_lattice_block_kernel  any maxU: one block per (sample, direction), threads striding over u, predecessors read from
//                              the global arrays the block wrote, one barrier per diagonal
//   3 ar_coef_kernel           a thread per row: the posteriors of the row's two out-edges -> the gradient record, written
//                              over the cell record of stage 1; kPadded on padding AND on out-of-band rows
//   4 mblank_grad_kernel / mblank_grad_elem_kernel (rnnt_mblank_kernels.h) with K = 0: the record is the multi-blank one
//
// Lattice values are base-2 logs.  The value stored for a cell of diagonal d = t + u is RELATIVE to an fp64 offset off[d]
// (offa / offb, maxT + maxU per sample: diagonals 0 .. T_b + L_b - 1 and the terminal one), so stored values stay within a
// few edge weights of zero and keep fp32's relative precision however long the utterance.
#pragma once

#include "rnnt_mono_kernels.h"         // mono_lse2, mono_shift, MonoPair, mono_close; through it the record format and stage 4

namespace rnnt {

constexpr int kArRec = 4;               // == mblank_rec_stride(0)
constexpr int kArChunk = 8;             // diagonals per chunk of the wave form (prefetch distance, re-centring period)
constexpr int kArWaveMaxU = 64;         // the release rule: maxU <= 64 -> wave form, else block form
constexpr int kArMaxU = 4096;           // the bounds kernel: at most 64 labels per lane

// Per cell (b, t, u) of the workspace table, kArRec values of the lattice type:
//   after stage 1  [lp_blank, lp_label, logZ, -]      (lp: base 2; logZ: natural log; -inf = no edge)
//   after stage 3  [x, cb, cl, label]                 x = ln(cb + cl) - logZ
// label: the row's label index, -1 without a label edge (u = L_b), kPadded outside the band.
__host__ __device__ inline int ar_offsets(int maxT, int maxU) { return maxT + maxU; }

// ------------------------------------------------------------------------------------------
// Stage 0.  grid = N slice, block = 64 = one wavefront.  Lane j owns the labels [j c, (j + 1) c), c = ceil(maxU / 64) <= 64:
// a serial scan of its own, an exclusive scan over the lanes, a second serial pass that writes.  e and l: (N, maxU) int32,
// written for u <= L_b; ok[b]: 1 when the sample has a path.  Nothing else of these arrays is read later.  (L: the lattice
// type of the code object that holds the kernel; the work itself is integer.)
template <typename L>
__global__ __launch_bounds__(64) void ar_bounds_kernel(
        const int* __restrict__ lo, const int* __restrict__ hi, const int* __restrict__ xlen, const int* __restrict__ ylen,
        int* __restrict__ e, int* __restrict__ el, int* __restrict__ ok, int maxT, int maxU, int b0) {
    const int b = b0 + blockIdx.x, lane = threadIdx.x;
    int T, Lb;
    if (!tdt_lens(xlen, ylen, b, maxT, maxU, T, Lb)) return;         // (no later stage looks at this sample's bounds)
    const int c = (maxU + 63) / 64;
    const int u0 = lane * c, u1 = u0 + c < Lb ? u0 + c : Lb;         // labels [u0, u1) of this lane (none: u0 >= u1)
    const int* plo = lo + static_cast<size_t>(b) * (maxU - 1);
    const int* phi = hi + static_cast<size_t>(b) * (maxU - 1);
    int* pe = e + static_cast<size_t>(b) * maxU;
    int* pl = el + static_cast<size_t>(b) * maxU;
    int mx = 0, mn = T - 1;                                          // (the identities: e_0 = 0, l_{L_b} = T_b - 1)
    for (int u = u0; u < u1; ++u) { mx = max(mx, plo[u]); mn = min(mn, phi[u]); }
    // inclusive scans over the lanes: the maximum of lanes <= this one, the minimum of lanes >= this one
    int imx = mx, imn = mn;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(imx, o, kWave), z = __shfl_down(imn, o, kWave);
        if (lane >= o) imx = max(imx, a);
        if (lane + o < 64) imn = min(imn, z);
    }
    int ex = __shfl_up(imx, 1, kWave), sn = __shfl_down(imn, 1, kWave);
    if (lane == 0) ex = 0;
    if (lane == 63) sn = T - 1;
    // e_u for u in [u0, u1]: e_{u0} = ex, e_{u+1} = max(e_u, lo_u); the lane that holds L_b writes e_{L_b} too
    bool good = true;
    int cur = ex;
    for (int u = u0; u < u1; ++u) { pe[u] = cur; cur = max(cur, plo[u]); }
    if (u0 <= Lb && Lb < u0 + c) pe[Lb] = cur;                       // (u1 == L_b here; lane 0 when L_b = 0)
    // l_u for u in [u0, u1): l_u = min(l_{u+1}, hi_u), from the top; l_{u1} = sn
    int nxt = sn;
    for (int u = u1 - 1; u >= u0; --u) { nxt = min(nxt, phi[u]); pl[u] = nxt; }
    if (u0 <= Lb && Lb < u0 + c) pl[Lb] = T - 1;
    // a path: e_{u+1} <= l_u for every u < L_b (l_u: this lane's own stores of the pass above)
    cur = ex;
    for (int u = u0; u < u1; ++u) {
        cur = max(cur, plo[u]);                                      // e_{u+1}
        good = good && cur <= pl[u];
    }
    const bool all = __all(good);
    if (lane == 0) ok[b] = all ? 1 : 0;
}

// (t, u) of a feasible sample lies inside the band
__device__ __forceinline__ bool ar_live(int t, int eu, int lu) { return eu <= t && t <= lu; }

// ------------------------------------------------------------------------------------------
// Stage 1.  G lanes per row (G = 4, 16, 64), 256 / G rows per block.  grid = (ceil(maxT * maxU * G / 256), N slice): the
// launch covers every row and the groups of rows outside the band leave after reading the sample's two bounds; band rows
// go through row_lse (rnnt_row_lse.h).
template <typename Tag, int G>
__global__ __launch_bounds__(256) void ar_stats_kernel(
        const typename Tag::store* __restrict__ acts, const int* __restrict__ labels, const int* __restrict__ xlen,
        const int* __restrict__ ylen, const int* __restrict__ e, const int* __restrict__ l, const int* __restrict__ okf,
        typename Tag::comp* __restrict__ tab, int maxT, int maxU, int A, int blank, int b0, int* __restrict__ poison) {
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
    C* rec = tab + tdt_cell(b, t, u, maxT, maxU) * kArRec;
    const size_t bu = static_cast<size_t>(b) * maxU + u;
    const int lu = l[bu];
    if (okf[b] == 0 || !ar_live(t, e[bu], lu)) {                                  // outside the band: no edge, never read
        if (gl == 0) { rec[0] = neg_inf<C>(); rec[1] = neg_inf<C>(); rec[2] = C(0); }
        return;
    }
    const bool has_lab = u < Lb && e[bu + 1] <= t;                                // (inside the band: lo_u <= t <= hi_u)
    const int lab = u < Lb ? row_label(labels, b, u, maxU, A) : blank;
    const St* row = acts + tdt_cell(b, t, u, maxT, maxU) * A;
    const C xb = load1<Tag>(row + blank);
    const C xl = load1<Tag>(row + lab);
    const C logZ = row_lse<Tag, G>(row, A, gl).log();
    if (gl != 0) return;
    // the blank edge (t, u) -> (t + 1, u) stays inside the band iff t + 1 <= l_u; the final blank leaves (T_b - 1, L_b)
    const bool has_blank = t + 1 <= lu || (t == T - 1 && u == Lb);
    rec[0] = has_blank ? (xb - logZ) * C(kLog2e) : neg_inf<C>();
    rec[1] = has_lab ? (xl - logZ) * C(kLog2e) : neg_inf<C>();
    rec[2] = logZ;
    if (non_finite(logZ)) poison[b] = 1;                                          // (several bad rows race: any store will do)
}

// ------------------------------------------------------------------------------------------
// Stage 2.  Both forms: grid = (N slice, 2), blockIdx.y = 0 alpha, 1 beta.  With D = T_b + L_b diagonals d = t + u:
//   alpha(0, 0) = 0;  alpha(t, u) = lse(alpha(t - 1, u) + lp_blank(t - 1, u), alpha(t, u - 1) + lp_label(t, u - 1))
//   beta(t, u) = lse(lp_blank(t, u) + beta(t + 1, u), lp_label(t, u) + beta(t, u + 1)),  beta(T_b, L_b) = 0 the terminal node
// Both predecessors of a cell lie on the neighbouring diagonal.  alpha and beta are stored for the in-lattice cells, relative
// to offa[d] / offb[d]; offb[D] = 0 is the terminal node's.  The forward side closes the sample: log P = alpha(T_b, L_b),
// one more step of the recurrence (ll, base 2, absolute) and the cost -- the invalid-lengths marker, NaN for a poisoned
// sample, +inf when no path exists (the infeasible samples have no edge at all).
//
// Wave form: block = 64 = one wavefront, lane u.  Step s = 0 .. D - 1 works on diagonal d = s (alpha) or D - 1 - s (beta),
// lane u on the cell (d - u, u); a lane whose t = d - u is outside [0, T_b) takes "no edge" for that step, which both keeps
// its own value at -inf and hands -inf to its neighbour.  With w the record of the lane's cell on the step's diagonal the
// step is mono's: alpha: a <- lse(a + w.blank, shift_down(a + w.label)); beta: a <- lse(a + w.blank, shift_up(a) + w.label).
// The records of chunk j + 1 are requested before chunk j's steps; at a chunk's end the wave re-centres on its maximum.
template <typename L, bool FWD>
__device__ __forceinline__ void ar_wave_sweep(const L* __restrict__ tab, L* __restrict__ val, double* __restrict__ off,
                                              int b, int T, int Lb, int maxT, int maxU, int u, double& base, L& a) {
    using P = typename MonoPair<L>::type;
    constexpr int CH = kArChunk;
    const int D = T + Lb;
    const bool in = u <= Lb;                                         // (lanes past L_b hold -inf and touch no memory)
    const int uc = in ? u : Lb;
    const P none = {neg_inf<L>(), neg_inf<L>()};
    const auto diag = [&](int s) { return FWD ? s : D - 1 - s; };
    const auto request = [&](int s0, P (&w)[CH]) {
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            int t = diag(s0 + k < D ? s0 + k : D - 1) - uc;          // (outside the lattice: the nearest row, no branch on the load)
            t = t < 0 ? 0 : (t >= T ? T - 1 : t);
            w[k] = *reinterpret_cast<const P*>(tab + tdt_cell(b, t, uc, maxT, maxU) * kArRec);
        }
    };
    P cur[CH], nxt[CH];
    request(0, cur);
    for (int s0 = 0; s0 < D; s0 += CH) {
        request(s0 + CH, nxt);                                       // (unconditional, as mono_wave_sweep's)
        L out[CH];
        bool live[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int t = diag(s0 + k) - u;
            live[k] = in && s0 + k < D && t >= 0 && t < T;
            const P w = live[k] ? cur[k] : none;
            if (FWD) {
                out[k] = a;                                          // alpha(t, u)
                if (s0 + k < D) a = mono_lse2<L>(a + w.x, mono_shift<true>(a + w.y));
            } else {
                if (s0 + k < D) a = mono_lse2<L>(a + w.x, mono_shift<false>(a) + w.y);
                out[k] = a;                                          // beta(t, u)
            }
        }
#pragma unroll
        for (int k = 0; k < CH; ++k)
            if (live[k]) val[tdt_cell(b, diag(s0 + k) - u, u, maxT, maxU)] = out[k];
        if (u < CH && s0 + u < D) off[diag(s0 + u)] = base;          // the chunk's diagonals share one offset
        if (s0 + CH < D) {
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
__global__ __launch_bounds__(64) void ar_lattice_wave_kernel(
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
    const size_t o0 = static_cast<size_t>(b) * ar_offsets(maxT, maxU);
    double base = 0.0;
    if (fwd) {
        L a = u == 0 ? L(0) : neg_inf<L>();
        ar_wave_sweep<L, true>(tab, alpha, offa + o0, b, T, Lb, maxT, maxU, u, base, a);
        if (u == Lb) mono_close<L>(a == neg_inf<L>() ? static_cast<double>(a) : base + static_cast<double>(a), b, poison, ll, costs);
    } else {
        L a = u == Lb ? L(0) : neg_inf<L>();
        if (u == 0) offb[o0 + T + Lb] = 0.0;
        ar_wave_sweep<L, false>(tab, beta, offb + o0, b, T, Lb, maxT, maxU, u, base, a);
    }
}

// Block form: block = any multiple of 64 up to 1024.  Per diagonal every thread takes cells of it, then the block's maximum
// sets the next diagonal's offset; the partial maxima are double-buffered, so ONE barrier per diagonal orders both them and
// the diagonal's values (written to the global arrays, read back by other threads of the block in the next diagonal).
template <typename L>
__global__ __launch_bounds__(1024) void ar_lattice_block_kernel(
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
    const int D = T + Lb;
    double* off = (fwd ? offa : offb) + static_cast<size_t>(b) * ar_offsets(maxT, maxU);
    L* val = fwd ? alpha : beta;
    if (!fwd && tid == 0) off[D] = 0.0;
    double base = 0.0;                                               // off[d] of the diagonal being computed
    L rel = L(0);                                                    // off[previous diagonal of the sweep] - base
    for (int k = 0; k < D; ++k) {
        const int d = fwd ? k : D - 1 - k;
        if (tid == 0) off[d] = base;
        L tmax = neg_inf<L>();
        const int ulo = d - (T - 1) > 0 ? d - (T - 1) : 0, uhi = d < Lb ? d : Lb;
        for (int u = ulo + tid; u <= uhi; u += blockDim.x) {
            const int t = d - u;
            const size_t c = tdt_cell(b, t, u, maxT, maxU);
            L v;
            if (fwd) {
                if (d == 0) {
                    v = L(0);
                } else {                                             // blank (t - 1, u), label (t, u - 1) -> (t, u)
                    const L x = t >= 1 ? val[c - maxU] + rel + tab[(c - maxU) * kArRec] : neg_inf<L>();
                    const L y = u >= 1 ? val[c - 1] + rel + tab[(c - 1) * kArRec + 1] : neg_inf<L>();
                    v = mono_lse2<L>(x, y);
                }
            } else {
                // beta(t + 1, u): the terminal node behind (T_b - 1, L_b), no edge behind the other cells of the last frame
                const L bu = t + 1 < T ? val[c + maxU] + rel : (u == Lb ? L(0) : neg_inf<L>());
                const L bu1 = u < Lb ? val[c + 1] + rel : neg_inf<L>();
                v = mono_lse2<L>(tab[c * kArRec] + bu, tab[c * kArRec + 1] + bu1);
            }
            val[c] = v;
            tmax = vmax(tmax, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tmax = vmax(tmax, __shfl_xor(tmax, o, kWave));
        if (lane == 0) wmax[k & 1][wave] = tmax;
        __syncthreads();                                             // the diagonal's values and its partial maxima
        L M = wmax[k & 1][0];
        for (int w = 1; w < nw; ++w) M = vmax(M, wmax[k & 1][w]);
        const double prev = base;
        if (M - M == L(0)) base += static_cast<double>(M);           // (a diagonal without a finite value keeps the offset)
        rel = static_cast<L>(prev - base);
    }
    if (!fwd || tid != 0) return;
    // log P = alpha(T_b - 1, L_b) + the final blank, behind the last barrier
    const size_t c = tdt_cell(b, T - 1, Lb, maxT, maxU);
    const L v = val[c] + tab[c * kArRec];
    mono_close<L>(v == neg_inf<L>() ? static_cast<double>(v) : off[D - 1] + static_cast<double>(v), b, poison, ll, costs);
}

// ------------------------------------------------------------------------------------------
// Stage 3.  A thread per row: grid = (ceil(maxT * maxU / 256), N slice), block = 256.
//   cb = 2^(alpha(t, u) + lp_blank + beta(t + 1, u) - log P),   cl = the same with lp_label and beta(t, u + 1),
// the fp64 offsets summed first (both successors lie on diagonal t + u + 1); beta(T_b, L_b) = 0 is the terminal node.
// Padding rows, rows outside the band and every row of a sample whose lengths do not fit get kPadded (the gradient stream
// zero-fills them without reading their logits); a poisoned sample or one without a path gets NaN records on every
// in-lattice row.
template <typename L>
__global__ __launch_bounds__(256) void ar_coef_kernel(
        L* tab, const L* __restrict__ alpha, const L* __restrict__ beta, const double* __restrict__ offa,
        const double* __restrict__ offb, const double* __restrict__ ll, const int* __restrict__ xlen,
        const int* __restrict__ ylen, const int* __restrict__ labels, const int* __restrict__ e, const int* __restrict__ l,
        const int* __restrict__ poison, int maxT, int maxU, int A, int b0) {
    const int b = b0 + blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= maxT * maxU) return;
    const int t = q / maxU, u = q - t * maxU;
    const size_t c = tdt_cell(b, t, u, maxT, maxU);
    L* r = tab + c * kArRec;
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
    const size_t bu = static_cast<size_t>(b) * maxU + u;             // (log P is finite: the sample has a path)
    if (!ar_live(t, e[bu], l[bu])) {
        r[3] = static_cast<L>(kPadded);
        return;
    }
    const size_t o0 = static_cast<size_t>(b) * ar_offsets(maxT, maxU);
    const L o = static_cast<L>(offa[o0 + t + u] + offb[o0 + t + u + 1] - lp);
    const L a = alpha[c] + o;
    const L lb = r[0], ltok = r[1], lz = r[2];
    const L bt = t + 1 < T ? beta[c + maxU] : (u == Lb ? L(0) : neg_inf<L>());
    const L bl = u < Lb ? beta[c + 1] : neg_inf<L>();
    const L cb = fast_exp2(a + lb + bt);
    const L cl = u < Lb ? fast_exp2(a + ltok + bl) : L(0);
    r[0] = acc_log(cb + cl) - lz;
    r[1] = cb;
    r[2] = cl;
    r[3] = static_cast<L>(lab);
}

}  // namespace rnnt
