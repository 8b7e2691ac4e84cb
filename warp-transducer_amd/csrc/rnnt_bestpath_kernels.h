// rnnt_bestpath_kernels.h -- the gfx950 kernels of the best path over edge log-probabilities (include/rnnt_bestpath.h).
//
//   1 bestpath_sweep_kernel   one block per sample.  SWEEP: the max-plus recursion on the row-sweep schedule rnnt_pxpy.h
//                             describes, with a thread per K consecutive lattice rows (row = s - s0) and chunks of
//                             kBpChunk (K = 1) or kBpChunkWide steps.  p, the emit candidate p + px and the stay candidate
//                             p + py are fp64 registers; the emit candidate of the thread's LAST row is the value handed
//                             to the next thread.  A thread collects the decision bits of a row 64 frames at a time in a
//                             register and stores whole words of `back`: no ballot, no atomics, one layout for both types.
//                             TRACEBACK, same launch: the block zeroes the words of `back` outside the rectangle and
//                             frames outside [s0, s1), stages the rectangle's words into LDS a range of rows at a time, and
//                             thread 0 walks from (s1, t1) to row s0.  The score leaves the block LAST (the host-scores
//                             entry parks it in a word of `back` and runs the launch a second time to restore the word).
//   2 bestpath_edges_kernel   element-wise over the coordinates (b, s, t) of px_path / py_path, t fastest: reads frames,
//                             the score and the boundary (block-uniform) and stores both indicators coalesced along t.
//
// The sweep is HAND-WRITTEN here, not a call of pxpy_sweep.  A port of pxpy_sweep with a rows-per-thread parameter was
// cross-compiled for gfx950 and matched every form but one: bestpath_sweep_kernel<F64, false, 4, true> uses exactly the 128
// VGPRs a 1024-thread block allows, and the port spilled 4 of them (20 bytes of scratch) in two variants.  A change to the
// parity exchange or to a bounds predicate in rnnt_pxpy.h has to be made here as well.
// (DESIGN.md 8o lists the modified type's 16-byte packets as open.)
#pragma once

#include "rnnt_pxpy.h"                 // PxRect / px_rect; through rnnt_kernels.h lds_barrier, cost_invalid, load1 / store1, wave_shr1

namespace rnnt {

constexpr int kBpChunk = 8;             // steps per prefetched chunk, a row per thread
constexpr int kBpChunkWide = 2;         // ... with kBpWideRows rows per thread (the registers of 1024 threads)
constexpr int kBpWideRows = 4;          // rows per thread above 1024 lattice rows
constexpr int kBpWaveMaxU = 64;         // S + 1 up to here: one wavefront, no LDS exchange
constexpr int kBpLdsWords = 6144;       // traceback staging: 48 KB of decision words per range of rows

// Thread 0's walk from node (s, t) -- the rectangle's coordinates -- down to row `lo` (row 0 needs no decision): at t == 0 the
// symbol edge, otherwise the bit.  word(row, w) = word w (absolute) of the row's decision bits.  A word is fetched once per
// row and 64 frames, and the frame edges between two symbol decisions are taken in one step (the highest set bit at or
// below t): S + T / 64 dependent reads instead of S + T.
template <bool MOD, typename Word>
__device__ __forceinline__ void bp_walk(int& s, int& t, int lo, int s0, int t0, int* __restrict__ fr, Word word) {
    int cs = -1, cw = -1;
    unsigned long long wd = 0;
    while (s >= lo && t >= 0) {
        if (t > 0) {
            const int ta = t0 + t, w = ta >> 6;
            if (s != cs || w != cw) { cs = s; cw = w; wd = word(s, w); }
            const unsigned long long m = wd & (~0ull >> (63 - (ta & 63)));      // the decisions at or below t in this word
            if (m == 0) {                                                        // frame edges down to the word's first node
                const int nt = (w << 6) - 1 - t0;
                t = nt < 0 ? 0 : nt;
                continue;
            }
            t = (w << 6) + 63 - __clzll(static_cast<long long>(m)) - t0;         // (bits below t0 are zero: t >= 0)
        }
        fr[s0 + s - 1] = t0 + (MOD ? t - 1 : t);
        --s;
        if (MOD) --t;
    }
}

// grid = B, block = 64 (MULTI == false: S + 1 <= kBpWaveMaxU) or 64 * ceil(ceil((S + 1) / K) / 64) <= 1024.
// scores[b * score_stride] (scores may be NULL: the restoring launch of the host-scores entry).
template <typename Tag, bool MOD, int K, bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void bestpath_sweep_kernel(
        const typename Tag::store* __restrict__ px, const typename Tag::store* __restrict__ py,
        const long long* __restrict__ boundary, double* scores, long long score_stride, int* __restrict__ frames,
        unsigned long long* back, int S, int T) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    constexpr int CH = K == 1 ? kBpChunk : kBpChunkWide;
    __shared__ unsigned long long sbits[kBpLdsWords];
    __shared__ double edge[2][16];
    __shared__ double sh_score;
    __shared__ int sh_bad, walk_s, walk_t;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    const int nthreads = static_cast<int>(blockDim.x);
    const int TX = MOD ? T : T + 1, U = S + 1, NW = (T + 64) >> 6;
    const PxRect r = px_rect(boundary, b, S, T);
    const int s0 = r.s0, t0 = r.t0, Sr = r.Sr, Tr = r.Tr;
    const double NEG = -__builtin_huge_val(), INF = __builtin_huge_val();
    unsigned long long* bk = back + static_cast<size_t>(b) * U * NW;
    int* fr = frames + static_cast<size_t>(b) * S;
    if (tid == 0) { sh_bad = 0; sh_score = NEG; }
    __syncthreads();

    if (r.ok) {
        double stay[K], emit[K];
        unsigned long long word[K];
        const St *rx[K], *ry[K];
        int ls[K];
        bool hasx[K], hasy[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            ls[k] = tid * K + k;
            hasy[k] = ls[k] <= Sr;
            hasx[k] = ls[k] < Sr;
            const size_t s = static_cast<size_t>(s0 + (hasy[k] ? ls[k] : 0));
            rx[k] = px + (static_cast<size_t>(b) * S + (hasx[k] ? s : 0)) * TX + t0;     // (never dereferenced unless hasx)
            ry[k] = py + (static_cast<size_t>(b) * U + s) * T + t0;
            stay[k] = emit[k] = NEG;
            word[k] = 0;
        }
        const int nsteps = MOD ? Tr + 1 : Tr + Sr + 1;
        const int lastx = MOD ? Tr - 1 : Tr;                         // the last frame position with a symbol edge
        bool bad = false, have_fin = false;
        double fin = NEG;
        // steps d0 .. d0 + CH - 1 of every row of the thread; an element outside the rectangle's edges is never read
        auto load = [&](int d0, C (&bx)[K][CH], C (&by)[K][CH]) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int j = d0 + i - (MOD ? 0 : ls[k]);
                    bx[k][i] = (hasx[k] && j >= 0 && j <= lastx) ? load1<Tag>(rx[k] + j) : C(0);
                    by[k][i] = (hasy[k] && j >= 0 && j < Tr) ? load1<Tag>(ry[k] + j) : C(0);
                }
            }
        };
        C ax[K][CH], ay[K][CH], bx[K][CH], by[K][CH];
        load(0, ax, ay);
        // The two buffers keep FIXED roles per call site (the loop is unrolled by two chunks), as pxpy_sweep's.
        auto chunk = [&](int d0, C (&cx)[K][CH], C (&cy)[K][CH], C (&nx)[K][CH], C (&ny)[K][CH]) {
            if (d0 + CH < nsteps) load(d0 + CH, nx, ny);
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int d = d0 + i;
                if (d >= nsteps) break;
                double left = wave_shr1(NEG, emit[K - 1]);           // lane 0 keeps -inf: row -1 is no row
                if (MULTI) {
                    if (lane == 63) edge[d & 1][wave] = emit[K - 1];
                    lds_barrier();
                    if (lane == 0 && wave > 0) left = edge[d & 1][wave - 1];
                }
#pragma unroll
                for (int k = K - 1; k >= 0; --k) {                   // downwards: row k reads row k - 1's OLD candidate
                    const int j = d - (MOD ? 0 : ls[k]);
                    const bool act = hasy[k] && j >= 0 && j <= Tr;
                    const double x = k > 0 ? emit[k > 0 ? k - 1 : 0] : left;
                    const double y = stay[k];
                    const bool sym = x > y;                          // strict: an exact tie keeps the frame edge
                    double p = sym ? x : y;
                    if (ls[k] == 0 && j == 0) p = 0.0;               // the source (x = y = -inf there: sym is false)
                    const bool ex = act && hasx[k] && j <= lastx, ey = act && j < Tr;
                    const double wx = static_cast<double>(cx[k][i]), wy = static_cast<double>(cy[k][i]);
                    bad = bad || (ex && !(wx < INF)) || (ey && !(wy < INF));       // NaN or +inf on an edge of the rectangle
                    emit[k] = ex ? p + wx : NEG;
                    stay[k] = ey ? p + wy : NEG;
                    if (act) {
                        const int t = t0 + j;
                        if (sym) word[k] |= 1ull << (t & 63);
                        if ((t & 63) == 63 || j == Tr) {
                            bk[static_cast<size_t>(s0 + ls[k]) * NW + (t >> 6)] = word[k];
                            word[k] = 0;
                        }
                        if (ls[k] == Sr && j == Tr) { fin = p; have_fin = true; }
                    }
                }
            }
        };
        for (int d0 = 0; d0 < nsteps; d0 += 2 * CH) {
            chunk(d0, ax, ay, bx, by);
            if (d0 + CH < nsteps) chunk(d0 + CH, bx, by, ax, ay);
        }
        if (bad) sh_bad = 1;                                         // (several bad edges race: any store will do)
        if (have_fin) sh_score = fin;
    }
    __threadfence_block();
    __syncthreads();

    // ---- traceback stage
    const double sc = !r.ok ? cost_invalid<double>() : (sh_bad != 0 ? __builtin_nan("") : sh_score);
    const bool path = r.ok && sc - sc == 0.0;                        // finite
    const int w0 = t0 >> 6, w1 = (t0 + Tr) >> 6, nw = w1 - w0 + 1;
    for (size_t i = tid; i < static_cast<size_t>(U) * NW; i += nthreads) {
        const int s = static_cast<int>(i / NW), w = static_cast<int>(i - static_cast<size_t>(s) * NW);
        if (!(r.ok && s >= s0 && s <= s0 + Sr && w >= w0 && w <= w1)) bk[i] = 0;
    }
    for (int s = tid; s < S; s += nthreads)
        if (!(path && s >= s0 && s < s0 + Sr)) fr[s] = -1;
    if (path && Sr > 0) {                                            // (block-uniform)
        const int rows = kBpLdsWords / nw;                           // rows per staged range; 0: a row does not fit
        int s = Sr, t = Tr;                                          // thread 0's walk, in the rectangle's coordinates
        if (rows == 0) {
            if (tid == 0)
                bp_walk<MOD>(s, t, 1, s0, t0, fr, [&](int row, int w) { return bk[static_cast<size_t>(s0 + row) * NW + w]; });
        } else {
            int hi = Sr;
            while (hi > 0) {
                const int lo = hi - rows + 1 > 1 ? hi - rows + 1 : 1;     // row 0 needs no decision
                const int words = (hi - lo + 1) * nw;
                for (int i = tid; i < words; i += nthreads) {
                    const int q = i / nw, w = i - q * nw;
                    sbits[i] = bk[static_cast<size_t>(s0 + lo + q) * NW + w0 + w];
                }
                __syncthreads();
                if (tid == 0) {
                    bp_walk<MOD>(s, t, lo, s0, t0, fr, [&](int row, int w) { return sbits[(row - lo) * nw + w - w0]; });
                    walk_s = s;
                    walk_t = t;
                }
                __syncthreads();
                hi = walk_t < 0 ? 0 : walk_s;
            }
        }
    }
    __syncthreads();
    if (tid == 0 && scores != nullptr) scores[static_cast<size_t>(b) * score_stride] = sc;
}

// grid = (ceil((T + 1) / 256), S + 1, B slice), block = 256: thread (b, s, t) stores py_path[b, s, t] (t < T) and
// px_path[b, s, t] (s < S, t < T + 1 regular | T modified).  scale: B doubles or NULL for 1.
template <typename Tag, bool MOD>
__global__ __launch_bounds__(256) void bestpath_edges_kernel(
        const int* __restrict__ frames, const double* __restrict__ scores, long long score_stride,
        const long long* __restrict__ boundary, const double* __restrict__ scale, typename Tag::store* __restrict__ px_path,
        typename Tag::store* __restrict__ py_path, int S, int T, int b0) {
    using C = typename Tag::comp;
    const int b = b0 + blockIdx.z, s = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    const int TX = MOD ? T : T + 1, U = S + 1;
    if (t > T) return;
    const PxRect r = px_rect(boundary, b, S, T);
    const int s0 = r.s0, t0 = r.t0, s1 = r.s0 + r.Sr, t1 = r.t0 + r.Tr;
    const double sc = scores[static_cast<size_t>(b) * score_stride];
    const bool nan = r.ok && sc != sc, path = r.ok && sc - sc == 0.0;
    const double g = scale != nullptr ? scale[b] : 1.0;
    const int* fr = frames + static_cast<size_t>(b) * S;
    const C one = static_cast<C>(g), qnan = static_cast<C>(__builtin_nan(""));
    if (t < T) {
        C v = C(0);
        if (r.ok && s >= s0 && s <= s1 && t >= t0 && t < t1) {
            if (nan) {
                v = qnan;
            } else if (path) {
                const int lo = s == s0 ? t0 : fr[s - 1] + (MOD ? 1 : 0), hi = s == s1 ? t1 : fr[s];
                v = (t >= lo && t < hi) ? one : C(0);
            }
        }
        store1<Tag>(py_path + (static_cast<size_t>(b) * U + s) * T + t, v);
    }
    if (s < S && t < TX) {
        C v = C(0);
        if (r.ok && s >= s0 && s < s1 && t >= t0 && t <= (MOD ? t1 - 1 : t1)) {
            if (nan) v = qnan;
            else if (path) v = fr[s] == t ? one : C(0);
        }
        store1<Tag>(px_path + (static_cast<size_t>(b) * S + s) * TX + t, v);
    }
}

}  // namespace rnnt
