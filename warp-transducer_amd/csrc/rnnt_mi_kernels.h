// rnnt_mi_kernels.h -- the gfx950 kernels of the lattice primitive on edge log-probabilities (include/rnnt_mi.h).
//
// The caller's px (B, S, T + 1 | T) and py (B, S + 1, T) are contiguous along t; the lattice kernels of this tree want one
// four-word cell record [lp_blank, lp_label, -, -] per node, contiguous along u, in base 2.  Three stages:
//   1 mi_pack_kernel      a tiled transpose through LDS: rows of px / py read along t, 16-byte records written along u.  The
//                         same pass shifts the rectangle's origin (s0, t0) to the table's (0, 0), writes the derived
//                         per-sample lengths, the terminal column of the regular type, -inf on every edge that cannot lie on
//                         a path, and the poison flag
//   2 ar_lattice_wave_kernel / ar_lattice_block_kernel (rnnt_ar_kernels.h; regular type: T_b + 1 node columns are its
//     "frames", the symbol edge stays in its column) or mono_lattice_wave_kernel / mono_lattice_block_kernel
//     (rnnt_mono_kernels.h; modified type: the symbol edge consumes a frame), instantiated in this library's code objects;
//     then mi_score_kernel, a thread per sample: the lattice kernels close a sample with a COST (-log P, +inf without a
//     path) and refuse a sample of zero frames, the header wants log P itself and has a value for the modified type's
//     t1 == t0
//   3 mi_unpack_kernel    the coefficient kernel fused with the transpose back: alpha, beta, the offsets and the record read
//                         once along u, the two edge posteriors times the sample's scale through LDS, px_grad / py_grad
//                         written along t -- every element of both, zeros outside the rectangle's edges included
//
// THE TABLE of sample b: node (s, t) of the rectangle is cell (t' = t - t0, u = s - s0) of a (maxTt, maxU) table, maxTt =
// T + 1 (regular) or T (modified), maxU = S + 1; cell index tdt_cell(b, t', u, maxTt, maxU).  The lattice kernels take the
// sample's lengths from two int arrays this library keeps in its workspace: xlen[b] = node columns with out-edges (t1 - t0 + 1
// regular: the last column's symbol edges are real; t1 - t0 modified), ylen[b] = s1 - s0.  A boundary outside the tensor:
// xlen = 0, ylen = -1; the modified type's t1 == t0: xlen = 0, ylen = s1 - s0 (no edge at all; the score is 0 when
// s1 == s0 and -inf otherwise).
//
// THE TRANSPOSE TILE.  kMiTile x kMiTile values of the lattice type per array, rows padded by one value: a wavefront's
// ds_write of a row is contiguous, and its transposed ds_read walks a stride of kMiTile + 1 values -- 33 dwords for fp32, 66
// for fp64 -- which puts the 32 lanes of a half-wave on 32 different banks (fp64: on 32 different bank pairs).
#pragma once

#include "rnnt_ar_kernels.h"           // stage 2: both lattices; through it mono_lse2, tdt_cell, the record format
#include "rnnt_pxpy.h"                 // PxRect / px_rect: the rectangle of a sample

namespace rnnt {

constexpr int kMiTile = 32;             // the transpose tile's edge, both axes
constexpr int kMiRec = kArRec;          // == kMonoRec: four lattice values per cell
static_assert(kArRec == kMonoRec && kArRec == 4, "one record format for both lattices");

// [lp_blank, lp_label, 0, 0] as 16-byte stores
__device__ __forceinline__ void mi_store_rec(float* p, float b, float l) {
    *reinterpret_cast<float4*>(p) = make_float4(b, l, 0.0f, 0.0f);
}
__device__ __forceinline__ void mi_store_rec(double* p, double b, double l) {
    reinterpret_cast<double2*>(p)[0] = make_double2(b, l);
    reinterpret_cast<double2*>(p)[1] = make_double2(0.0, 0.0);
}

// ------------------------------------------------------------------------------------------
// Stage 1.  grid = (tiles along u * tiles along t', N slice), block = 256 = 32 lanes along the contiguous axis by 8 rows,
// four rows per thread and phase.  Phase 1: lane = t', row = u (the inputs' order); phase 2: lane = u, row = t' (the
// table's).  Every cell of the (maxTt, maxU) table of a sample with a lattice is written, "no edge" outside its rectangle.
// Natural log -> base 2 in fp64, one rounding to the lattice type (as the delay library's gauge).
//
// Masking: the lattice kernels have no band test, so an edge that cannot lie on a path (0, 0) -> (Sr, Tr) is written as
// -inf.  Regular type: every edge of the rectangle can; the terminal column t' = Tr has no frame edge but the weight-0 one
// out of (Tr, Sr), which the lattice kernels take as the "final blank".  Modified type: node (t', u) is live iff u <= t'
// and Sr - u <= Tr - t'; a frame edge out of a live node leaves the band iff Sr - u == Tr - t'.
template <typename Tag, bool MOD>
__global__ __launch_bounds__(256) void mi_pack_kernel(
        const typename Tag::store* __restrict__ px, const typename Tag::store* __restrict__ py,
        const long long* __restrict__ boundary, typename Tag::comp* __restrict__ tab, int* __restrict__ xlen,
        int* __restrict__ ylen, int* __restrict__ org, int* __restrict__ poison, int S, int T, int tiles_u, int b0) {
    using C = typename Tag::comp;
    __shared__ C wb[kMiTile][kMiTile + 1], wl[kMiTile][kMiTile + 1];
    const int b = b0 + blockIdx.y, tid = threadIdx.x;
    const int tu = blockIdx.x % tiles_u, tt = blockIdx.x / tiles_u;
    const PxRect rc = px_rect(boundary, b, S, T);
    const int s0 = rc.s0, t0 = rc.t0, Sr = rc.Sr, Tr = rc.Tr;
    const bool ok = rc.ok;
    const int Tn = ok ? (MOD ? Tr : Tr + 1) : 0;                     // node columns with out-edges
    if (blockIdx.x == 0 && tid == 0) {
        xlen[b] = Tn;
        ylen[b] = Sr;
        org[2 * b] = s0;
        org[2 * b + 1] = t0;
    }
    if (Tn == 0) return;                                             // (the whole block: no lattice, the table is not read)
    const int maxTt = MOD ? T : T + 1, maxU = S + 1;                 // (maxTt is the length of a row of px as well)
    const int lane = tid & (kMiTile - 1), row0 = tid / kMiTile;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kMiTile / 8; ++k) {
        const int r = row0 + 8 * k;
        const int u = tu * kMiTile + r, tp = tt * kMiTile + lane;
        C vb = neg_inf<C>(), vl = neg_inf<C>();
        if (u <= Sr && tp < Tn) {
            const size_t s = static_cast<size_t>(s0 + u), t = static_cast<size_t>(t0 + tp);
            if (tp < Tr) {
                const C x = load1<Tag>(py + (static_cast<size_t>(b) * maxU + s) * T + t);
                bad = bad || x != x || x == -neg_inf<C>();
                vb = static_cast<C>(static_cast<double>(x) * kLog2e);
            } else if (!MOD && u == Sr) {
                vb = C(0);                                           // the terminal column: out of (Tr, Sr) only
            }
            if (u < Sr) {
                const C x = load1<Tag>(px + (static_cast<size_t>(b) * S + s) * maxTt + t);
                bad = bad || x != x || x == -neg_inf<C>();
                vl = static_cast<C>(static_cast<double>(x) * kLog2e);
            }
            if (MOD) {
                const int du = Sr - u, dt = Tr - tp;
                if (u > tp || du > dt) vb = vl = neg_inf<C>();       // outside the band
                else if (du == dt) vb = neg_inf<C>();                // the frame edge would leave it
            }
        }
        wb[r][lane] = vb;
        wl[r][lane] = vl;
    }
    if (bad) poison[b] = 1;                                          // (several bad edges race: any store will do)
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kMiTile / 8; ++k) {
        const int r = row0 + 8 * k;
        const int u = tu * kMiTile + lane, tp = tt * kMiTile + r;
        if (tp < maxTt && u < maxU) mi_store_rec(tab + tdt_cell(b, tp, u, maxTt, maxU) * kMiRec, wb[lane][r], wl[lane][r]);
    }
}

// ------------------------------------------------------------------------------------------
// Behind stage 2.  A thread per sample: grid = ceil(N / 256).  ll[b] = log2 of the total, absolute, left by the lattice
// kernel's forward side for every sample with a lattice.
template <typename L>
__global__ __launch_bounds__(256) void mi_score_kernel(const double* __restrict__ ll, const int* __restrict__ xlen,
                                                        const int* __restrict__ ylen, const int* __restrict__ poison,
                                                        L* __restrict__ scores, int N) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= N) return;
    const int Tn = xlen[b], Sr = ylen[b];
    L v;
    if (Sr < 0) {
        v = cost_invalid<L>();                                       // a boundary outside the tensor
    } else if (Tn == 0) {
        v = Sr == 0 ? L(0) : neg_inf<L>();                           // modified, t1 == t0: the empty path, or none
    } else {
        const double lp = ll[b];
        v = (poison[b] != 0 || lp != lp) ? static_cast<L>(__builtin_nan("")) : static_cast<L>(lp * kLn2);
    }
    scores[b] = v;
}

// ------------------------------------------------------------------------------------------
// Stage 3.  grid = (tiles along s * tiles along t, N slice) over the OUTPUT's coordinates -- s in [0, S], t in [0, maxTt) --
// so that every element of both arrays has a thread; block = 256 as stage 1.  Phase 1: lane = s, row = t: the cell
// (t - t0, s - s0) if the node lies in the rectangle,
//   regular    cy = 2^(alpha(t', u) + lp_blank + beta(t' + 1, u) - log P)        (t' < Tr)
//              cx = 2^(alpha(t', u) + lp_label + beta(t', u + 1) - log P)        (u < Sr)
//   modified   cy as above with beta(Tr, .) the terminal row, 0 at Sr            (t' < Tr)
//              cx = 2^(alpha(t', u) + lp_label + beta(t' + 1, u + 1) - log P)    (u < Sr, t' < Tr)
// the fp64 offsets summed first, as delay_coef_kernel does; times the sample's scale.  Phase 2: lane = t, row = s.
// A sample without a lattice or without a path: zeros everywhere; a poisoned one: NaN on the rectangle's edges.
template <typename Tag, bool MOD>
__global__ __launch_bounds__(256) void mi_unpack_kernel(
        typename Tag::store* __restrict__ px_grad, typename Tag::store* __restrict__ py_grad,
        const typename Tag::comp* __restrict__ scale, const typename Tag::comp* __restrict__ tab,
        const typename Tag::comp* __restrict__ alpha, const typename Tag::comp* __restrict__ beta,
        const double* __restrict__ offa, const double* __restrict__ offb, const double* __restrict__ ll,
        const int* __restrict__ xlen, const int* __restrict__ ylen, const int* __restrict__ org,
        const int* __restrict__ poison, int S, int T, int tiles_s, int b0) {
    using C = typename Tag::comp;
    using P = typename MonoPair<C>::type;
    __shared__ C gy[kMiTile][kMiTile + 1], gx[kMiTile][kMiTile + 1];
    const int b = b0 + blockIdx.y, tid = threadIdx.x;
    const int ts = blockIdx.x % tiles_s, tt = blockIdx.x / tiles_s;
    const int maxTt = MOD ? T : T + 1, maxU = S + 1;
    const int Tn = xlen[b], Sr = ylen[b], s0 = org[2 * b], t0 = org[2 * b + 1];
    const int Tr = MOD ? Tn : Tn - 1;
    const bool lattice = Sr >= 0 && Tn >= 1;
    const double lp = lattice ? ll[b] : 0.0;
    const bool nan = lattice && (poison[b] != 0 || lp != lp);
    const bool path = lattice && !nan && lp - lp == 0.0;             // (log P = -inf: no path, zeros)
    const C g = scale != nullptr ? scale[b] : C(1);
    const size_t o0 = static_cast<size_t>(b) * (MOD ? mono_offsets(maxTt) : ar_offsets(maxTt, maxU));
    const int lane = tid & (kMiTile - 1), row0 = tid / kMiTile;
#pragma unroll
    for (int k = 0; k < kMiTile / 8; ++k) {
        const int r = row0 + 8 * k;
        const int u = ts * kMiTile + lane - s0, tp = tt * kMiTile + r - t0;
        C cy = C(0), cx = C(0);
        if (lattice && u >= 0 && u <= Sr && tp >= 0 && tp < Tn) {
            const bool ey = tp < Tr, ex = u < Sr && (!MOD || tp < Tr);
            if (nan) {
                const C v = static_cast<C>(__builtin_nan(""));
                if (ey) cy = v;
                if (ex) cx = v;
            } else if (path && (ey || ex)) {
                const size_t c = tdt_cell(b, tp, u, maxTt, maxU);
                const int d = MOD ? tp : tp + u;
                const C a = alpha[c] + static_cast<C>(offa[o0 + d] + offb[o0 + d + 1] - lp);
                const P w = *reinterpret_cast<const P*>(tab + c * kMiRec);
                if (ey) {
                    const C bt = tp + 1 < Tn ? beta[c + maxU] : (u == Sr ? C(0) : neg_inf<C>());
                    cy = fast_exp2(a + w.x + bt) * g;
                }
                if (ex) {
                    C bx;
                    if (MOD) bx = tp + 1 < Tn ? beta[c + maxU + 1] : (u + 1 == Sr ? C(0) : neg_inf<C>());
                    else bx = beta[c + 1];
                    cx = fast_exp2(a + w.y + bx) * g;
                }
            }
        }
        gy[r][lane] = cy;
        gx[r][lane] = cx;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kMiTile / 8; ++k) {
        const int r = row0 + 8 * k;
        const int s = ts * kMiTile + r, t = tt * kMiTile + lane;
        if (s <= S && t < T) store1<Tag>(py_grad + (static_cast<size_t>(b) * maxU + s) * T + t, gy[lane][r]);
        if (s < S && t < maxTt) store1<Tag>(px_grad + (static_cast<size_t>(b) * S + s) * maxTt + t, gx[lane][r]);
    }
}

}  // namespace rnnt
