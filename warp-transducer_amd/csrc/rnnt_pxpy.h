// rnnt_pxpy.h -- what the kernels on px / py edge log-probabilities share (bestpath, expect, sample; mi's pack stage): the
// rectangle of a sample and THE ROW SWEEP, the schedule of expect_fwd_kernel, expect_bwd_kernel and sample_fwd_kernel.
//
// The lattice: px (B, S, T + 1 | T) symbol edges, py (B, S + 1, T) frame edges, contiguous along t; sample b's rectangle
// [s0, s1] x [t0, t1] comes from `boundary` (px_rect).  Regular type: the symbol edge stays in its frame; modified type:
// it consumes one.
//
// THE ROW SWEEP (pxpy_sweep).  One block per sample, a thread per lattice row (row = s - s0).  Regular type: row r meets
// frame position j = d - r on anti-diagonal d, Tr + Sr + 1 steps; modified type: every row meets j = d, Tr + 1 steps.  A
// thread walks ITS OWN rows [b, s, :] in t order -- no transpose, no pack stage, no workspace -- one chunk of CH steps ahead
// of use, in two register buffers with FIXED roles per call site (the loop is unrolled by two chunks: a buffer never
// changes hands through a copy).  The NV doubles a row hands to its neighbour per step travel through 2 NV DPP moves
// (wave_shr1 / wave_shl1 on the halves) inside a wavefront and, between wavefronts, through NV LDS words per wavefront
// and step parity behind an LDS-only barrier: the word of parity d & 1 is rewritten two steps later, behind the barrier
// of step d + 1, which every reader of step d has passed.  The predicates hasx / hasy (the row has symbol / frame
// edges), act (the step meets a node of the rectangle) and ex / ey (that node has the out-edge) keep every load inside the
// rectangle's edges.  The caller keeps the semiring: its body is called once per step.
//
// bestpath_sweep_kernel walks the same lattice on a hand-written copy of this schedule with K rows per thread
// (rnnt_bestpath_kernels.h says why).  Loads are element-wise: in the regular type the rows of a wavefront are at 64
// different frames, so a lane's position in a 16-byte packet is lane-variant and a packet saves no instruction.
#pragma once

#include "rnnt_kernels.h"              // lds_barrier, cost_invalid; through rnnt_device.h the tags, load1 / store1, wave_shr1

namespace rnnt {

// The rectangle of sample b: ok == false for a boundary outside the tensor (then s0 = t0 = 0, Sr = -1, Tr = 0).
struct PxRect { int s0, t0, Sr, Tr; bool ok; };
__device__ __forceinline__ PxRect px_rect(const long long* __restrict__ boundary, int b, int S, int T) {
    long long q0 = 0, r0 = 0, q1 = S, r1 = T;
    if (boundary != nullptr) {
        const long long* bd = boundary + static_cast<size_t>(b) * 4;
        q0 = bd[0]; r0 = bd[1]; q1 = bd[2]; r1 = bd[3];
    }
    const bool ok = 0 <= q0 && q0 <= q1 && q1 <= S && 0 <= r0 && r0 <= r1 && r1 <= T;
    return {ok ? static_cast<int>(q0) : 0, ok ? static_cast<int>(r0) : 0, ok ? static_cast<int>(q1 - q0) : -1,
            ok ? static_cast<int>(r1 - r0) : 0, ok};
}

struct PxNoX {};                        // X of a sweep that prefetches nothing but the edges

// The sweep of row `ls` (= threadIdx.x: every thread of the block calls this) of a rectangle of Sr + 1 rows and Tr + 1
// frame positions.
//   REV     steps run backwards (step e is anti-diagonal nsteps - 1 - e) and the neighbour is the row ABOVE (wave_shl1);
//           otherwise the row below (wave_shr1)
//   NE      edge arrays of each kind: rx[k] / ry[k] point at position 0 of the row's symbol / frame edges (rx is never
//           dereferenced unless ls < Sr)
//   NV      doubles handed to the neighbour per step; `none` is what the row past the block's end hands over, and what
//           every row hands over before its first step
//   X, pre  a per-step value prefetched with the edges: pre(j, in), in = the step meets a node of the rectangle
//   body(j, act, ex, ey, nb, wx, wy, x, out)   once per step: nb[NV] the neighbour's hand-over of the step before, wx[NE] /
//           wy[NE] the node's out-edges (0 where ex / ey is false), out[NV] the row's own hand-over, the step before's on
//           entry and this step's on return
// edge: the block's LDS words (MULTI; blockDim.x <= 1024).
template <typename Tag, bool MOD, bool MULTI, bool REV, int NE, int NV, int CH, typename X, typename Pre, typename Body>
__device__ __forceinline__ void pxpy_sweep(const typename Tag::store* const (&rx)[NE],
                                           const typename Tag::store* const (&ry)[NE], int ls, int Sr, int Tr,
                                           double (&edge)[2][16][NV], const double (&none)[NV], Pre pre, Body body) {
    using C = typename Tag::comp;
    // MULTI: the lane that writes the wavefront's word, the lane that reads the neighbouring wavefront's
    const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6), nwaves = static_cast<int>(blockDim.x) >> 6;
    [[maybe_unused]] const bool sends = lane == (REV ? 0 : 63);
    [[maybe_unused]] const bool takes = REV ? lane == 63 && wave + 1 < nwaves : lane == 0 && wave > 0;
    const bool hasy = ls <= Sr, hasx = ls < Sr;
    const int nsteps = MOD ? Tr + 1 : Tr + Sr + 1;
    const int lastx = MOD ? Tr - 1 : Tr;                             // the last frame position with a symbol edge
    auto frame = [&](int d) { return (REV ? nsteps - 1 - d : d) - (MOD ? 0 : ls); };
    // A chunk of CH prefetched steps.  Each kind's edges are a local array OF ITS OWN, not a row of one [NE][CH] array: the
    // compiler keeps a local array in one register tuple, and tuples of NE * CH values cost expect_fwd_kernel<F32> 26
    // VGPRs and expect_bwd_kernel<F16> a spill.  (NE == 1: the second kind's arrays are dead.)
    static_assert(NE == 1 || NE == 2, "one local array per kind: add a kind here");
    struct Chunk { C (&wx0)[CH]; C (&wy0)[CH]; C (&wx1)[CH]; C (&wy1)[CH]; X (&xs)[CH]; };
    C awx0[CH], awy0[CH], awx1[CH], awy1[CH], bwx0[CH], bwy0[CH], bwx1[CH], bwy1[CH];
    X axs[CH], bxs[CH];
    const Chunk a = {awx0, awy0, awx1, awy1, axs}, b = {bwx0, bwy0, bwx1, bwy1, bxs};
    // steps d0 .. d0 + CH - 1 of the thread's row; an element outside the rectangle's edges is never read
    auto load = [&](int d0, const Chunk& c) {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int j = frame(d0 + i);
            const bool ex = hasx && j >= 0 && j <= lastx, ey = hasy && j >= 0 && j < Tr;
            c.wx0[i] = ex ? load1<Tag>(rx[0] + j) : C(0);
            if constexpr (NE > 1) c.wx1[i] = ex ? load1<Tag>(rx[NE - 1] + j) : C(0);
            c.wy0[i] = ey ? load1<Tag>(ry[0] + j) : C(0);
            if constexpr (NE > 1) c.wy1[i] = ey ? load1<Tag>(ry[NE - 1] + j) : C(0);
            c.xs[i] = pre(j, hasy && j >= 0 && j <= Tr);
        }
    };
    double out[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) out[v] = none[v];
    load(0, a);
    // The two chunks keep FIXED roles per call site (the loop is unrolled by two chunks).
    auto chunk = [&](int d0, const Chunk& c, const Chunk& next) {
        if (d0 + CH < nsteps) load(d0 + CH, next);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int d = d0 + i;
            if (d >= nsteps) break;
            double nb[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) nb[v] = REV ? wave_shl1(none[v], out[v]) : wave_shr1(none[v], out[v]);
            if constexpr (MULTI) {
                if (sends) {
#pragma unroll
                    for (int v = 0; v < NV; ++v) edge[d & 1][wave][v] = out[v];
                }
                lds_barrier();
                if (takes) {
#pragma unroll
                    for (int v = 0; v < NV; ++v) nb[v] = edge[d & 1][REV ? wave + 1 : wave - 1][v];
                }
            }
            const int j = frame(d);
            const bool act = hasy && j >= 0 && j <= Tr;
            C wx[NE], wy[NE];
            wx[0] = c.wx0[i]; wy[0] = c.wy0[i];
            if constexpr (NE > 1) { wx[NE - 1] = c.wx1[i]; wy[NE - 1] = c.wy1[i]; }
            body(j, act, act && hasx && j <= lastx, act && j < Tr, nb, wx, wy, c.xs[i], out);
        }
    };
    for (int d0 = 0; d0 < nsteps; d0 += 2 * CH) {
        chunk(d0, a, b);
        if (d0 + CH < nsteps) chunk(d0 + CH, b, a);
    }
}

}  // namespace rnnt
