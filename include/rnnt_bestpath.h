/* rnnt_bestpath.h -- C-ABI of libwarprnnt_bestpath.so: the BEST PATH (Viterbi alignment) of the transducer lattice over edge
 * log-probabilities the caller built -- the max-plus twin of include/rnnt_mi.h, which sums over the paths.  The weights of
 * the lattice's edges come in; the weight of the best path, the frame of each of its symbol edges, the back-pointer bits
 * of the sweep and the 0/1 indicator of its edges go out.  Pruned, HAT, delay-penalised and monotonic models and lattices
 * with edited edges get an alignment by the route they already use: logprobs -> edit -> lattice.  A library of its own, so
 * that a caller of libwarprnnt.so never loads it.  It takes NO workspace: the one array the sweep leaves behind, the
 * back-pointer bits, is an output the caller allocates.
 *
 * Conventions and inputs are exactly those of include/rnnt_mi.h: `rnntOptions` by value, of which only loc (must be
 * RNNT_GPU) and stream (the HIP stream everything is enqueued on) are read; dtype codes 0 fp32, 1 fp64, 2 bf16, 3 fp16
 * (the storage of px, py, px_path, py_path).  Nothing here allocates memory, and the forms with scores in device memory
 * only enqueue (they can be captured in a HIP graph).
 *
 * INPUTS, all on the device, contiguous, natural logs.  B = minibatch, S >= 0 symbols, T >= 1 frames.
 *     py (B, S + 1, T)          py[b, s, t]: the edge that consumes frame t with s symbols emitted, (s, t) -> (s, t + 1)
 *     px, modified == 0 ("regular")   (B, S, T + 1)   px[b, s, t]: the edge that emits symbol s at frame position t,
 *                                                     (s, t) -> (s + 1, t)
 *     px, modified != 0               (B, S, T)       the symbol edge consumes frame t as well, (s, t) -> (s + 1, t + 1)
 *     boundary (B, 4) int64     [s0, t0, s1, t1] per sample, or NULL for [0, 0, S, T] everywhere
 * -inf is a legal weight and means "no edge".  With S == 0 px, px_path and frames have no element and the pointers are
 * not looked at.  Input elements outside the rectangle's edges (include/rnnt_mi.h) are never read.
 *
 * RECURSION of sample b over the nodes s0 <= s <= s1, t0 <= t <= t1, p[s0, t0] = 0, a missing in-edge counting as -inf:
 *     regular    x = p[s - 1, t]     + px[s - 1, t]          y = p[s, t - 1] + py[s, t - 1]
 *     modified   x = p[s - 1, t - 1] + px[s - 1, t - 1]      y = p[s, t - 1] + py[s, t - 1]
 *     p[s, t] = max(x, y);   bit(s, t) = (x > y)       -- strict: on an exact tie the frame edge, the rule of include/rnnt.h
 *     score[b] = p[s1, t1]
 * the log weight of the best path (s0, t0) -> (s1, t1): k2's sign, NOT a cost.
 *
 * ARITHMETIC.  Every stored weight is upcast exactly to fp64 and used as it is: no change of base, no rescaling.  p is
 * held in fp64 for every storage type; each x and y is ONE IEEE addition.  A host fp64 program that performs the same
 * additions gets the same bits.
 *
 * OUTPUTS, all caller-allocated; every element is written by every call that takes them.
 *     scores (B) double         device or host memory, as in compute_rnnt_mi.  Host memory: copied behind the last kernel and
 *                               the stream synchronised; a bad-boundary marker then gives RNNT_STATUS_INVALID_VALUE.
 *     frames (B, S) int32       for s0 <= s < s1 the t of the edge px[b, s, t] on the best path, in tensor coordinates:
 *                               non-decreasing within [t0, t1] (regular), strictly increasing within [t0, t1) (modified);
 *                               -1 elsewhere.  Traceback from (s1, t1): at t == t0 the symbol edge, at s == s0 the frame
 *                               edge, otherwise the bit.  Among several best paths this one emits every symbol earliest.
 *     back (B, S + 1, ceil((T + 1) / 64)) 64-bit words
 *                               bit(s, t) at word [b, s, t >> 6], bit t & 63, absolute coordinates; 0 outside the
 *                               rectangle's nodes.
 *     px_path, py_path          both given or both NULL; shapes and dtypes of px / py.  The 0/1 indicator of the best path's
 *                               edges -- the (sub)gradient of score -- times grad_scale_device[b] where an entry takes one
 *                               (B doubles, or NULL for 1).  From frames: row s of py_path is 1 on [lo, hi), lo = t0 for
 *                               s == s0, else frames[s - 1] (regular) or frames[s - 1] + 1 (modified); hi = t1 for
 *                               s == s1, else frames[s].  px_path[s, t] is 1 where t == frames[s].
 *
 * EDGE CASES, as include/rnnt_mi.h.
 *     no path (every path crosses -inf)          score -inf, frames -1, indicators zero, back the recursion's bits
 *     NaN or +inf on an edge of the rectangle    score NaN, frames -1, indicators NaN on the rectangle's edges and zero
 *                                                outside, back written (value unspecified; two runs give the same bits)
 *     boundary outside 0 <= s0 <= s1 <= S, 0 <= t0 <= t1 <= T
 *                                                score the invalid-arguments marker of include/rnnt.h, frames -1,
 *                                                indicators zero, back zero
 * Other samples are unaffected in every case.  Degenerate rectangles (s1 == s0, t1 == t0, the modified type with more
 * symbols than frames) follow the recursion.
 *
 * LIMITS.  S + 1 <= 4096, (T + 1) (S + 1) < 2^25, B (T + 1) (S + 1) < 2^32.  REFUSED with RNNT_STATUS_INVALID_VALUE before
 * anything is touched: a limit exceeded; S < 0, T < 1, minibatch < 1; a dtype code outside 0..3; loc != RNNT_GPU; a
 * required pointer that is NULL (py, scores, back; px and frames unless S == 0; in the edges entry frames, scores_device,
 * py_path and px_path likewise); one of px_path / py_path without the other; an output that overlaps an input or another
 * output, or that lies off an element boundary.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One call: sweep, traceback and, with both indicator pointers given, the edges (at scale 1). */
rnntStatus_t compute_rnnt_bestpath(const void* px, const void* py, const void* boundary, int S, int T, int minibatch,
                                   int modified, void* scores, int* frames, void* back, void* px_path, void* py_path,
                                   rnntOptions options, int dtype_code);

/* The indicators from the outputs of an earlier call (frames, device scores): the backward of score.  Reads neither px
 * nor py; enqueue only. */
rnntStatus_t compute_rnnt_bestpath_edges(const int* frames, const void* scores_device, const void* boundary,
                                         const void* grad_scale_device, int S, int T, int minibatch, int modified,
                                         void* px_path, void* py_path, rnntOptions options, int dtype_code);

#ifdef __cplusplus
}
#endif
