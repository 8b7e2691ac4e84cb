/* rnnt_ranges.h -- C-ABI of libwarprnnt_ranges.so: PRUNE RANGES FROM EDGE OCCUPATIONS, and the posterior mass a set of
 * windows keeps.  The pruned-transducer recipe runs a cheap lattice, takes window starts from its occupations and runs the
 * joiner and the pruned loss on those windows.  include/rnnt_mi.h returns the occupations px_grad / py_grad of ANY lattice a
 * caller can build (smoothed, delay-penalised, HAT-style, internal-LM-subtracted, regular or modified);
 * include/rnnt_pruned.h, rnnt_pstream.h, rnnt_joiner.h and rnnt_logprobs.h consume `ranges` int32 (B, T).  This library is
 * the step between the two -- k2's get_rnnt_prune_ranges -- with the rule of include/rnnt_pruned.h, a fixed order of every
 * addition, and the answer to "how much of the posterior do these windows keep".  A library of its own, so that a caller
 * of libwarprnnt.so never loads it.
 *
 * Conventions as the other include/rnnt_*.h: `rnntOptions` by value, of which only loc (must be RNNT_GPU) and stream (the
 * HIP stream everything is enqueued on) are read; dtype codes 0 fp32, 1 fp64, 2 bf16, 3 fp16, ONE code for both arrays.
 * The library takes NO workspace, allocates nothing, never synchronises and reads device memory on the device only: every
 * entry only enqueues and can be captured in a HIP graph.  No atomics: two calls give identical bits.
 *
 * INPUTS, all on the device, contiguous, READ-ONLY.  B = minibatch, S >= 0 symbols, T >= 1 frames.
 *     py_grad (B, S + 1, T)
 *     px_grad (B, S, T + 1) with modified == 0 (the regular type), (B, S, T) with modified != 0.  With S == 0 it is not
 *                               looked at.
 *     boundary (B, 4) int64     or NULL.  Only columns 2 and 3 are read: S_b and T_b, clamped into [0, S] and [0, T] as
 *                               include/rnnt_logprobs.h does (NULL: S and T).
 *     R                         the window width, 1 <= R <= S + 1
 *     step                      the largest advance of the start from one frame to the next, 1 <= step <= max(1, R - 1)
 * The occupations must be the UNSCALED ones (compute_rnnt_mi at scale 1, `return_grad=True`): non-negative.  Gradients that
 * carry a negative grad_output turn the argmax round.
 *
 * DEFINITION.  For t < T_b and 0 <= u <= S_b
 *     g[u] = double(py_grad[b, u, t]) + (u < S_b ? double(px_grad[b, u, t]) : 0.0)
 * -- the occupancy of node (u, t): the mass of its two out-edges.  The upcasts are exact and the sum is ONE IEEE fp64
 * addition.  Rows u > S_b and frames t >= T_b are never read (nor is column T of the regular px_grad).
 * With smax = max(0, S_b + 1 - R) every start s in [0, smax] has the window sum
 *     w(s) = (((0.0 + g[s]) + g[s + 1]) + ...) + g[min(s + R - 1, S_b)]
 * added from 0.0 in ASCENDING u, one IEEE fp64 addition per element: a host loop gets the same bits.  (This is the order of
 * compute_rnnt_prune_ranges_add's window kernel.)  COST: (smax + 1) R additions per column, by definition; a sliding sum
 * would change the bits and is not used.
 *   1. Frame t's RAW START is the s with the largest w(s), the smallest s among equals.  A NaN sum never wins; if no sum
 *      wins (every one is NaN), the start is 0.
 *   2. REPAIR, the passes of include/rnnt_pruned.h with S - 1 there replaced by `step`:
 *        clamp into [max(0, smax - (T_b - 1 - t) step), min(smax, t step)];
 *        a non-decreasing forward pass, s_t = max(s_t, s_{t-1});
 *        a backward pass, s_t = max(s_t, s_{t+1} - step);
 *        frames t >= T_b get 0.
 *      Then s_0 = 0, the steps lie in [0, step] and s_{T_b - 1} = smax: with R >= 2 consecutive windows overlap and a path
 *      through the windows exists.
 *   3. When smax > (T_b - 1) step no chain of windows reaches smax, and s_t = min(t step, smax).
 * For step = R - 1 condition 3 is include/rnnt_pruned.h's L_b > T_b (S - 1), and on the same occupancy the rule is
 * compute_rnnt_prune_ranges_add's.  (Both passes are integer maxima, so the order they are evaluated in does not change them:
 * s_t after the forward pass is the running maximum, after the backward pass max over j >= t of s_j - (j - t) step.)
 *
 * ENTRY 1, compute_rnnt_prune_ranges_occ: ranges (B, T) int32 by the rule above.  Every element is written.
 * ENTRY 2, compute_rnnt_range_coverage: kept (B, T) double.  For t < T_b
 *     kept[b, t] = w(clamp(ranges[b, t], 0, S_b)) / c        c = (((0.0 + g[0]) + g[1]) + ...) + g[S_b]
 * with both sums in the fixed ascending order above and the quotient ONE fp64 division; 0.0 when c == 0; 0.0 for t >= T_b.
 * Every element is written.  The ranges may come from anywhere: entry 1, compute_rnnt_prune_ranges_add, hand-made.
 *
 * EDGE CASES, each per column or sample; others are unaffected.
 *     all-equal occupations                      ties go to the smallest start, the repair then moves what it must
 *     all-zero occupations (no path)             every w(s) is 0.0: raw start 0; kept 0.0
 *     a NaN in a column                          the windows that hold it never win; kept of that column is NaN when its
 *                                                window or c holds it
 *     T_b == 0                                   ranges 0, kept 0.0
 *
 * LIMITS, those of include/rnnt_mi.h, so that anything it produces can be consumed: S + 1 <= 4096, (T + 1) (S + 1) < 2^25,
 * B (T + 1) (S + 1) < 2^32.  Any minibatch within them is taken (the samples go over the grid in slices of 65535).
 * REFUSED with RNNT_STATUS_INVALID_VALUE before anything is launched: a limit exceeded; S < 0, T < 1, minibatch < 1; R or
 * step outside the sets above; a dtype code outside 0..3; loc != RNNT_GPU; a required pointer that is NULL (every pointer
 * but boundary, and px_grad unless S == 0) or that lies off its element boundary; an output that overlaps an input.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Window starts from the occupations: raw starts, then the repair. */
rnntStatus_t compute_rnnt_prune_ranges_occ(const void* px_grad, const void* py_grad, const void* boundary, int S, int T,
                                           int minibatch, int modified, int R, int step, int* ranges, rnntOptions options,
                                           int dtype_code);

/* The share of every frame's occupancy that lies inside its window. */
rnntStatus_t compute_rnnt_range_coverage(const void* px_grad, const void* py_grad, const void* boundary, const int* ranges,
                                         int S, int T, int minibatch, int modified, int R, double* kept, rnntOptions options,
                                         int dtype_code);

#ifdef __cplusplus
}
#endif
