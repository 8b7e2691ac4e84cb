/* rnnt_mi.h -- C-ABI of libwarprnnt_mi.so: the transducer lattice over edge log-probabilities the CALLER built -- k2 /
 * fast_rnnt's `mutual_information_recursion(px, py, boundary)` -- with the edge occupations as its gradient.  No logits, no
 * softmax, no labels: the weights of the lattice's edges come in, the log of the total over the paths and the posterior of
 * every edge go out.  A library of its own, so that a caller of libwarprnnt.so never loads it.
 *
 * Conventions as include/rnnt_delay.h: `rnntOptions` by value, of which only loc (must be RNNT_GPU) and stream (the HIP
 * stream everything is enqueued on) are read; dtype codes 0 fp32, 1 fp64, 2 bf16, 3 fp16 (storage; 16-bit and fp32 storage
 * run an fp32 lattice and return float scores, fp64 an fp64 lattice and double scores).  Nothing here allocates memory, and
 * the enqueue-only entries do not synchronise (they can be captured in a HIP graph).
 *
 * INPUTS, all on the device, contiguous, natural logs.  B = minibatch, S >= 0 symbols, T >= 1 frames.
 *     py (B, S + 1, T)          py[b, s, t]: the edge that consumes frame t with s symbols emitted, (s, t) -> (s, t + 1)
 *     px, modified == 0 ("regular")   (B, S, T + 1)   px[b, s, t]: the edge that emits symbol s at frame position t,
 *                                                     (s, t) -> (s + 1, t)
 *     px, modified != 0               (B, S, T)       the symbol edge consumes frame t as well, (s, t) -> (s + 1, t + 1)
 *     boundary (B, 4) int64     [s0, t0, s1, t1] per sample, or NULL for [0, 0, S, T] everywhere
 * -inf is a legal weight and means "no edge" (k2 itself puts -inf in column T of px).  With S == 0 px and px_grad have no
 * element and the pointers are not looked at.
 *
 * RECURSION of sample b over the nodes s0 <= s <= s1, t0 <= t <= t1, p[s0, t0] = 0:
 *     regular    p[s, t] = logaddexp(p[s - 1, t] + px[s - 1, t]          (s > s0),
 *                                    p[s, t - 1] + py[s, t - 1]          (t > t0))
 *     modified   p[s, t] = logaddexp(p[s - 1, t - 1] + px[s - 1, t - 1]  (s > s0 and t > t0),
 *                                    p[s, t - 1] + py[s, t - 1]          (t > t0))
 *     score[b] = p[s1, t1]
 * the log of the total weight of the paths (s0, t0) -> (s1, t1): k2's sign, NOT a cost.  In the regular type column t1 of
 * px is a real set of edges (symbols can be emitted after the last frame).  Degenerate rectangles (s1 == s0 or t1 == t0)
 * follow the recursion, and so does the modified type with more symbols than frames: there is no path, the score is -inf.
 *
 * THE RECTANGLE'S EDGES of sample b:
 *     px   s0 <= s < s1,  t0 <= t <= t1 (regular)  or  t0 <= t < t1 (modified)
 *     py   s0 <= s <= s1, t0 <= t < t1
 * Input elements outside these sets are never read.
 *
 * GRADIENTS.  px_grad: shape and dtype of px; py_grad: those of py.  d score[b] / d px[b, s, t] is the posterior of that edge
 * under the path distribution -- the edge's occupation, inside [0, 1] -- times grad_scale_device[b] where the call takes
 * one (B values of the scores' type, or NULL for 1).  EVERY element of both arrays is written by every call that takes them;
 * elements outside the rectangle's edges are exact 0.  No atomics: two calls give identical bits.  The gradient arrays may
 * not overlap the inputs, each other or the workspace, and lie on element boundaries (RNNT_STATUS_INVALID_VALUE).
 *
 * EDGE CASES.  A sample without a path (every path crosses a -inf edge) scores -inf and gets exact-zero gradients, as k2's
 * guard gives: a -inf weight is routine and does not poison a batch.  A NaN or +inf on one of the rectangle's edges gives
 * that sample a NaN score, NaN gradients on the rectangle's edges and zeros outside it; other samples are unaffected.  A
 * boundary that breaks 0 <= s0 <= s1 <= S or 0 <= t0 <= t1 <= T gives the sample the invalid-arguments marker of
 * include/rnnt.h as its score and zero gradients; with host scores the one-call entry returns RNNT_STATUS_INVALID_VALUE.
 *
 * LIMITS.  S + 1 <= 4096, (T + 1) (S + 1) < 2^25, B (T + 1) (S + 1) < 2^32: otherwise RNNT_STATUS_INVALID_VALUE before
 * anything is touched.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of every entry below for this shape, type and dtype code. */
rnntStatus_t get_workspace_size_mi(int S, int T, int minibatch, int modified, int dtype_code, size_t* size_bytes);

/* One call: scores and, with both gradient pointers given (both, or both NULL), the gradients.  scores in DEVICE memory:
 * enqueue only.  scores in HOST memory: copied behind the last kernel and the stream synchronised; a score marker (bad
 * boundary) -> RNNT_STATUS_INVALID_VALUE. */
rnntStatus_t compute_rnnt_mi(const void* px, const void* py, const void* boundary, int S, int T, int minibatch, int modified,
                             void* scores, void* px_grad, void* py_grad, void* workspace, rnntOptions options,
                             int dtype_code);

/* Two phases.  The forward call writes device scores and, with prepare_backward != 0, leaves in the workspace what the
 * backward call needs (without it the lattice is swept forward only): between the two calls only the workspace must stay
 * alive.  The backward call writes both gradients, sample b times grad_scale_device[b]. */
rnntStatus_t compute_rnnt_mi_fwd(const void* px, const void* py, const void* boundary, int S, int T, int minibatch,
                                 int modified, void* scores_device, void* workspace, rnntOptions options, int dtype_code,
                                 int prepare_backward);
rnntStatus_t compute_rnnt_mi_bwd(void* px_grad, void* py_grad, const void* grad_scale_device, int S, int T, int minibatch,
                                 int modified, void* workspace, rnntOptions options, int dtype_code);

#ifdef __cplusplus
}
#endif
