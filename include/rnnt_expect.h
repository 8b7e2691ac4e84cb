/* rnnt_expect.h -- C-ABI of libwarprnnt_expect.so: the EXPECTED COST of a path of the transducer lattice over edge
 * log-probabilities the caller built -- the expectation semiring on the lattice of include/rnnt_mi.h (which sums the
 * paths) and include/rnnt_bestpath.h (which maximises over them).  The weights AND an additive cost of every edge come in;
 * log Z, E[C] under the lattice posterior p(path) ~ exp W(path), the prefix pairs of every node and the gradients of both
 * scalars go out.  d E[C] / d weight is a covariance: no number of calls of libwarprnnt_mi.so yields it.  Minimum expected
 * latency (cost of a symbol edge = its frame), alignment entropy (cost = weight: H = log Z - E[W]) and Bayes-risk style
 * objectives are this one primitive.  A library of its own, so that a caller of libwarprnnt.so never loads it.  It takes NO
 * workspace: the one array the forward sweep leaves behind, `nodes`, is an output the caller allocates.
 *
 * Conventions and inputs are exactly those of include/rnnt_bestpath.h: `rnntOptions` by value, of which only loc (must be
 * RNNT_GPU) and stream (the HIP stream everything is enqueued on) are read; dtype codes 0 fp32, 1 fp64, 2 bf16, 3 fp16
 * (the storage of px, py, cx, cy and the four gradients).  Nothing here allocates memory, and the forms with scores in
 * device memory only enqueue (they can be captured in a HIP graph).
 *
 * INPUTS, all on the device, contiguous, natural logs, READ-ONLY.  B = minibatch, S >= 0 symbols, T >= 1 frames.
 *     py (B, S + 1, T)          py[b, s, t]: the edge that consumes frame t with s symbols emitted, (s, t) -> (s, t + 1)
 *     px, modified == 0 ("regular")   (B, S, T + 1)   px[b, s, t]: the edge that emits symbol s at frame position t,
 *                                                     (s, t) -> (s + 1, t)
 *     px, modified != 0               (B, S, T)       the symbol edge consumes frame t as well, (s, t) -> (s + 1, t + 1)
 *     cx, cy                    shape and dtype of px / py: the additive cost of each edge.  Costs may alias the weights
 *                               (cx == px, cy == py).
 *     boundary (B, 4) int64     [s0, t0, s1, t1] per sample, or NULL for [0, 0, S, T] everywhere
 * -inf is a legal weight and means "no edge".  With S == 0 px, cx and their gradients have no element and the pointers
 * are not looked at.  Input elements outside the rectangle's edges (include/rnnt_mi.h) are never read.
 *
 * FORWARD of sample b over the nodes s0 <= s <= s1, t0 <= t <= t1; t' = t (regular) or t - 1 (modified); a[s0, t0] = 0,
 * A[s0, t0] = 0, a missing in-edge counting as -inf:
 *     x = a[s - 1, t'] + px[s - 1, t']          y = a[s, t - 1] + py[s, t - 1]
 *     a[s, t] = logaddexp(x, y)                 r = exp(x - a[s, t])              -- the symbol in-edge's share
 *     A[s, t] = r (A[s - 1, t'] + cx[s - 1, t']) + (1 - r) (A[s, t - 1] + cy[s, t - 1])
 * A term whose candidate is -inf is SELECTED OUT, not multiplied: its cost is never looked at, so -inf or NaN costs on -inf
 * edges are legal and c = w works.  An unreachable node has a = -inf, A = 0.
 *     score[b]  = a[s1, t1]     log Z of the rectangle: k2's sign, NOT a cost; equal to compute_rnnt_mi's score
 *     expect[b] = A[s1, t1]     E over the paths pi, p(pi) ~ exp W(pi), of the sum of c_e over the edges of pi
 * BACKWARD mirrors it from bt[s1, t1] = 0, Bc[s1, t1] = 0: bt the log weight of the suffixes of a node, Bc their expected
 * cost.  For an edge e = u -> v of weight w and cost c:
 *     occ_e = exp(a[u] + w + bt[v] - score)
 *     d expect / d c_e = occ_e      d expect / d w_e = occ_e (A[u] + c + Bc[v] - expect)      d score / d w_e = occ_e
 * The backward entry takes two per-sample scales, g_expect[b] and g_score[b] (doubles; NULL means 1 and 0), and writes
 *     px_grad, py_grad = g_expect occ (A + c + Bc - expect) + g_score occ         cx_grad, cy_grad = g_expect occ
 * (an edge of occupation exactly 0 has gradients exactly 0: selected, not multiplied).  Hence the alignment entropy is
 * score - expect(c = w); autograd sums the two gradients into px itself.
 *
 * ARITHMETIC.  Every stored weight and cost is upcast exactly to fp64; a, A, bt and Bc are fp64 for every storage type.
 * Gradients are rounded once to the storage type.
 *
 * OUTPUTS, all caller-allocated; every element is written by every call that takes them.
 *     scores, expect (B) double device or host memory, as in compute_rnnt_mi.  Host memory: copied behind the last kernel and
 *                               the stream synchronised; a bad-boundary marker then gives RNNT_STATUS_INVALID_VALUE.
 *     nodes (B, S + 1, T + 1, 2) double
 *                               the pair (a, A) of every node of the tensor, absolute coordinates; (-inf, 0) outside the
 *                               rectangle's nodes.  Prefix log-probability and expected prefix cost.  The pair is the
 *                               array's element: it starts on a 16-byte boundary.
 *     px_grad, py_grad          both given or both NULL; shapes and dtypes of px / py; exact 0 outside the rectangle's edges.
 *     cx_grad, cy_grad          both given or both NULL (they may be NULL where px_grad / py_grad are given), likewise.
 *
 * EDGE CASES, as include/rnnt_mi.h.
 *     no path (every path crosses -inf)          score -inf, expect 0, all gradients exact 0
 *     NaN or +inf WEIGHT on an edge of the rectangle
 *                                                score and expect NaN; all four gradients NaN on the rectangle's edges
 *                                                and 0 outside; nodes written (values unspecified)
 *     boundary outside 0 <= s0 <= s1 <= S, 0 <= t0 <= t1 <= T
 *                                                score the invalid-arguments marker of include/rnnt.h, expect 0,
 *                                                gradients 0, nodes (-inf, 0)
 *     a non-finite COST on a reachable edge of finite weight
 *                                                expect NaN for that sample; gradients unspecified, but the same bits
 *                                                on a rerun
 * Other samples are unaffected in every case.  Degenerate rectangles (s1 == s0, t1 == t0, the modified type with more
 * symbols than frames) follow the recursion.
 *
 * LIMITS.  S + 1 <= 1024, (T + 1) (S + 1) < 2^25, B (T + 1) (S + 1) < 2^32.  REFUSED with RNNT_STATUS_INVALID_VALUE before
 * anything is touched: a limit exceeded; S < 0, T < 1, minibatch < 1; a dtype code outside 0..3; loc != RNNT_GPU; a
 * required pointer that is NULL (py, cy, scores, expect, nodes; px and cx unless S == 0; in the backward entry
 * scores_device, expect_device and py_grad, px_grad unless S == 0); one of px_grad / py_grad without the other; one of
 * cx_grad / cy_grad without the other, or cost gradients without weight gradients; an output that overlaps an input or
 * another output, or that lies off an element boundary.  Inputs may alias inputs.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One call: the forward sweep and, with gradient pointers given, the backward sweep at scales 1 and 0. */
rnntStatus_t compute_rnnt_expect(const void* px, const void* py, const void* cx, const void* cy, const void* boundary,
                                 int S, int T, int minibatch, int modified, void* scores, void* expect, void* nodes,
                                 void* px_grad, void* py_grad, void* cx_grad, void* cy_grad, rnntOptions options,
                                 int dtype_code);

/* The forward sweep alone; scores and expect in device memory; enqueue only. */
rnntStatus_t compute_rnnt_expect_fwd(const void* px, const void* py, const void* cx, const void* cy, const void* boundary,
                                     int S, int T, int minibatch, int modified, void* scores_device, void* expect_device,
                                     void* nodes, rnntOptions options, int dtype_code);

/* The backward sweep from the outputs of a forward call; cx_grad / cy_grad may both be NULL; enqueue only. */
rnntStatus_t compute_rnnt_expect_bwd(const void* px, const void* py, const void* cx, const void* cy, const void* boundary,
                                     const void* nodes, const void* scores_device, const void* expect_device,
                                     const void* g_expect_device, const void* g_score_device, int S, int T, int minibatch,
                                     int modified, void* px_grad, void* py_grad, void* cx_grad, void* cy_grad,
                                     rnntOptions options, int dtype_code);

#ifdef __cplusplus
}
#endif
