/* rnnt_sample.h -- C-ABI of libwarprnnt_sample.so: ALIGNMENTS DRAWN from the posterior of the transducer lattice over edge
 * log-probabilities the caller built, p(path) ~ exp W(path) -- the lattice of include/rnnt_mi.h (which sums the paths),
 * include/rnnt_bestpath.h (which maximises over them) and include/rnnt_expect.h (which takes expectations of additive
 * costs).  One forward sweep, then K walks back from the terminal node that choose every in-edge with its posterior share:
 * the product of the shares along a walk is exp(W - log Z), so the walk is an exact sampler, without rejection or burn-in.
 * With the weight of a given path as a function of px / py (and its gradient, the path's edge indicator), Monte-Carlo and
 * score-function estimators of objectives that are NOT sums over edges, hard-alignment losses and importance weights are a
 * few lines on top.  A library of its own, so that a caller of libwarprnnt.so never loads it.  It takes NO workspace and
 * holds NO random generator: the uniforms are an input.
 *
 * Conventions and inputs are exactly those of include/rnnt_expect.h: `rnntOptions` by value, of which only loc (must be
 * RNNT_GPU) and stream (the HIP stream everything is enqueued on) are read; dtype codes 0 fp32, 1 fp64, 2 bf16, 3 fp16
 * (the storage of px, py, px_acc, py_acc).  Nothing here allocates memory; every entry only enqueues (it can be captured
 * in a HIP graph, on one branch); every output is in DEVICE memory, caller-allocated, and every element of it is written
 * by every call that takes it.
 *
 * INPUTS, all on the device, contiguous, natural logs, READ-ONLY.  B = minibatch, S >= 0 symbols, T >= 1 frames, K walks.
 *     py (B, S + 1, T)          py[b, s, t]: the edge that consumes frame t with s symbols emitted, (s, t) -> (s, t + 1)
 *     px, modified == 0 ("regular")   (B, S, T + 1)   px[b, s, t]: the edge that emits symbol s at frame position t,
 *                                                     (s, t) -> (s + 1, t)
 *     px, modified != 0               (B, S, T)       the symbol edge consumes frame t as well, (s, t) -> (s + 1, t + 1)
 *     boundary (B, 4) int64     [s0, t0, s1, t1] per sample, or NULL for [0, 0, S, T] everywhere
 *     uniforms (B, K, S + T) float32 in [0, 1), upcast exactly.  The node (s, t) of walk k consults
 *                               uniforms[b, k, (s - s0) + (t - t0) - 1]: every node of a path has an index of its own.
 *                               Elements that no decision consults are not read.
 * -inf is a legal weight and means "no edge".  With S == 0 px, px_acc, frames and uniforms are not looked at (no decision
 * is ever made).  Input elements outside the rectangle's edges (include/rnnt_mi.h) are never read.
 *
 * FORWARD SWEEP of sample b over the nodes s0 <= s <= s1, t0 <= t <= t1; t' = t (regular) or t - 1 (modified);
 * a[s0, t0] = 0, a missing in-edge counting as -inf:
 *     x = a[s - 1, t'] + px[s - 1, t']          y = a[s, t - 1] + py[s, t - 1]          a[s, t] = logaddexp(x, y)
 * in fp64 on exactly upcast values, for every storage type.  A candidate of -inf is SELECTED OUT: a[s, t] is then the other
 * candidate bit for bit.
 *     alpha (B, S + 1, T + 1) double   a of every node, absolute coordinates; -inf outside the rectangle's nodes
 *     scores (B) double                a[s1, t1]: log Z, compute_rnnt_mi's score and nodes[..., 0] of compute_rnnt_expect at
 *                                      the terminal
 *
 * WALK k of sample b, from (s, t) = (s1, t1) down to (s0, t0).  At s == s0 the frame in-edge.  Otherwise, in fp64,
 *     r = exp(alpha[s - 1, t'] + px[s - 1, t'] - alpha[s, t])       u = uniforms[b, k, (s - s0) + (t - t0) - 1]
 * and the symbol in-edge iff u < r.  That comparison is the whole rule: a forced symbol edge has r == 1 exactly, a -inf
 * symbol candidate r == 0.
 *     frames (B, K, S) int32    include/rnnt_bestpath.h's convention: for s0 <= s < s1 the t of the symbol edge px[b, s, t] on
 *                               the walk, tensor coordinates; -1 elsewhere
 *     weights (B, K) double     W(path): from 0.0, each edge's exactly upcast weight added in walk order (the terminal's
 *                               in-edge first), ONE IEEE addition per edge.  A host fp64 loop over the same frames gets the
 *                               same bits.  log q(path) = weights - scores.
 *
 * GIVEN PATHS (entries 3 and 4): `frames` (B, K, S) from wherever it came -- a sampler, compute_rnnt_bestpath (K = 1), a
 * forced alignment.  A row is a path of its rectangle iff for s0 <= s < s1 its values lie in [t0, t1] and do not decrease
 * (regular), or lie in [t0, t1) and strictly increase (modified); values outside [s0, s1) are not looked at.  With
 * s1 == s0 every row is the one path of frame edges.
 *     weights (B, K) double     W of the path.  ORDER of the additions (fixed; two runs give the same bits): 64 partial sums,
 *                               partial l taking from 0.0 the symbol edges of the rows s0 + l, s0 + l + 64, ... in
 *                               ascending s, then row by row in ascending s the frame edges py[s, t] of the row's interval
 *                               [lo, hi) at t = lo + l, lo + l + 64, ...; the partials are then added pairwise, l with
 *                               l ^ 32, 16, 8, 4, 2, 1.  Every value is an fp64 sum of n = (number of edges) terms, so
 *                               |weights - W| <= (n - 1) 2^-53 / (1 - (n - 1) 2^-53) sum |w_e| for finite weights; a -inf
 *                               edge gives -inf exactly.  A row that is no path: NaN.
 *     px_acc, py_acc            shapes and dtypes of px / py: sum over k in ASCENDING order of coeff[b, k] 1[edge on path k],
 *                               accumulated in fp64 without atomics and rounded ONCE to the storage type; bit-identical
 *                               from run to run; exact 0 outside the rectangle's edges.  coeff (B, K) double, or NULL
 *                               for 1.  This is the backward of sum_k coeff_k W(path_k); px and py are not read.  The
 *                               edges of a row follow from frames as include/rnnt_bestpath.h states for px_path / py_path:
 *                               row s of py is on the path on [lo, hi), lo = t0 for s == s0, else frames[s - 1] (regular)
 *                               or frames[s - 1] + 1 (modified); hi = t1 for s == s1, else frames[s]; px[s, t] where
 *                               t == frames[s].  A row that is no path contributes nothing (selected out: its coeff is
 *                               not looked at).
 *
 * EDGE CASES, each per sample; other samples are unaffected.
 *     no path (every path crosses -inf)          score -inf, frames -1, weights -inf
 *     NaN or +inf on an edge of the rectangle    score NaN, frames -1, weights NaN; alpha written (values unspecified)
 *     boundary outside 0 <= s0 <= s1 <= S, 0 <= t0 <= t1 <= T
 *                                                score the invalid-arguments marker of include/rnnt.h, alpha -inf,
 *                                                frames -1, weights NaN; entries 3 and 4: weights NaN, accumulators 0
 *     entries 3 and 4, a row of frames that is no path
 *                                                weight NaN; contributes nothing to the accumulators
 * The sampler's rows of a sample without a path (all -1) are no paths where s1 > s0, so they add nothing in entry 4; with
 * s1 == s0 the all -1 row IS the one path of frame edges, whatever its weight: entry 4 reads neither px nor py.
 * Degenerate rectangles (s1 == s0, t1 == t0, the modified type with more symbols than frames) follow the recursion.
 * compute_rnnt_sample_walk trusts `alpha` and `scores_device` to come from compute_rnnt_sample on the same px, py and
 * boundary; with others it stays inside its buffers and its results are unspecified.
 *
 * LIMITS.  S + 1 <= 1024, (T + 1) (S + 1) < 2^25, B (T + 1) (S + 1) < 2^32, 1 <= K <= 1024, B K max(S, 1) < 2^31.  REFUSED
 * with RNNT_STATUS_INVALID_VALUE before anything is touched: a limit exceeded; S < 0, T < 1, minibatch < 1; a dtype code
 * outside 0..3; loc != RNNT_GPU; a required pointer that is NULL (every pointer but boundary and coeff; px, px_acc, frames
 * and uniforms unless S == 0); an output that overlaps an input or another output, or a buffer that lies off an element
 * boundary.  Inputs may alias inputs.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The forward sweep followed by K walks per sample. */
rnntStatus_t compute_rnnt_sample(const void* px, const void* py, const void* boundary, const float* uniforms, int S, int T,
                                 int minibatch, int K, int modified, void* scores, void* alpha, int* frames, void* weights,
                                 rnntOptions options, int dtype_code);

/* K more walks from the alpha and scores of an earlier compute_rnnt_sample; no sweep. */
rnntStatus_t compute_rnnt_sample_walk(const void* px, const void* py, const void* boundary, const void* alpha,
                                      const void* scores_device, const float* uniforms, int S, int T, int minibatch, int K,
                                      int modified, int* frames, void* weights, rnntOptions options, int dtype_code);

/* W of the paths given by frames. */
rnntStatus_t compute_rnnt_path_weights(const void* px, const void* py, const void* boundary, const int* frames, int S, int T,
                                       int minibatch, int K, int modified, void* weights, rnntOptions options,
                                       int dtype_code);

/* sum_k coeff[b, k] 1[edge on path k]: the backward of sum_k coeff_k W(path_k).  Reads neither px nor py. */
rnntStatus_t compute_rnnt_path_edges(const int* frames, const void* coeff, const void* boundary, int S, int T, int minibatch,
                                     int K, int modified, void* px_acc, void* py_acc, rnntOptions options, int dtype_code);

#ifdef __cplusplus
}
#endif
