/* rnnt_tdt_align.h -- C-ABI of libwarprnnt_tdt_align.so: the best path (Viterbi alignment) through the lattice of the
 * Token-and-Duration Transducer, per token the frame at which it is emitted and the duration the model chose for it.  A
 * library of its own, so that a caller of libwarprnnt.so or libwarprnnt_tdt.so never loads it.
 *
 * Inputs, lattice, edge weights, sigma, the duration rules, label clamping and the limits are those of include/rnnt_tdt.h,
 * word for word:
 *
 * Conventions as include/rnnt.h: `rnntOptions` by value (loc must be RNNT_GPU; maxT = time dimension, maxU = max label
 * length + 1; blank_label = the blank's token column; stream = the HIP stream everything is enqueued on), dtype codes 0 fp32,
 * 1 fp64, 2 bf16, 3 fp16 (storage; 16-bit and fp32 storage run an fp32 lattice, fp64 an fp64 lattice), flat labels
 * (N, maxU - 1) int32, lengths (N) int32, all on the device.  Nothing here allocates memory or synchronises: the call only
 * enqueues (it can be captured in a HIP graph).
 *
 * INPUTS.  Raw logits (N, maxT, maxU, A + D).  The first A columns are tokens, blank (blank_label) included; the last D are the
 * logits of the durations durations[0 .. D-1].  For cell (t, u):
 *     lp_tok(t, u, k) = log_softmax(z[:A])[k] - sigma          (sigma: TDT's logit under-normalisation, natural log)
 *     lp_dur(t, u, j) = log_softmax(z[A:])[j]
 * DURATIONS: a HOST int array (its values go into kernel arguments); 1 <= D <= 8, strictly increasing, non-negative, the
 * largest in [1, 64].  Anything else: RNNT_STATUS_INVALID_VALUE.
 *
 * LATTICE of sample b: nodes (t, u), 0 <= t < T_b, 0 <= u <= L_b, and the terminal node (T_b, L_b).
 *     blank edges (t, u) -> (t + d, u) for every d > 0, weight lp_tok(blank) + lp_dur(j), when t + d < T_b, or when
 *                 t + d == T_b and u == L_b (into the terminal node);
 *     label edges (t, u) -> (t + d, u + 1) for every d (0 included), weight lp_tok(y_u) + lp_dur(j), when u < L_b and
 *                 t + d < T_b.
 * Blank never takes duration 0.  Labels outside [0, A) are clamped into it.
 *
 * OUTPUTS, per sample b:
 *     score[b]      double (always fp64): the natural-log weight of the single best path (0, 0) -> terminal, sigma terms
 *                   included; score[b] <= -cost[b] of compute_tdt_loss.
 *     frames[b, u]  int32 (N, maxU - 1): for u < L_b the frame t of the source node of label u's edge
 *                   (t, u) -> (t + d, u + 1), non-decreasing in u; -1 for u >= L_b.
 *     durs[b, u]    int32 (N, maxU - 1): the duration VALUE d (not its index) of that edge, so
 *                   frames[b, u] + durs[b, u] <= frames[b, u + 1]; -1 for u >= L_b.
 * The blank jumps between two labels are not returned (given frames and durs, the best filling is a shortest-path problem of
 * its own).
 *
 * TIES.  A cell's in-edges are tried in the order duration index 0 .. D-1, blank before label for each; a candidate replaces
 * the current best only if strictly greater.  The same order applies to the final blanks into the terminal node.  The rule is
 * about the sums as the kernel computes them (base-2 logs, relative to a per-diagonal fp64 offset).
 *
 * NON-FINITE INPUTS AND EDGE CASES (compute_rnnt_align's conventions).  No finite path: score = -inf.  A NaN / +inf /
 * all-(-inf) row inside the lattice (token or duration part): score = NaN.  Lengths that do not fit the tensor (T_b outside
 * [1, maxT], L_b outside [0, maxU - 1]): score = NaN.  In all three cases that sample's frames and durs are all -1; other
 * samples are unaffected, and none of these is an error status.  Rows with t >= T_b or u > L_b are padding: never read.
 *
 * LIMITS.  maxU <= 4096, blank_label in [0, A), N maxT maxU < 2^32 rows, maxT maxU < 2^25: otherwise
 * RNNT_STATUS_INVALID_VALUE, as are NULL pointers and loc != RNNT_GPU -- refused before anything is launched.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of compute_tdt_align for this shape, number of durations and dtype code. */
rnntStatus_t get_workspace_size_tdt_align(int maxT, int maxU, int minibatch, int num_durations, int dtype_code,
                                          size_t* size_bytes);

/* score_device (N) double, frames_device and durs_device (N, maxU - 1) int32, all in device memory (with maxU == 1 the two
 * arrays are empty: any non-NULL pointer, never written). */
rnntStatus_t compute_tdt_align(const void* activations, const int* durations, int num_durations, float sigma,
                               const int* flat_labels, const int* label_lengths, const int* input_lengths,
                               int alphabet_size, int minibatch, void* score_device, void* frames_device,
                               void* durs_device, void* workspace, rnntOptions options, int dtype_code);

#ifdef __cplusplus
}
#endif
