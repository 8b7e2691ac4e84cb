/* rnnt_mblank.h -- C-ABI of libwarprnnt_mblank.so: the multi-blank transducer loss (Xu et al., "Multi-blank Transducers for
 * Speech Recognition", ICASSP 2023; NeMo's MultiblankRNNTLoss).  A library of its own, so that a caller of libwarprnnt.so
 * never loads it.
 *
 * Conventions as include/rnnt_tdt.h: `rnntOptions` by value (loc must be RNNT_GPU; maxT = time dimension, maxU = max label
 * length + 1; blank_label = the standard blank's column; stream = the HIP stream everything is enqueued on), dtype codes 0
 * fp32, 1 fp64, 2 bf16, 3 fp16 (storage; 16-bit and fp32 storage run an fp32 lattice and return float costs, fp64 an fp64
 * lattice and double costs), flat labels (N, maxU - 1) int32, lengths (N) int32, all on the device.  Nothing here allocates
 * memory, and the enqueue-only entries do not synchronise (they can be captured in a HIP graph).
 *
 * INPUTS.  Raw logits (N, maxT, maxU, A), ONE softmax over all A columns.  For cell (t, u):
 *     lp(t, u, k) = log_softmax(z)[k] - sigma                  (sigma: the logit under-normalisation, natural log)
 * The standard blank is column blank_label.  BIG BLANKS: two HOST int arrays of length K (their values go into kernel
 * arguments), big_blank_columns[i] = the column of big blank i, big_blank_durations[i] = the frames it consumes.
 * 0 <= K <= 8 (K == 0: both arrays may be NULL); the columns distinct, inside [0, A) and different from blank_label; the
 * durations strictly increasing and inside [2, 64].  Anything else: RNNT_STATUS_INVALID_VALUE.
 *
 * LATTICE of sample b: nodes (t, u), 0 <= t < T_b, 0 <= u <= L_b, and the terminal node (T_b, L_b).
 *     label edges (t, u) -> (t, u + 1), weight lp(y_u), when u < L_b;
 *     blank edges (t, u) -> (t + d, u), d = 1 for the standard blank and d = big_blank_durations[i] for big blank i, weight
 *                 lp of the blank's own column, when t + d < T_b, or when t + d == T_b and u == L_b (into the terminal
 *                 node).  An edge that would overshoot T_b does not exist.
 * cost_b = -log sum over the paths (0, 0) -> terminal of exp(sum of the weights).  With K = 0 and sigma = 0 this is
 * compute_rnnt_loss_async of include/rnnt.h on the same tensor.
 *
 * GRADIENT (d cost_b / d logits).  gamma_e = posterior of edge e; for a row (t, u) inside the lattice, c = the sum of gamma
 * over all its out-edges:
 *     column k     c softmax_k - sum of gamma_e over the row's out-edges e that use column k
 * A label that equals blank_label or a big-blank column is legal here: that column then carries both edges' posteriors,
 * the true derivative.  Rows with t >= T_b or u > L_b are padding: never read, gradient exactly 0.  gradients ==
 * activations (in place) is allowed; other overlaps are not (RNNT_STATUS_INVALID_VALUE).
 *
 * NON-FINITE INPUTS AND EDGE CASES.  A NaN / +inf / all-(-inf) row inside the lattice gives its sample a NaN cost and NaN
 * gradients on its in-lattice rows; other samples are unaffected.  A sample with no path to the terminal node costs +inf,
 * with NaN in-lattice gradients.  Lengths that do not fit the tensor (T_b outside [1, maxT], L_b outside [0, maxU - 1])
 * give the sample the invalid-arguments cost marker of include/rnnt.h (with host costs the one-call entry returns
 * RNNT_STATUS_INVALID_VALUE) and zero gradients.
 *
 * LIMITS.  maxU <= 4096, A <= 2^23, blank_label in [0, A), N maxT maxU < 2^32 rows, maxT maxU < 2^25: otherwise
 * RNNT_STATUS_INVALID_VALUE.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of every entry below for this shape, number of big blanks (0 .. 8) and dtype code. */
rnntStatus_t get_workspace_size_mblank(int maxT, int maxU, int minibatch, int num_big_blanks, int dtype_code,
                                       size_t* size_bytes);

/* One call: costs and (gradients != NULL) the gradient.  costs in DEVICE memory: enqueue only.  costs in HOST memory: copied
 * behind the last kernel and the stream synchronised; a cost marker (bad lengths) -> RNNT_STATUS_INVALID_VALUE. */
rnntStatus_t compute_mblank_loss(const void* activations, void* gradients, const int* big_blank_columns,
                                 const int* big_blank_durations, int num_big_blanks, float sigma, const int* flat_labels,
                                 const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch,
                                 void* costs, void* workspace, rnntOptions options, int dtype_code);

/* Two phases.  The forward call writes device costs and, with prepare_backward != 0, leaves in the workspace what the
 * backward call needs (the per-row gradient records): between the two calls only the workspace must stay alive, and the
 * activations unchanged.  The backward call takes the same big blanks and blank_label and writes the gradient;
 * grad_scale_device (N values of the costs' type, or NULL for 1) multiplies sample b's gradient. */
rnntStatus_t compute_mblank_loss_fwd(const void* activations, const int* big_blank_columns, const int* big_blank_durations,
                                     int num_big_blanks, float sigma, const int* flat_labels, const int* label_lengths,
                                     const int* input_lengths, int alphabet_size, int minibatch, void* costs_device,
                                     void* workspace, rnntOptions options, int dtype_code, int prepare_backward);
rnntStatus_t compute_mblank_loss_bwd(const void* activations, void* gradients, const void* grad_scale_device,
                                     const int* big_blank_columns, const int* big_blank_durations, int num_big_blanks,
                                     int alphabet_size, int minibatch, void* workspace, rnntOptions options,
                                     int dtype_code);

#ifdef __cplusplus
}
#endif
