/* rnnt_hat.h -- C-ABI of libwarprnnt_hat.so: the Hybrid Autoregressive Transducer (HAT) loss (Variani et al., ICASSP 2020),
 * the transducer with a factorised blank.  A library of its own, so that a caller of libwarprnnt.so never loads it.
 *
 * Conventions as include/rnnt.h: `rnntOptions` by value (loc must be RNNT_GPU; maxT = time dimension, maxU = max label
 * length + 1; blank_label = the blank's column; stream = the HIP stream everything is enqueued on), dtype codes 0 fp32,
 * 1 fp64, 2 bf16, 3 fp16 (storage; 16-bit and fp32 storage run an fp32 lattice and return float costs, fp64 an fp64 lattice
 * and double costs), flat labels (N, maxU - 1) int32, lengths (N) int32, all on the device.  Nothing here allocates memory,
 * and the enqueue-only entries do not synchronise (they can be captured in a HIP graph).
 *
 * INPUTS.  Raw logits z (N, maxT, maxU, A), blank_label in [0, A), A >= 2.  For cell (t, u), with b = sigmoid(z_blank):
 *     lp_blank(t, u)    = log b                  = -softplus(-z_blank)
 *     lp_label(t, u, k) = log(1 - b) + z_k - logsumexp_{j != blank} z_j = -softplus(z_blank) + log q_k       (k != blank)
 * q = the softmax over the A - 1 non-blank columns; softplus(x) = max(x, 0) + log1p(exp(-|x|)), so |z_blank| = 80 in fp32
 * (or bf16) storage gives finite, correct log-probabilities on both sides.
 *
 * LATTICE, COST, TERMINAL BLANK: those of include/rnnt.h.  Nodes (t, u), 0 <= t < T_b, 0 <= u <= L_b; blank edges
 * (t, u) -> (t + 1, u), label edges (t, u) -> (t, u + 1) with label y_u, and the blank out of (T_b - 1, L_b) closes a path.
 * cost_b = -log sum over the paths of exp(sum of the weights), natural log.
 *
 * LABELS.  A label equal to blank_label has no probability under HAT.  Such a label among a sample's first L_b labels makes
 * that sample's cost NaN and the gradient of its in-lattice rows NaN (the treatment of a poisoned row, below); other samples
 * are unaffected, labels behind L_b are never looked at.  Labels outside [0, A) are clamped into it, as in include/rnnt.h.
 *
 * GRADIENT (d cost_b / d z).  For a row (t, u) inside the lattice, cb / cl = the posteriors of its blank / label out-edge,
 * c = cb + cl:
 *     blank column        c b - cb
 *     column k != blank   cl q_k - cl [k == y_u]
 * Rows with t >= T_b or u > L_b are padding: never read, gradient exactly 0.  gradients == activations (in place) is
 * allowed; other overlaps are not (RNNT_STATUS_INVALID_VALUE).
 *
 * NON-FINITE INPUTS AND EDGE CASES.  A NaN anywhere in an in-lattice row, a +inf label logit, or a row whose label logits
 * are all -inf poison that sample only: NaN cost, NaN gradients on its in-lattice rows, zeros on its padding.  z_blank = -inf
 * and z_blank = +inf are legitimate limits (b = 0, b = 1) and give the limit values of the cost and the gradient.  A sample
 * with no path of positive probability left (for instance b = 0 in the terminal cell) costs +inf, with NaN in-lattice
 * gradients.  Lengths that do not fit the tensor (T_b outside [1, maxT], L_b outside [0, maxU - 1]) give the sample the
 * invalid-arguments cost marker of include/rnnt.h (with host costs the one-call entry returns RNNT_STATUS_INVALID_VALUE)
 * and zero gradients.
 *
 * LIMITS.  2 <= A <= 2^23, maxU <= 1024, maxT maxU < 2^29, one sample's (maxT + maxU + 31) x ceil8(maxU) table of value
 * pairs below 2 GB, N maxT maxU < 2^32 rows: otherwise RNNT_STATUS_INVALID_VALUE.  The tensors themselves may hold more than
 * 2^31 elements.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of every entry below for this shape and dtype code. */
rnntStatus_t get_workspace_size_hat(int maxT, int maxU, int minibatch, int dtype_code, size_t* size_bytes);

/* One call: costs and (gradients != NULL) the gradient.  costs in DEVICE memory: enqueue only.  costs in HOST memory: copied
 * behind the last kernel and the stream synchronised; a cost marker (bad lengths) -> RNNT_STATUS_INVALID_VALUE. */
rnntStatus_t compute_hat_loss(const void* activations, void* gradients, const int* flat_labels, const int* label_lengths,
                              const int* input_lengths, int alphabet_size, int minibatch, void* costs, void* workspace,
                              rnntOptions options, int dtype_code);

/* Two phases.  The forward call writes device costs and, with prepare_backward != 0, leaves in the workspace what the
 * backward call needs (the per-row gradient records): between the two calls only the workspace must stay alive, and the
 * activations unchanged.  The backward call writes the gradient; grad_scale_device (N values of the costs' type, or NULL
 * for 1) multiplies sample b's gradient. */
rnntStatus_t compute_hat_loss_fwd(const void* activations, const int* flat_labels, const int* label_lengths,
                                  const int* input_lengths, int alphabet_size, int minibatch, void* costs_device,
                                  void* workspace, rnntOptions options, int dtype_code, int prepare_backward);
rnntStatus_t compute_hat_loss_bwd(const void* activations, void* gradients, const void* grad_scale_device,
                                  int alphabet_size, int minibatch, void* workspace, rnntOptions options, int dtype_code);

#ifdef __cplusplus
}
#endif
