/* rnnt_pstream.h -- C-ABI of libwarprnnt_pstream.so: the pruned RNN-T loss (Kuang et al., Interspeech 2022) with the two more
 * arguments of k2's `rnnt_loss_pruned` that streaming recipes set: rnnt_type ("regular" or "modified") and delay_penalty
 * (Kang et al., "Delay-penalized transducer for low-latency streaming ASR", 2022).  A library of its own, so that a caller
 * of libwarprnnt.so or libwarprnnt_pruned.so never loads it.
 *
 * Conventions as include/rnnt_pruned.h and include/rnnt_delay.h: `rnntOptions` by value (loc must be RNNT_GPU; maxT = time
 * dimension, maxU = max label length + 1; blank_label = the blank's column; stream = the HIP stream everything is enqueued
 * on), dtype codes 0 fp32, 1 fp64, 2 bf16, 3 fp16 (storage; 16-bit and fp32 storage run an fp32 lattice and return float
 * costs, fp64 an fp64 lattice and double costs), flat labels (N, maxU - 1) int32, lengths (N) int32, all on the device.
 * Nothing here allocates memory, and the enqueue-only entries do not synchronise (they can be captured in a HIP graph).
 *
 * INPUTS.  Raw logits z (N, maxT, S, A), ONE softmax over all A columns of a row, 1 <= S <= maxU.
 *   ranges      int32 (N, maxT) on the device: row (b, t, k) of the tensor is the joint output of lattice state
 *               u = ranges[b, t] + k (the start-per-frame convention of include/rnnt_pruned.h; k2's ranges[:, :, 0]).
 *   rnnt_type   0 regular, 1 modified.  Any other value: RNNT_STATUS_INVALID_VALUE.
 *   delay_penalty   a float: every finite value is accepted, negative ones (which reward late emission) included.  NaN and
 *               +-inf: RNNT_STATUS_INVALID_VALUE.
 *
 * LATTICE of sample b.  Nodes (t, u), 0 <= t < T_b, 0 <= u <= L_b; s_t = ranges[b, t].  A node has out-edges only if it lies
 * in its frame's window, s_t <= u < s_t + S; lp(t, u, .) = log_softmax(z(b, t, u - s_t, .)).
 *     blank edge (t, u) -> (t + 1, u), weight lp(t, u, blank_label);
 *     label edge, for u < L_b, weight lp(t, u, y_u) + delay_penalty * ((T_b - 1) / 2 - t):
 *         regular type    (t, u) -> (t, u + 1); a path ends with the final blank out of (T_b - 1, L_b);
 *         modified type   (t, u) -> (t + 1, u + 1); the terminal node is (T_b, L_b), and an edge into row T_b exists only if
 *                         it lands there (the blank out of (T_b - 1, L_b), the label out of (T_b - 1, L_b - 1)).  This is
 *                         exactly the lattice of include/rnnt_mono.h: a node lies on a path only inside the BAND u <= t,
 *                         L_b - u <= T_b - t.
 *     cost_b = -log sum over the paths from (0, 0) of exp(sum of the weights), natural log.
 * The cost includes the penalty term (as k2's does when it adds `penalty` to px).  The bias is formed in fp64 per row from the
 * float's value and rounded once to the lattice type.
 *
 * GRADIENT (d cost_b / d z).  For a row (t, u), cb / cl = the posteriors of its blank / label out-edge under the TILTED path
 * distribution (a path's weight includes its bias), as in include/rnnt_delay.h:
 *     column k     (cb + cl) softmax_k - [k == blank_label] cb - [k == y_u] cl
 * A label that equals blank_label is legal: that column then carries both posteriors.  gradients == activations (in place)
 * is allowed; other overlaps are not (RNNT_STATUS_INVALID_VALUE).
 *
 * ROWS NEVER READ, with gradient exactly 0: padding rows (t >= T_b or s_t + k > L_b) and, in the modified type, rows outside
 * the band.  A NaN in such a row changes nothing.
 *
 * NON-FINITE INPUTS AND EDGE CASES.  A start outside [0, L_b] in any frame t < T_b, or lengths that do not fit the tensor
 * (T_b outside [1, maxT], L_b outside [0, maxU - 1]), give the sample the invalid-arguments cost marker of include/rnnt.h
 * (with host costs the one-call entry returns RNNT_STATUS_INVALID_VALUE) and zero gradients.  A sample whose windows hold no
 * path -- the modified type with T_b < L_b is one -- costs +inf, with NaN gradients on its in-lattice rows (t < T_b,
 * s_t + k <= L_b; as in include/rnnt_mono.h the band does not exempt a row of such a sample).  A NaN / +inf / all-(-inf)
 * row that is read gives its sample a NaN cost and the same NaN gradients; other samples are unaffected.  Labels outside
 * [0, A) are clamped into it.
 *
 * IDENTITIES.  rnnt_type 0 at delay_penalty 0 is compute_rnnt_loss_pruned (include/rnnt_pruned.h) on the same tensor.  With
 * S = maxU and every start 0 the tensor is the materialised one: rnnt_type 0 is compute_rnnt_loss_delay
 * (include/rnnt_delay.h), rnnt_type 1 at delay_penalty 0 is compute_rnnt_loss_mono (include/rnnt_mono.h).
 *
 * LIMITS.  maxU <= 4096, A <= 2^23, blank_label in [0, A), N maxT maxU < 2^32 cells, maxT maxU < 2^25: otherwise
 * RNNT_STATUS_INVALID_VALUE.  The tensors themselves may hold more than 2^31 elements.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of every entry below for this shape, window size and dtype code. */
rnntStatus_t get_workspace_size_pstream(int maxT, int maxU, int S, int minibatch, int dtype_code, size_t* size_bytes);

/* One call: costs and (gradients != NULL) the gradient.  costs in DEVICE memory: enqueue only.  costs in HOST memory: copied
 * behind the last kernel and the stream synchronised; a cost marker (bad start, bad lengths) -> RNNT_STATUS_INVALID_VALUE. */
rnntStatus_t compute_rnnt_loss_pstream(const void* activations, void* gradients, const int* ranges, int S, int rnnt_type,
                                       float delay_penalty, const int* flat_labels, const int* label_lengths,
                                       const int* input_lengths, int alphabet_size, int minibatch, void* costs,
                                       void* workspace, rnntOptions options, int dtype_code);

/* Two phases.  The forward call writes device costs and, with prepare_backward != 0, leaves in the workspace what the
 * backward call needs (the per-row gradient records, which carry the type and the penalty: the backward call takes
 * neither): between the two calls only the workspace must stay alive, and the activations unchanged.  The backward call
 * takes the same S and blank_label and writes the gradient; grad_scale_device (N values of the costs' type, or NULL for 1)
 * multiplies sample b's gradient. */
rnntStatus_t compute_rnnt_loss_pstream_fwd(const void* activations, const int* ranges, int S, int rnnt_type,
                                           float delay_penalty, const int* flat_labels, const int* label_lengths,
                                           const int* input_lengths, int alphabet_size, int minibatch, void* costs_device,
                                           void* workspace, rnntOptions options, int dtype_code, int prepare_backward);
rnntStatus_t compute_rnnt_loss_pstream_bwd(const void* activations, void* gradients, const void* grad_scale_device, int S,
                                           int alphabet_size, int minibatch, void* workspace, rnntOptions options,
                                           int dtype_code);

#ifdef __cplusplus
}
#endif
