/* rnnt_delay.h -- C-ABI of libwarprnnt_delay.so: the delay-penalized RNN-T loss (Kang et al., "Delay-penalized transducer for
 * low-latency streaming ASR", 2022; k2's `delay_penalty` with rnnt_type="regular") and the expected frame at which each label
 * is emitted under the lattice's posterior.  A library of its own, so that a caller of libwarprnnt.so never loads it.
 *
 * Conventions as include/rnnt_mono.h: `rnntOptions` by value (loc must be RNNT_GPU; maxT = time dimension, maxU = max label
 * length + 1; blank_label = the blank's column; stream = the HIP stream everything is enqueued on), dtype codes 0 fp32,
 * 1 fp64, 2 bf16, 3 fp16 (storage; 16-bit and fp32 storage run an fp32 lattice and return float costs, fp64 an fp64 lattice
 * and double costs), flat labels (N, maxU - 1) int32, lengths (N) int32, all on the device.  Nothing here allocates memory,
 * and the enqueue-only entries do not synchronise (they can be captured in a HIP graph).
 *
 * INPUTS.  Raw logits z (N, maxT, maxU, A), ONE softmax over all A columns of a row, and the penalty, a float: every finite
 * value is accepted, negative ones (which reward late emission) included.
 *
 * LATTICE of sample b: the standard RNN-T lattice of include/rnnt_ar.h, a label edge stays in its frame.  Nodes (t, u),
 * 0 <= t < T_b, 0 <= u <= L_b.
 *     blank edges (t, u) -> (t + 1, u), weight lp_blank(t, u) = log_softmax(z(t, u, .))[blank_label]; the final blank leaves
 *                                       (T_b - 1, L_b);
 *     label edges (t, u) -> (t, u + 1), weight lp_label(t, u) = log_softmax(z(t, u, .))[y_u]
 *                                                               + delay_penalty * ((T_b - 1) / 2 - t)            (u < L_b).
 *     cost_b = -log sum over the paths of exp(sum of the weights)
 *            = -log sum over the paths of P(path) * exp(delay_penalty * sum_u ((T_b - 1) / 2 - t_u)),
 * natural log, t_u the frame at which the path emits label u.  The cost includes the penalty term (as k2's does when it adds
 * `penalty` to px); delay_penalty = 0 is the loss of include/rnnt.h on raw logits.  The bias is formed in fp64 per row from
 * the float's value and then rounded to the lattice type.
 *
 * GRADIENT (d cost_b / d z).  For a row (t, u), cb / cl = the posteriors of its blank / label out-edge under the TILTED path
 * distribution (a path's weight includes its bias):
 *     column k     (cb + cl) softmax_k - [k == blank_label] cb - [k == y_u] cl
 * The bias is a constant, so softmax_k is the row's own.  A label that equals blank_label is legal: that column then carries
 * both posteriors.  gradients == activations (in place) is allowed; other overlaps are not (RNNT_STATUS_INVALID_VALUE).
 *
 * EXPECTED EMISSION FRAMES.  emit_frames: (N, maxU - 1) values of the costs' type on the device, or NULL (not wanted):
 *     emit_frames[b, u] = sum_t t * cl(t, u)      (u < L_b),
 * the posterior mean, under the same tilted distribution, of the frame at which label u is emitted; nondecreasing in u and
 * inside [0, T_b - 1].  Entries at u >= L_b are written as exact 0: every element of the array is written by every forward
 * call that takes it.  The sum runs in fp64 in a fixed order (no atomics): two calls give identical bits.
 *     d cost_b / d delay_penalty = -sum_{u < L_b} ((T_b - 1) / 2 - emit_frames[b, u]).
 * emit_frames may not overlap the activations, the gradients or the workspace (RNNT_STATUS_INVALID_VALUE), and must lie on an
 * element boundary.  With maxU == 1 the array has no element and the pointer is not looked at.
 *
 * ROWS NEVER READ.  Padding rows (t >= T_b or u > L_b) are never read and their gradient is exactly 0.
 *
 * NON-FINITE INPUTS AND EDGE CASES.  A NaN / +inf / all-(-inf) row inside the lattice gives its sample a NaN cost, NaN
 * gradients on its in-lattice rows and NaN emit_frames for u < L_b; other samples are unaffected.  A sample whose paths all
 * have probability 0 costs +inf, with the same NaNs.  Lengths that do not fit the tensor (T_b outside [1, maxT], L_b outside
 * [0, maxU - 1]) give the sample the invalid-arguments cost marker of include/rnnt.h (with host costs the one-call entry
 * returns RNNT_STATUS_INVALID_VALUE), zero gradients and zero emit_frames.  Labels outside [0, A) are clamped into it, as in
 * include/rnnt.h.  A delay_penalty that is NaN or infinite: RNNT_STATUS_INVALID_VALUE.
 *
 * LIMITS.  maxU <= 4096, A <= 2^23, blank_label in [0, A), N maxT maxU < 2^32 rows, maxT maxU < 2^25: otherwise
 * RNNT_STATUS_INVALID_VALUE.  The tensors themselves may hold more than 2^31 elements.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of every entry below for this shape and dtype code. */
rnntStatus_t get_workspace_size_delay(int maxT, int maxU, int minibatch, int dtype_code, size_t* size_bytes);

/* One call: costs, (gradients != NULL) the gradient and (emit_frames != NULL) the expected emission frames.  costs in DEVICE
 * memory: enqueue only.  costs in HOST memory: copied behind the last kernel and the stream synchronised; a cost marker (bad
 * lengths) -> RNNT_STATUS_INVALID_VALUE. */
rnntStatus_t compute_rnnt_loss_delay(const void* activations, float delay_penalty, void* gradients, const int* flat_labels,
                                     const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch,
                                     void* costs, void* emit_frames, void* workspace, rnntOptions options, int dtype_code);

/* Two phases.  The forward call writes device costs and, with prepare_backward != 0, leaves in the workspace what the
 * backward call needs (the per-row gradient records, which carry the penalty: the backward call takes none): between the two
 * calls only the workspace must stay alive, and the activations unchanged.  A non-NULL emit_frames makes the forward call
 * build those records whatever prepare_backward says.  The backward call takes the same blank_label and writes the gradient;
 * grad_scale_device (N values of the costs' type, or NULL for 1) multiplies sample b's gradient. */
rnntStatus_t compute_rnnt_loss_delay_fwd(const void* activations, float delay_penalty, const int* flat_labels,
                                         const int* label_lengths, const int* input_lengths, int alphabet_size,
                                         int minibatch, void* costs_device, void* emit_frames, void* workspace,
                                         rnntOptions options, int dtype_code, int prepare_backward);
rnntStatus_t compute_rnnt_loss_delay_bwd(const void* activations, void* gradients, const void* grad_scale_device,
                                         int alphabet_size, int minibatch, void* workspace, rnntOptions options,
                                         int dtype_code);

#ifdef __cplusplus
}
#endif
