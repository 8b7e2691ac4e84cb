/* rnnt_ar.h -- C-ABI of libwarprnnt_ar.so: the alignment-restricted RNN-T loss (Mahadeokar et al., "Alignment Restricted
 * Streaming Recurrent Neural Network Transducer", SLT 2021): label u of a sample may be emitted only inside a window of
 * frames [emit_lo_u, emit_hi_u], typically [a_u - b_l, a_u + b_r] around the frame a_u of a forced alignment.  A library of
 * its own, so that a caller of libwarprnnt.so never loads it.
 *
 * Conventions as include/rnnt_mono.h: `rnntOptions` by value (loc must be RNNT_GPU; maxT = time dimension, maxU = max label
 * length + 1; blank_label = the blank's column; stream = the HIP stream everything is enqueued on), dtype codes 0 fp32,
 * 1 fp64, 2 bf16, 3 fp16 (storage; 16-bit and fp32 storage run an fp32 lattice and return float costs, fp64 an fp64 lattice
 * and double costs), flat labels (N, maxU - 1) int32, lengths (N) int32, all on the device.  Nothing here allocates memory,
 * and the enqueue-only entries do not synchronise (they can be captured in a HIP graph).
 *
 * INPUTS.  Raw logits z (N, maxT, maxU, A), ONE softmax over all A columns of a row.  For cell (t, u):
 *     lp(t, u, k) = log_softmax(z(t, u, .))[k]
 * WINDOWS.  emit_lo, emit_hi: int32 (N, maxU - 1) on the device, the inclusive first and last frame at which label u of
 * sample b may be emitted.  Entries at u >= L_b are never looked at.  Values outside [0, T_b - 1] are legal and simply
 * intersect with it: lo <= 0 and hi >= T_b - 1 mean "unrestricted", and with every label unrestricted this is the loss of
 * include/rnnt.h.
 *
 * LATTICE of sample b: the standard RNN-T lattice, a label edge stays in its frame.  Nodes (t, u), 0 <= t < T_b,
 * 0 <= u <= L_b.
 *     blank edges (t, u) -> (t + 1, u), weight lp(t, u, blank_label); the final blank leaves (T_b - 1, L_b);
 *     label edges (t, u) -> (t, u + 1), weight lp(t, u, y_u), ONLY when lo_u <= t <= hi_u.
 * cost_b = -log sum over the paths (0, 0) -> final blank of exp(sum of the weights), natural log.
 *
 * BAND.  With e_0 = 0, e_{u+1} = max(e_u, lo_u) (prefix maximum) and l_{L_b} = T_b - 1, l_u = min(l_{u+1}, hi_u) (suffix
 * minimum):
 *     the sample has a path               iff  e_{u+1} <= l_u for every u < L_b  (e_u <= l_u for all u is NOT sufficient);
 *     node (t, u) lies on a path          iff  e_u <= t <= l_u;
 *     its label edge lies on a path       iff  e_{u+1} <= t <= l_u;
 *     its blank edge lies on a path       iff  t + 1 <= l_u, or (t, u) is the final node (T_b - 1, L_b).
 * ROWS NEVER READ.  Only band rows (e_u <= t <= l_u) are read.  Padding rows (t >= T_b or u > L_b) and in-lattice rows
 * outside the band are never read, and their gradient is exactly 0 (but see the samples with NaN gradients below).  A NaN in
 * such a row changes nothing.  A sample without a path has no band: none of its rows is read.
 *
 * GRADIENT (d cost_b / d z).  For a row (t, u), cb / cl = the posteriors of its blank / label out-edge:
 *     column k     (cb + cl) softmax_k - [k == blank_label] cb - [k == y_u] cl
 * A label that equals blank_label is legal: that column then carries both posteriors, the true derivative.  gradients ==
 * activations (in place) is allowed; other overlaps are not (RNNT_STATUS_INVALID_VALUE).
 *
 * NON-FINITE INPUTS AND EDGE CASES.  A sample with no path costs +inf, with NaN gradients on its in-lattice rows: an empty
 * window (lo_u > hi_u, or a window wholly outside [0, T_b - 1]), windows that cannot be ordered (e_{u+1} > l_u), and any
 * sample whose paths all have probability 0.  A NaN / +inf / all-(-inf) row inside the band gives its sample a NaN cost and
 * NaN gradients on its in-lattice rows (those outside the band included); other samples are unaffected.  Padding rows stay
 * exactly 0 in every case.  Lengths that do not fit the tensor (T_b outside [1, maxT], L_b outside [0, maxU - 1]) give the
 * sample the invalid-arguments cost marker of include/rnnt.h (with host costs the one-call entry returns
 * RNNT_STATUS_INVALID_VALUE) and zero gradients.  Labels outside [0, A) are clamped into it, as in include/rnnt.h.  A NULL
 * emit_lo or emit_hi: RNNT_STATUS_INVALID_VALUE.
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
rnntStatus_t get_workspace_size_ar(int maxT, int maxU, int minibatch, int dtype_code, size_t* size_bytes);

/* One call: costs and (gradients != NULL) the gradient.  costs in DEVICE memory: enqueue only.  costs in HOST memory: copied
 * behind the last kernel and the stream synchronised; a cost marker (bad lengths) -> RNNT_STATUS_INVALID_VALUE. */
rnntStatus_t compute_rnnt_loss_ar(const void* activations, void* gradients, const int* flat_labels,
                                  const int* label_lengths, const int* input_lengths, const int* emit_lo,
                                  const int* emit_hi, int alphabet_size, int minibatch, void* costs, void* workspace,
                                  rnntOptions options, int dtype_code);

/* Two phases.  The forward call writes device costs and, with prepare_backward != 0, leaves in the workspace what the
 * backward call needs (the per-row gradient records, which also mark the rows outside the band: the backward call takes no
 * windows): between the two calls only the workspace must stay alive, and the activations unchanged.  The backward call
 * takes the same blank_label and writes the gradient; grad_scale_device (N values of the costs' type, or NULL for 1)
 * multiplies sample b's gradient. */
rnntStatus_t compute_rnnt_loss_ar_fwd(const void* activations, const int* flat_labels, const int* label_lengths,
                                      const int* input_lengths, const int* emit_lo, const int* emit_hi,
                                      int alphabet_size, int minibatch, void* costs_device, void* workspace,
                                      rnntOptions options, int dtype_code, int prepare_backward);
rnntStatus_t compute_rnnt_loss_ar_bwd(const void* activations, void* gradients, const void* grad_scale_device,
                                      int alphabet_size, int minibatch, void* workspace, rnntOptions options,
                                      int dtype_code);

#ifdef __cplusplus
}
#endif
