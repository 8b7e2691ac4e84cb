/* rnnt_mono.h -- C-ABI of libwarprnnt_mono.so: the monotonic (one label per frame) transducer loss (Tripathi et al.,
 * "Monotonic Recurrent Neural Network Transducer and Decoding Strategies", ASRU 2019; k2's rnnt_type="modified").  A library
 * of its own, so that a caller of libwarprnnt.so never loads it.
 *
 * Conventions as include/rnnt_mblank.h: `rnntOptions` by value (loc must be RNNT_GPU; maxT = time dimension, maxU = max label
 * length + 1; blank_label = the blank's column; stream = the HIP stream everything is enqueued on), dtype codes 0 fp32,
 * 1 fp64, 2 bf16, 3 fp16 (storage; 16-bit and fp32 storage run an fp32 lattice and return float costs, fp64 an fp64 lattice
 * and double costs), flat labels (N, maxU - 1) int32, lengths (N) int32, all on the device.  Nothing here allocates memory,
 * and the enqueue-only entries do not synchronise (they can be captured in a HIP graph).
 *
 * INPUTS.  Raw logits z (N, maxT, maxU, A), ONE softmax over all A columns of a row.  For cell (t, u):
 *     lp(t, u, k) = log_softmax(z(t, u, .))[k]
 *
 * LATTICE of sample b: nodes (t, u), 0 <= t < T_b, 0 <= u <= L_b, and the terminal node (T_b, L_b).
 *     blank edges (t, u) -> (t + 1, u),     weight lp(t, u, blank_label);
 *     label edges (t, u) -> (t + 1, u + 1), weight lp(t, u, y_u), when u < L_b: a label consumes a frame as a blank does.
 * An edge into row T_b exists only if it lands on the terminal node (T_b, L_b).
 * cost_b = -log sum over the paths (0, 0) -> terminal of exp(sum of the weights), natural log.  Every path has exactly T_b
 * edges, L_b of them label edges: at most one label per frame.
 *
 * GRADIENT (d cost_b / d z).  For a row (t, u), cb / cl = the posteriors of its blank / label out-edge:
 *     column k     (cb + cl) softmax_k - [k == blank_label] cb - [k == y_u] cl
 * A label that equals blank_label is legal: that column then carries both posteriors, the true derivative.  gradients ==
 * activations (in place) is allowed; other overlaps are not (RNNT_STATUS_INVALID_VALUE).
 *
 * ROWS NEVER READ.  No path passes through a node outside the BAND  u <= t  and  L_b - u <= T_b - t  (too few frames
 * behind it for its labels, or too few ahead for the remaining ones): (L_b + 1)(T_b - L_b) + L_b of the sample's
 * T_b (L_b + 1) in-lattice rows lie inside it.  Padding rows (t >= T_b or u > L_b) and in-lattice rows outside the band are
 * never read, and their gradient is exactly 0 (but see the samples with NaN gradients below).  A NaN in such a row changes
 * nothing.
 *
 * NON-FINITE INPUTS AND EDGE CASES.  T_b < L_b leaves no path (the band is empty): the sample costs +inf, with NaN gradients
 * on its in-lattice rows.  So does any sample whose paths all have probability 0.  A NaN / +inf / all-(-inf) row inside the
 * band gives its sample a NaN cost and NaN gradients on its in-lattice rows (those outside the band included); other samples
 * are unaffected.  Padding rows stay exactly 0 in every case.  Lengths that do not fit the tensor (T_b outside [1, maxT],
 * L_b outside [0, maxU - 1]) give the sample the invalid-arguments cost marker of include/rnnt.h (with host costs the
 * one-call entry returns RNNT_STATUS_INVALID_VALUE) and zero gradients.  Labels outside [0, A) are clamped into it, as in
 * include/rnnt.h.
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
rnntStatus_t get_workspace_size_mono(int maxT, int maxU, int minibatch, int dtype_code, size_t* size_bytes);

/* One call: costs and (gradients != NULL) the gradient.  costs in DEVICE memory: enqueue only.  costs in HOST memory: copied
 * behind the last kernel and the stream synchronised; a cost marker (bad lengths) -> RNNT_STATUS_INVALID_VALUE. */
rnntStatus_t compute_rnnt_loss_mono(const void* activations, void* gradients, const int* flat_labels,
                                    const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch,
                                    void* costs, void* workspace, rnntOptions options, int dtype_code);

/* Two phases.  The forward call writes device costs and, with prepare_backward != 0, leaves in the workspace what the
 * backward call needs (the per-row gradient records): between the two calls only the workspace must stay alive, and the
 * activations unchanged.  The backward call takes the same blank_label and writes the gradient; grad_scale_device (N values
 * of the costs' type, or NULL for 1) multiplies sample b's gradient. */
rnntStatus_t compute_rnnt_loss_mono_fwd(const void* activations, const int* flat_labels, const int* label_lengths,
                                        const int* input_lengths, int alphabet_size, int minibatch, void* costs_device,
                                        void* workspace, rnntOptions options, int dtype_code, int prepare_backward);
rnntStatus_t compute_rnnt_loss_mono_bwd(const void* activations, void* gradients, const void* grad_scale_device,
                                        int alphabet_size, int minibatch, void* workspace, rnntOptions options,
                                        int dtype_code);

#ifdef __cplusplus
}
#endif
