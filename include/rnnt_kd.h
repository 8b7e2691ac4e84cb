/* rnnt_kd.h -- C-ABI of libwarprnnt_kd.so: the transducer lattice distillation loss (Panchapagesan et al., ICASSP 2021,
 * "Efficient knowledge distillation for RNN-transducer models"): at every lattice node (t, u) the KL divergence from a
 * teacher transducer's output distribution to a student's, usually collapsed to three classes.  A library of its own, so
 * that a caller of libwarprnnt.so never loads it.
 *
 * Conventions as include/rnnt.h: `rnntOptions` by value (loc must be RNNT_GPU; maxT = time dimension, maxU = max label
 * length + 1; blank_label = the blank's column, in [0, A); stream = the HIP stream everything is enqueued on), dtype codes
 * 0 fp32, 1 fp64, 2 bf16, 3 fp16 (storage; codes 0, 2, 3 compute in fp32 and return float costs, code 1 in fp64 and returns
 * double costs), flat labels (N, maxU - 1) int32, lengths (N) int32, all on the device.  Nothing here allocates memory, and
 * the enqueue-only entries do not synchronise (they can be captured in a HIP graph).
 *
 * INPUTS.  Student logits z (`activations`) and teacher logits w (`teacher`), both (N, maxT, maxU, A), contiguous, of the
 * same dtype code; mode (0 collapsed, 1 full) and temperature tau (finite, > 0).  Per row (t, u):
 *     p = softmax(z / tau)        q = softmax(w / tau)
 *
 * CLASSES.  Collapsed (mode 0): the classes of row (t, u) are blank = {blank_label}, label = {y_u} and rest = every other
 * column.  A row has only the two classes blank and rest where it has no label (u = L_b) and where y_u == blank_label.
 * Labels outside [0, A) are clamped into it, as in include/rnnt.h.  With A = 2 and a label, rest is empty: it contributes
 * nothing and no column belongs to it.  P(k), Q(k) = the sums of p, q over class k.  Full (mode 1): every column is a class
 * of its own.
 *
 * COST.  cost_b = sum over the rows inside the lattice (t < T_b, u <= L_b) of sum_k Q(k) (log Q(k) - log P(k)), natural
 * log; a class with Q(k) = 0 contributes 0.  No tau^2 factor and no normalisation by the number of rows: the caller scales.
 * The per-sample sum is formed in fp64 in a fixed order: two runs give identical bits.
 *
 * GRADIENT (d cost_b / d z; the teacher gets none).  With c(v) the class of column v:
 *     d cost_b / d z_v = (1 / tau) [ p_v - exp(log p_v + log Q(c(v)) - log P(c(v))) ]
 * which in full mode is (p_v - q_v) / tau.  The second term is ONE exponential of a sum, so that a P(c) that underflows does
 * not produce inf * 0.
 *
 * NUMERICS.  Each class sum is accumulated over its own columns, never as "1 minus the others"; the log of a class whose
 * probability exceeds 1/2 is log1p(-(the other classes' probabilities)).
 *
 * PADDING AND IN PLACE.  Rows with t >= T_b or u > L_b are padding: never read in either tensor, gradient exactly 0.
 * gradients == activations (in place) is allowed, and so is teacher == activations.  Gradients that overlap the teacher,
 * any other partial overlap of two of the three tensors, and a pointer off its element boundary are refused
 * (RNNT_STATUS_INVALID_VALUE).
 *
 * NON-FINITE INPUTS AND EDGE CASES.  A NaN or a +inf logit in a row inside the lattice, of either tensor, or such a row that
 * is all -inf in either tensor, poisons that sample only: NaN cost, NaN gradients on its in-lattice rows, zeros on its
 * padding.  P(k) = 0 with Q(k) > 0 costs +inf, with NaN in-lattice gradients for that sample.  Lengths that do not fit the
 * tensor (T_b outside [1, maxT], L_b outside [0, maxU - 1]) give the sample the invalid-arguments cost marker of
 * include/rnnt.h (with host costs the one-call entry returns RNNT_STATUS_INVALID_VALUE) and zero gradients.  Other samples
 * are never affected.
 *
 * LIMITS.  2 <= A <= 2^23, maxT maxU < 2^31, N maxT maxU < 2^32 rows: otherwise RNNT_STATUS_INVALID_VALUE.  The tensors
 * themselves may hold more than 2^31 elements.  A mode outside {0, 1} and a temperature that is not finite and positive
 * are refused before anything is launched.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of every entry below for this shape and dtype code (either mode). */
rnntStatus_t get_workspace_size_kd(int maxT, int maxU, int minibatch, int dtype_code, size_t* size_bytes);

/* One call: costs and (gradients != NULL) the gradient.  costs in DEVICE memory: enqueue only.  costs in HOST memory: copied
 * behind the last kernel and the stream synchronised; a cost marker (bad lengths) -> RNNT_STATUS_INVALID_VALUE. */
rnntStatus_t compute_kd_loss(const void* activations, const void* teacher, void* gradients, const int* flat_labels,
                             const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch,
                             void* costs, void* workspace, rnntOptions options, int dtype_code, int mode,
                             float temperature);

/* Two phases.  The forward call writes device costs and, with prepare_backward != 0, leaves in the workspace what the
 * backward call needs (the per-row records): between the two calls only the workspace must stay alive, and both tensors
 * unchanged.  The backward call writes the gradient; grad_scale_device (N values of the costs' type, or NULL for 1)
 * multiplies sample b's gradient.  Collapsed mode's backward call reads the student only and takes teacher == NULL, so that
 * the teacher need not be kept between the two calls; full mode's reads both tensors. */
rnntStatus_t compute_kd_loss_fwd(const void* activations, const void* teacher, const int* flat_labels,
                                 const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch,
                                 void* costs_device, void* workspace, rnntOptions options, int dtype_code, int mode,
                                 float temperature, int prepare_backward);
rnntStatus_t compute_kd_loss_bwd(const void* activations, const void* teacher, void* gradients,
                                 const void* grad_scale_device, int alphabet_size, int minibatch, void* workspace,
                                 rnntOptions options, int dtype_code, int mode, float temperature);

#ifdef __cplusplus
}
#endif
