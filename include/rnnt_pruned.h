/* rnnt_pruned.h -- C-ABI of libwarprnnt_pruned.so: the pruned RNN-T loss and the prune ranges of the additive joint
 * (pruned RNN-T: Kuang et al., Interspeech 2022).  A library of its own, so that a caller of libwarprnnt.so never loads it.
 *
 * Conventions as include/rnnt.h: `rnntOptions` by value (loc must be RNNT_GPU; maxT = time dimension, maxU = max label
 * length + 1; stream = the HIP stream everything is enqueued on), dtype codes 0 fp32, 1 fp64, 2 bf16, 3 fp16 (storage; 16-bit
 * and fp32 storage run an fp32 lattice and return float costs, fp64 an fp64 lattice and double costs), flat labels
 * (N, maxU - 1) int32, lengths (N) int32, all on the device.  Nothing here allocates memory, and the enqueue-only entries
 * do not synchronise (they can be captured in a HIP graph).
 *
 * RANGES: int32 (N, maxT) on the device.  Frame t of sample b sees the lattice states u in [s, s + S), s = ranges[b, t].
 *
 * THE PRUNED LOSS.  Activations: raw logits (N, maxT, S, A); row (b, t, k) is the joint output of state u = ranges[b, t] + k.
 * For t < T_b and u <= L_b the row's log-softmax gives the cell (t, u) its blank edge (t, u) -> (t + 1, u) and, for u < L_b,
 * its label edge (t, u) -> (t, u + 1); lattice cells outside their frame's window have no edges.  cost_b = -log of the sum
 * over the paths from (0, 0) through the final blank.  Rows with t >= T_b or u > L_b are padding: never read, gradient 0.
 * 1 <= S <= maxU.  A start outside [0, L_b] gives the sample the invalid-arguments cost marker (a NaN; with host costs the
 * one-call entry returns RNNT_STATUS_INVALID_VALUE, as for lengths that do not fit the tensor) and zero gradients.  A sample
 * whose windows hold no path costs +inf, with NaN gradients on its in-lattice rows.  With S = maxU and every start 0 this is
 * compute_rnnt_loss_async on the same tensor.  gradients == activations (in place) is allowed; other overlaps are not.
 *
 * BATCH SIZE.  The loss takes any minibatch with N maxT S < 2^32 rows (its kernels run the batch in slices of 65535
 * samples).  compute_rnnt_prune_ranges_add runs the additive joint's partition kernels, which keep the samples on one grid
 * dimension: minibatch > 65535 -> RNNT_STATUS_INVALID_VALUE, nothing written (as compute_rnnt_loss_add, include/rnnt.h).
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of every entry below for this shape and dtype code. */
rnntStatus_t get_workspace_size_pruned(int maxT, int maxU, int minibatch, int dtype_code, size_t* size_bytes);

/* One call: costs and (gradients != NULL) the gradient.  costs in DEVICE memory: enqueue only.  costs in HOST memory: copied
 * behind the last kernel and the stream synchronised; a cost marker (bad start, bad lengths) -> RNNT_STATUS_INVALID_VALUE. */
rnntStatus_t compute_rnnt_loss_pruned(const void* activations, void* gradients, const int* ranges, int S,
                                      const int* flat_labels, const int* label_lengths, const int* input_lengths,
                                      int alphabet_size, int minibatch, void* costs, void* workspace,
                                      rnntOptions options, int dtype_code);

/* Two phases.  The forward call writes device costs and, with prepare_backward != 0, leaves in the workspace what the
 * backward call needs (the windows and the coefficient table): between the two calls only the workspace must stay alive,
 * and the activations unchanged.  The backward call writes the gradient; grad_scale_device (N values of the costs' type, or
 * NULL for 1) multiplies sample b's gradient. */
rnntStatus_t compute_rnnt_loss_pruned_fwd(const void* activations, const int* ranges, int S, const int* flat_labels,
                                          const int* label_lengths, const int* input_lengths, int alphabet_size,
                                          int minibatch, void* costs_device, void* workspace, rnntOptions options,
                                          int dtype_code, int prepare_backward);
rnntStatus_t compute_rnnt_loss_pruned_bwd(const void* activations, void* gradients, const void* grad_scale_device, int S,
                                          int alphabet_size, int minibatch, void* workspace, rnntOptions options,
                                          int dtype_code);

/* Prune ranges from the additive joint f (N, maxT, A) + g (N, maxU, A) (dtype code 0 fp32, 2 bf16, 3 fp16), 2 <= S <= maxU:
 * gamma(t, u) = exp(alpha + beta - log P) of that lattice; per frame the smallest s in [0, smax], smax = max(0, L_b + 1 - S),
 * with the largest window sum of gamma over [s, min(s + S - 1, L_b)]; clamped into [max(0, smax - (T_b - 1 - t)(S - 1)),
 * min(smax, t (S - 1))]; made non-decreasing (forward pass); consecutive windows made to overlap (backward pass,
 * s_t = max(s_t, s_{t+1} - (S - 1))); frames t >= T_b get 0.  When L_b <= T_b (S - 1) a path through the windows exists
 * (s_0 = 0, steps in [0, S - 1], s_{T_b - 1} = smax); otherwise s_t = min(t (S - 1), smax).  Writes ranges (N, maxT).
 * minibatch <= 65535 (BATCH SIZE above). */
rnntStatus_t compute_rnnt_prune_ranges_add(const void* trans_acts, const void* pred_acts, const int* flat_labels,
                                           const int* label_lengths, const int* input_lengths, int alphabet_size,
                                           int minibatch, int S, int* ranges, void* workspace, rnntOptions options,
                                           int dtype_code);

#ifdef __cplusplus
}
#endif
