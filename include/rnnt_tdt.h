/* rnnt_tdt.h -- C-ABI of libwarprnnt_tdt.so: the Token-and-Duration Transducer (TDT) loss (Xu et al., ICML 2023).  A library
 * of its own, so that a caller of libwarprnnt.so never loads it.
 *
 * Conventions as include/rnnt.h: `rnntOptions` by value (loc must be RNNT_GPU; maxT = time dimension, maxU = max label
 * length + 1; blank_label = the blank's token column; stream = the HIP stream everything is enqueued on), dtype codes 0 fp32,
 * 1 fp64, 2 bf16, 3 fp16 (storage; 16-bit and fp32 storage run an fp32 lattice and return float costs, fp64 an fp64 lattice
 * and double costs), flat labels (N, maxU - 1) int32, lengths (N) int32, all on the device.  Nothing here allocates memory,
 * and the enqueue-only entries do not synchronise (they can be captured in a HIP graph).
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
 * Blank never takes duration 0 (that mass is lost).  cost_b = -log sum over the paths (0, 0) -> terminal of exp(sum of
 * the weights).
 *
 * GRADIENT (d cost_b / d logits).  gamma_e = posterior of edge e; for a row (t, u) inside the lattice, cb = sum of gamma
 * over its blank out-edges, cl = over its label out-edges, c = cb + cl, gamma_dur_j = over its out-edges of duration j:
 *     token column k     c softmax_k - cb [k == blank] - cl [k == y_u]
 *     duration column j  c p_dur_j - gamma_dur_j
 * Rows with t >= T_b or u > L_b are padding: never read, gradient exactly 0.  gradients == activations (in place) is
 * allowed; other overlaps are not.
 *
 * NON-FINITE INPUTS AND EDGE CASES.  A NaN / +inf / all-(-inf) row inside the lattice (token or duration part) gives its
 * sample a NaN cost and NaN gradients on its in-lattice rows; other samples are unaffected.  A sample with no path to the
 * terminal node costs +inf, with NaN in-lattice gradients.  Lengths that do not fit the tensor (T_b outside [1, maxT], L_b
 * outside [0, maxU - 1]) give the sample the invalid-arguments cost marker of include/rnnt.h (with host costs the one-call
 * entry returns RNNT_STATUS_INVALID_VALUE) and zero gradients.
 *
 * LIMITS.  maxU <= 4096, blank_label in [0, A), N maxT maxU < 2^32 rows, maxT maxU < 2^25: otherwise
 * RNNT_STATUS_INVALID_VALUE.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of every entry below for this shape, number of durations and dtype code. */
rnntStatus_t get_workspace_size_tdt(int maxT, int maxU, int minibatch, int num_durations, int dtype_code,
                                    size_t* size_bytes);

/* One call: costs and (gradients != NULL) the gradient.  costs in DEVICE memory: enqueue only.  costs in HOST memory: copied
 * behind the last kernel and the stream synchronised; a cost marker (bad lengths) -> RNNT_STATUS_INVALID_VALUE. */
rnntStatus_t compute_tdt_loss(const void* activations, void* gradients, const int* durations, int num_durations,
                              float sigma, const int* flat_labels, const int* label_lengths, const int* input_lengths,
                              int alphabet_size, int minibatch, void* costs, void* workspace, rnntOptions options,
                              int dtype_code);

/* Two phases.  The forward call writes device costs and, with prepare_backward != 0, leaves in the workspace what the
 * backward call needs (the per-row gradient records): between the two calls only the workspace must stay alive, and the
 * activations unchanged.  The backward call takes the same durations and writes the gradient; grad_scale_device (N values
 * of the costs' type, or NULL for 1) multiplies sample b's gradient. */
rnntStatus_t compute_tdt_loss_fwd(const void* activations, const int* durations, int num_durations, float sigma,
                                  const int* flat_labels, const int* label_lengths, const int* input_lengths,
                                  int alphabet_size, int minibatch, void* costs_device, void* workspace,
                                  rnntOptions options, int dtype_code, int prepare_backward);
rnntStatus_t compute_tdt_loss_bwd(const void* activations, void* gradients, const void* grad_scale_device,
                                  const int* durations, int num_durations, int alphabet_size, int minibatch,
                                  void* workspace, rnntOptions options, int dtype_code);

#ifdef __cplusplus
}
#endif
