/* rnnt_logprobs.h -- C-ABI of libwarprnnt_logprobs.so: the edge log-probabilities px, py of a transducer lattice and the
 * normaliser lse, from joint or pruned logits -- k2 / fast_rnnt's get_rnnt_logprobs_joint and get_rnnt_logprobs_pruned in one
 * read of the logits -- and the backward that resumes at the logit gradient.  Between the two calls the caller may edit the
 * edges (internal-LM subtraction, blank scaling, penalties, a z-loss on lse) and run the lattice of include/rnnt_mi.h.  A
 * library of its own, so that a caller of libwarprnnt.so never loads it.
 *
 * Conventions as the other include/rnnt_*.h: `rnntOptions` by value, of which only `loc` (must be RNNT_GPU), `stream` and
 * `blank_label` are read; dtype codes 0 fp32, 1 fp64, 2 bf16, 3 fp16 (the logits' storage; px, py, lse and their gradients
 * are in the lattice type: fp32, fp64 for fp64).  Nothing here allocates memory, reads device memory on the host or
 * synchronises: every entry only enqueues and can be captured in a HIP graph.  The library takes NO workspace: lse is an
 * output of the forward call and all the backward call needs besides the logits.
 *
 * SIZES.  B = minibatch samples, T frames, U = S + 1 lattice rows (S = the second extent of symbols), C classes.  K = 0: the
 * joint form, logits (B, T, U, C).  1 <= K <= U: the pruned form, logits (B, T, K, C) with ranges int32 (B, T), the frame
 * starts of include/rnnt_pruned.h.  K' = U (joint) or K (pruned) is the third extent of logits, lse and dlogits.  symbols
 * int32 (B, S); boundary int64 (B, 4) or NULL, of which only columns 2 and 3 are read: S_b and T_b, clamped into [0, S] and
 * [0, T] (NULL: S and T).  All on the device, contiguous.
 *
 * ROWS.  Row (b, t, k) of the logits is lattice row u = k (joint) or u = r + k with r = ranges[b, t] clamped into [0, U - K]
 * (pruned).  A row is REAL when t < T_b and u <= S_b.  Rows that are not real are never read.
 *
 * FORWARD, in the lattice type.
 *   lse (B, T, K')   logsumexp over c of z[b, t, k, c]; exact 0 on rows that are not real.
 *   py  (B, U, T)    z[b, t, k, blank] - lse where a real row covers (t, u), else -inf.
 *   px  (B, S, T + 1) for rnnt_type 0 (regular), (B, S, T) for rnnt_type 1 (modified): z[b, t, k, symbols[b, u]] - lse where a
 *                    real row covers (t, u) and u < S_b, else -inf; column T of the regular type and every column t >= T_b is
 *                    -inf.  A symbol outside [0, C) gives -inf and no gradient.
 * Every element of the three outputs is written.  A row with -inf entries and a finite one behaves as torch's log_softmax;
 * a row that is all -inf, or that holds a NaN or +inf, gives NaN in that row's lse, edges and gradient only.
 *
 * BACKWARD.  With gx, gy, gl the incoming gradients of the row's px, py and lse elements (0 where that element is not real,
 * whatever the buffer holds; lse_grad NULL: 0):
 *     dz[c] = gx [c == symbols[b, u]] + gy [c == blank] + (gl - gx - gy) exp(z[c] - lse)
 * formed in the lattice type and rounded once to the logits' type.  Every element of dlogits (B, T, K', C) is written, rows
 * that are not real as exact zeros.  The pass is elementwise given lse: dlogits may be logits itself (the exact alias).  No
 * atomics; the summation order is fixed by the shape alone: two calls give identical bits.
 *
 * REFUSED with RNNT_STATUS_INVALID_VALUE before anything is launched: a required pointer that is NULL (logits, py, lse;
 * py_grad, dlogits; symbols, px and px_grad unless U = 1; ranges when K > 0); K outside {0} and [1, U]; an rnnt_type or dtype
 * code outside the sets above; T, U, C or minibatch <= 0; blank_label outside [0, C); more than 2^31 - 1 rows (B T K');
 * loc != RNNT_GPU; dlogits overlapping anything the call reads other than being logits exactly; px, py and lse overlapping
 * one another.
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

rnntStatus_t compute_rnnt_logprobs_fwd(const void* logits, const int* symbols, const int* ranges /*NULL when K = 0*/, int K,
                                       const long long* boundary /*or NULL*/, int rnnt_type, int T, int U, int C, int minibatch,
                                       void* px, void* py, void* lse, rnntOptions options, int dtype_code);

rnntStatus_t compute_rnnt_logprobs_bwd(const void* logits, const void* lse, const int* symbols, const int* ranges /*NULL when K = 0*/,
                                       int K, const long long* boundary /*or NULL*/, int rnnt_type, const void* px_grad,
                                       const void* py_grad, const void* lse_grad /*or NULL*/, int T, int U, int C, int minibatch,
                                       void* dlogits, rnntOptions options, int dtype_code);

#ifdef __cplusplus
}
#endif
