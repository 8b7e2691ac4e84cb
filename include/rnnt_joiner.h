/* rnnt_joiner.h -- C-ABI of libwarprnnt_joiner.so: the joiner's hidden tensor act(f + g) of a transducer, written directly in
 * the layout each loss of this project reads -- padded (include/rnnt.h), packed (compute_rnnt_loss_packed_*) or pruned
 * (include/rnnt_pruned.h, include/rnnt_pstream.h) -- and its backward: df and dg from ONE read of dout.  A library of its
 * own, so that a caller of libwarprnnt.so never loads it.
 *
 * Conventions as the other include/rnnt_*.h: `rnntOptions` by value, of which only `loc` (must be RNNT_GPU) and `stream` are
 * read; dtype codes 0 fp32, 1 fp64, 2 bf16, 3 fp16 (storage; the arithmetic is fp32, fp64 for fp64); lengths (N) int32 on
 * the device.  Nothing here allocates memory, reads device memory on the host or synchronises: every entry only enqueues
 * and can be captured in a HIP graph.
 *
 * INPUTS.  f (N, T, H) from the encoder, g (N, U, H) from the predictor (U = maxU = max label length + 1), both contiguous,
 * of one dtype, on one GPU.  T_b = input_lengths[b] (T when NULL), L_b = label_lengths[b] (U - 1 when NULL); values outside
 * [0, T] / [0, U - 1] are clamped into it.
 *
 * ACTIVATION.  act 0 identity, 1 relu, 2 tanh.  x = f[b, t, :] + g[b, u, :] is formed in fp32 (fp64 for fp64) and
 * act(x) rounded ONCE to the storage type.
 *
 * LAYOUT of `out`, H values per row.
 *   0 padded   (N, T, U, H).  Row (b, t, u) = act(x) for t < T_b and u <= L_b; every other row is written as exact zeros.
 *              input_lengths and label_lengths may each be NULL.
 *   1 packed   (R, H), row offsets[b] + t (L_b + 1) + u for t < T_b, u <= L_b; offsets = the int64 (N + 1) cumulative row
 *              counts on the device (offsets[b + 1] - offsets[b] = T_b (L_b + 1)), R = offsets[N].  No padding exists;
 *              both lengths are required.
 *   2 pruned   (N, T, S, H), 1 <= S <= U, with ranges int32 (N, T) on the device: row (b, t, k) =
 *              act(f[b, t, :] + g[b, min(ranges[b, t] + k, U - 1), :]).  With input_lengths, rows t >= T_b are exact zeros
 *              and ranges[b, t] is not read for them; label_lengths is not read.  A start outside [0, U - 1] in a frame
 *              that is read makes ALL rows of that sample zeros, its contribution to df and dg zero, and sets the sample's
 *              flag: the first N int32 of the workspace rounded up to a 256-byte boundary, 1 for such a sample, else 0
 *              (written by every layout-2 call, forward or backward).  Nothing faults.
 *
 * BACKWARD.  e = dout * act'(out), act' = 1 (identity), [out > 0] (relu), 1 - out^2 (tanh), from the STORED out: neither f
 * nor g is read.  df[b, t, :] = sum of e over the real rows of frame (b, t); dg[b, u, :] = sum of e over the real rows whose
 * g row is u (in layout 2 the clamped duplicates all land on row U - 1).  Sums in fp32 (fp64 for fp64), one rounding to
 * the storage type.  Every element of df (N, T, H) and dg (N, U, H) is written; padding frames, label rows u > L_b and
 * label rows no window covers are exact 0.  Rows of dout and out that are not real are never read; identity does not
 * read out (it may be NULL).  The summation order is fixed by the shape alone: two calls give identical bits.
 *
 * REFUSED with RNNT_STATUS_INVALID_VALUE before anything is launched: a required pointer that is NULL (f, g, out; dout, df,
 * dg; out of the backward call unless act = 0; ranges in layout 2; offsets and both lengths in layout 1; the workspace);
 * a layout, act or dtype code outside the sets above; S outside [1, U] in layout 2; T, U, H or minibatch <= 0; more than
 * 2^31 - 1 rows (N T max(U, S)); loc != RNNT_GPU; dout overlapping df or dg, or df overlapping dg (in layout 1 the host does
 * not know R: the first row of dout is what is compared).
 */
#pragma once

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace bytes of both entries below: the bad-start flags and, for the backward call, the partial dg sums of a walk
 * split over T (csrc/rnnt_joiner_impl.h has the rule).  S is read in layout 2 only. */
rnntStatus_t get_workspace_size_joiner(int T, int U, int S, int H, int minibatch, int layout, int dtype_code, size_t* bytes);

rnntStatus_t compute_rnnt_joiner_fwd(const void* f, const void* g, void* out, int layout, int act,
                                     const int* ranges /*layout 2*/, int S, const long long* offsets /*layout 1*/,
                                     const int* label_lengths, const int* input_lengths, int T, int U, int H, int minibatch,
                                     void* workspace, rnntOptions options, int dtype_code);

rnntStatus_t compute_rnnt_joiner_bwd(const void* out /*NULL for act 0*/, const void* dout, void* df, void* dg, int layout, int act,
                                     const int* ranges /*layout 2*/, int S, const long long* offsets /*layout 1*/,
                                     const int* label_lengths, const int* input_lengths, int T, int U, int H, int minibatch,
                                     void* workspace, rnntOptions options, int dtype_code);

#ifdef __cplusplus
}
#endif
