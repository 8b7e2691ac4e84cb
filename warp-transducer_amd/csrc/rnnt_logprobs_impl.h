// rnnt_logprobs_impl.h -- host driver of libwarprnnt_logprobs.so (include/rnnt_logprobs.h): run_logprobs_fwd<Tag>,
// run_logprobs_bwd<Tag>.  One instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_logprobs.hip   F32 (+ every C entry point)     rnnt_logprobs_f64.hip   F64     rnnt_logprobs_h16.hip   BF16, F16
// The library has no workspace: lse is an output of the forward call and all the backward call needs.
//
// LAUNCH RULE (tests/logprobs_forms.py restates it).  esz = bytes of a stored element, rows = B T K'.
//   forward   logprobs_lse_kernel<Tag, G>: G = 4 lanes per row while C * esz <= kLpNarrowBytes, 16 up to kLpWideBytes, else
//             64; ceil(rows * G / 256) blocks of 256 threads.  Then logprobs_edges_kernel<Tag>, a grid-stride loop of at most
//             2^20 blocks over the B U (T + 1 - rnnt_type) positions of the outputs.
//   backward  logprobs_grad_kernel<Tag, VEC>.  VEC: C * esz is a multiple of 16 and logits and dlogits start on a 16-byte
//             boundary; else element-wise.  P = C / V accesses per row (V = 16 / esz, or 1), blocks of (PX, 256 / PX) threads,
//             PX = P rounded up to a power of two, at most 256; a grid-stride loop over the rows of at most 2^20 blocks.
#pragma once
#include "rnnt_side_host.h"
#include "rnnt_logprobs_kernels.h"
#include "../../include/rnnt_logprobs.h"

namespace rnnt {

// The arguments of both calls, untyped as they cross the C-ABI.
struct LogprobsCall {
    const void* logits;
    const void *lse_in, *px_grad, *py_grad, *lse_grad;     // backward
    void *px, *py, *lse, *dlogits;                          // forward: px, py, lse; backward: dlogits
    LpArgs a;
    hipStream_t stream;
};

static inline int lp_pow2_ceil(int x) { int p = 1; while (p < x) p <<= 1; return p; }
static inline int lp_lanes(size_t row_bytes) {
    return row_bytes <= static_cast<size_t>(kLpNarrowBytes) ? 4 : row_bytes <= static_cast<size_t>(kLpWideBytes) ? 16 : 64;
}
static inline unsigned lp_grid(long long work, int per_block) {
    const long long blocks = (work + per_block - 1) / per_block;
    return static_cast<unsigned>(blocks < kLpMaxGrid ? (blocks ? blocks : 1) : kLpMaxGrid);
}

template <typename Tag> rnntStatus_t run_logprobs_fwd(const LogprobsCall& c) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    (void)hipGetLastError();                           // a stale error of an unrelated earlier HIP call is not ours
    const LpArgs& a = c.a;
    const long long rows = static_cast<long long>(a.B) * a.T * a.Kp;
    const St* z = static_cast<const St*>(c.logits);
    C *px = static_cast<C*>(c.px), *py = static_cast<C*>(c.py), *lse = static_cast<C*>(c.lse);
    const int G = lp_lanes(static_cast<size_t>(a.C) * sizeof(St));
    const dim3 grid(static_cast<unsigned>((rows * G + 255) / 256));
    stats_dispatch(G, [&](auto g) {
        hipLaunchKernelGGL((logprobs_lse_kernel<Tag, decltype(g)::value>), grid, dim3(256), 0, c.stream, z, lse, a, rows);
    });
    if (hipGetLastError() != hipSuccess) return RNNT_STATUS_EXECUTION_FAILED;
    const long long cells = static_cast<long long>(a.B) * a.U * (a.T + 1 - a.mod);
    hipLaunchKernelGGL((logprobs_edges_kernel<Tag>), dim3(lp_grid(cells, 256)), dim3(256), 0, c.stream, z, lse, px, py, a);
    return hipGetLastError() == hipSuccess ? RNNT_STATUS_SUCCESS : RNNT_STATUS_EXECUTION_FAILED;
}

template <typename Tag> rnntStatus_t run_logprobs_bwd(const LogprobsCall& c) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    (void)hipGetLastError();
    const LpArgs& a = c.a;
    const long long rows = static_cast<long long>(a.B) * a.T * a.Kp;
    const bool vec = packets_aligned(c.logits, c.dlogits) && (static_cast<size_t>(a.C) * sizeof(St)) % 16 == 0;
    const int V = vec ? static_cast<int>(16 / sizeof(St)) : 1;
    const int P = a.C / V;
    const int PX = lp_pow2_ceil(P) < 256 ? lp_pow2_ceil(P) : 256;
    const dim3 block(PX, 256 / PX), grid(lp_grid(rows, 256 / PX));
    const St* z = static_cast<const St*>(c.logits);
    St* d = static_cast<St*>(c.dlogits);
    const C *lse = static_cast<const C*>(c.lse_in), *gx = static_cast<const C*>(c.px_grad), *gy = static_cast<const C*>(c.py_grad),
            *gl = static_cast<const C*>(c.lse_grad);
    if (vec) hipLaunchKernelGGL((logprobs_grad_kernel<Tag, true>), grid, block, 0, c.stream, z, d, lse, gx, gy, gl, a, rows, P);
    else hipLaunchKernelGGL((logprobs_grad_kernel<Tag, false>), grid, block, 0, c.stream, z, d, lse, gx, gy, gl, a, rows, P);
    return hipGetLastError() == hipSuccess ? RNNT_STATUS_SUCCESS : RNNT_STATUS_EXECUTION_FAILED;
}

#ifndef RNNT_LOGPROBS_INSTANTIATE_F32
extern template rnntStatus_t run_logprobs_fwd<F32>(const LogprobsCall&);
extern template rnntStatus_t run_logprobs_bwd<F32>(const LogprobsCall&);
#endif
#ifndef RNNT_LOGPROBS_INSTANTIATE_F64
extern template rnntStatus_t run_logprobs_fwd<F64>(const LogprobsCall&);
extern template rnntStatus_t run_logprobs_bwd<F64>(const LogprobsCall&);
#endif
#ifndef RNNT_LOGPROBS_INSTANTIATE_H16
extern template rnntStatus_t run_logprobs_fwd<BF16>(const LogprobsCall&);
extern template rnntStatus_t run_logprobs_bwd<BF16>(const LogprobsCall&);
extern template rnntStatus_t run_logprobs_fwd<F16>(const LogprobsCall&);
extern template rnntStatus_t run_logprobs_bwd<F16>(const LogprobsCall&);
#endif

}  // namespace rnnt
