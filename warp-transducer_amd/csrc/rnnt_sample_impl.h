// rnnt_sample_impl.h -- host driver of libwarprnnt_sample.so (include/rnnt_sample.h): run_sample<Tag>.  One instantiation
// per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_sample.hip   F32 (+ every C entry point)     rnnt_sample_f64.hip   F64     rnnt_sample_h16.hip   BF16, F16
// The library has no workspace: scores, alpha, frames, weights and the two accumulators are outputs.
//
// LAUNCH RULE (tests/sample_forms.py restates it).  U = S + 1 lattice rows of the TENSOR (not of a sample's rectangle).
//   sweep      sample_fwd_kernel<Tag, MOD, MULTI>, a block per sample on grid.x:
//                U <= kSaWaveMaxU          one wavefront (MULTI = false)
//                U <= kSaMaxU              64 * ceil(U / 64) threads
//   walk       sample_walk_kernel<Tag, MOD>, grid (B, ceil(K / block)), block = min(kSaWalkBlock, 64 * ceil(K / 64))
//   weights    path_weights_kernel<Tag, MOD>, min(B K, 2^20) blocks of one wavefront
//   edges      path_edges_kernel<Tag, MOD>, grid (B, min(U, kSaEdgeSlices)), block = kSaEdgeBlock
#pragma once
#include "rnnt_side_host.h"
#include "rnnt_sample_kernels.h"
#include "../../include/rnnt_sample.h"

namespace rnnt {

constexpr int kSaMaxU = 1024;           // S + 1 at most: a thread per row

// The arguments of the four entries, untyped as they cross the C-ABI.  phases: bit 0 = sweep, bit 1 = walk, bit 2 = path
// weights, bit 3 = path edges.
struct SampleCall {
    const void *px, *py, *boundary, *uniforms, *coeff;
    void *scores, *alpha;
    int* frames;
    void* weights;
    void *px_acc, *py_acc;
    int S, T, N, K;
    bool modified;
    hipStream_t stream;
    int phases;
};

static inline bool sa_shape_ok(int S, int T, int N, int K) {
    if (!side_lattice_ok(S, T, N, kSaMaxU) || K < 1 || K > kSaMaxK) return false;
    return static_cast<unsigned long long>(N) * K * (S > 1 ? S : 1) < (1ull << 31);
}

template <typename Tag, bool MOD>
static rnntStatus_t run_sample_type(const SampleCall& c) {
    using St = typename Tag::store;
    const int U = c.S + 1;
    const St *px = static_cast<const St*>(c.px), *py = static_cast<const St*>(c.py);
    const long long* bd = static_cast<const long long*>(c.boundary);
    if (c.phases & 1) {
#define RNNT_SA_FWD(MULTI, THREADS)                                                                                      \
    hipLaunchKernelGGL((sample_fwd_kernel<Tag, MOD, MULTI>), dim3(c.N), dim3(THREADS), 0, c.stream, px, py, bd,          \
                       static_cast<double*>(c.scores), static_cast<double*>(c.alpha), c.S, c.T)
        if (U <= kSaWaveMaxU) RNNT_SA_FWD(false, 64);
        else RNNT_SA_FWD(true, (U + 63) / 64 * 64);
#undef RNNT_SA_FWD
        if (hipGetLastError() != hipSuccess) return RNNT_STATUS_EXECUTION_FAILED;
    }
    if (c.phases & 2) {
        const int block = c.K >= kSaWalkBlock ? kSaWalkBlock : (c.K + 63) / 64 * 64;
        hipLaunchKernelGGL((sample_walk_kernel<Tag, MOD>), dim3(c.N, (c.K + block - 1) / block), dim3(block), 0, c.stream, px,
                           py, bd, static_cast<const double*>(c.alpha), static_cast<const double*>(c.scores),
                           static_cast<const float*>(c.uniforms), c.frames, static_cast<double*>(c.weights), c.S, c.T, c.K);
        if (hipGetLastError() != hipSuccess) return RNNT_STATUS_EXECUTION_FAILED;
    }
    if (c.phases & 4) {
        const long long BK = static_cast<long long>(c.N) * c.K;
        hipLaunchKernelGGL((path_weights_kernel<Tag, MOD>), dim3(static_cast<unsigned>(BK < (1 << 20) ? BK : (1 << 20))),
                           dim3(64), 0, c.stream, px, py, bd, c.frames, static_cast<double*>(c.weights), c.S, c.T, c.K, BK);
        if (hipGetLastError() != hipSuccess) return RNNT_STATUS_EXECUTION_FAILED;
    }
    if (c.phases & 8) {
        hipLaunchKernelGGL((path_edges_kernel<Tag, MOD>), dim3(c.N, U < kSaEdgeSlices ? U : kSaEdgeSlices), dim3(kSaEdgeBlock),
                           0, c.stream, c.frames, static_cast<const double*>(c.coeff), bd, static_cast<St*>(c.px_acc),
                           static_cast<St*>(c.py_acc), c.S, c.T, c.K);
        if (hipGetLastError() != hipSuccess) return RNNT_STATUS_EXECUTION_FAILED;
    }
    return RNNT_STATUS_SUCCESS;
}

// The call `c`, checked by the C entries (pointers, shape, overlaps): only the launches are left.
template <typename Tag>
rnntStatus_t run_sample(const SampleCall& c) {
    (void)hipGetLastError();                               // a stale error of an unrelated earlier HIP call is not ours
    return c.modified ? run_sample_type<Tag, true>(c) : run_sample_type<Tag, false>(c);
}

#ifndef RNNT_SAMPLE_INSTANTIATE_F32
extern template rnntStatus_t run_sample<F32>(const SampleCall&);
#endif
#ifndef RNNT_SAMPLE_INSTANTIATE_F64
extern template rnntStatus_t run_sample<F64>(const SampleCall&);
#endif
#ifndef RNNT_SAMPLE_INSTANTIATE_H16
extern template rnntStatus_t run_sample<BF16>(const SampleCall&);
extern template rnntStatus_t run_sample<F16>(const SampleCall&);
#endif

}  // namespace rnnt
