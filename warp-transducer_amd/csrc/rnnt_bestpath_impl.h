// rnnt_bestpath_impl.h -- host driver of libwarprnnt_bestpath.so (include/rnnt_bestpath.h): run_bestpath<Tag>.  One
// instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_bestpath.hip   F32 (+ every C entry point)     rnnt_bestpath_f64.hip   F64     rnnt_bestpath_h16.hip   BF16, F16
// The library has no workspace: scores, frames, back and the indicators are outputs.
//
// LAUNCH RULE (tests/bestpath_forms.py restates it).  U = S + 1 lattice rows of the TENSOR (not of a sample's rectangle).
//   sweep + traceback   bestpath_sweep_kernel<Tag, MOD, K, MULTI>, a block per sample:
//                         U <= kBpWaveMaxU          K = 1, one wavefront (MULTI = false)
//                         U <= 1024                 K = 1, 64 * ceil(U / 64) threads
//                         else                      K = kBpWideRows, 64 * ceil(ceil(U / K) / 64) threads
//   edges               bestpath_edges_kernel<Tag, MOD>, grid (ceil((T + 1) / 256), U, samples), when the indicators are taken
// HOST SCORES.  Without a workspace the scores have no device home but an output: the sweep launch parks score b in word
// [b, 0, 0] of `back` (the last thing a block does), the edges kernel reads it there, a strided copy takes it to the host, and
// the sweep launch runs a second time without a score pointer, which restores the word.
#pragma once
#include "rnnt_side_host.h"
#include "rnnt_bestpath_kernels.h"
#include "../../include/rnnt_bestpath.h"

namespace rnnt {

constexpr int kBpMaxU = 4096;           // S + 1 at most: kBpWideRows rows for each of 1024 threads

// The arguments of both entries, untyped as they cross the C-ABI.  phases: bit 0 = sweep and traceback, bit 1 = edges.
struct BestpathCall {
    const void *px, *py, *boundary;
    void *scores_dev, *scores_host;
    int* frames;
    void* back;
    const void* grad_scale;
    void *px_path, *py_path;
    int S, T, N;
    bool modified;
    hipStream_t stream;
    int phases;
};

static inline bool bp_shape_ok(int S, int T, int N) { return side_lattice_ok(S, T, N, kBpMaxU); }
static inline unsigned long long bp_back_words(int S, int T) {
    return static_cast<unsigned long long>(S + 1) * ((T + 64) >> 6);
}

template <typename Tag, bool MOD>
static bool launch_bp_sweep(const BestpathCall& c, double* scores, long long stride) {
    using St = typename Tag::store;
    const int U = c.S + 1;
    const St *px = static_cast<const St*>(c.px), *py = static_cast<const St*>(c.py);
    const long long* bd = static_cast<const long long*>(c.boundary);
    unsigned long long* back = static_cast<unsigned long long*>(c.back);
    const dim3 grid(c.N);
#define RNNT_BP_SWEEP(K, MULTI, THREADS)                                                                                \
    hipLaunchKernelGGL((bestpath_sweep_kernel<Tag, MOD, K, MULTI>), grid, dim3(THREADS), 0, c.stream, px, py, bd, scores, \
                       stride, c.frames, back, c.S, c.T)
    if (U <= kBpWaveMaxU) RNNT_BP_SWEEP(1, false, 64);
    else if (U <= 1024) RNNT_BP_SWEEP(1, true, (U + 63) / 64 * 64);
    else RNNT_BP_SWEEP(kBpWideRows, true, ((U + kBpWideRows - 1) / kBpWideRows + 63) / 64 * 64);
#undef RNNT_BP_SWEEP
    return hipGetLastError() == hipSuccess;
}

template <typename Tag, bool MOD>
static bool launch_bp_edges(const BestpathCall& c, const double* scores, long long stride) {
    using St = typename Tag::store;
    for (int b0 = 0; b0 < c.N; b0 += kGridSamples) {
        const dim3 grid((c.T + 256) / 256, c.S + 1, grid_samples(c.N, b0));
        hipLaunchKernelGGL((bestpath_edges_kernel<Tag, MOD>), grid, dim3(256), 0, c.stream, c.frames, scores, stride,
                           static_cast<const long long*>(c.boundary), static_cast<const double*>(c.grad_scale),
                           static_cast<St*>(c.px_path), static_cast<St*>(c.py_path), c.S, c.T, b0);
        if (hipGetLastError() != hipSuccess) return false;
    }
    return true;
}

template <typename Tag, bool MOD>
static rnntStatus_t run_bestpath_type(const BestpathCall& c) {
    const bool sweep = (c.phases & 1) != 0, edges = (c.phases & 2) != 0;
    if (c.scores_host == nullptr) {
        double* scores = static_cast<double*>(c.scores_dev);
        if (sweep && !launch_bp_sweep<Tag, MOD>(c, scores, 1)) return RNNT_STATUS_EXECUTION_FAILED;
        if (edges && !launch_bp_edges<Tag, MOD>(c, scores, 1)) return RNNT_STATUS_EXECUTION_FAILED;
        return RNNT_STATUS_SUCCESS;
    }
    // host scores (the one-call entry): see HOST SCORES above
    double* home = static_cast<double*>(c.back);
    const long long stride = static_cast<long long>(bp_back_words(c.S, c.T));
    if (!launch_bp_sweep<Tag, MOD>(c, home, stride)) return RNNT_STATUS_EXECUTION_FAILED;
    if (edges && !launch_bp_edges<Tag, MOD>(c, home, stride)) return RNNT_STATUS_EXECUTION_FAILED;
    double* host = static_cast<double*>(c.scores_host);
    if (hipMemcpy2DAsync(host, sizeof(double), home, static_cast<size_t>(stride) * sizeof(double), sizeof(double), c.N,
                         hipMemcpyDeviceToHost, c.stream) != hipSuccess)
        return RNNT_STATUS_MEMOPS_FAILED;
    if (!launch_bp_sweep<Tag, MOD>(c, nullptr, 0)) return RNNT_STATUS_EXECUTION_FAILED;
    if (hipStreamSynchronize(c.stream) != hipSuccess) return RNNT_STATUS_EXECUTION_FAILED;
    for (int b = 0; b < c.N; ++b)
        if (is_cost_invalid<double>(host[b])) return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

// The call `c`, checked by the C entries (pointers, shape, overlaps): only the launches are left.
template <typename Tag>
rnntStatus_t run_bestpath(const BestpathCall& c) {
    (void)hipGetLastError();                               // a stale error of an unrelated earlier HIP call is not ours
    return c.modified ? run_bestpath_type<Tag, true>(c) : run_bestpath_type<Tag, false>(c);
}

#ifndef RNNT_BESTPATH_INSTANTIATE_F32
extern template rnntStatus_t run_bestpath<F32>(const BestpathCall&);
#endif
#ifndef RNNT_BESTPATH_INSTANTIATE_F64
extern template rnntStatus_t run_bestpath<F64>(const BestpathCall&);
#endif
#ifndef RNNT_BESTPATH_INSTANTIATE_H16
extern template rnntStatus_t run_bestpath<BF16>(const BestpathCall&);
extern template rnntStatus_t run_bestpath<F16>(const BestpathCall&);
#endif

}  // namespace rnnt
