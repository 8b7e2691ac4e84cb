// rnnt_expect_impl.h -- host driver of libwarprnnt_expect.so (include/rnnt_expect.h): run_expect<Tag>.  One
// instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_expect.hip   F32 (+ every C entry point)     rnnt_expect_f64.hip   F64     rnnt_expect_h16.hip   BF16, F16
// The library has no workspace: scores, expect, nodes and the gradients are outputs.
//
// LAUNCH RULE (tests/expect_forms.py restates it).  U = S + 1 lattice rows of the TENSOR (not of a sample's rectangle).
//   forward    expect_fwd_kernel<Tag, MOD, MULTI>, a block per sample on grid.x:
//                U <= kExWaveMaxU          one wavefront (MULTI = false)
//                U <= kExMaxU              64 * ceil(U / 64) threads
//   backward   expect_bwd_kernel<Tag, MOD, MULTI, WITH_COST_GRADS>, the same rule; WITH_COST_GRADS: cx_grad / cy_grad taken
// HOST SCORES.  Without a workspace the two scalars have no device home but an output: the forward launch parks them in the
// pair nodes[b, 0, 0] (the last thing a block does), the backward launch reads them there (it never reads that pair as a
// node: it is the rectangle's source, (0, 0) by definition, or outside the rectangle), two strided copies take them to the
// host, and expect_restore_kernel<Tag> puts the node's own pair back.
#pragma once
#include "rnnt_side_host.h"
#include "rnnt_expect_kernels.h"
#include "../../include/rnnt_expect.h"

namespace rnnt {

constexpr int kExMaxU = 1024;           // S + 1 at most: a thread per row

// The arguments of the three entries, untyped as they cross the C-ABI.  phases: bit 0 = forward, bit 1 = backward.
struct ExpectCall {
    const void *px, *py, *cx, *cy, *boundary;
    void *scores_dev, *expect_dev, *scores_host, *expect_host;
    void* nodes;
    const void *g_expect, *g_score;
    void *px_grad, *py_grad, *cx_grad, *cy_grad;
    int S, T, N;
    bool modified;
    hipStream_t stream;
    int phases;
};

static inline bool ex_shape_ok(int S, int T, int N) { return side_lattice_ok(S, T, N, kExMaxU); }

template <typename Tag, bool MOD>
static bool launch_ex_fwd(const ExpectCall& c, double* scores, double* expect, long long stride) {
    using St = typename Tag::store;
    const int U = c.S + 1;
    const dim3 grid(c.N);
#define RNNT_EX_FWD(MULTI, THREADS)                                                                                      \
    hipLaunchKernelGGL((expect_fwd_kernel<Tag, MOD, MULTI>), grid, dim3(THREADS), 0, c.stream,                           \
                       static_cast<const St*>(c.px), static_cast<const St*>(c.py), static_cast<const St*>(c.cx),         \
                       static_cast<const St*>(c.cy), static_cast<const long long*>(c.boundary), scores, expect, stride,  \
                       static_cast<double*>(c.nodes), c.S, c.T)
    if (U <= kExWaveMaxU) RNNT_EX_FWD(false, 64);
    else RNNT_EX_FWD(true, (U + 63) / 64 * 64);
#undef RNNT_EX_FWD
    return hipGetLastError() == hipSuccess;
}

template <typename Tag, bool MOD, bool WCG>
static bool launch_ex_bwd(const ExpectCall& c, const double* scores, const double* expect, long long stride) {
    using St = typename Tag::store;
    const int U = c.S + 1;
    const dim3 grid(c.N);
#define RNNT_EX_BWD(MULTI, THREADS)                                                                                      \
    hipLaunchKernelGGL((expect_bwd_kernel<Tag, MOD, MULTI, WCG>), grid, dim3(THREADS), 0, c.stream,                      \
                       static_cast<const St*>(c.px), static_cast<const St*>(c.py), static_cast<const St*>(c.cx),         \
                       static_cast<const St*>(c.cy), static_cast<const long long*>(c.boundary),                          \
                       static_cast<const double*>(c.nodes), scores, expect, stride,                                      \
                       static_cast<const double*>(c.g_expect), static_cast<const double*>(c.g_score),                    \
                       static_cast<St*>(c.px_grad), static_cast<St*>(c.py_grad), static_cast<St*>(c.cx_grad),            \
                       static_cast<St*>(c.cy_grad), c.S, c.T)
    if (U <= kExWaveMaxU) RNNT_EX_BWD(false, 64);
    else RNNT_EX_BWD(true, (U + 63) / 64 * 64);
#undef RNNT_EX_BWD
    return hipGetLastError() == hipSuccess;
}

template <typename Tag, bool MOD>
static rnntStatus_t run_expect_type(const ExpectCall& c) {
    const bool fwd = (c.phases & 1) != 0, bwd = (c.phases & 2) != 0, wcg = c.cy_grad != nullptr;
    auto backward = [&](const double* sc, const double* ec, long long stride) {
        return wcg ? launch_ex_bwd<Tag, MOD, true>(c, sc, ec, stride) : launch_ex_bwd<Tag, MOD, false>(c, sc, ec, stride);
    };
    if (c.scores_host == nullptr) {
        double *sc = static_cast<double*>(c.scores_dev), *ec = static_cast<double*>(c.expect_dev);
        if (fwd && !launch_ex_fwd<Tag, MOD>(c, sc, ec, 1)) return RNNT_STATUS_EXECUTION_FAILED;
        if (bwd && !backward(sc, ec, 1)) return RNNT_STATUS_EXECUTION_FAILED;
        return RNNT_STATUS_SUCCESS;
    }
    // host scalars (the one-call entry): see HOST SCORES above
    double* home = static_cast<double*>(c.nodes);
    const long long stride = 2LL * (c.S + 1) * (c.T + 1);
    if (!launch_ex_fwd<Tag, MOD>(c, home, home + 1, stride)) return RNNT_STATUS_EXECUTION_FAILED;
    if (bwd && !backward(home, home + 1, stride)) return RNNT_STATUS_EXECUTION_FAILED;
    double *hs = static_cast<double*>(c.scores_host), *he = static_cast<double*>(c.expect_host);
    const size_t pitch = static_cast<size_t>(stride) * sizeof(double);
    if (hipMemcpy2DAsync(hs, sizeof(double), home, pitch, sizeof(double), c.N, hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
        hipMemcpy2DAsync(he, sizeof(double), home + 1, pitch, sizeof(double), c.N, hipMemcpyDeviceToHost, c.stream) != hipSuccess)
        return RNNT_STATUS_MEMOPS_FAILED;
    hipLaunchKernelGGL((expect_restore_kernel<Tag>), dim3((c.N + 255) / 256), dim3(256), 0, c.stream,
                       static_cast<const long long*>(c.boundary), home, c.S, c.T, c.N);
    if (hipGetLastError() != hipSuccess) return RNNT_STATUS_EXECUTION_FAILED;
    if (hipStreamSynchronize(c.stream) != hipSuccess) return RNNT_STATUS_EXECUTION_FAILED;
    for (int b = 0; b < c.N; ++b)
        if (is_cost_invalid<double>(hs[b])) return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

// The call `c`, checked by the C entries (pointers, shape, overlaps): only the launches are left.
template <typename Tag>
rnntStatus_t run_expect(const ExpectCall& c) {
    (void)hipGetLastError();                               // a stale error of an unrelated earlier HIP call is not ours
    return c.modified ? run_expect_type<Tag, true>(c) : run_expect_type<Tag, false>(c);
}

#ifndef RNNT_EXPECT_INSTANTIATE_F32
extern template rnntStatus_t run_expect<F32>(const ExpectCall&);
#endif
#ifndef RNNT_EXPECT_INSTANTIATE_F64
extern template rnntStatus_t run_expect<F64>(const ExpectCall&);
#endif
#ifndef RNNT_EXPECT_INSTANTIATE_H16
extern template rnntStatus_t run_expect<BF16>(const ExpectCall&);
extern template rnntStatus_t run_expect<F16>(const ExpectCall&);
#endif

}  // namespace rnnt
