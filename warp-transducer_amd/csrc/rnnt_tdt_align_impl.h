// rnnt_tdt_align_impl.h -- host driver of libwarprnnt_tdt_align.so (include/rnnt_tdt_align.h): the TDT best-path alignment
// (run_tdt_align<Tag>).  One instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_tdt_align.hip   F32 (+ every C entry point)     rnnt_tdt_align_f64.hip   F64     rnnt_tdt_align_h16.hip   BF16, F16
// Stage 1 is the TDT loss's statistics kernel through its own launcher (launch_tdt_stats, rnnt_tdt_impl.h, which also has the
// duration and shape rules and the workspace layout); stages 2 and 3 are rnnt_tdt_align_kernels.h's.  run_tdt is never
// instantiated here, so these code objects hold none of the loss's other kernels.
#pragma once
#include "rnnt_tdt_impl.h"
#include "rnnt_tdt_align_kernels.h"
#include "../../include/rnnt_tdt_align.h"

namespace rnnt {

// What the C entry hands over, untyped.
struct TdtAlignCall {
    const void* acts;
    const int *labels, *label_lengths, *input_lengths;
    double* score;
    int *frames, *durs;
    void* workspace;
    int A, N;
    rnntOptions opt;
};

// Workspace: the loss's cell table (tdt_layout).  alpha holds the cell values, beta the back-pointer bytes (N maxT maxU
// bytes, at most a quarter of it), ll the best base-2 weight, the costs slot the duration index of the final blank.  The
// per-diagonal offsets live only in the lattice kernel's LDS ring: the layout's offa array stays unused.
template <typename Tag>
rnntStatus_t run_tdt_align(const TdtAlignCall& c, const int* durations, int D, float sigma) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const St* acts = static_cast<const St*>(c.acts);
    const int A = c.A, N = c.N, maxT = c.opt.maxT, maxU = c.opt.maxU, blank = c.opt.blank_label;
    (void)hipGetLastError();                           // a stale error of an unrelated earlier HIP call is not ours
    TdtDurations dur;
    if (!tdt_durations(durations, D, dur)) return RNNT_STATUS_INVALID_VALUE;
    if (!tdt_shape_ok(A, D, N, maxT, maxU, blank) || !(sigma - sigma == 0.0f)) return RNNT_STATUS_INVALID_VALUE;
    if (reinterpret_cast<uintptr_t>(c.acts) % sizeof(St) != 0) return RNNT_STATUS_INVALID_VALUE;
    const CellTable<C> w = carve_cell_table<C>(tdt_layout(maxT, maxU, N, D, sizeof(C)), c.workspace, nullptr);
    unsigned char* bp = reinterpret_cast<unsigned char*>(w.beta);
    int* fin = reinterpret_cast<int*>(w.costs);
    hipStream_t s = reinterpret_cast<hipStream_t>(c.opt.stream);

    bool ok = hipMemsetAsync(w.poison, 0, sizeof(int) * N, s) == hipSuccess;
    ok = ok && launch_tdt_stats<Tag>(acts, c.labels, c.input_lengths, c.label_lengths, w.tab, w.poison, N, maxT, maxU, A, D,
                                     blank, sigma, s);
    // lattice: a block per sample, a thread per cell of the widest diagonal (up to 1024)
    const int threads = maxU >= 1024 ? 1024 : (maxU + 63) / 64 * 64;
    for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
        hipLaunchKernelGGL((tdt_align_lattice_kernel<C>), dim3(grid_samples(N, b0)), dim3(threads), 0, s, w.tab, w.alpha, bp,
                           w.ll, fin, c.input_lengths, c.label_lengths, dur, maxT, maxU, b0);
        ok = hipGetLastError() == hipSuccess;
    }
    if (ok) {
        hipLaunchKernelGGL((tdt_align_traceback_kernel<C>), dim3((N + 63) / 64), dim3(64), 0, s, bp, w.ll, fin, w.poison,
                           c.input_lengths, c.label_lengths, c.score, c.frames, c.durs, dur, maxT, maxU, N);
        ok = hipGetLastError() == hipSuccess;
    }
    return ok ? RNNT_STATUS_SUCCESS : RNNT_STATUS_EXECUTION_FAILED;
}

#ifndef RNNT_TDT_ALIGN_INSTANTIATE_F32
extern template rnntStatus_t run_tdt_align<F32>(const TdtAlignCall&, const int*, int, float);
#endif
#ifndef RNNT_TDT_ALIGN_INSTANTIATE_F64
extern template rnntStatus_t run_tdt_align<F64>(const TdtAlignCall&, const int*, int, float);
#endif
#ifndef RNNT_TDT_ALIGN_INSTANTIATE_H16
extern template rnntStatus_t run_tdt_align<BF16>(const TdtAlignCall&, const int*, int, float);
extern template rnntStatus_t run_tdt_align<F16>(const TdtAlignCall&, const int*, int, float);
#endif

}  // namespace rnnt
