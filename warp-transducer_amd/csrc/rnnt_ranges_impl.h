// rnnt_ranges_impl.h -- host driver of libwarprnnt_ranges.so (include/rnnt_ranges.h): run_ranges<Tag>.  One instantiation
// per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_ranges.hip   F32 (+ every C entry point)     rnnt_ranges_f64.hip   F64     rnnt_ranges_h16.hip   BF16, F16
// The library has no workspace: the raw starts go to `ranges`, which the repair then rewrites in place.
//
// LAUNCH RULE.  U = S + 1 rows of the TENSOR, TF = rg_tile(U) frames per tile (rnnt_ranges_kernels.h: 32 up to U = 191, then
// 16, 8, 4, 2 and 1 from U = 3072).  The samples go over grid.y (window, coverage) or grid.x (repair) in slices of
// kGridSamples.
//   entry 1    ranges_window_kernel<Tag, MOD>, grid (ceil(T / TF), slice), block 64 * min(4, TF), TF * (U | 1) doubles of LDS;
//              then ranges_repair_kernel<0>, grid (slice), block kRgRepairBlock
//   entry 2    ranges_coverage_kernel<Tag, MOD>, grid, block and LDS of the window kernel
#pragma once
#include "rnnt_side_host.h"
#include "rnnt_ranges_kernels.h"
#include "../../include/rnnt_ranges.h"

namespace rnnt {

constexpr int kRgMaxU = 4096;           // S + 1 at most: include/rnnt_mi.h's

// The arguments of both entries, untyped as they cross the C-ABI.  kept == nullptr: entry 1 (ranges is the output);
// otherwise entry 2 (ranges is an input).
struct RangesCall {
    const void *px, *py, *boundary;
    int* ranges;
    double* kept;
    int S, T, N, R, step;
    bool modified;
    hipStream_t stream;
};

static inline bool rg_shape_ok(int S, int T, int N) { return side_lattice_ok(S, T, N, kRgMaxU); }

template <typename Tag, bool MOD>
static rnntStatus_t run_ranges_type(const RangesCall& c) {
    using St = typename Tag::store;
    const int U = c.S + 1, TF = rg_tile(U);
    int lg = 0;
    while ((1 << lg) < TF) ++lg;
    const unsigned threads = 64u * (TF < 4 ? TF : 4), gx = static_cast<unsigned>((c.T + TF - 1) / TF);
    const size_t lds = static_cast<size_t>(TF) * rg_stride(U) * sizeof(double);
    const St *px = static_cast<const St*>(c.px), *py = static_cast<const St*>(c.py);
    const long long* bd = static_cast<const long long*>(c.boundary);
    for (int b0 = 0; b0 < c.N; b0 += kGridSamples) {
        const dim3 grid(gx, grid_samples(c.N, b0));
        if (c.kept == nullptr)
            hipLaunchKernelGGL((ranges_window_kernel<Tag, MOD>), grid, dim3(threads), lds, c.stream, px, py, bd, c.ranges, c.S,
                               c.T, c.R, lg, b0);
        else
            hipLaunchKernelGGL((ranges_coverage_kernel<Tag, MOD>), grid, dim3(threads), lds, c.stream, px, py, bd, c.ranges,
                               c.kept, c.S, c.T, c.R, lg, b0);
        if (hipGetLastError() != hipSuccess) return RNNT_STATUS_EXECUTION_FAILED;
    }
    if (c.kept == nullptr) {
        for (int b0 = 0; b0 < c.N; b0 += kGridSamples) {
            hipLaunchKernelGGL(ranges_repair_kernel<0>, dim3(grid_samples(c.N, b0)), dim3(kRgRepairBlock), 0, c.stream, bd,
                               c.ranges, c.S, c.T, c.R, c.step, b0);
            if (hipGetLastError() != hipSuccess) return RNNT_STATUS_EXECUTION_FAILED;
        }
    }
    return RNNT_STATUS_SUCCESS;
}

// The call `c`, checked by the C entries (pointers, shape, R and step, overlaps): only the launches are left.
template <typename Tag>
rnntStatus_t run_ranges(const RangesCall& c) {
    (void)hipGetLastError();                               // a stale error of an unrelated earlier HIP call is not ours
    return c.modified ? run_ranges_type<Tag, true>(c) : run_ranges_type<Tag, false>(c);
}

#ifndef RNNT_RANGES_INSTANTIATE_F32
extern template rnntStatus_t run_ranges<F32>(const RangesCall&);
#endif
#ifndef RNNT_RANGES_INSTANTIATE_F64
extern template rnntStatus_t run_ranges<F64>(const RangesCall&);
#endif
#ifndef RNNT_RANGES_INSTANTIATE_H16
extern template rnntStatus_t run_ranges<BF16>(const RangesCall&);
extern template rnntStatus_t run_ranges<F16>(const RangesCall&);
#endif

}  // namespace rnnt
