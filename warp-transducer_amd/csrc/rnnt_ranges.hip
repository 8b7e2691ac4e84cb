// rnnt_ranges.hip -- libwarprnnt_ranges.so: the C entry points of include/rnnt_ranges.h and the fp32 instantiation
// (run_ranges<F32>); rnnt_ranges_impl.h has the driver and the launch rule, rnnt_ranges_kernels.h the kernels.
#define RNNT_RANGES_INSTANTIATE_F32 1
#include "rnnt_ranges_impl.h"

namespace rnnt {
template rnntStatus_t run_ranges<F32>(const RangesCall&);
}  // namespace rnnt

using namespace rnnt;

namespace {

bool rg_bad_common(const void* px, const void* py, int S, int T, int N, int R, const rnntOptions& o, int dtype_code) {
    return !rg_shape_ok(S, T, N) || dtype_code < 0 || dtype_code > 3 || loc_of(o) != RNNT_GPU || R < 1 || R > S + 1 ||
           py == nullptr || (S > 0 && px == nullptr);
}

// The sizes of a call's buffers in bytes: the element, px, py, boundary, ranges, kept.
struct RgSizes { unsigned long long esz, xb, yb, bd, rg, kp; };
RgSizes rg_sizes(int S, int T, int N, int modified, int dtype_code) {
    const unsigned long long esz = dtype_code == 1 ? 8 : dtype_code == 0 ? 4 : 2, B = static_cast<unsigned long long>(N);
    return {esz, B * S * (modified != 0 ? T : T + 1) * esz, B * (S + 1) * T * esz, B * 4 * sizeof(long long),
            B * T * sizeof(int), B * T * sizeof(double)};
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t compute_rnnt_prune_ranges_occ(const void* px_grad, const void* py_grad, const void* boundary, int S, int T,
                                           int minibatch, int modified, int R, int step, int* ranges, rnntOptions options,
                                           int dtype_code) {
    if (rg_bad_common(px_grad, py_grad, S, T, minibatch, R, options, dtype_code) || ranges == nullptr || step < 1 ||
        step > (R - 1 > 1 ? R - 1 : 1))
        return RNNT_STATUS_INVALID_VALUE;
    const RgSizes z = rg_sizes(S, T, minibatch, modified, dtype_code);
    const SideBuf in[] = {{S > 0 ? px_grad : nullptr, z.xb, z.esz}, {py_grad, z.yb, z.esz}, {boundary, z.bd, sizeof(long long)}};
    const SideBuf out = {ranges, z.rg, sizeof(int)};
    if (side_bad_buffers(in, 3, &out, 1)) return RNNT_STATUS_INVALID_VALUE;
    const RangesCall c = {px_grad, py_grad, boundary, ranges, nullptr, S, T, minibatch, R, step, modified != 0,
                          reinterpret_cast<hipStream_t>(options.stream)};
    return side_dispatch(dtype_code, [&](auto tag) { return run_ranges<decltype(tag)>(c); });
}

rnntStatus_t compute_rnnt_range_coverage(const void* px_grad, const void* py_grad, const void* boundary, const int* ranges,
                                         int S, int T, int minibatch, int modified, int R, double* kept, rnntOptions options,
                                         int dtype_code) {
    if (rg_bad_common(px_grad, py_grad, S, T, minibatch, R, options, dtype_code) || ranges == nullptr || kept == nullptr)
        return RNNT_STATUS_INVALID_VALUE;
    const RgSizes z = rg_sizes(S, T, minibatch, modified, dtype_code);
    const SideBuf in[] = {{S > 0 ? px_grad : nullptr, z.xb, z.esz}, {py_grad, z.yb, z.esz}, {boundary, z.bd, sizeof(long long)},
                          {ranges, z.rg, sizeof(int)}};
    const SideBuf out = {kept, z.kp, sizeof(double)};
    if (side_bad_buffers(in, 4, &out, 1)) return RNNT_STATUS_INVALID_VALUE;
    const RangesCall c = {px_grad, py_grad, boundary, const_cast<int*>(ranges), kept, S, T, minibatch, R, 1, modified != 0,
                          reinterpret_cast<hipStream_t>(options.stream)};
    return side_dispatch(dtype_code, [&](auto tag) { return run_ranges<decltype(tag)>(c); });
}

}  // extern "C"
#pragma GCC visibility pop
