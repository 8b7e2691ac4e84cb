// rnnt_bestpath.hip -- libwarprnnt_bestpath.so: the C entry points of include/rnnt_bestpath.h and the fp32 instantiation
// (run_bestpath<F32>); rnnt_bestpath_impl.h has the driver and the launch rule, rnnt_bestpath_kernels.h the kernels.
#define RNNT_BESTPATH_INSTANTIATE_F32 1
#include "rnnt_bestpath_impl.h"

namespace rnnt {
template rnntStatus_t run_bestpath<F32>(const BestpathCall&);
}  // namespace rnnt

using namespace rnnt;

namespace {

bool bp_bad_common(int S, int T, int N, const rnntOptions& o, int dtype_code) {
    return !bp_shape_ok(S, T, N) || dtype_code < 0 || dtype_code > 3 || loc_of(o) != RNNT_GPU;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t compute_rnnt_bestpath(const void* px, const void* py, const void* boundary, int S, int T, int minibatch,
                                   int modified, void* scores, int* frames, void* back, void* px_path, void* py_path,
                                   rnntOptions options, int dtype_code) {
    if (bp_bad_common(S, T, minibatch, options, dtype_code) || py == nullptr || scores == nullptr || back == nullptr ||
        (S > 0 && (px == nullptr || frames == nullptr)))
        return RNNT_STATUS_INVALID_VALUE;
    // both indicators or neither (S == 0: px_path has no element, the pointer is not looked at)
    if (S > 0 && (px_path == nullptr) != (py_path == nullptr)) return RNNT_STATUS_INVALID_VALUE;
    const unsigned long long esz = dtype_code == 1 ? 8 : dtype_code == 0 ? 4 : 2, B = static_cast<unsigned long long>(minibatch);
    const unsigned long long xb = B * S * (modified != 0 ? T : T + 1) * esz, yb = B * (S + 1) * T * esz;
    const bool edges = py_path != nullptr;
    const SideBuf in[] = {{px, xb, esz}, {py, yb, esz}, {boundary, B * 4 * sizeof(long long), sizeof(long long)}};
    const SideBuf out[] = {{scores, B * sizeof(double), sizeof(double)}, {frames, B * S * sizeof(int), sizeof(int)},
                           {back, B * bp_back_words(S, T) * 8, 8}, {edges ? px_path : nullptr, xb, esz},
                           {edges ? py_path : nullptr, yb, esz}};
    if (side_bad_buffers(in, 3, out, 5)) return RNNT_STATUS_INVALID_VALUE;
    const bool dev = is_device_pointer(scores);
    const BestpathCall c = {px, py, boundary, dev ? scores : nullptr, dev ? nullptr : scores, frames, back, nullptr,
                            px_path, py_path, S, T, minibatch, modified != 0, reinterpret_cast<hipStream_t>(options.stream),
                            edges ? 3 : 1};
    return side_dispatch(dtype_code, [&](auto tag) { return run_bestpath<decltype(tag)>(c); });
}

rnntStatus_t compute_rnnt_bestpath_edges(const int* frames, const void* scores_device, const void* boundary,
                                         const void* grad_scale_device, int S, int T, int minibatch, int modified,
                                         void* px_path, void* py_path, rnntOptions options, int dtype_code) {
    if (bp_bad_common(S, T, minibatch, options, dtype_code) || scores_device == nullptr || py_path == nullptr ||
        (S > 0 && (frames == nullptr || px_path == nullptr)))
        return RNNT_STATUS_INVALID_VALUE;
    const unsigned long long esz = dtype_code == 1 ? 8 : dtype_code == 0 ? 4 : 2, B = static_cast<unsigned long long>(minibatch);
    const unsigned long long xb = B * S * (modified != 0 ? T : T + 1) * esz, yb = B * (S + 1) * T * esz;
    const SideBuf in[] = {{frames, B * S * sizeof(int), sizeof(int)}, {scores_device, B * sizeof(double), sizeof(double)},
                          {boundary, B * 4 * sizeof(long long), sizeof(long long)},
                          {grad_scale_device, B * sizeof(double), sizeof(double)}};
    const SideBuf out[] = {{px_path, xb, esz}, {py_path, yb, esz}};
    if (side_bad_buffers(in, 4, out, 2)) return RNNT_STATUS_INVALID_VALUE;
    const BestpathCall c = {nullptr, nullptr, boundary, const_cast<void*>(scores_device), nullptr, const_cast<int*>(frames),
                            nullptr, grad_scale_device, px_path, py_path, S, T, minibatch, modified != 0,
                            reinterpret_cast<hipStream_t>(options.stream), 2};
    return side_dispatch(dtype_code, [&](auto tag) { return run_bestpath<decltype(tag)>(c); });
}

}  // extern "C"
#pragma GCC visibility pop
