// rnnt_mi.hip -- libwarprnnt_mi.so: the C entry points of include/rnnt_mi.h and the fp32 instantiation (run_mi<F32>);
// rnnt_mi_impl.h has the driver, rnnt_mi_kernels.h the kernels.
#define RNNT_MI_INSTANTIATE_F32 1
#include "rnnt_mi_impl.h"

namespace rnnt {
template rnntStatus_t run_mi<F32>(const MiCall&);

// What every entry refuses before the dtype switch: the shape (limits included), the location, the workspace.
static bool mi_bad_call(int S, int T, int N, const void* workspace, const rnntOptions& o) {
    return !mi_shape_ok(S, T, N) || workspace == nullptr || loc_of(o) != RNNT_GPU;
}
}  // namespace rnnt

using namespace rnnt;

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t get_workspace_size_mi(int S, int T, int minibatch, int modified, int dtype_code, size_t* size_bytes) {
    if (minibatch <= 0 || S < 0 || T <= 0 || size_bytes == nullptr || dtype_code < 0 || dtype_code > 3)
        return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = mi_layout(S, T, minibatch, modified != 0, dtype_code == 1 ? 8 : 4).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_mi(const void* px, const void* py, const void* boundary, int S, int T, int minibatch, int modified,
                             void* scores, void* px_grad, void* py_grad, void* workspace, rnntOptions options,
                             int dtype_code) {
    if (mi_bad_call(S, T, minibatch, workspace, options) || scores == nullptr || py == nullptr || (S > 0 && px == nullptr))
        return RNNT_STATUS_INVALID_VALUE;
    // both gradients or neither (S == 0: px_grad has no element, the pointer is not looked at)
    if (S > 0 && (px_grad == nullptr) != (py_grad == nullptr)) return RNNT_STATUS_INVALID_VALUE;
    const bool dev = is_device_pointer(scores);
    const MiCall c = {px, py, boundary, px_grad, py_grad, nullptr, dev ? scores : nullptr, dev ? nullptr : scores, workspace,
                      S, T, minibatch, modified != 0, options, 3, py_grad != nullptr};
    return side_dispatch(dtype_code, [&](auto tag) { return run_mi<decltype(tag)>(c); });
}

rnntStatus_t compute_rnnt_mi_fwd(const void* px, const void* py, const void* boundary, int S, int T, int minibatch,
                                 int modified, void* scores_device, void* workspace, rnntOptions options, int dtype_code,
                                 int prepare_backward) {
    if (mi_bad_call(S, T, minibatch, workspace, options) || scores_device == nullptr || py == nullptr ||
        (S > 0 && px == nullptr))
        return RNNT_STATUS_INVALID_VALUE;
    const MiCall c = {px, py, boundary, nullptr, nullptr, nullptr, scores_device, nullptr, workspace,
                      S, T, minibatch, modified != 0, options, 1, prepare_backward != 0};
    return side_dispatch(dtype_code, [&](auto tag) { return run_mi<decltype(tag)>(c); });
}

rnntStatus_t compute_rnnt_mi_bwd(void* px_grad, void* py_grad, const void* grad_scale_device, int S, int T, int minibatch,
                                 int modified, void* workspace, rnntOptions options, int dtype_code) {
    if (mi_bad_call(S, T, minibatch, workspace, options) || py_grad == nullptr || (S > 0 && px_grad == nullptr))
        return RNNT_STATUS_INVALID_VALUE;
    const MiCall c = {nullptr, nullptr, nullptr, px_grad, py_grad, grad_scale_device, nullptr, nullptr, workspace,
                      S, T, minibatch, modified != 0, options, 2, true};
    return side_dispatch(dtype_code, [&](auto tag) { return run_mi<decltype(tag)>(c); });
}

}  // extern "C"
#pragma GCC visibility pop
