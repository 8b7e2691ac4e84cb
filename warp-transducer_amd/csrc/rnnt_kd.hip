// rnnt_kd.hip -- libwarprnnt_kd.so: the C entry points of include/rnnt_kd.h and the fp32 instantiation (run_kd<F32>);
// rnnt_kd_impl.h has the driver, rnnt_kd_kernels.h the kernels.
#define RNNT_KD_INSTANTIATE_F32 1
#include "rnnt_kd_impl.h"

namespace rnnt {
template rnntStatus_t run_kd<F32>(const SideCall&, const void*, int, float);
}  // namespace rnnt

using namespace rnnt;

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t get_workspace_size_kd(int maxT, int maxU, int minibatch, int dtype_code, size_t* size_bytes) {
    if (minibatch <= 0 || maxT <= 0 || maxU <= 0 || size_bytes == nullptr || dtype_code < 0 || dtype_code > 3)
        return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = kd_layout(maxT, maxU, minibatch, dtype_code == 1 ? 8 : 4).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_kd_loss(const void* activations, const void* teacher, void* gradients, const int* flat_labels,
                             const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch,
                             void* costs, void* workspace, rnntOptions options, int dtype_code, int mode,
                             float temperature) {
    SideCall c;
    if (!kd_params_ok(mode, temperature) || teacher == nullptr ||
        side_entry_loss(c, activations, gradients, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, costs,
                        workspace, options))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_kd<decltype(tag)>(c, teacher, mode, temperature); });
}

rnntStatus_t compute_kd_loss_fwd(const void* activations, const void* teacher, const int* flat_labels,
                                 const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch,
                                 void* costs_device, void* workspace, rnntOptions options, int dtype_code, int mode,
                                 float temperature, int prepare_backward) {
    SideCall c;
    if (!kd_params_ok(mode, temperature) || teacher == nullptr ||
        side_entry_fwd(c, activations, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, costs_device,
                       workspace, options, prepare_backward))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_kd<decltype(tag)>(c, teacher, mode, temperature); });
}

rnntStatus_t compute_kd_loss_bwd(const void* activations, const void* teacher, void* gradients,
                                 const void* grad_scale_device, int alphabet_size, int minibatch, void* workspace,
                                 rnntOptions options, int dtype_code, int mode, float temperature) {
    SideCall c;
    if (!kd_params_ok(mode, temperature) || (teacher == nullptr && mode == 1) ||      // (collapsed: the stream reads the student only)
        side_entry_bwd(c, activations, gradients, grad_scale_device, alphabet_size, minibatch, workspace, options))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_kd<decltype(tag)>(c, teacher, mode, temperature); });
}

}  // extern "C"
#pragma GCC visibility pop
