// rnnt_delay.hip -- libwarprnnt_delay.so: the C entry points of include/rnnt_delay.h and the fp32 instantiation
// (run_delay<F32>); rnnt_delay_impl.h has the driver, rnnt_delay_kernels.h the kernels.
#define RNNT_DELAY_INSTANTIATE_F32 1
#include "rnnt_delay_impl.h"

namespace rnnt {
template rnntStatus_t run_delay<F32>(const SideCall&, float, void*);
}  // namespace rnnt

using namespace rnnt;

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t get_workspace_size_delay(int maxT, int maxU, int minibatch, int dtype_code, size_t* size_bytes) {
    if (minibatch <= 0 || maxT <= 0 || maxU <= 0 || size_bytes == nullptr || dtype_code < 0 || dtype_code > 3)
        return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = delay_layout(maxT, maxU, minibatch, dtype_code == 1 ? 8 : 4).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_loss_delay(const void* activations, float delay_penalty, void* gradients, const int* flat_labels,
                                     const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch,
                                     void* costs, void* emit_frames, void* workspace, rnntOptions options, int dtype_code) {
    SideCall c;
    if (!std::isfinite(delay_penalty) ||
        side_entry_loss(c, activations, gradients, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, costs,
                        workspace, options))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_delay<decltype(tag)>(c, delay_penalty, emit_frames); });
}

rnntStatus_t compute_rnnt_loss_delay_fwd(const void* activations, float delay_penalty, const int* flat_labels,
                                         const int* label_lengths, const int* input_lengths, int alphabet_size,
                                         int minibatch, void* costs_device, void* emit_frames, void* workspace,
                                         rnntOptions options, int dtype_code, int prepare_backward) {
    SideCall c;
    if (!std::isfinite(delay_penalty) ||
        side_entry_fwd(c, activations, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, costs_device,
                       workspace, options, prepare_backward))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_delay<decltype(tag)>(c, delay_penalty, emit_frames); });
}

rnntStatus_t compute_rnnt_loss_delay_bwd(const void* activations, void* gradients, const void* grad_scale_device,
                                         int alphabet_size, int minibatch, void* workspace, rnntOptions options,
                                         int dtype_code) {
    SideCall c;
    if (side_entry_bwd(c, activations, gradients, grad_scale_device, alphabet_size, minibatch, workspace, options))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_delay<decltype(tag)>(c, 0.0f, nullptr); });
}

}  // extern "C"
#pragma GCC visibility pop
