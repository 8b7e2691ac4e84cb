// rnnt_ar.hip -- libwarprnnt_ar.so: the C entry points of include/rnnt_ar.h and the fp32 instantiation (run_ar<F32>);
// rnnt_ar_impl.h has the driver, rnnt_ar_kernels.h the kernels.
#define RNNT_AR_INSTANTIATE_F32 1
#include "rnnt_ar_impl.h"

namespace rnnt {
template rnntStatus_t run_ar<F32>(const SideCall&, const int*, const int*);
}  // namespace rnnt

using namespace rnnt;

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t get_workspace_size_ar(int maxT, int maxU, int minibatch, int dtype_code, size_t* size_bytes) {
    if (minibatch <= 0 || maxT <= 0 || maxU <= 0 || size_bytes == nullptr || dtype_code < 0 || dtype_code > 3)
        return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = ar_layout(maxT, maxU, minibatch, dtype_code == 1 ? 8 : 4).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_loss_ar(const void* activations, void* gradients, const int* flat_labels, const int* label_lengths,
                                  const int* input_lengths, const int* emit_lo, const int* emit_hi, int alphabet_size,
                                  int minibatch, void* costs, void* workspace, rnntOptions options, int dtype_code) {
    SideCall c;
    if (emit_lo == nullptr || emit_hi == nullptr ||
        side_entry_loss(c, activations, gradients, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, costs,
                        workspace, options))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_ar<decltype(tag)>(c, emit_lo, emit_hi); });
}

rnntStatus_t compute_rnnt_loss_ar_fwd(const void* activations, const int* flat_labels, const int* label_lengths,
                                      const int* input_lengths, const int* emit_lo, const int* emit_hi, int alphabet_size,
                                      int minibatch, void* costs_device, void* workspace, rnntOptions options, int dtype_code,
                                      int prepare_backward) {
    SideCall c;
    if (emit_lo == nullptr || emit_hi == nullptr ||
        side_entry_fwd(c, activations, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, costs_device,
                       workspace, options, prepare_backward))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_ar<decltype(tag)>(c, emit_lo, emit_hi); });
}

rnntStatus_t compute_rnnt_loss_ar_bwd(const void* activations, void* gradients, const void* grad_scale_device,
                                      int alphabet_size, int minibatch, void* workspace, rnntOptions options, int dtype_code) {
    SideCall c;
    if (side_entry_bwd(c, activations, gradients, grad_scale_device, alphabet_size, minibatch, workspace, options))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_ar<decltype(tag)>(c, nullptr, nullptr); });
}

}  // extern "C"
#pragma GCC visibility pop
