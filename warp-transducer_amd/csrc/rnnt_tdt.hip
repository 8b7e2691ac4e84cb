// rnnt_tdt.hip -- libwarprnnt_tdt.so: the C entry points of include/rnnt_tdt.h and the fp32 instantiation (run_tdt<F32>);
// rnnt_tdt_impl.h has the driver, rnnt_tdt_kernels.h the kernels.
#define RNNT_TDT_INSTANTIATE_F32 1
#include "rnnt_tdt_impl.h"

namespace rnnt {
template rnntStatus_t run_tdt<F32>(const SideCall&, const int*, int, float);
}  // namespace rnnt

using namespace rnnt;

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t get_workspace_size_tdt(int maxT, int maxU, int minibatch, int num_durations, int dtype_code,
                                    size_t* size_bytes) {
    if (minibatch <= 0 || maxT <= 0 || maxU <= 0 || size_bytes == nullptr || dtype_code < 0 || dtype_code > 3 ||
        num_durations < 1 || num_durations > kTdtMaxDurations)
        return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = tdt_layout(maxT, maxU, minibatch, num_durations, dtype_code == 1 ? 8 : 4).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_tdt_loss(const void* activations, void* gradients, const int* durations, int num_durations,
                              float sigma, const int* flat_labels, const int* label_lengths, const int* input_lengths,
                              int alphabet_size, int minibatch, void* costs, void* workspace, rnntOptions options,
                              int dtype_code) {
    SideCall c;
    if (side_entry_loss(c, activations, gradients, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, costs,
                        workspace, options))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_tdt<decltype(tag)>(c, durations, num_durations, sigma); });
}

rnntStatus_t compute_tdt_loss_fwd(const void* activations, const int* durations, int num_durations, float sigma,
                                  const int* flat_labels, const int* label_lengths, const int* input_lengths,
                                  int alphabet_size, int minibatch, void* costs_device, void* workspace,
                                  rnntOptions options, int dtype_code, int prepare_backward) {
    SideCall c;
    if (side_entry_fwd(c, activations, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, costs_device,
                       workspace, options, prepare_backward))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_tdt<decltype(tag)>(c, durations, num_durations, sigma); });
}

rnntStatus_t compute_tdt_loss_bwd(const void* activations, void* gradients, const void* grad_scale_device,
                                  const int* durations, int num_durations, int alphabet_size, int minibatch,
                                  void* workspace, rnntOptions options, int dtype_code) {
    SideCall c;
    if (side_entry_bwd(c, activations, gradients, grad_scale_device, alphabet_size, minibatch, workspace, options))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_tdt<decltype(tag)>(c, durations, num_durations, 0.0f); });
}

}  // extern "C"
#pragma GCC visibility pop
