// rnnt_pstream.hip -- libwarprnnt_pstream.so: the C entry points of include/rnnt_pstream.h and the fp32 instantiation
// (run_pstream<F32>); rnnt_pstream_impl.h has the driver, rnnt_pstream_kernels.h the kernels.
#define RNNT_PSTREAM_INSTANTIATE_F32 1
#include "rnnt_pstream_impl.h"

namespace rnnt {
template rnntStatus_t run_pstream<F32>(const SideCall&, const int*, int, int, float);
}  // namespace rnnt

using namespace rnnt;

// the lattice type and the penalty of a forward call: 0 regular, 1 modified; every finite float
static inline bool pstream_bad_type(int rnnt_type, float delay_penalty) {
    return (rnnt_type != 0 && rnnt_type != 1) || !std::isfinite(delay_penalty);
}

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t get_workspace_size_pstream(int maxT, int maxU, int S, int minibatch, int dtype_code, size_t* size_bytes) {
    if (minibatch <= 0 || maxT <= 0 || maxU <= 0 || S < 1 || S > maxU || size_bytes == nullptr || dtype_code < 0 ||
        dtype_code > 3)
        return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = ps_layout(maxT, maxU, S, minibatch, dtype_code == 1 ? 8 : 4).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_loss_pstream(const void* activations, void* gradients, const int* ranges, int S, int rnnt_type,
                                       float delay_penalty, const int* flat_labels, const int* label_lengths,
                                       const int* input_lengths, int alphabet_size, int minibatch, void* costs,
                                       void* workspace, rnntOptions options, int dtype_code) {
    SideCall c;
    if (ranges == nullptr || pstream_bad_type(rnnt_type, delay_penalty) ||
        side_entry_loss(c, activations, gradients, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, costs,
                        workspace, options))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code,
                         [&](auto tag) { return run_pstream<decltype(tag)>(c, ranges, S, rnnt_type, delay_penalty); });
}

rnntStatus_t compute_rnnt_loss_pstream_fwd(const void* activations, const int* ranges, int S, int rnnt_type,
                                           float delay_penalty, const int* flat_labels, const int* label_lengths,
                                           const int* input_lengths, int alphabet_size, int minibatch, void* costs_device,
                                           void* workspace, rnntOptions options, int dtype_code, int prepare_backward) {
    SideCall c;
    if (ranges == nullptr || pstream_bad_type(rnnt_type, delay_penalty) ||
        side_entry_fwd(c, activations, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, costs_device,
                       workspace, options, prepare_backward))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code,
                         [&](auto tag) { return run_pstream<decltype(tag)>(c, ranges, S, rnnt_type, delay_penalty); });
}

rnntStatus_t compute_rnnt_loss_pstream_bwd(const void* activations, void* gradients, const void* grad_scale_device, int S,
                                           int alphabet_size, int minibatch, void* workspace, rnntOptions options,
                                           int dtype_code) {
    SideCall c;
    if (side_entry_bwd(c, activations, gradients, grad_scale_device, alphabet_size, minibatch, workspace, options))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_pstream<decltype(tag)>(c, nullptr, S, 0, 0.0f); });
}

}  // extern "C"
#pragma GCC visibility pop
