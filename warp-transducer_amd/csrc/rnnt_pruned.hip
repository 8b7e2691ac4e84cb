// rnnt_pruned.hip -- libwarprnnt_pruned.so: the C entry points of include/rnnt_pruned.h and the fp32 instantiations
// (run_pruned<F32>, run_prune_ranges<F32>); rnnt_pruned_impl.h has the driver, rnnt_pruned_kernels.h the kernels.
#define RNNT_PRUNED_INSTANTIATE_F32 1
#include "rnnt_pruned_impl.h"

#include <type_traits>

namespace rnnt {
template rnntStatus_t run_pruned<F32>(const SideCall&, const int*, int);
template rnntStatus_t run_prune_ranges<F32>(const SideCall&, const void*, int, int*);
}  // namespace rnnt

using namespace rnnt;

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t get_workspace_size_pruned(int maxT, int maxU, int minibatch, int dtype_code, size_t* size_bytes) {
    if (minibatch <= 0 || maxT <= 0 || maxU <= 0 || size_bytes == nullptr || dtype_code < 0 || dtype_code > 3)
        return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = pruned_layout(maxT, maxU, minibatch, dtype_code == 1 ? 8 : 4).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_loss_pruned(const void* activations, void* gradients, const int* ranges, int S,
                                      const int* flat_labels, const int* label_lengths, const int* input_lengths,
                                      int alphabet_size, int minibatch, void* costs, void* workspace,
                                      rnntOptions options, int dtype_code) {
    SideCall c;
    if (ranges == nullptr || side_entry_loss(c, activations, gradients, flat_labels, label_lengths, input_lengths,
                                             alphabet_size, minibatch, costs, workspace, options))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_pruned<decltype(tag)>(c, ranges, S); });
}

rnntStatus_t compute_rnnt_loss_pruned_fwd(const void* activations, const int* ranges, int S, const int* flat_labels,
                                          const int* label_lengths, const int* input_lengths, int alphabet_size,
                                          int minibatch, void* costs_device, void* workspace, rnntOptions options,
                                          int dtype_code, int prepare_backward) {
    SideCall c;
    if (ranges == nullptr || side_entry_fwd(c, activations, flat_labels, label_lengths, input_lengths, alphabet_size,
                                            minibatch, costs_device, workspace, options, prepare_backward))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_pruned<decltype(tag)>(c, ranges, S); });
}

rnntStatus_t compute_rnnt_loss_pruned_bwd(const void* activations, void* gradients, const void* grad_scale_device, int S,
                                          int alphabet_size, int minibatch, void* workspace, rnntOptions options,
                                          int dtype_code) {
    SideCall c;
    if (side_entry_bwd(c, activations, gradients, grad_scale_device, alphabet_size, minibatch, workspace, options))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) { return run_pruned<decltype(tag)>(c, nullptr, S); });
}

rnntStatus_t compute_rnnt_prune_ranges_add(const void* trans_acts, const void* pred_acts, const int* flat_labels,
                                           const int* label_lengths, const int* input_lengths, int alphabet_size,
                                           int minibatch, int S, int* ranges, void* workspace, rnntOptions options,
                                           int dtype_code) {
    SideCall c;                // (a forward-only call whose output, in the place of the costs, is the ranges)
    if (pred_acts == nullptr || side_entry_fwd(c, trans_acts, flat_labels, label_lengths, input_lengths, alphabet_size,
                                               minibatch, ranges, workspace, options, 0))
        return RNNT_STATUS_INVALID_VALUE;
    return side_dispatch(dtype_code, [&](auto tag) -> rnntStatus_t {
        using Tag = decltype(tag);
        if constexpr (std::is_same<Tag, F64>::value) return RNNT_STATUS_INVALID_VALUE;     // (the additive joint has no fp64 form)
        else return run_prune_ranges<Tag>(c, pred_acts, S, ranges);
    });
}

}  // extern "C"
#pragma GCC visibility pop
