// rnnt_pruned.hip -- libwarprnnt_pruned.so: the C entry points of include/rnnt_pruned.h and the fp32 instantiations
// (run_pruned<F32>, run_prune_ranges<F32>); rnnt_pruned_impl.h has the driver, rnnt_pruned_kernels.h the kernels.
#define RNNT_PRUNED_INSTANTIATE_F32 1
#include "rnnt_pruned_impl.h"

namespace rnnt {
template rnntStatus_t run_pruned<F32>(const float*, float*, const float*, const int*, int, const int*, const int*, const int*,
                                      int, int, float*, float*, void*, const rnntOptions&, int, bool);
template rnntStatus_t run_prune_ranges<F32>(const float*, const float*, const int*, const int*, const int*, int, int, int, int*,
                                            void*, const rnntOptions&);
}  // namespace rnnt

using namespace rnnt;

namespace {
rnntStatus_t dispatch(const void* acts, void* grads, const void* scale, const int* ranges, int S, const int* labels,
                      const int* label_lengths, const int* input_lengths, int A, int N, void* costs_dev, void* costs_host,
                      void* workspace, const rnntOptions& o, int dtype_code, int phases, bool want_grad) {
    switch (dtype_code) {
        case 0:
            return run_pruned<F32>(static_cast<const float*>(acts), static_cast<float*>(grads), static_cast<const float*>(scale),
                                   ranges, S, labels, label_lengths, input_lengths, A, N, static_cast<float*>(costs_dev),
                                   static_cast<float*>(costs_host), workspace, o, phases, want_grad);
        case 1:
            return run_pruned<F64>(static_cast<const double*>(acts), static_cast<double*>(grads), static_cast<const double*>(scale),
                                   ranges, S, labels, label_lengths, input_lengths, A, N, static_cast<double*>(costs_dev),
                                   static_cast<double*>(costs_host), workspace, o, phases, want_grad);
        case 2:
            return run_pruned<BF16>(static_cast<const uint16_t*>(acts), static_cast<uint16_t*>(grads),
                                    static_cast<const float*>(scale), ranges, S, labels, label_lengths, input_lengths, A, N,
                                    static_cast<float*>(costs_dev), static_cast<float*>(costs_host), workspace, o, phases,
                                    want_grad);
        case 3:
            return run_pruned<F16>(static_cast<const uint16_t*>(acts), static_cast<uint16_t*>(grads),
                                   static_cast<const float*>(scale), ranges, S, labels, label_lengths, input_lengths, A, N,
                                   static_cast<float*>(costs_dev), static_cast<float*>(costs_host), workspace, o, phases,
                                   want_grad);
        default: return RNNT_STATUS_INVALID_VALUE;
    }
}
}  // namespace

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
    if (bad_args(activations, flat_labels, label_lengths, input_lengths, costs, workspace, alphabet_size, minibatch,
                 options) || ranges == nullptr || loc_of(options) != RNNT_GPU)
        return RNNT_STATUS_INVALID_VALUE;
    const bool dev = is_device_pointer(costs);
    return dispatch(activations, gradients, nullptr, ranges, S, flat_labels, label_lengths, input_lengths, alphabet_size,
                    minibatch, dev ? costs : nullptr, dev ? nullptr : costs, workspace, options, dtype_code, 3,
                    gradients != nullptr);
}

rnntStatus_t compute_rnnt_loss_pruned_fwd(const void* activations, const int* ranges, int S, const int* flat_labels,
                                          const int* label_lengths, const int* input_lengths, int alphabet_size,
                                          int minibatch, void* costs_device, void* workspace, rnntOptions options,
                                          int dtype_code, int prepare_backward) {
    if (bad_args(activations, flat_labels, label_lengths, input_lengths, costs_device, workspace, alphabet_size, minibatch,
                 options) || ranges == nullptr || loc_of(options) != RNNT_GPU)
        return RNNT_STATUS_INVALID_VALUE;
    return dispatch(activations, nullptr, nullptr, ranges, S, flat_labels, label_lengths, input_lengths, alphabet_size,
                    minibatch, costs_device, nullptr, workspace, options, dtype_code, 1, prepare_backward != 0);
}

rnntStatus_t compute_rnnt_loss_pruned_bwd(const void* activations, void* gradients, const void* grad_scale_device, int S,
                                          int alphabet_size, int minibatch, void* workspace, rnntOptions options,
                                          int dtype_code) {
    if (activations == nullptr || gradients == nullptr || workspace == nullptr || alphabet_size <= 0 || minibatch <= 0 ||
        options.maxT <= 0 || options.maxU <= 0 || loc_of(options) != RNNT_GPU)
        return RNNT_STATUS_INVALID_VALUE;
    return dispatch(activations, gradients, grad_scale_device, nullptr, S, nullptr, nullptr, nullptr, alphabet_size,
                    minibatch, nullptr, nullptr, workspace, options, dtype_code, 2, true);
}

rnntStatus_t compute_rnnt_prune_ranges_add(const void* trans_acts, const void* pred_acts, const int* flat_labels,
                                           const int* label_lengths, const int* input_lengths, int alphabet_size,
                                           int minibatch, int S, int* ranges, void* workspace, rnntOptions options,
                                           int dtype_code) {
    if (bad_args(trans_acts, flat_labels, label_lengths, input_lengths, ranges, workspace, alphabet_size, minibatch,
                 options) || pred_acts == nullptr || loc_of(options) != RNNT_GPU)
        return RNNT_STATUS_INVALID_VALUE;
    switch (dtype_code) {
        case 0: return run_prune_ranges<F32>(static_cast<const float*>(trans_acts), static_cast<const float*>(pred_acts),
                                             flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, S, ranges,
                                             workspace, options);
        case 2: return run_prune_ranges<BF16>(static_cast<const uint16_t*>(trans_acts), static_cast<const uint16_t*>(pred_acts),
                                              flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, S, ranges,
                                              workspace, options);
        case 3: return run_prune_ranges<F16>(static_cast<const uint16_t*>(trans_acts), static_cast<const uint16_t*>(pred_acts),
                                             flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, S, ranges,
                                             workspace, options);
        default: return RNNT_STATUS_INVALID_VALUE;
    }
}

}  // extern "C"
#pragma GCC visibility pop
