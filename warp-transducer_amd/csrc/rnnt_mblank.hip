// rnnt_mblank.hip -- libwarprnnt_mblank.so: the C entry points of include/rnnt_mblank.h and the fp32 instantiation
// (run_mblank<F32>); rnnt_mblank_impl.h has the driver, rnnt_mblank_kernels.h the kernels.
#define RNNT_MBLANK_INSTANTIATE_F32 1
#include "rnnt_mblank_impl.h"

namespace rnnt {
template rnntStatus_t run_mblank<F32>(const float*, float*, const float*, const int*, const int*, int, float, const int*,
                                      const int*, const int*, int, int, float*, float*, void*, const rnntOptions&, int,
                                      bool);
}  // namespace rnnt

using namespace rnnt;

namespace {
rnntStatus_t dispatch(const void* acts, void* grads, const void* scale, const int* columns, const int* durations, int K,
                      float sigma, const int* labels, const int* label_lengths, const int* input_lengths, int A, int N,
                      void* costs_dev, void* costs_host, void* workspace, const rnntOptions& o, int dtype_code, int phases,
                      bool want_grad) {
    switch (dtype_code) {
        case 0:
            return run_mblank<F32>(static_cast<const float*>(acts), static_cast<float*>(grads),
                                   static_cast<const float*>(scale), columns, durations, K, sigma, labels, label_lengths,
                                   input_lengths, A, N, static_cast<float*>(costs_dev), static_cast<float*>(costs_host),
                                   workspace, o, phases, want_grad);
        case 1:
            return run_mblank<F64>(static_cast<const double*>(acts), static_cast<double*>(grads),
                                   static_cast<const double*>(scale), columns, durations, K, sigma, labels, label_lengths,
                                   input_lengths, A, N, static_cast<double*>(costs_dev), static_cast<double*>(costs_host),
                                   workspace, o, phases, want_grad);
        case 2:
            return run_mblank<BF16>(static_cast<const uint16_t*>(acts), static_cast<uint16_t*>(grads),
                                    static_cast<const float*>(scale), columns, durations, K, sigma, labels, label_lengths,
                                    input_lengths, A, N, static_cast<float*>(costs_dev), static_cast<float*>(costs_host),
                                    workspace, o, phases, want_grad);
        case 3:
            return run_mblank<F16>(static_cast<const uint16_t*>(acts), static_cast<uint16_t*>(grads),
                                   static_cast<const float*>(scale), columns, durations, K, sigma, labels, label_lengths,
                                   input_lengths, A, N, static_cast<float*>(costs_dev), static_cast<float*>(costs_host),
                                   workspace, o, phases, want_grad);
        default: return RNNT_STATUS_INVALID_VALUE;
    }
}
}  // namespace

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t get_workspace_size_mblank(int maxT, int maxU, int minibatch, int num_big_blanks, int dtype_code,
                                       size_t* size_bytes) {
    if (minibatch <= 0 || maxT <= 0 || maxU <= 0 || size_bytes == nullptr || dtype_code < 0 || dtype_code > 3 ||
        num_big_blanks < 0 || num_big_blanks > kMbMaxBig)
        return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = mblank_layout(maxT, maxU, minibatch, num_big_blanks, dtype_code == 1 ? 8 : 4).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_mblank_loss(const void* activations, void* gradients, const int* big_blank_columns,
                                 const int* big_blank_durations, int num_big_blanks, float sigma, const int* flat_labels,
                                 const int* label_lengths, const int* input_lengths, int alphabet_size, int minibatch,
                                 void* costs, void* workspace, rnntOptions options, int dtype_code) {
    if (bad_args(activations, flat_labels, label_lengths, input_lengths, costs, workspace, alphabet_size, minibatch,
                 options) || loc_of(options) != RNNT_GPU || dtype_code < 0 || dtype_code > 3)
        return RNNT_STATUS_INVALID_VALUE;
    const bool dev = is_device_pointer(costs);
    return dispatch(activations, gradients, nullptr, big_blank_columns, big_blank_durations, num_big_blanks, sigma,
                    flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, dev ? costs : nullptr,
                    dev ? nullptr : costs, workspace, options, dtype_code, 3, gradients != nullptr);
}

rnntStatus_t compute_mblank_loss_fwd(const void* activations, const int* big_blank_columns, const int* big_blank_durations,
                                     int num_big_blanks, float sigma, const int* flat_labels, const int* label_lengths,
                                     const int* input_lengths, int alphabet_size, int minibatch, void* costs_device,
                                     void* workspace, rnntOptions options, int dtype_code, int prepare_backward) {
    if (bad_args(activations, flat_labels, label_lengths, input_lengths, costs_device, workspace, alphabet_size, minibatch,
                 options) || loc_of(options) != RNNT_GPU)
        return RNNT_STATUS_INVALID_VALUE;
    return dispatch(activations, nullptr, nullptr, big_blank_columns, big_blank_durations, num_big_blanks, sigma,
                    flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, costs_device, nullptr, workspace,
                    options, dtype_code, 1, prepare_backward != 0);
}

rnntStatus_t compute_mblank_loss_bwd(const void* activations, void* gradients, const void* grad_scale_device,
                                     const int* big_blank_columns, const int* big_blank_durations, int num_big_blanks,
                                     int alphabet_size, int minibatch, void* workspace, rnntOptions options,
                                     int dtype_code) {
    if (activations == nullptr || gradients == nullptr || workspace == nullptr || alphabet_size <= 0 || minibatch <= 0 ||
        options.maxT <= 0 || options.maxU <= 0 || loc_of(options) != RNNT_GPU)
        return RNNT_STATUS_INVALID_VALUE;
    return dispatch(activations, gradients, grad_scale_device, big_blank_columns, big_blank_durations, num_big_blanks, 0.0f,
                    nullptr, nullptr, nullptr, alphabet_size, minibatch, nullptr, nullptr, workspace, options, dtype_code, 2,
                    true);
}

}  // extern "C"
#pragma GCC visibility pop
