// rnnt_tdt_align.hip -- libwarprnnt_tdt_align.so: the C entry points of include/rnnt_tdt_align.h and the fp32 instantiation
// (run_tdt_align<F32>); rnnt_tdt_align_impl.h has the driver, rnnt_tdt_align_kernels.h the kernels.
#define RNNT_TDT_ALIGN_INSTANTIATE_F32 1
#include "rnnt_tdt_align_impl.h"

namespace rnnt {
template rnntStatus_t run_tdt_align<F32>(const TdtAlignCall&, const int*, int, float);
}  // namespace rnnt

using namespace rnnt;

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t get_workspace_size_tdt_align(int maxT, int maxU, int minibatch, int num_durations, int dtype_code,
                                          size_t* size_bytes) {
    if (minibatch <= 0 || maxT <= 0 || maxU <= 0 || size_bytes == nullptr || dtype_code < 0 || dtype_code > 3 ||
        num_durations < 1 || num_durations > kTdtMaxDurations)
        return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = tdt_layout(maxT, maxU, minibatch, num_durations, dtype_code == 1 ? 8 : 4).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_tdt_align(const void* activations, const int* durations, int num_durations, float sigma,
                               const int* flat_labels, const int* label_lengths, const int* input_lengths,
                               int alphabet_size, int minibatch, void* score_device, void* frames_device,
                               void* durs_device, void* workspace, rnntOptions options, int dtype_code) {
    if (bad_args(activations, flat_labels, label_lengths, input_lengths, score_device, workspace, alphabet_size, minibatch,
                 options) ||
        frames_device == nullptr || durs_device == nullptr || loc_of(options) != RNNT_GPU)
        return RNNT_STATUS_INVALID_VALUE;
    const TdtAlignCall c = {activations, flat_labels, label_lengths, input_lengths, static_cast<double*>(score_device),
                            static_cast<int*>(frames_device), static_cast<int*>(durs_device), workspace, alphabet_size,
                            minibatch, options};
    return side_dispatch(dtype_code,
                         [&](auto tag) { return run_tdt_align<decltype(tag)>(c, durations, num_durations, sigma); });
}

}  // extern "C"
#pragma GCC visibility pop
