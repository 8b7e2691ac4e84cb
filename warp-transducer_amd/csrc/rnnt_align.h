// rnnt_align.h -- the host launcher of the best-path alignment (compute_rnnt_align*, include/rnnt.h) as the drivers see it.
// The kernels (rnnt_align_kernels.h) are instantiated in ONE translation unit, rnnt_joint.hip, for both lattice types: the
// code objects of the materialised path (rnnt_gpu*.hip) keep exactly the kernels their inventory lists
// (tests/kernel_forms.py), and an alignment loads the fp32 additive-joint code object on its first call.
#pragma once

#include <hip/hip_runtime.h>

#include "rnnt_kernels.h"

namespace rnnt {

template <typename L> struct AlignArgs {
    const LogPair<L>* lp2;          // the statistics stage's output (sample 0's array, as Plan::lp2) ...
    const L* logz;                  // ... and log Z (the poison hint is checked against it)
    L* beta;                        // sample 0's beta array: the decision bits go here
    double* best;                   // N doubles of workspace: base-2 best-path scores between the two kernels
    int* poison;
    const int *xlen, *ylen;
    int N, maxT, maxU, Up;
    double* score;                  // N (device)
    int* frames;                    // N x (maxU - 1) (device)
    hipStream_t stream;
};

template <typename L> bool launch_align(const AlignArgs<L>& args);
extern template bool launch_align<float>(const AlignArgs<float>&);
extern template bool launch_align<double>(const AlignArgs<double>&);

}  // namespace rnnt
