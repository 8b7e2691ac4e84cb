// rnnt_mblank_h16.hip -- the multi-blank loss for bf16 and fp16 storage (fp32 lattice), a code object of its own
// (rnnt_mblank_impl.h says why).
#define RNNT_MBLANK_INSTANTIATE_H16 1
#include "rnnt_mblank_impl.h"

namespace rnnt {
template rnntStatus_t run_mblank<BF16>(const SideCall&, const int*, const int*, int, float);
template rnntStatus_t run_mblank<F16>(const SideCall&, const int*, const int*, int, float);
}  // namespace rnnt
