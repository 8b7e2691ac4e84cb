// rnnt_kd_h16.hip -- the lattice distillation loss for bf16 and fp16 storage (fp32 arithmetic), a code object of its own
// (rnnt_kd_impl.h says why).
#define RNNT_KD_INSTANTIATE_H16 1
#include "rnnt_kd_impl.h"

namespace rnnt {
template rnntStatus_t run_kd<BF16>(const SideCall&, const void*, int, float);
template rnntStatus_t run_kd<F16>(const SideCall&, const void*, int, float);
}  // namespace rnnt
