// rnnt_hat_h16.hip -- the HAT loss for bf16 and fp16 storage (fp32 lattice), a code object of its own (rnnt_hat_impl.h says
// why).
#define RNNT_HAT_INSTANTIATE_H16 1
#include "rnnt_hat_impl.h"

namespace rnnt {
template rnntStatus_t run_hat<BF16>(const SideCall&);
template rnntStatus_t run_hat<F16>(const SideCall&);
}  // namespace rnnt
