// rnnt_delay_h16.hip -- the delay-penalized loss for bf16 and fp16 storage (fp32 lattice), a code object of its own
// (rnnt_delay_impl.h says why).
#define RNNT_DELAY_INSTANTIATE_H16 1
#include "rnnt_delay_impl.h"

namespace rnnt {
template rnntStatus_t run_delay<BF16>(const SideCall&, float, void*);
template rnntStatus_t run_delay<F16>(const SideCall&, float, void*);
}  // namespace rnnt
