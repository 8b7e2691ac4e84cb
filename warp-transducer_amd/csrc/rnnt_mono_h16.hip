// rnnt_mono_h16.hip -- the monotonic loss for bf16 and fp16 storage (fp32 lattice), a code object of its own
// (rnnt_mono_impl.h says why).
#define RNNT_MONO_INSTANTIATE_H16 1
#include "rnnt_mono_impl.h"

namespace rnnt {
template rnntStatus_t run_mono<BF16>(const SideCall&);
template rnntStatus_t run_mono<F16>(const SideCall&);
}  // namespace rnnt
