// rnnt_mono_f64.hip -- the monotonic loss for fp64 storage (fp64 lattice): run_mono<F64> and its kernels, a code object
// of its own (rnnt_mono_impl.h says why).
#define RNNT_MONO_INSTANTIATE_F64 1
#include "rnnt_mono_impl.h"

namespace rnnt {
template rnntStatus_t run_mono<F64>(const SideCall&);
}  // namespace rnnt
