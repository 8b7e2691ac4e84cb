// rnnt_delay_f64.hip -- the delay-penalized loss for fp64 storage (fp64 lattice): run_delay<F64> and its kernels, a code
// object of its own (rnnt_delay_impl.h says why).
#define RNNT_DELAY_INSTANTIATE_F64 1
#include "rnnt_delay_impl.h"

namespace rnnt {
template rnntStatus_t run_delay<F64>(const SideCall&, float, void*);
}  // namespace rnnt
