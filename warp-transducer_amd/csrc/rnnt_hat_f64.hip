// rnnt_hat_f64.hip -- the HAT loss for fp64 storage (fp64 lattice): run_hat<F64> and its kernels, a code object of its own
// (rnnt_hat_impl.h says why).
#define RNNT_HAT_INSTANTIATE_F64 1
#include "rnnt_hat_impl.h"

namespace rnnt {
template rnntStatus_t run_hat<F64>(const SideCall&);
}  // namespace rnnt
