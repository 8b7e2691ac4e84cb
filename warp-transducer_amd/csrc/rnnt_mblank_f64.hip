// rnnt_mblank_f64.hip -- the multi-blank loss for fp64 storage (fp64 lattice): run_mblank<F64> and its kernels, a code
// object of its own (rnnt_mblank_impl.h says why).
#define RNNT_MBLANK_INSTANTIATE_F64 1
#include "rnnt_mblank_impl.h"

namespace rnnt {
template rnntStatus_t run_mblank<F64>(const SideCall&, const int*, const int*, int, float);
}  // namespace rnnt
