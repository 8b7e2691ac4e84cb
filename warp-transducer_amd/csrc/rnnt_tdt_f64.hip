// rnnt_tdt_f64.hip -- the TDT loss for fp64 storage (fp64 lattice): run_tdt<F64> and its kernels, a code object of its own
// (rnnt_tdt_impl.h says why).
#define RNNT_TDT_INSTANTIATE_F64 1
#include "rnnt_tdt_impl.h"

namespace rnnt {
template rnntStatus_t run_tdt<F64>(const SideCall&, const int*, int, float);
}  // namespace rnnt
