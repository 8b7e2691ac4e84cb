// rnnt_pruned_f64.hip -- the pruned loss for fp64 storage (fp64 lattice): run_pruned<F64> and its kernels, a code object of
// its own (rnnt_pruned_impl.h says why).
#define RNNT_PRUNED_INSTANTIATE_F64 1
#include "rnnt_pruned_impl.h"

namespace rnnt {
template rnntStatus_t run_pruned<F64>(const SideCall&, const int*, int);
}  // namespace rnnt
