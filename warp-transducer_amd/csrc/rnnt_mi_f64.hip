// rnnt_mi_f64.hip -- the lattice primitive on px / py for fp64 storage (fp64 lattice): run_mi<F64> and its kernels, a code
// object of its own (rnnt_mi_impl.h says why).
#define RNNT_MI_INSTANTIATE_F64 1
#include "rnnt_mi_impl.h"

namespace rnnt {
template rnntStatus_t run_mi<F64>(const MiCall&);
}  // namespace rnnt
