// rnnt_ar_f64.hip -- the alignment-restricted loss for fp64 storage (fp64 lattice): run_ar<F64> and its kernels, a code
// object of its own (rnnt_ar_impl.h says why).
#define RNNT_AR_INSTANTIATE_F64 1
#include "rnnt_ar_impl.h"

namespace rnnt {
template rnntStatus_t run_ar<F64>(const SideCall&, const int*, const int*);
}  // namespace rnnt
