// rnnt_kd_f64.hip -- the lattice distillation loss for fp64 storage (fp64 arithmetic), a code object of its own
// (rnnt_kd_impl.h says why).
#define RNNT_KD_INSTANTIATE_F64 1
#include "rnnt_kd_impl.h"

namespace rnnt {
template rnntStatus_t run_kd<F64>(const SideCall&, const void*, int, float);
}  // namespace rnnt
