// rnnt_tdt_align_f64.hip -- the TDT alignment for fp64 storage (fp64 lattice), a code object of its own
// (rnnt_tdt_align_impl.h says why).
#define RNNT_TDT_ALIGN_INSTANTIATE_F64 1
#include "rnnt_tdt_align_impl.h"

namespace rnnt {
template rnntStatus_t run_tdt_align<F64>(const TdtAlignCall&, const int*, int, float);
}  // namespace rnnt
