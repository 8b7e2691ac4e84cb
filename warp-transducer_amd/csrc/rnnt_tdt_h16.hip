// rnnt_tdt_h16.hip -- the TDT loss for bf16 and fp16 storage (fp32 lattice), a code object of its own (rnnt_tdt_impl.h says
// why).
#define RNNT_TDT_INSTANTIATE_H16 1
#include "rnnt_tdt_impl.h"

namespace rnnt {
template rnntStatus_t run_tdt<BF16>(const SideCall&, const int*, int, float);
template rnntStatus_t run_tdt<F16>(const SideCall&, const int*, int, float);
}  // namespace rnnt
