// rnnt_tdt_align_h16.hip -- the TDT alignment for bf16 and fp16 storage (fp32 lattice), a code object of its own
// (rnnt_tdt_align_impl.h says why).
#define RNNT_TDT_ALIGN_INSTANTIATE_H16 1
#include "rnnt_tdt_align_impl.h"

namespace rnnt {
template rnntStatus_t run_tdt_align<BF16>(const TdtAlignCall&, const int*, int, float);
template rnntStatus_t run_tdt_align<F16>(const TdtAlignCall&, const int*, int, float);
}  // namespace rnnt
