// rnnt_ar_h16.hip -- the alignment-restricted loss for bf16 and fp16 storage (fp32 lattice), a code object of its own
// (rnnt_ar_impl.h says why).
#define RNNT_AR_INSTANTIATE_H16 1
#include "rnnt_ar_impl.h"

namespace rnnt {
template rnntStatus_t run_ar<BF16>(const SideCall&, const int*, const int*);
template rnntStatus_t run_ar<F16>(const SideCall&, const int*, const int*);
}  // namespace rnnt
