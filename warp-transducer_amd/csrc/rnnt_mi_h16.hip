// rnnt_mi_h16.hip -- the lattice primitive on px / py for bf16 and fp16 storage (fp32 lattice), a code object of its own
// (rnnt_mi_impl.h says why).
#define RNNT_MI_INSTANTIATE_H16 1
#include "rnnt_mi_impl.h"

namespace rnnt {
template rnntStatus_t run_mi<BF16>(const MiCall&);
template rnntStatus_t run_mi<F16>(const MiCall&);
}  // namespace rnnt
