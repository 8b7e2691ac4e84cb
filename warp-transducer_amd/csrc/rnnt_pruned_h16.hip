// rnnt_pruned_h16.hip -- the pruned loss and the prune ranges for bf16 and fp16 storage (fp32 lattice), a code object of its
// own (rnnt_pruned_impl.h says why).
#define RNNT_PRUNED_INSTANTIATE_H16 1
#include "rnnt_pruned_impl.h"

namespace rnnt {
template rnntStatus_t run_pruned<BF16>(const SideCall&, const int*, int);
template rnntStatus_t run_pruned<F16>(const SideCall&, const int*, int);
template rnntStatus_t run_prune_ranges<BF16>(const SideCall&, const void*, int, int*);
template rnntStatus_t run_prune_ranges<F16>(const SideCall&, const void*, int, int*);
}  // namespace rnnt
