// rnnt_pruned_h16.hip -- the pruned loss and the prune ranges for bf16 and fp16 storage (fp32 lattice), a code object of its
// own (rnnt_pruned_impl.h says why).
#define RNNT_PRUNED_INSTANTIATE_H16 1
#include "rnnt_pruned_impl.h"

namespace rnnt {
template rnntStatus_t run_pruned<BF16>(const uint16_t*, uint16_t*, const float*, const int*, int, const int*, const int*,
                                       const int*, int, int, float*, float*, void*, const rnntOptions&, int, bool);
template rnntStatus_t run_pruned<F16>(const uint16_t*, uint16_t*, const float*, const int*, int, const int*, const int*,
                                      const int*, int, int, float*, float*, void*, const rnntOptions&, int, bool);
template rnntStatus_t run_prune_ranges<BF16>(const uint16_t*, const uint16_t*, const int*, const int*, const int*, int, int,
                                             int, int*, void*, const rnntOptions&);
template rnntStatus_t run_prune_ranges<F16>(const uint16_t*, const uint16_t*, const int*, const int*, const int*, int, int,
                                            int, int*, void*, const rnntOptions&);
}  // namespace rnnt
