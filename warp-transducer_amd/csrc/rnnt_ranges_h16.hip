// rnnt_ranges_h16.hip -- libwarprnnt_ranges.so: the bf16 and fp16 instantiations (exact upcasts, fp64 sums), a code object of their own.
#define RNNT_RANGES_INSTANTIATE_H16 1
#include "rnnt_ranges_impl.h"

namespace rnnt {
template rnntStatus_t run_ranges<BF16>(const RangesCall&);
template rnntStatus_t run_ranges<F16>(const RangesCall&);
}  // namespace rnnt
