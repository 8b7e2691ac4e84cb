// rnnt_ranges_f64.hip -- libwarprnnt_ranges.so: the fp64 instantiation, a code object of its own.
#define RNNT_RANGES_INSTANTIATE_F64 1
#include "rnnt_ranges_impl.h"

namespace rnnt {
template rnntStatus_t run_ranges<F64>(const RangesCall&);
}  // namespace rnnt
