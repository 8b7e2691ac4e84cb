// rnnt_bestpath_h16.hip -- libwarprnnt_bestpath.so: the bf16 and fp16 instantiations (exact upcasts, fp64 sweep), a code object of their own.
#define RNNT_BESTPATH_INSTANTIATE_H16 1
#include "rnnt_bestpath_impl.h"

namespace rnnt {
template rnntStatus_t run_bestpath<BF16>(const BestpathCall&);
template rnntStatus_t run_bestpath<F16>(const BestpathCall&);
}  // namespace rnnt
