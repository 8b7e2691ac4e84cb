// rnnt_bestpath_f64.hip -- libwarprnnt_bestpath.so: the fp64 instantiation, a code object of its own.
#define RNNT_BESTPATH_INSTANTIATE_F64 1
#include "rnnt_bestpath_impl.h"

namespace rnnt {
template rnntStatus_t run_bestpath<F64>(const BestpathCall&);
}  // namespace rnnt
