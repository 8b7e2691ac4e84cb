// rnnt_joiner_f64.hip -- libwarprnnt_joiner.so: the fp64 instantiation, a code object of its own.
#define RNNT_JOINER_INSTANTIATE_F64 1
#include "rnnt_joiner_impl.h"

namespace rnnt {
template rnntStatus_t run_joiner_fwd<F64>(const JoinerCall&);
template rnntStatus_t run_joiner_bwd<F64>(const JoinerCall&);
}  // namespace rnnt
