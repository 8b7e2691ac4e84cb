// rnnt_logprobs_f64.hip -- libwarprnnt_logprobs.so: the fp64 instantiation, a code object of its own.
#define RNNT_LOGPROBS_INSTANTIATE_F64 1
#include "rnnt_logprobs_impl.h"

namespace rnnt {
template rnntStatus_t run_logprobs_fwd<F64>(const LogprobsCall&);
template rnntStatus_t run_logprobs_bwd<F64>(const LogprobsCall&);
}  // namespace rnnt
