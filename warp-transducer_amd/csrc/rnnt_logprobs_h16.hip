// rnnt_logprobs_h16.hip -- libwarprnnt_logprobs.so: the bf16 and fp16 instantiations (fp32 arithmetic), a code object of their own.
#define RNNT_LOGPROBS_INSTANTIATE_H16 1
#include "rnnt_logprobs_impl.h"

namespace rnnt {
template rnntStatus_t run_logprobs_fwd<BF16>(const LogprobsCall&);
template rnntStatus_t run_logprobs_bwd<BF16>(const LogprobsCall&);
template rnntStatus_t run_logprobs_fwd<F16>(const LogprobsCall&);
template rnntStatus_t run_logprobs_bwd<F16>(const LogprobsCall&);
}  // namespace rnnt
