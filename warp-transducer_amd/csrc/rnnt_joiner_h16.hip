// rnnt_joiner_h16.hip -- libwarprnnt_joiner.so: the bf16 and fp16 instantiations (fp32 arithmetic), a code object of their own.
#define RNNT_JOINER_INSTANTIATE_H16 1
#include "rnnt_joiner_impl.h"

namespace rnnt {
template rnntStatus_t run_joiner_fwd<BF16>(const JoinerCall&);
template rnntStatus_t run_joiner_bwd<BF16>(const JoinerCall&);
template rnntStatus_t run_joiner_fwd<F16>(const JoinerCall&);
template rnntStatus_t run_joiner_bwd<F16>(const JoinerCall&);
}  // namespace rnnt
