// rnnt_expect_h16.hip -- libwarprnnt_expect.so: the bf16 and fp16 instantiations (exact upcasts, fp64 sweeps), a code object of their own.
#define RNNT_EXPECT_INSTANTIATE_H16 1
#include "rnnt_expect_impl.h"

namespace rnnt {
template rnntStatus_t run_expect<BF16>(const ExpectCall&);
template rnntStatus_t run_expect<F16>(const ExpectCall&);
}  // namespace rnnt
