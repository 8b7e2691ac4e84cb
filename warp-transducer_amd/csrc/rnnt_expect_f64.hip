// rnnt_expect_f64.hip -- libwarprnnt_expect.so: the fp64 instantiation, a code object of its own.
#define RNNT_EXPECT_INSTANTIATE_F64 1
#include "rnnt_expect_impl.h"

namespace rnnt {
template rnntStatus_t run_expect<F64>(const ExpectCall&);
}  // namespace rnnt
