// rnnt_sample_h16.hip -- libwarprnnt_sample.so: the bf16 and fp16 instantiations (exact upcasts, fp64 sweep and walks), a code object of their own.
#define RNNT_SAMPLE_INSTANTIATE_H16 1
#include "rnnt_sample_impl.h"

namespace rnnt {
template rnntStatus_t run_sample<BF16>(const SampleCall&);
template rnntStatus_t run_sample<F16>(const SampleCall&);
}  // namespace rnnt
