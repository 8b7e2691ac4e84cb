// rnnt_sample_f64.hip -- libwarprnnt_sample.so: the fp64 instantiation, a code object of its own.
#define RNNT_SAMPLE_INSTANTIATE_F64 1
#include "rnnt_sample_impl.h"

namespace rnnt {
template rnntStatus_t run_sample<F64>(const SampleCall&);
}  // namespace rnnt
