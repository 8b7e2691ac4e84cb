// rnnt_pstream_h16.hip -- the pruned loss with lattice type and delay penalty for bf16 and fp16 storage (fp32 lattice), a
// code object of its own (rnnt_pstream_impl.h says why).
#define RNNT_PSTREAM_INSTANTIATE_H16 1
#include "rnnt_pstream_impl.h"

namespace rnnt {
template rnntStatus_t run_pstream<BF16>(const SideCall&, const int*, int, int, float);
template rnntStatus_t run_pstream<F16>(const SideCall&, const int*, int, int, float);
}  // namespace rnnt
