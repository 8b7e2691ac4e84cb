// rnnt_pstream_f64.hip -- the pruned loss with lattice type and delay penalty for fp64 storage (fp64 lattice):
// run_pstream<F64> and its kernels, a code object of its own (rnnt_pstream_impl.h says why).
#define RNNT_PSTREAM_INSTANTIATE_F64 1
#include "rnnt_pstream_impl.h"

namespace rnnt {
template rnntStatus_t run_pstream<F64>(const SideCall&, const int*, int, int, float);
}  // namespace rnnt
