// rnnt_joiner.hip -- libwarprnnt_joiner.so: the C entry points of include/rnnt_joiner.h and the fp32 instantiation
// (run_joiner_fwd<F32>, run_joiner_bwd<F32>); rnnt_joiner_impl.h has the driver and the launch rule, rnnt_joiner_kernels.h
// the kernels.
#define RNNT_JOINER_INSTANTIATE_F32 1
#include "rnnt_joiner_impl.h"

namespace rnnt {
template rnntStatus_t run_joiner_fwd<F32>(const JoinerCall&);
template rnntStatus_t run_joiner_bwd<F32>(const JoinerCall&);
}  // namespace rnnt

using namespace rnnt;

// what both calls share; true: refused
static bool joiner_bad_common(int layout, int act, const int* ranges, int S, const long long* offsets, const int* label_lengths,
                              const int* input_lengths, int T, int U, int H, int N, const void* workspace,
                              const rnntOptions& o, int dtype_code) {
    if (layout < 0 || layout > 2 || act < 0 || act > 2 || dtype_code < 0 || dtype_code > 3) return true;
    if (T <= 0 || U <= 0 || H <= 0 || N <= 0 || workspace == nullptr || loc_of(o) != RNNT_GPU) return true;
    if (layout == 2 && (ranges == nullptr || S < 1 || S > U)) return true;
    if (layout == 1 && (offsets == nullptr || label_lengths == nullptr || input_lengths == nullptr)) return true;
    const long long rows = static_cast<long long>(N) * T * (layout == 2 ? S : U);
    return rows > 0x7fffffffLL;
}

// [p, p + n) and [q, q + m) share a byte
static bool joiner_overlap(const void* p, unsigned long long n, const void* q, unsigned long long m) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + m && b < a + n;
}

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t get_workspace_size_joiner(int T, int U, int S, int H, int minibatch, int layout, int dtype_code, size_t* bytes) {
    if (T <= 0 || U <= 0 || H <= 0 || minibatch <= 0 || layout < 0 || layout > 2 || dtype_code < 0 || dtype_code > 3 ||
        bytes == nullptr || (layout == 2 && (S < 1 || S > U)))
        return RNNT_STATUS_INVALID_VALUE;
    *bytes = jn_layout(T, U, H, minibatch, dtype_code == 1 ? 8 : 4).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_joiner_fwd(const void* f, const void* g, void* out, int layout, int act, const int* ranges, int S,
                                     const long long* offsets, const int* label_lengths, const int* input_lengths, int T, int U,
                                     int H, int minibatch, void* workspace, rnntOptions options, int dtype_code) {
    if (f == nullptr || g == nullptr || out == nullptr ||
        joiner_bad_common(layout, act, ranges, S, offsets, label_lengths, input_lengths, T, U, H, minibatch, workspace, options,
                          dtype_code))
        return RNNT_STATUS_INVALID_VALUE;
    const JoinerCall c = {f, g, out, nullptr, nullptr, nullptr, ranges, offsets, label_lengths, input_lengths, layout, act, S, T, U,
                          H, minibatch, workspace, reinterpret_cast<hipStream_t>(options.stream)};
    return side_dispatch(dtype_code, [&](auto tag) { return run_joiner_fwd<decltype(tag)>(c); });
}

rnntStatus_t compute_rnnt_joiner_bwd(const void* out, const void* dout, void* df, void* dg, int layout, int act,
                                     const int* ranges, int S, const long long* offsets, const int* label_lengths,
                                     const int* input_lengths, int T, int U, int H, int minibatch, void* workspace,
                                     rnntOptions options, int dtype_code) {
    if (dout == nullptr || df == nullptr || dg == nullptr ||
        joiner_bad_common(layout, act, ranges, S, offsets, label_lengths, input_lengths, T, U, H, minibatch, workspace, options,
                          dtype_code) ||
        (act != 0 && out == nullptr))
        return RNNT_STATUS_INVALID_VALUE;
    // dout holds N T J rows; in the packed layout the host does not know how many (offsets[N] is on the device): at least one
    const unsigned long long esz = dtype_code == 1 ? 8 : dtype_code == 0 ? 4 : 2;
    const unsigned long long rows = layout == 1 ? 1 : static_cast<unsigned long long>(minibatch) * T * (layout == 2 ? S : U);
    const unsigned long long nd = rows * H * esz, nf = static_cast<unsigned long long>(minibatch) * T * H * esz,
                             ng = static_cast<unsigned long long>(minibatch) * U * H * esz;
    if (joiner_overlap(dout, nd, df, nf) || joiner_overlap(dout, nd, dg, ng) || joiner_overlap(df, nf, dg, ng))
        return RNNT_STATUS_INVALID_VALUE;
    const JoinerCall c = {nullptr, nullptr, out, dout, df, dg, ranges, offsets, label_lengths, input_lengths, layout, act, S, T, U,
                          H, minibatch, workspace, reinterpret_cast<hipStream_t>(options.stream)};
    return side_dispatch(dtype_code, [&](auto tag) { return run_joiner_bwd<decltype(tag)>(c); });
}

}  // extern "C"
#pragma GCC visibility pop
