// rnnt_logprobs.hip -- libwarprnnt_logprobs.so: the C entry points of include/rnnt_logprobs.h and the fp32 instantiation
// (run_logprobs_fwd<F32>, run_logprobs_bwd<F32>); rnnt_logprobs_impl.h has the driver and the launch rule,
// rnnt_logprobs_kernels.h the kernels.
#define RNNT_LOGPROBS_INSTANTIATE_F32 1
#include "rnnt_logprobs_impl.h"

namespace rnnt {
template rnntStatus_t run_logprobs_fwd<F32>(const LogprobsCall&);
template rnntStatus_t run_logprobs_bwd<F32>(const LogprobsCall&);
}  // namespace rnnt

using namespace rnnt;

// what both calls share; true: refused
static bool logprobs_bad_common(const void* logits, const int* symbols, const int* ranges, int K, int rnnt_type, int T, int U,
                                int C, int N, const rnntOptions& o, int dtype_code) {
    if (logits == nullptr || (symbols == nullptr && U > 1)) return true;
    if (dtype_code < 0 || dtype_code > 3 || rnnt_type < 0 || rnnt_type > 1) return true;
    if (T <= 0 || U <= 0 || C <= 0 || N <= 0 || loc_of(o) != RNNT_GPU) return true;
    if (K < 0 || K > U || (K > 0 && ranges == nullptr)) return true;
    if (o.blank_label < 0 || o.blank_label >= C) return true;
    const long long rows = static_cast<long long>(N) * T * (K > 0 ? K : U);
    return rows > 0x7fffffffLL;
}

// [p, p + n) and [q, q + m) share a byte
static bool logprobs_overlap(const void* p, unsigned long long n, const void* q, unsigned long long m) {
    if (p == nullptr || q == nullptr || n == 0 || m == 0) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + m && b < a + n;
}

static LpArgs logprobs_args(const int* symbols, const int* ranges, int K, const long long* boundary, int rnnt_type, int T, int U,
                            int C, int N, const rnntOptions& o) {
    return {symbols, K > 0 ? ranges : nullptr, boundary, K, K > 0 ? K : U, T, U, C, N, o.blank_label, rnnt_type};
}

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t compute_rnnt_logprobs_fwd(const void* logits, const int* symbols, const int* ranges, int K, const long long* boundary,
                                       int rnnt_type, int T, int U, int C, int minibatch, void* px, void* py, void* lse,
                                       rnntOptions options, int dtype_code) {
    if (logprobs_bad_common(logits, symbols, ranges, K, rnnt_type, T, U, C, minibatch, options, dtype_code) ||
        (px == nullptr && U > 1) || py == nullptr || lse == nullptr)
        return RNNT_STATUS_INVALID_VALUE;
    const unsigned long long lat = dtype_code == 1 ? 8 : 4, B = static_cast<unsigned long long>(minibatch);
    const unsigned long long nx = B * (U - 1) * (T + 1 - rnnt_type) * lat, ny = B * U * T * lat, nl = B * T * (K > 0 ? K : U) * lat;
    if (logprobs_overlap(px, nx, py, ny) || logprobs_overlap(px, nx, lse, nl) || logprobs_overlap(py, ny, lse, nl))
        return RNNT_STATUS_INVALID_VALUE;
    const LogprobsCall c = {logits, nullptr, nullptr, nullptr, nullptr, px, py, lse, nullptr,
                            logprobs_args(symbols, ranges, K, boundary, rnnt_type, T, U, C, minibatch, options),
                            reinterpret_cast<hipStream_t>(options.stream)};
    return side_dispatch(dtype_code, [&](auto tag) { return run_logprobs_fwd<decltype(tag)>(c); });
}

rnntStatus_t compute_rnnt_logprobs_bwd(const void* logits, const void* lse, const int* symbols, const int* ranges, int K,
                                       const long long* boundary, int rnnt_type, const void* px_grad, const void* py_grad,
                                       const void* lse_grad, int T, int U, int C, int minibatch, void* dlogits, rnntOptions options,
                                       int dtype_code) {
    if (logprobs_bad_common(logits, symbols, ranges, K, rnnt_type, T, U, C, minibatch, options, dtype_code) || lse == nullptr ||
        (px_grad == nullptr && U > 1) || py_grad == nullptr || dlogits == nullptr)
        return RNNT_STATUS_INVALID_VALUE;
    const unsigned long long lat = dtype_code == 1 ? 8 : 4, esz = dtype_code == 1 ? 8 : dtype_code == 0 ? 4 : 2;
    const unsigned long long B = static_cast<unsigned long long>(minibatch), Kp = K > 0 ? K : U;
    const unsigned long long nx = B * (U - 1) * (T + 1 - rnnt_type) * lat, ny = B * U * T * lat, nl = B * T * Kp * lat;
    const unsigned long long nz = B * T * Kp * C * esz;
    // dlogits may be logits exactly (the pass is elementwise given lse) and must not touch anything else the call reads
    if ((dlogits != logits && logprobs_overlap(dlogits, nz, logits, nz)) || logprobs_overlap(dlogits, nz, lse, nl) ||
        logprobs_overlap(dlogits, nz, px_grad, nx) || logprobs_overlap(dlogits, nz, py_grad, ny) ||
        logprobs_overlap(dlogits, nz, lse_grad, nl) || logprobs_overlap(dlogits, nz, symbols, B * (U - 1) * sizeof(int)) ||
        logprobs_overlap(dlogits, nz, ranges, K > 0 ? B * T * sizeof(int) : 0) ||
        logprobs_overlap(dlogits, nz, boundary, B * 4 * sizeof(long long)))
        return RNNT_STATUS_INVALID_VALUE;
    const LogprobsCall c = {logits, lse, px_grad, py_grad, lse_grad, nullptr, nullptr, nullptr, dlogits,
                            logprobs_args(symbols, ranges, K, boundary, rnnt_type, T, U, C, minibatch, options),
                            reinterpret_cast<hipStream_t>(options.stream)};
    return side_dispatch(dtype_code, [&](auto tag) { return run_logprobs_bwd<decltype(tag)>(c); });
}

}  // extern "C"
#pragma GCC visibility pop
