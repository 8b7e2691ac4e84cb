// rnnt_sample.hip -- libwarprnnt_sample.so: the C entry points of include/rnnt_sample.h and the fp32 instantiation
// (run_sample<F32>); rnnt_sample_impl.h has the driver and the launch rule, rnnt_sample_kernels.h the kernels.
#define RNNT_SAMPLE_INSTANTIATE_F32 1
#include "rnnt_sample_impl.h"

namespace rnnt {
template rnntStatus_t run_sample<F32>(const SampleCall&);
}  // namespace rnnt

using namespace rnnt;

namespace {

bool sa_bad_common(int S, int T, int N, int K, const rnntOptions& o, int dtype_code) {
    return !sa_shape_ok(S, T, N, K) || dtype_code < 0 || dtype_code > 3 || loc_of(o) != RNNT_GPU;
}

// The sizes of a call's buffers in bytes: px, py, boundary, scores, alpha, uniforms, frames, weights / coeff.
struct SaSizes { unsigned long long esz, xb, yb, bd, sc, al, un, fr, wk; };
SaSizes sa_sizes(int S, int T, int N, int K, int modified, int dtype_code) {
    const unsigned long long esz = dtype_code == 1 ? 8 : dtype_code == 0 ? 4 : 2, B = static_cast<unsigned long long>(N);
    return {esz, B * S * (modified != 0 ? T : T + 1) * esz, B * (S + 1) * T * esz, B * 4 * sizeof(long long),
            B * sizeof(double), B * (S + 1) * (T + 1) * sizeof(double), B * K * (S + T) * sizeof(float),
            B * K * S * sizeof(int), B * K * sizeof(double)};
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t compute_rnnt_sample(const void* px, const void* py, const void* boundary, const float* uniforms, int S, int T,
                                 int minibatch, int K, int modified, void* scores, void* alpha, int* frames, void* weights,
                                 rnntOptions options, int dtype_code) {
    if (sa_bad_common(S, T, minibatch, K, options, dtype_code) || py == nullptr || scores == nullptr || alpha == nullptr ||
        weights == nullptr || (S > 0 && (px == nullptr || uniforms == nullptr || frames == nullptr)))
        return RNNT_STATUS_INVALID_VALUE;
    const SaSizes z = sa_sizes(S, T, minibatch, K, modified, dtype_code);
    const bool sym = S > 0;
    const SideBuf in[] = {{sym ? px : nullptr, z.xb, z.esz}, {py, z.yb, z.esz}, {boundary, z.bd, sizeof(long long)},
                          {sym ? uniforms : nullptr, z.un, sizeof(float)}};
    const SideBuf out[] = {{scores, z.sc, sizeof(double)}, {alpha, z.al, sizeof(double)},
                           {sym ? frames : nullptr, z.fr, sizeof(int)}, {weights, z.wk, sizeof(double)}};
    if (side_bad_buffers(in, 4, out, 4)) return RNNT_STATUS_INVALID_VALUE;
    const SampleCall c = {px, py, boundary, uniforms, nullptr, scores, alpha, frames, weights, nullptr, nullptr, S, T,
                          minibatch, K, modified != 0, reinterpret_cast<hipStream_t>(options.stream), 3};
    return side_dispatch(dtype_code, [&](auto tag) { return run_sample<decltype(tag)>(c); });
}

rnntStatus_t compute_rnnt_sample_walk(const void* px, const void* py, const void* boundary, const void* alpha,
                                      const void* scores_device, const float* uniforms, int S, int T, int minibatch, int K,
                                      int modified, int* frames, void* weights, rnntOptions options, int dtype_code) {
    if (sa_bad_common(S, T, minibatch, K, options, dtype_code) || py == nullptr || scores_device == nullptr ||
        alpha == nullptr || weights == nullptr || (S > 0 && (px == nullptr || uniforms == nullptr || frames == nullptr)))
        return RNNT_STATUS_INVALID_VALUE;
    const SaSizes z = sa_sizes(S, T, minibatch, K, modified, dtype_code);
    const bool sym = S > 0;
    const SideBuf in[] = {{sym ? px : nullptr, z.xb, z.esz}, {py, z.yb, z.esz}, {boundary, z.bd, sizeof(long long)},
                          {sym ? uniforms : nullptr, z.un, sizeof(float)}, {alpha, z.al, sizeof(double)},
                          {scores_device, z.sc, sizeof(double)}};
    const SideBuf out[] = {{sym ? frames : nullptr, z.fr, sizeof(int)}, {weights, z.wk, sizeof(double)}};
    if (side_bad_buffers(in, 6, out, 2)) return RNNT_STATUS_INVALID_VALUE;
    const SampleCall c = {px, py, boundary, uniforms, nullptr, const_cast<void*>(scores_device), const_cast<void*>(alpha),
                          frames, weights, nullptr, nullptr, S, T, minibatch, K, modified != 0,
                          reinterpret_cast<hipStream_t>(options.stream), 2};
    return side_dispatch(dtype_code, [&](auto tag) { return run_sample<decltype(tag)>(c); });
}

rnntStatus_t compute_rnnt_path_weights(const void* px, const void* py, const void* boundary, const int* frames, int S, int T,
                                       int minibatch, int K, int modified, void* weights, rnntOptions options,
                                       int dtype_code) {
    if (sa_bad_common(S, T, minibatch, K, options, dtype_code) || py == nullptr || weights == nullptr ||
        (S > 0 && (px == nullptr || frames == nullptr)))
        return RNNT_STATUS_INVALID_VALUE;
    const SaSizes z = sa_sizes(S, T, minibatch, K, modified, dtype_code);
    const bool sym = S > 0;
    const SideBuf in[] = {{sym ? px : nullptr, z.xb, z.esz}, {py, z.yb, z.esz}, {boundary, z.bd, sizeof(long long)},
                          {sym ? frames : nullptr, z.fr, sizeof(int)}};
    const SideBuf out[] = {{weights, z.wk, sizeof(double)}};
    if (side_bad_buffers(in, 4, out, 1)) return RNNT_STATUS_INVALID_VALUE;
    const SampleCall c = {px, py, boundary, nullptr, nullptr, nullptr, nullptr, const_cast<int*>(frames), weights, nullptr,
                          nullptr, S, T, minibatch, K, modified != 0, reinterpret_cast<hipStream_t>(options.stream), 4};
    return side_dispatch(dtype_code, [&](auto tag) { return run_sample<decltype(tag)>(c); });
}

rnntStatus_t compute_rnnt_path_edges(const int* frames, const void* coeff, const void* boundary, int S, int T, int minibatch,
                                     int K, int modified, void* px_acc, void* py_acc, rnntOptions options, int dtype_code) {
    if (sa_bad_common(S, T, minibatch, K, options, dtype_code) || py_acc == nullptr ||
        (S > 0 && (px_acc == nullptr || frames == nullptr)))
        return RNNT_STATUS_INVALID_VALUE;
    const SaSizes z = sa_sizes(S, T, minibatch, K, modified, dtype_code);
    const bool sym = S > 0;
    const SideBuf in[] = {{sym ? frames : nullptr, z.fr, sizeof(int)}, {coeff, z.wk, sizeof(double)},
                          {boundary, z.bd, sizeof(long long)}};
    const SideBuf out[] = {{sym ? px_acc : nullptr, z.xb, z.esz}, {py_acc, z.yb, z.esz}};
    if (side_bad_buffers(in, 3, out, 2)) return RNNT_STATUS_INVALID_VALUE;
    const SampleCall c = {nullptr, nullptr, boundary, nullptr, coeff, nullptr, nullptr, const_cast<int*>(frames), nullptr,
                          px_acc, py_acc, S, T, minibatch, K, modified != 0, reinterpret_cast<hipStream_t>(options.stream), 8};
    return side_dispatch(dtype_code, [&](auto tag) { return run_sample<decltype(tag)>(c); });
}

}  // extern "C"
#pragma GCC visibility pop
