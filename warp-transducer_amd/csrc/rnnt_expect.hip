// rnnt_expect.hip -- libwarprnnt_expect.so: the C entry points of include/rnnt_expect.h and the fp32 instantiation
// (run_expect<F32>); rnnt_expect_impl.h has the driver and the launch rule, rnnt_expect_kernels.h the kernels.
#define RNNT_EXPECT_INSTANTIATE_F32 1
#include "rnnt_expect_impl.h"

namespace rnnt {
template rnntStatus_t run_expect<F32>(const ExpectCall&);
}  // namespace rnnt

using namespace rnnt;

namespace {

bool ex_bad_common(int S, int T, int N, const rnntOptions& o, int dtype_code) {
    return !ex_shape_ok(S, T, N) || dtype_code < 0 || dtype_code > 3 || loc_of(o) != RNNT_GPU;
}

// The sizes of a call's buffers in bytes.
struct ExSizes { unsigned long long esz, xb, yb, bd, sc, nd; };
ExSizes ex_sizes(int S, int T, int N, int modified, int dtype_code) {
    const unsigned long long esz = dtype_code == 1 ? 8 : dtype_code == 0 ? 4 : 2, B = static_cast<unsigned long long>(N);
    return {esz, B * S * (modified != 0 ? T : T + 1) * esz, B * (S + 1) * T * esz, B * 4 * sizeof(long long),
            B * sizeof(double), B * (S + 1) * (T + 1) * 2 * sizeof(double)};
}

// Both of a pair of gradients or neither (S == 0: the x one has no element, its pointer is not looked at).  true: refused.
bool ex_one_of_pair(int S, const void* gx, const void* gy) { return S > 0 && (gx == nullptr) != (gy == nullptr); }

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

rnntStatus_t compute_rnnt_expect(const void* px, const void* py, const void* cx, const void* cy, const void* boundary,
                                 int S, int T, int minibatch, int modified, void* scores, void* expect, void* nodes,
                                 void* px_grad, void* py_grad, void* cx_grad, void* cy_grad, rnntOptions options,
                                 int dtype_code) {
    if (ex_bad_common(S, T, minibatch, options, dtype_code) || py == nullptr || cy == nullptr || scores == nullptr ||
        expect == nullptr || nodes == nullptr || (S > 0 && (px == nullptr || cx == nullptr)))
        return RNNT_STATUS_INVALID_VALUE;
    if (ex_one_of_pair(S, px_grad, py_grad) || ex_one_of_pair(S, cx_grad, cy_grad) || (cy_grad != nullptr && py_grad == nullptr))
        return RNNT_STATUS_INVALID_VALUE;
    const ExSizes z = ex_sizes(S, T, minibatch, modified, dtype_code);
    const bool grads = py_grad != nullptr, cgrads = cy_grad != nullptr;
    const SideBuf in[] = {{px, z.xb, z.esz}, {py, z.yb, z.esz}, {cx, z.xb, z.esz}, {cy, z.yb, z.esz},
                          {boundary, z.bd, sizeof(long long)}};
    const SideBuf out[] = {{scores, z.sc, sizeof(double)}, {expect, z.sc, sizeof(double)}, {nodes, z.nd, 2 * sizeof(double)},
                           {grads ? px_grad : nullptr, z.xb, z.esz}, {grads ? py_grad : nullptr, z.yb, z.esz},
                           {cgrads ? cx_grad : nullptr, z.xb, z.esz}, {cgrads ? cy_grad : nullptr, z.yb, z.esz}};
    if (side_bad_buffers(in, 5, out, 7)) return RNNT_STATUS_INVALID_VALUE;
    const bool dev = is_device_pointer(scores);
    if (dev != is_device_pointer(expect)) return RNNT_STATUS_INVALID_VALUE;    // both scalars in one kind of memory
    const ExpectCall c = {px, py, cx, cy, boundary, dev ? scores : nullptr, dev ? expect : nullptr, dev ? nullptr : scores,
                          dev ? nullptr : expect, nodes, nullptr, nullptr, px_grad, py_grad, cgrads ? cx_grad : nullptr,
                          cgrads ? cy_grad : nullptr, S, T, minibatch, modified != 0,
                          reinterpret_cast<hipStream_t>(options.stream), grads ? 3 : 1};
    return side_dispatch(dtype_code, [&](auto tag) { return run_expect<decltype(tag)>(c); });
}

rnntStatus_t compute_rnnt_expect_fwd(const void* px, const void* py, const void* cx, const void* cy, const void* boundary,
                                     int S, int T, int minibatch, int modified, void* scores_device, void* expect_device,
                                     void* nodes, rnntOptions options, int dtype_code) {
    if (ex_bad_common(S, T, minibatch, options, dtype_code) || py == nullptr || cy == nullptr || scores_device == nullptr ||
        expect_device == nullptr || nodes == nullptr || (S > 0 && (px == nullptr || cx == nullptr)))
        return RNNT_STATUS_INVALID_VALUE;
    const ExSizes z = ex_sizes(S, T, minibatch, modified, dtype_code);
    const SideBuf in[] = {{px, z.xb, z.esz}, {py, z.yb, z.esz}, {cx, z.xb, z.esz}, {cy, z.yb, z.esz},
                          {boundary, z.bd, sizeof(long long)}};
    const SideBuf out[] = {{scores_device, z.sc, sizeof(double)}, {expect_device, z.sc, sizeof(double)},
                           {nodes, z.nd, 2 * sizeof(double)}};
    if (side_bad_buffers(in, 5, out, 3)) return RNNT_STATUS_INVALID_VALUE;
    const ExpectCall c = {px, py, cx, cy, boundary, scores_device, expect_device, nullptr, nullptr, nodes, nullptr, nullptr,
                          nullptr, nullptr, nullptr, nullptr, S, T, minibatch, modified != 0,
                          reinterpret_cast<hipStream_t>(options.stream), 1};
    return side_dispatch(dtype_code, [&](auto tag) { return run_expect<decltype(tag)>(c); });
}

rnntStatus_t compute_rnnt_expect_bwd(const void* px, const void* py, const void* cx, const void* cy, const void* boundary,
                                     const void* nodes, const void* scores_device, const void* expect_device,
                                     const void* g_expect_device, const void* g_score_device, int S, int T, int minibatch,
                                     int modified, void* px_grad, void* py_grad, void* cx_grad, void* cy_grad,
                                     rnntOptions options, int dtype_code) {
    if (ex_bad_common(S, T, minibatch, options, dtype_code) || py == nullptr || cy == nullptr || nodes == nullptr ||
        scores_device == nullptr || expect_device == nullptr || py_grad == nullptr ||
        (S > 0 && (px == nullptr || cx == nullptr || px_grad == nullptr)))
        return RNNT_STATUS_INVALID_VALUE;
    if (ex_one_of_pair(S, cx_grad, cy_grad)) return RNNT_STATUS_INVALID_VALUE;
    const ExSizes z = ex_sizes(S, T, minibatch, modified, dtype_code);
    const bool cgrads = cy_grad != nullptr;
    const SideBuf in[] = {{px, z.xb, z.esz}, {py, z.yb, z.esz}, {cx, z.xb, z.esz}, {cy, z.yb, z.esz},
                          {boundary, z.bd, sizeof(long long)}, {nodes, z.nd, 2 * sizeof(double)},
                          {scores_device, z.sc, sizeof(double)}, {expect_device, z.sc, sizeof(double)},
                          {g_expect_device, z.sc, sizeof(double)}, {g_score_device, z.sc, sizeof(double)}};
    const SideBuf out[] = {{px_grad, z.xb, z.esz}, {py_grad, z.yb, z.esz}, {cgrads ? cx_grad : nullptr, z.xb, z.esz},
                           {cgrads ? cy_grad : nullptr, z.yb, z.esz}};
    if (side_bad_buffers(in, 10, out, 4)) return RNNT_STATUS_INVALID_VALUE;
    const ExpectCall c = {px, py, cx, cy, boundary, const_cast<void*>(scores_device), const_cast<void*>(expect_device), nullptr,
                          nullptr, const_cast<void*>(nodes), g_expect_device, g_score_device, px_grad, py_grad,
                          cgrads ? cx_grad : nullptr, cgrads ? cy_grad : nullptr, S, T, minibatch, modified != 0,
                          reinterpret_cast<hipStream_t>(options.stream), 2};
    return side_dispatch(dtype_code, [&](auto tag) { return run_expect<decltype(tag)>(c); });
}

}  // extern "C"
#pragma GCC visibility pop
