// test_kd_args.cpp -- the host driver of libwarprnnt_kd.so under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// program of its own (`make side-asan` builds the library's three translation units with the sanitizers on the host side
// and links them with this file; it needs no GPU): the workspace arithmetic of get_workspace_size_kd and the argument
// refusals of the three compute entries of include/rnnt_kd.h, all of which return before anything is launched.  Left
// out: what only a finished kernel can tell (device-side lengths that do not fit the tensor, non-finite logits).  The
// pointers handed over are never dereferenced on these paths.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/rnnt_kd.h"

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)
#define REFUSED(call) EXPECT((call) == RNNT_STATUS_INVALID_VALUE)

static rnntOptions opts(int T, int U, int blank, rnntComputeLocation loc = RNNT_GPU) {
    rnntOptions o{};
    o.loc = loc;
    o.blank_label = blank;
    o.maxT = T;
    o.maxU = U;
    o.batch_first = true;
    return o;
}

int main() {
    // sizes: one per dtype code; fp64 needs more than fp32, 16-bit storage what fp32 does; per row a record of four
    // values, a label word and a KL value, per sample a cost and a multiplier, per batch a word; no limit on maxU; 2^40 bytes
    size_t n = 0, n32 = 0, n64 = 0, n1 = 0;
    EXPECT(get_workspace_size_kd(150, 21, 128, 0, &n32) == RNNT_STATUS_SUCCESS && n32 > 0);
    EXPECT(get_workspace_size_kd(150, 21, 128, 1, &n64) == RNNT_STATUS_SUCCESS && n64 > n32);
    EXPECT(get_workspace_size_kd(150, 21, 128, 2, &n) == RNNT_STATUS_SUCCESS && n == n32);
    EXPECT(get_workspace_size_kd(150, 21, 128, 3, &n) == RNNT_STATUS_SUCCESS && n == n32);
    const size_t rows = size_t(128) * 150 * 21, per_sample = size_t(128) * 2 * sizeof(double) + sizeof(int);
    EXPECT(n32 >= rows * (4 * 4 + 4 + 4) + per_sample && n32 < rows * (4 * 4 + 4 + 4) + per_sample + 8 * 256);
    EXPECT(n64 >= rows * (4 * 8 + 4 + 8) + per_sample && n64 < rows * (4 * 8 + 4 + 8) + per_sample + 8 * 256);
    EXPECT(get_workspace_size_kd(151, 21, 128, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_kd(150, 22, 128, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_kd(150, 21, 129, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_kd(1, 1, 1, 0, &n1) == RNNT_STATUS_SUCCESS && n1 >= 4 * 6 + 2 * sizeof(double) + sizeof(int));
    EXPECT(get_workspace_size_kd(4, 5000, 2, 0, &n) == RNNT_STATUS_SUCCESS && n > 0);
    EXPECT(get_workspace_size_kd(1 << 15, 4096, 1 << 15, 1, &n) == RNNT_STATUS_SUCCESS && n > (size_t(1) << 40));
    REFUSED(get_workspace_size_kd(0, 3, 2, 0, &n));
    REFUSED(get_workspace_size_kd(4, 0, 2, 0, &n));
    REFUSED(get_workspace_size_kd(4, 3, 0, 0, &n));
    REFUSED(get_workspace_size_kd(4, 3, 2, -1, &n));
    REFUSED(get_workspace_size_kd(4, 3, 2, 4, &n));
    REFUSED(get_workspace_size_kd(4, 3, 2, 0, nullptr));

    constexpr int N = 2, T = 4, U = 3, A = 7;
    constexpr int E = N * T * U * A;
    std::vector<float> acts(2 * E + 8), teach(2 * E + 8), grads(2 * E + 8), costs(N), scale(N, 1.0f);   // (room for fp64)
    std::vector<int> labels(N * (U - 1)), lens(N, 1);
    EXPECT(get_workspace_size_kd(T, U, N, 1, &n) == RNNT_STATUS_SUCCESS);
    std::vector<char> ws(n);
    const rnntOptions ok = opts(T, U, 0);
    const float *a = acts.data(), *t = teach.data();
    float *g = grads.data(), *c = costs.data();
    const int *l = labels.data(), *ln = lens.data();
    char* w = ws.data();
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    // the one-call entry: NULL pointers (gradients may be NULL: costs only)
    REFUSED(compute_kd_loss(nullptr, t, g, l, ln, ln, A, N, c, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss(a, nullptr, g, l, ln, ln, A, N, c, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss(a, t, g, nullptr, ln, ln, A, N, c, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss(a, t, g, l, nullptr, ln, A, N, c, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss(a, t, g, l, ln, nullptr, A, N, c, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, N, nullptr, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, N, c, nullptr, ok, 0, 0, 1.0f));
    // the mode and the temperature
    for (int mode : {-1, 2, 7}) REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, N, c, w, ok, 0, mode, 1.0f));
    for (float tau : {0.0f, -1.0f, inf, -inf, nan}) {
        REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, N, c, w, ok, 0, 0, tau));
        REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, N, c, w, ok, 0, 1, tau));
        REFUSED(compute_kd_loss_fwd(a, t, l, ln, ln, A, N, c, w, ok, 0, 0, tau, 1));
        REFUSED(compute_kd_loss_bwd(a, t, g, scale.data(), A, N, w, ok, 0, 1, tau));
    }
    // sizes, the CPU location, dtype codes
    REFUSED(compute_kd_loss(a, t, g, l, ln, ln, 0, N, c, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, 0, c, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, N, c, w, opts(0, U, 0), 0, 0, 1.0f));
    REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, N, c, w, opts(T, 0, 0), 0, 0, 1.0f));
    REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, N, c, w, opts(T, U, 0, RNNT_CPU), 0, 0, 1.0f));
    for (int code : {-1, 4}) REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, N, c, w, ok, code, 0, 1.0f));
    for (int code = 0; code <= 3; ++code)
        for (int mode = 0; mode <= 1; ++mode) {
            // the limits: blank outside [0, A), a single column, A past 2^23, maxT maxU >= 2^31, 2^32 rows
            REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, N, c, w, opts(T, U, A), code, mode, 1.0f));
            REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, N, c, w, opts(T, U, -1), code, mode, 1.0f));
            REFUSED(compute_kd_loss(a, t, g, l, ln, ln, 1, N, c, w, ok, code, mode, 1.0f));
            REFUSED(compute_kd_loss(a, t, g, l, ln, ln, (1 << 23) + 1, N, c, w, ok, code, mode, 1.0f));
            REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, 1, c, w, opts(1 << 16, 1 << 15, 0), code, mode, 1.0f));
            REFUSED(compute_kd_loss(a, t, g, l, ln, ln, A, 1 << 16, c, w, opts(1 << 12, 16, 0), code, mode, 1.0f));
            // tensors off their element boundary
            REFUSED(compute_kd_loss(reinterpret_cast<const char*>(a) + 1, t, g, l, ln, ln, A, N, c, w, ok, code, mode, 1.0f));
            REFUSED(compute_kd_loss(a, reinterpret_cast<const char*>(t) + 1, g, l, ln, ln, A, N, c, w, ok, code, mode, 1.0f));
            REFUSED(compute_kd_loss(a, t, reinterpret_cast<char*>(g) + 1, l, ln, ln, A, N, c, w, ok, code, mode, 1.0f));
            // gradients that overlap the activations without being them; gradients on or over the teacher; a teacher that
            // overlaps the activations without being them
            REFUSED(compute_kd_loss(a, t, const_cast<float*>(a) + 4, l, ln, ln, A, N, c, w, ok, code, mode, 1.0f));
            REFUSED(compute_kd_loss(a, t, const_cast<float*>(t), l, ln, ln, A, N, c, w, ok, code, mode, 1.0f));
            REFUSED(compute_kd_loss(a, t, const_cast<float*>(t) + 4, l, ln, ln, A, N, c, w, ok, code, mode, 1.0f));
            REFUSED(compute_kd_loss(a, a, const_cast<float*>(a), l, ln, ln, A, N, c, w, ok, code, mode, 1.0f));
            REFUSED(compute_kd_loss(a, a + 4, g, l, ln, ln, A, N, c, w, ok, code, mode, 1.0f));
            REFUSED(compute_kd_loss_fwd(a, a + 4, l, ln, ln, A, N, c, w, ok, code, mode, 1.0f, 1));
            REFUSED(compute_kd_loss_bwd(a, t, const_cast<float*>(t), scale.data(), A, N, w, ok, code, mode, 1.0f));
            REFUSED(compute_kd_loss_bwd(a, t, const_cast<float*>(a) + 4, scale.data(), A, N, w, ok, code, mode, 1.0f));
        }
    // _fwd: the same refusals
    REFUSED(compute_kd_loss_fwd(nullptr, t, l, ln, ln, A, N, c, w, ok, 0, 0, 1.0f, 1));
    REFUSED(compute_kd_loss_fwd(a, nullptr, l, ln, ln, A, N, c, w, ok, 0, 0, 1.0f, 1));
    REFUSED(compute_kd_loss_fwd(a, t, nullptr, ln, ln, A, N, c, w, ok, 0, 0, 1.0f, 1));
    REFUSED(compute_kd_loss_fwd(a, t, l, nullptr, ln, A, N, c, w, ok, 0, 0, 1.0f, 1));
    REFUSED(compute_kd_loss_fwd(a, t, l, ln, nullptr, A, N, c, w, ok, 0, 0, 1.0f, 1));
    REFUSED(compute_kd_loss_fwd(a, t, l, ln, ln, A, N, nullptr, w, ok, 0, 0, 1.0f, 1));
    REFUSED(compute_kd_loss_fwd(a, t, l, ln, ln, A, N, c, nullptr, ok, 0, 0, 1.0f, 1));
    REFUSED(compute_kd_loss_fwd(a, t, l, ln, ln, A, N, c, w, opts(T, U, 0, RNNT_CPU), 0, 0, 1.0f, 1));
    REFUSED(compute_kd_loss_fwd(a, t, l, ln, ln, A, N, c, w, opts(T, U, A), 0, 0, 1.0f, 1));
    REFUSED(compute_kd_loss_fwd(a, t, l, ln, ln, A, N, c, w, ok, 0, 2, 1.0f, 0));
    for (int code : {-1, 4}) REFUSED(compute_kd_loss_fwd(a, t, l, ln, ln, A, N, c, w, ok, code, 0, 1.0f, 1));
    // _bwd
    REFUSED(compute_kd_loss_bwd(nullptr, t, g, scale.data(), A, N, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss_bwd(a, nullptr, g, scale.data(), A, N, w, ok, 0, 1, 1.0f));      // (full mode reads the teacher)
    REFUSED(compute_kd_loss_bwd(a, nullptr, const_cast<float*>(a) + 4, scale.data(), A, N, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss_bwd(a, t, nullptr, scale.data(), A, N, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss_bwd(a, t, g, scale.data(), A, N, nullptr, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss_bwd(a, t, g, scale.data(), 0, N, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss_bwd(a, t, g, scale.data(), A, 0, w, ok, 0, 0, 1.0f));
    REFUSED(compute_kd_loss_bwd(a, t, g, scale.data(), A, N, w, opts(T, U, 0, RNNT_CPU), 0, 0, 1.0f));
    REFUSED(compute_kd_loss_bwd(a, t, g, scale.data(), A, N, w, opts(T, U, A), 0, 0, 1.0f));
    REFUSED(compute_kd_loss_bwd(a, t, g, scale.data(), A, N, w, ok, 0, -1, 1.0f));
    for (int code : {-1, 4}) REFUSED(compute_kd_loss_bwd(a, t, g, scale.data(), A, N, w, ok, code, 0, 1.0f));
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("distillation loss argument checks: all refused as include/rnnt_kd.h says\n");
    return 0;
}
