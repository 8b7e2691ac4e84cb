// test_ar_args.cpp -- the host driver of libwarprnnt_ar.so under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// program of its own (`make side-asan` builds the library's three translation units with the sanitizers on the host side
// and links them with this file; it needs no GPU): the workspace arithmetic of get_workspace_size_ar and the argument
// refusals of the three compute entries of include/rnnt_ar.h, all of which return before anything is launched.  Left
// out: what only a finished kernel can tell (device-side lengths that do not fit the tensor, windows without a path).  The
// pointers handed over are never dereferenced on these paths.
#include <cstdio>
#include <vector>

#include "../../include/rnnt_ar.h"

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
    // sizes: one per dtype code; the fp64 lattice needs more than the fp32 one, 16-bit storage the fp32 lattice's; the
    // arrays the layout must hold (four-word records, alpha, beta, maxT + maxU offsets per sample and direction, the two
    // bound arrays of maxU words per sample); 2^40 bytes
    size_t n = 0, n32 = 0, n64 = 0, n1 = 0;
    EXPECT(get_workspace_size_ar(150, 21, 128, 0, &n32) == RNNT_STATUS_SUCCESS && n32 > 0);
    EXPECT(get_workspace_size_ar(150, 21, 128, 1, &n64) == RNNT_STATUS_SUCCESS && n64 > n32);
    EXPECT(get_workspace_size_ar(150, 21, 128, 2, &n) == RNNT_STATUS_SUCCESS && n == n32);
    EXPECT(get_workspace_size_ar(150, 21, 128, 3, &n) == RNNT_STATUS_SUCCESS && n == n32);
    const size_t cells = size_t(128) * 150 * 21, offs = size_t(128) * (150 + 21) * 2 * sizeof(double) + size_t(128) * 21 * 2 * sizeof(int);
    EXPECT(n32 >= cells * 4 * (4 + 1 + 1) + offs && n32 < cells * 4 * (4 + 1 + 1) + offs + 128 * 64 + 20 * 256);
    EXPECT(n64 >= cells * 8 * (4 + 1 + 1) + offs);
    EXPECT(get_workspace_size_ar(151, 21, 128, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_ar(150, 22, 128, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_ar(150, 21, 129, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_ar(1, 1, 1, 0, &n1) == RNNT_STATUS_SUCCESS && n1 >= 4 * 6 + 2 * 2 * sizeof(double) + 3 * sizeof(int));
    EXPECT(get_workspace_size_ar(1 << 15, 4096, 1 << 15, 1, &n) == RNNT_STATUS_SUCCESS && n > (size_t(1) << 40));
    REFUSED(get_workspace_size_ar(0, 3, 2, 0, &n));
    REFUSED(get_workspace_size_ar(4, 0, 2, 0, &n));
    REFUSED(get_workspace_size_ar(4, 3, 0, 0, &n));
    REFUSED(get_workspace_size_ar(4, 3, 2, -1, &n));
    REFUSED(get_workspace_size_ar(4, 3, 2, 4, &n));
    REFUSED(get_workspace_size_ar(4, 3, 2, 0, nullptr));

    constexpr int N = 2, T = 4, U = 3, A = 7;
    std::vector<float> acts(N * T * U * A + 8), grads(N * T * U * A + 8), costs(N), scale(N, 1.0f);
    std::vector<int> labels(N * (U - 1)), lens(N, 1), wlo(N * (U - 1), 0), whi(N * (U - 1), T - 1);
    EXPECT(get_workspace_size_ar(T, U, N, 1, &n) == RNNT_STATUS_SUCCESS);
    std::vector<char> ws(n);
    const rnntOptions ok = opts(T, U, 0);
    const float* a = acts.data();
    float *g = grads.data(), *c = costs.data();
    const int *l = labels.data(), *ln = lens.data(), *lo = wlo.data(), *hi = whi.data();
    char* w = ws.data();
    // the one-call entry: NULL pointers (gradients may be NULL: score only)
    REFUSED(compute_rnnt_loss_ar(nullptr, g, l, ln, ln, lo, hi, A, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar(a, g, nullptr, ln, ln, lo, hi, A, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar(a, g, l, nullptr, ln, lo, hi, A, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar(a, g, l, ln, nullptr, lo, hi, A, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, A, N, nullptr, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, A, N, c, nullptr, ok, 0));
    // NULL windows
    REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, nullptr, hi, A, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, nullptr, A, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar_fwd(a, l, ln, ln, nullptr, hi, A, N, c, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_ar_fwd(a, l, ln, ln, lo, nullptr, A, N, c, w, ok, 0, 0));
    // sizes, the CPU location, dtype codes
    REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, 0, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, A, 0, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, A, N, c, w, opts(0, U, 0), 0));
    REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, A, N, c, w, opts(T, 0, 0), 0));
    REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, A, N, c, w, opts(T, U, 0, RNNT_CPU), 0));
    for (int code : {-1, 4}) REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, A, N, c, w, ok, code));
    for (int code = 0; code <= 3; ++code) {
        // the limits: blank outside [0, A), A past 2^23, maxU past 4096, maxT maxU >= 2^25, 2^32 rows
        REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, A, N, c, w, opts(T, U, A), code));
        REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, A, N, c, w, opts(T, U, -1), code));
        REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, (1 << 23) + 1, N, c, w, ok, code));
        REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, A, N, c, w, opts(T, 4097, 0), code));
        REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, A, N, c, w, opts(1 << 13, 4096, 0), code));
        REFUSED(compute_rnnt_loss_ar(a, g, l, ln, ln, lo, hi, A, 1 << 16, c, w, opts(1 << 12, 16, 0), code));
        // tensors off their element boundary; gradients that overlap the activations without being them
        REFUSED(compute_rnnt_loss_ar(reinterpret_cast<const char*>(a) + 1, g, l, ln, ln, lo, hi, A, N, c, w, ok, code));
        REFUSED(compute_rnnt_loss_ar(a, reinterpret_cast<char*>(g) + 1, l, ln, ln, lo, hi, A, N, c, w, ok, code));
        REFUSED(compute_rnnt_loss_ar(a, const_cast<float*>(a) + 4, l, ln, ln, lo, hi, A, N, c, w, ok, code));
    }
    // _fwd: the same refusals
    REFUSED(compute_rnnt_loss_ar_fwd(nullptr, l, ln, ln, lo, hi, A, N, c, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_ar_fwd(a, nullptr, ln, ln, lo, hi, A, N, c, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_ar_fwd(a, l, nullptr, ln, lo, hi, A, N, c, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_ar_fwd(a, l, ln, nullptr, lo, hi, A, N, c, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_ar_fwd(a, l, ln, ln, lo, hi, A, N, nullptr, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_ar_fwd(a, l, ln, ln, lo, hi, A, N, c, nullptr, ok, 0, 1));
    REFUSED(compute_rnnt_loss_ar_fwd(a, l, ln, ln, lo, hi, A, N, c, w, opts(T, U, 0, RNNT_CPU), 0, 1));
    REFUSED(compute_rnnt_loss_ar_fwd(a, l, ln, ln, lo, hi, A, N, c, w, opts(T, U, A), 0, 1));
    REFUSED(compute_rnnt_loss_ar_fwd(a, l, ln, ln, lo, hi, A, N, c, w, opts(T, 4097, 0), 0, 0));
    for (int code : {-1, 4}) REFUSED(compute_rnnt_loss_ar_fwd(a, l, ln, ln, lo, hi, A, N, c, w, ok, code, 1));
    // _bwd
    REFUSED(compute_rnnt_loss_ar_bwd(nullptr, g, scale.data(), A, N, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar_bwd(a, nullptr, scale.data(), A, N, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar_bwd(a, g, scale.data(), A, N, nullptr, ok, 0));
    REFUSED(compute_rnnt_loss_ar_bwd(a, g, scale.data(), 0, N, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar_bwd(a, g, scale.data(), A, 0, w, ok, 0));
    REFUSED(compute_rnnt_loss_ar_bwd(a, g, scale.data(), A, N, w, opts(T, U, 0, RNNT_CPU), 0));
    REFUSED(compute_rnnt_loss_ar_bwd(a, g, scale.data(), A, N, w, opts(T, U, A), 0));
    REFUSED(compute_rnnt_loss_ar_bwd(a, const_cast<float*>(a) + 4, scale.data(), A, N, w, ok, 0));
    for (int code : {-1, 4}) REFUSED(compute_rnnt_loss_ar_bwd(a, g, scale.data(), A, N, w, ok, code));
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("alignment-restricted loss argument checks: all refused as include/rnnt_ar.h says\n");
    return 0;
}
