// test_pstream_args.cpp -- the host driver of libwarprnnt_pstream.so under AddressSanitizer + UndefinedBehaviorSanitizer, as
// a program of its own (`make side-asan` builds the library's three translation units with the sanitizers on the host side
// and links them with this file; it needs no GPU): the workspace arithmetic of get_workspace_size_pstream and the argument
// refusals of the three compute entries of include/rnnt_pstream.h, all of which return before anything is launched.  Left
// out: what only a finished kernel can tell (device-side lengths or starts that do not fit).  The refusals: a lattice type
// outside {0, 1}, a NaN or infinite delay_penalty, S outside [1, maxU], the limits, NULL pointers, the CPU location, bad
// dtype codes, overlapping buffers.  The pointers handed over are never dereferenced on these paths.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/rnnt_pstream.h"

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
    // arrays the layout must hold (four-word cell records, alpha, beta, maxT + maxU offsets per sample and direction, a
    // window word per frame, the compact table of four-word records per row of the tensor); growth in every argument
    size_t n = 0, n32 = 0, n64 = 0, n1 = 0;
    EXPECT(get_workspace_size_pstream(150, 21, 5, 128, 0, &n32) == RNNT_STATUS_SUCCESS && n32 > 0);
    EXPECT(get_workspace_size_pstream(150, 21, 5, 128, 1, &n64) == RNNT_STATUS_SUCCESS && n64 > n32);
    EXPECT(get_workspace_size_pstream(150, 21, 5, 128, 2, &n) == RNNT_STATUS_SUCCESS && n == n32);
    EXPECT(get_workspace_size_pstream(150, 21, 5, 128, 3, &n) == RNNT_STATUS_SUCCESS && n == n32);
    const size_t cells = size_t(128) * 150 * 21, rows = size_t(128) * 150 * 5;
    const size_t fixed = size_t(128) * (150 + 21) * 2 * sizeof(double) + size_t(128) * 150 * 8;
    EXPECT(n32 >= cells * 4 * (4 + 1 + 1) + rows * 4 * 4 + fixed);
    EXPECT(n32 < cells * 4 * (4 + 1 + 1) + rows * 4 * 4 + fixed + 128 * 64 + 20 * 256);
    EXPECT(n64 >= cells * 8 * (4 + 1 + 1) + rows * 8 * 4 + fixed);
    EXPECT(get_workspace_size_pstream(151, 21, 5, 128, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_pstream(150, 22, 5, 128, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_pstream(150, 21, 6, 128, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_pstream(150, 21, 5, 129, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_pstream(150, 21, 21, 128, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_pstream(1, 1, 1, 1, 0, &n1) == RNNT_STATUS_SUCCESS && n1 >= 4 * 6 + 4 * 4 + 2 * 2 * sizeof(double));
    EXPECT(get_workspace_size_pstream(1 << 15, 4096, 8, 1 << 15, 1, &n) == RNNT_STATUS_SUCCESS && n > (size_t(1) << 40));
    REFUSED(get_workspace_size_pstream(0, 3, 2, 2, 0, &n));
    REFUSED(get_workspace_size_pstream(4, 0, 1, 2, 0, &n));
    REFUSED(get_workspace_size_pstream(4, 3, 0, 2, 0, &n));
    REFUSED(get_workspace_size_pstream(4, 3, -1, 2, 0, &n));
    REFUSED(get_workspace_size_pstream(4, 3, 4, 2, 0, &n));
    REFUSED(get_workspace_size_pstream(4, 3, 2, 0, 0, &n));
    REFUSED(get_workspace_size_pstream(4, 3, 2, 2, -1, &n));
    REFUSED(get_workspace_size_pstream(4, 3, 2, 2, 4, &n));
    REFUSED(get_workspace_size_pstream(4, 3, 2, 2, 0, nullptr));

    constexpr int N = 2, T = 4, U = 3, S = 2, A = 7;
    std::vector<float> acts(N * T * U * A + 8), grads(N * T * U * A + 8), costs(N), scale(N, 1.0f);
    std::vector<int> labels(N * (U - 1)), lens(N, 1), ranges(N * T, 0);
    EXPECT(get_workspace_size_pstream(T, U, U, N, 1, &n) == RNNT_STATUS_SUCCESS);
    std::vector<char> ws(n);
    const rnntOptions ok = opts(T, U, 0);
    const float* a = acts.data();
    float *g = grads.data(), *c = costs.data();
    const int *l = labels.data(), *ln = lens.data(), *r = ranges.data();
    char* w = ws.data();
    const float P = 0.25f;
    const float inf = std::numeric_limits<float>::infinity();
    // the one-call entry: NULL pointers (gradients may be NULL: score only)
    REFUSED(compute_rnnt_loss_pstream(nullptr, g, r, S, 0, P, l, ln, ln, A, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream(a, g, nullptr, S, 0, P, l, ln, ln, A, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream(a, g, r, S, 0, P, nullptr, ln, ln, A, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream(a, g, r, S, 0, P, l, nullptr, ln, A, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream(a, g, r, S, 0, P, l, ln, nullptr, A, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream(a, g, r, S, 0, P, l, ln, ln, A, N, nullptr, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream(a, g, r, S, 0, P, l, ln, ln, A, N, c, nullptr, ok, 0));
    // sizes, the CPU location, dtype codes
    REFUSED(compute_rnnt_loss_pstream(a, g, r, S, 0, P, l, ln, ln, 0, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream(a, g, r, S, 0, P, l, ln, ln, A, 0, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream(a, g, r, S, 0, P, l, ln, ln, A, N, c, w, opts(0, U, 0), 0));
    REFUSED(compute_rnnt_loss_pstream(a, g, r, S, 0, P, l, ln, ln, A, N, c, w, opts(T, 0, 0), 0));
    REFUSED(compute_rnnt_loss_pstream(a, g, r, S, 0, P, l, ln, ln, A, N, c, w, opts(T, U, 0, RNNT_CPU), 0));
    for (int code : {-1, 4}) REFUSED(compute_rnnt_loss_pstream(a, g, r, S, 0, P, l, ln, ln, A, N, c, w, ok, code));
    for (int code = 0; code <= 3; ++code)
        for (int type = 0; type <= 1; ++type) {
            // the window size: 1 <= S <= maxU
            for (int s : {0, -1, U + 1}) {
                REFUSED(compute_rnnt_loss_pstream(a, g, r, s, type, P, l, ln, ln, A, N, c, w, ok, code));
                REFUSED(compute_rnnt_loss_pstream_fwd(a, r, s, type, P, l, ln, ln, A, N, c, w, ok, code, 1));
                REFUSED(compute_rnnt_loss_pstream_bwd(a, g, scale.data(), s, A, N, w, ok, code));
            }
            // the limits: blank outside [0, A), A past 2^23, maxU past 4096, maxT maxU >= 2^25, 2^32 cells
            REFUSED(compute_rnnt_loss_pstream(a, g, r, S, type, P, l, ln, ln, A, N, c, w, opts(T, U, A), code));
            REFUSED(compute_rnnt_loss_pstream(a, g, r, S, type, P, l, ln, ln, A, N, c, w, opts(T, U, -1), code));
            REFUSED(compute_rnnt_loss_pstream(a, g, r, S, type, P, l, ln, ln, (1 << 23) + 1, N, c, w, ok, code));
            REFUSED(compute_rnnt_loss_pstream(a, g, r, S, type, P, l, ln, ln, A, N, c, w, opts(T, 4097, 0), code));
            REFUSED(compute_rnnt_loss_pstream(a, g, r, S, type, P, l, ln, ln, A, N, c, w, opts(1 << 13, 4096, 0), code));
            REFUSED(compute_rnnt_loss_pstream(a, g, r, S, type, P, l, ln, ln, A, 1 << 16, c, w, opts(1 << 12, 16, 0), code));
            // tensors off their element boundary; gradients that overlap the activations without being them
            REFUSED(compute_rnnt_loss_pstream(reinterpret_cast<const char*>(a) + 1, g, r, S, type, P, l, ln, ln, A, N, c, w, ok,
                                              code));
            REFUSED(compute_rnnt_loss_pstream(a, reinterpret_cast<char*>(g) + 1, r, S, type, P, l, ln, ln, A, N, c, w, ok, code));
            REFUSED(compute_rnnt_loss_pstream(a, const_cast<float*>(a) + 4, r, S, type, P, l, ln, ln, A, N, c, w, ok, code));
        }
    // the lattice type and the penalty: refused in every entry that takes them, before the dtype switch (a dtype code that
    // is itself refused changes nothing), with and without gradients
    for (int code = -1; code <= 4; ++code) {
        for (int type : {-1, 2, 3, 1 << 30}) {
            REFUSED(compute_rnnt_loss_pstream(a, g, r, S, type, P, l, ln, ln, A, N, c, w, ok, code));
            REFUSED(compute_rnnt_loss_pstream(a, nullptr, r, S, type, P, l, ln, ln, A, N, c, w, ok, code));
            REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, type, P, l, ln, ln, A, N, c, w, ok, code, 0));
            REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, type, P, l, ln, ln, A, N, c, w, ok, code, 1));
        }
        for (float bad : {std::nanf(""), inf, -inf})
            for (int type = 0; type <= 1; ++type) {
                REFUSED(compute_rnnt_loss_pstream(a, g, r, S, type, bad, l, ln, ln, A, N, c, w, ok, code));
                REFUSED(compute_rnnt_loss_pstream(a, nullptr, r, S, type, bad, l, ln, ln, A, N, c, w, ok, code));
                REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, type, bad, l, ln, ln, A, N, c, w, ok, code, 0));
                REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, type, bad, l, ln, ln, A, N, c, w, ok, code, 1));
            }
    }
    // _fwd: the same refusals
    REFUSED(compute_rnnt_loss_pstream_fwd(nullptr, r, S, 1, P, l, ln, ln, A, N, c, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_pstream_fwd(a, nullptr, S, 1, P, l, ln, ln, A, N, c, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, 1, P, nullptr, ln, ln, A, N, c, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, 1, P, l, nullptr, ln, A, N, c, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, 1, P, l, ln, nullptr, A, N, c, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, 1, P, l, ln, ln, A, N, nullptr, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, 1, P, l, ln, ln, A, N, c, nullptr, ok, 0, 1));
    REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, 1, P, l, ln, ln, A, N, c, w, opts(T, U, 0, RNNT_CPU), 0, 1));
    REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, 1, P, l, ln, ln, A, N, c, w, opts(T, U, A), 0, 1));
    REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, 1, P, l, ln, ln, A, N, c, w, opts(T, 4097, 0), 0, 0));
    REFUSED(compute_rnnt_loss_pstream_fwd(reinterpret_cast<const char*>(a) + 2, r, S, 1, P, l, ln, ln, A, N, c, w, ok, 0, 1));
    for (int code : {-1, 4}) REFUSED(compute_rnnt_loss_pstream_fwd(a, r, S, 1, P, l, ln, ln, A, N, c, w, ok, code, 1));
    // _bwd
    REFUSED(compute_rnnt_loss_pstream_bwd(nullptr, g, scale.data(), S, A, N, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream_bwd(a, nullptr, scale.data(), S, A, N, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream_bwd(a, g, scale.data(), S, A, N, nullptr, ok, 0));
    REFUSED(compute_rnnt_loss_pstream_bwd(a, g, scale.data(), S, 0, N, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream_bwd(a, g, scale.data(), S, A, 0, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream_bwd(a, g, scale.data(), S, A, N, w, opts(T, U, 0, RNNT_CPU), 0));
    REFUSED(compute_rnnt_loss_pstream_bwd(a, g, scale.data(), S, A, N, w, opts(T, U, A), 0));
    REFUSED(compute_rnnt_loss_pstream_bwd(a, g, scale.data(), S, A, N, w, opts(T, 4097, 0), 0));
    REFUSED(compute_rnnt_loss_pstream_bwd(a, const_cast<float*>(a) + 4, scale.data(), S, A, N, w, ok, 0));
    REFUSED(compute_rnnt_loss_pstream_bwd(a, reinterpret_cast<char*>(g) + 1, scale.data(), S, A, N, w, ok, 0));
    for (int code : {-1, 4}) REFUSED(compute_rnnt_loss_pstream_bwd(a, g, scale.data(), S, A, N, w, ok, code));
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("pruned streaming loss argument checks: all refused as include/rnnt_pstream.h says\n");
    return 0;
}
