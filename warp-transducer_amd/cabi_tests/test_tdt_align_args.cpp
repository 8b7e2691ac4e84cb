// test_tdt_align_args.cpp -- the host driver of libwarprnnt_tdt_align.so under AddressSanitizer + UndefinedBehaviorSanitizer, as
// a program of its own (`make side-asan` builds the library's three translation units with the sanitizers on the host side
// and links them with this file; it needs no GPU): the workspace arithmetic of get_workspace_size_tdt_align and the argument
// refusals of compute_tdt_align, all of which return before anything is launched.  Left out: what only a finished kernel can
// tell (device-side lengths that do not fit the tensor).  The pointers handed over are never dereferenced on these paths;
// the duration arrays are real host arrays, read by the checks.
#include <cstdio>
#include <vector>

#include "../../include/rnnt_tdt_align.h"

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
    // sizes: one per dtype code, growing with D; the fp64 lattice needs more than the fp32 one; a layout past 2^40 bytes
    size_t n = 0, prev = 0, n32 = 0, n64 = 0;
    for (int D = 1; D <= 8; ++D)
        for (int code = 0; code <= 3; ++code) {
            EXPECT(get_workspace_size_tdt_align(150, 21, 128, D, code, &n) == RNNT_STATUS_SUCCESS && n > 0);
            if (code == 0) { EXPECT(n > prev); prev = n; }
        }
    EXPECT(get_workspace_size_tdt_align(150, 21, 128, 5, 0, &n32) == RNNT_STATUS_SUCCESS);
    EXPECT(get_workspace_size_tdt_align(150, 21, 128, 5, 1, &n64) == RNNT_STATUS_SUCCESS && n64 > n32);
    EXPECT(get_workspace_size_tdt_align(150, 21, 128, 5, 2, &n) == RNNT_STATUS_SUCCESS && n == n32);
    EXPECT(get_workspace_size_tdt_align(1 << 15, 4096, 1 << 15, 8, 1, &n) == RNNT_STATUS_SUCCESS && n > (size_t(1) << 40));
    // the back-pointer bytes (one per cell) fit the array they live in (one lattice value per cell)
    EXPECT(n32 >= size_t(128) * 150 * 21 * (4 * (5 + 5) + 4 + 4));
    REFUSED(get_workspace_size_tdt_align(0, 3, 2, 3, 0, &n));
    REFUSED(get_workspace_size_tdt_align(4, 0, 2, 3, 0, &n));
    REFUSED(get_workspace_size_tdt_align(4, 3, 0, 3, 0, &n));
    REFUSED(get_workspace_size_tdt_align(4, 3, 2, 0, 0, &n));
    REFUSED(get_workspace_size_tdt_align(4, 3, 2, 9, 0, &n));
    REFUSED(get_workspace_size_tdt_align(4, 3, 2, 3, -1, &n));
    REFUSED(get_workspace_size_tdt_align(4, 3, 2, 3, 4, &n));
    REFUSED(get_workspace_size_tdt_align(4, 3, 2, 3, 0, nullptr));

    constexpr int N = 2, T = 4, U = 3, A = 7;
    std::vector<float> acts(N * T * U * (A + 8) + 4);
    std::vector<double> score(N);
    std::vector<int> labels(N * (U - 1)), lens(N, 1), frames(N * (U - 1)), durs(N * (U - 1));
    EXPECT(get_workspace_size_tdt_align(T, U, N, 8, 1, &n) == RNNT_STATUS_SUCCESS);
    std::vector<char> ws(n);
    const int set[3] = {0, 1, 2};
    const rnntOptions ok = opts(T, U, 0);
    const float* a = acts.data();
    const int *l = labels.data(), *ln = lens.data();
    double* s = score.data();
    int *f = frames.data(), *d = durs.data();
    char* w = ws.data();
    // NULL pointers
    REFUSED(compute_tdt_align(nullptr, set, 3, 0.0f, l, ln, ln, A, N, s, f, d, w, ok, 0));
    REFUSED(compute_tdt_align(a, nullptr, 3, 0.0f, l, ln, ln, A, N, s, f, d, w, ok, 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, nullptr, ln, ln, A, N, s, f, d, w, ok, 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, nullptr, ln, A, N, s, f, d, w, ok, 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, nullptr, A, N, s, f, d, w, ok, 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, N, nullptr, f, d, w, ok, 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, N, s, nullptr, d, w, ok, 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, N, s, f, nullptr, w, ok, 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, N, s, f, d, nullptr, ok, 0));
    // sizes, the CPU location, dtype codes, a misaligned tensor, a NaN sigma
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, 0, N, s, f, d, w, ok, 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, 0, s, f, d, w, ok, 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, N, s, f, d, w, opts(0, U, 0), 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, N, s, f, d, w, opts(T, 0, 0), 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, N, s, f, d, w, opts(T, U, 0, RNNT_CPU), 0));
    for (int code : {-1, 4}) REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, N, s, f, d, w, ok, code));
    REFUSED(compute_tdt_align(reinterpret_cast<const char*>(a) + 1, set, 3, 0.0f, l, ln, ln, A, N, s, f, d, w, ok, 0));
    REFUSED(compute_tdt_align(a, set, 3, __builtin_nanf(""), l, ln, ln, A, N, s, f, d, w, ok, 0));
    // the duration set -- 1 <= D <= 8, strictly increasing, non-negative, largest in [1, 64] -- in every dtype
    struct Bad { std::vector<int> d; int D; };
    const std::vector<Bad> bad = {{{0, 1, 2}, 0}, {{0, 1, 2, 3, 4, 5, 6, 7, 8}, 9}, {{0, 1, 2}, -1}, {{0, 2, 2}, 3},
                                  {{0, 2, 1}, 3}, {{-1, 1, 2}, 3}, {{0}, 1}, {{0, 1, 65}, 3}};
    for (const Bad& b : bad)
        for (int code = 0; code <= 3; ++code)
            REFUSED(compute_tdt_align(a, b.d.data(), b.D, 0.0f, l, ln, ln, A, N, s, f, d, w, ok, code));
    // the limits: blank outside [0, A), maxU past 4096, maxT maxU >= 2^25, 2^32 rows
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, N, s, f, d, w, opts(T, U, A), 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, N, s, f, d, w, opts(T, U, -1), 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, N, s, f, d, w, opts(T, 4097, 0), 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, N, s, f, d, w, opts(1 << 13, 4096, 0), 0));
    REFUSED(compute_tdt_align(a, set, 3, 0.0f, l, ln, ln, A, 1 << 16, s, f, d, w, opts(1 << 12, 16, 0), 0));
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("TDT alignment argument checks: all refused as include/rnnt_tdt_align.h says\n");
    return 0;
}
