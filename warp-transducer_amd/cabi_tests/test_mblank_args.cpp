// test_mblank_args.cpp -- the host driver of libwarprnnt_mblank.so under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// program of its own (`make mblank-asan` builds the three translation units with the sanitizers on the host side and links
// them with this file; it needs no GPU): the workspace arithmetic of get_workspace_size_mblank and every argument refusal of
// the four entries, all of which return before anything is launched.  The pointers handed over are never dereferenced on
// these paths; the big-blank arrays are real host arrays, read by the checks.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/rnnt_mblank.h"

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

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
    size_t n = 0, prev = 0;
    for (int K = 0; K <= 8; ++K)
        for (int code = 0; code <= 3; ++code) {
            EXPECT(get_workspace_size_mblank(150, 21, 128, K, code, &n) == RNNT_STATUS_SUCCESS && n > 0);
            if (code == 0) { EXPECT(n > prev); prev = n; }          // the record stride grows with K
        }
    EXPECT(get_workspace_size_mblank(1 << 15, 4096, 1 << 15, 8, 1, &n) == RNNT_STATUS_SUCCESS && n > (size_t(1) << 40));
    EXPECT(get_workspace_size_mblank(4, 3, 1, 9, 0, &n) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(get_workspace_size_mblank(4, 3, 1, -1, 0, &n) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(get_workspace_size_mblank(4, 3, 1, 2, 4, &n) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(get_workspace_size_mblank(0, 3, 1, 2, 0, &n) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(get_workspace_size_mblank(4, 3, 1, 2, 0, nullptr) == RNNT_STATUS_INVALID_VALUE);

    const int N = 2, T = 4, U = 3, A = 7;
    std::vector<float> acts(N * T * U * A), grads(N * T * U * A), costs(N);
    std::vector<int> labels(N * (U - 1)), lens(N, 1);
    std::vector<char> ws(1 << 16);
    struct Bad { std::vector<int> cols, durs; int K; int blank; };
    const std::vector<Bad> bad = {
        {{1, 2, 3, 4, 5, 6, 1, 2, 3}, {2, 3, 4, 5, 6, 7, 8, 9, 10}, 9, 0},   // K = 9
        {{5, 6}, {2, 3}, -1, 0},                                              // K < 0
        {{5, 6}, {1, 3}, 2, 0}, {{5, 6}, {2, 65}, 2, 0},                      // a duration outside [2, 64]
        {{5, 6}, {3, 3}, 2, 0}, {{5, 6}, {4, 2}, 2, 0},                       // not strictly increasing
        {{5, 0}, {2, 3}, 2, 0}, {{5, 5}, {2, 3}, 2, 0},                       // the blank's column, a duplicate
        {{5, 7}, {2, 3}, 2, 0}, {{-1, 6}, {2, 3}, 2, 0},                      // outside [0, A)
        {{5, 6}, {2, 3}, 2, 7}, {{5, 6}, {2, 3}, 2, -1}};                     // the blank outside [0, A)
    for (const Bad& b : bad) {
        const rnntOptions o = opts(T, U, b.blank);
        EXPECT(compute_mblank_loss(acts.data(), grads.data(), b.cols.data(), b.durs.data(), b.K, 0.0f, labels.data(),
                                   lens.data(), lens.data(), A, N, costs.data(), ws.data(), o, 0) == RNNT_STATUS_INVALID_VALUE);
        EXPECT(compute_mblank_loss_fwd(acts.data(), b.cols.data(), b.durs.data(), b.K, 0.0f, labels.data(), lens.data(),
                                       lens.data(), A, N, costs.data(), ws.data(), o, 0, 1) == RNNT_STATUS_INVALID_VALUE);
        EXPECT(compute_mblank_loss_bwd(acts.data(), grads.data(), nullptr, b.cols.data(), b.durs.data(), b.K, A, N, ws.data(),
                                       o, 0) == RNNT_STATUS_INVALID_VALUE);
    }
    const int cols[2] = {5, 6}, durs[2] = {2, 3};
    const rnntOptions ok = opts(T, U, 0);
    // NULL big-blank arrays with K > 0, dtype codes, NULL tensors, the CPU location, maxU past the limit, sizes, NaN sigma
    EXPECT(compute_mblank_loss(acts.data(), nullptr, nullptr, durs, 2, 0.0f, labels.data(), lens.data(), lens.data(), A, N,
                               costs.data(), ws.data(), ok, 0) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(compute_mblank_loss(acts.data(), nullptr, cols, nullptr, 2, 0.0f, labels.data(), lens.data(), lens.data(), A, N,
                               costs.data(), ws.data(), ok, 0) == RNNT_STATUS_INVALID_VALUE);
    for (int code : {-1, 4})
        EXPECT(compute_mblank_loss(acts.data(), nullptr, cols, durs, 2, 0.0f, labels.data(), lens.data(), lens.data(), A, N,
                                   costs.data(), ws.data(), ok, code) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(compute_mblank_loss(nullptr, nullptr, cols, durs, 2, 0.0f, labels.data(), lens.data(), lens.data(), A, N,
                               costs.data(), ws.data(), ok, 0) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(compute_mblank_loss(acts.data(), nullptr, cols, durs, 2, 0.0f, labels.data(), lens.data(), lens.data(), A, N,
                               costs.data(), nullptr, ok, 0) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(compute_mblank_loss(acts.data(), nullptr, cols, durs, 2, 0.0f, labels.data(), lens.data(), lens.data(), A, N,
                               costs.data(), ws.data(), opts(T, U, 0, RNNT_CPU), 0) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(compute_mblank_loss(acts.data(), nullptr, cols, durs, 2, 0.0f, labels.data(), lens.data(), lens.data(), A, N,
                               costs.data(), ws.data(), opts(T, 4097, 0), 0) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(compute_mblank_loss(acts.data(), nullptr, cols, durs, 2, 0.0f, labels.data(), lens.data(), lens.data(), A, 0,
                               costs.data(), ws.data(), ok, 0) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(compute_mblank_loss(acts.data(), nullptr, cols, durs, 2, __builtin_nanf(""), labels.data(), lens.data(), lens.data(), A,
                               N, costs.data(), ws.data(), ok, 0) == RNNT_STATUS_INVALID_VALUE);
    // gradients that overlap the activations without being them; a misaligned gradient pointer
    EXPECT(compute_mblank_loss(acts.data(), acts.data() + 4, cols, durs, 2, 0.0f, labels.data(), lens.data(), lens.data(), A,
                               N, costs.data(), ws.data(), ok, 0) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(compute_mblank_loss_bwd(acts.data(), reinterpret_cast<char*>(grads.data()) + 1, nullptr, cols, durs, 2, A, N,
                                   ws.data(), ok, 0) == RNNT_STATUS_INVALID_VALUE);
    EXPECT(compute_mblank_loss_bwd(acts.data(), nullptr, nullptr, cols, durs, 2, A, N, ws.data(), ok, 0) ==
           RNNT_STATUS_INVALID_VALUE);
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("mblank argument checks: all refused as include/rnnt_mblank.h says\n");
    return 0;
}
