// test_delay_args.cpp -- the host driver of libwarprnnt_delay.so under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// program of its own (`make side-asan` builds the library's three translation units with the sanitizers on the host side
// and links them with this file; it needs no GPU): the workspace arithmetic of get_workspace_size_delay and the argument
// refusals of the three compute entries of include/rnnt_delay.h, all of which return before anything is launched.  Left
// out: what only a finished kernel can tell (device-side lengths that do not fit the tensor).  Added to the monotonic
// program's list: a NaN or infinite delay_penalty, and an emit_frames array off its element boundary or overlapping the
// activations, the gradients or the workspace.  The pointers handed over are never dereferenced on these paths.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/rnnt_delay.h"

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
    // arrays the layout must hold (four-word records, alpha, beta, maxT + maxU offsets per sample and direction); 2^40 bytes
    size_t n = 0, n32 = 0, n64 = 0, n1 = 0;
    EXPECT(get_workspace_size_delay(150, 21, 128, 0, &n32) == RNNT_STATUS_SUCCESS && n32 > 0);
    EXPECT(get_workspace_size_delay(150, 21, 128, 1, &n64) == RNNT_STATUS_SUCCESS && n64 > n32);
    EXPECT(get_workspace_size_delay(150, 21, 128, 2, &n) == RNNT_STATUS_SUCCESS && n == n32);
    EXPECT(get_workspace_size_delay(150, 21, 128, 3, &n) == RNNT_STATUS_SUCCESS && n == n32);
    const size_t cells = size_t(128) * 150 * 21, offs = size_t(128) * (150 + 21) * 2 * sizeof(double);
    EXPECT(n32 >= cells * 4 * (4 + 1 + 1) + offs && n32 < cells * 4 * (4 + 1 + 1) + offs + 128 * 64 + 16 * 256);
    EXPECT(n64 >= cells * 8 * (4 + 1 + 1) + offs);
    EXPECT(get_workspace_size_delay(151, 21, 128, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_delay(150, 22, 128, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_delay(150, 21, 129, 0, &n) == RNNT_STATUS_SUCCESS && n > n32);
    EXPECT(get_workspace_size_delay(1, 1, 1, 0, &n1) == RNNT_STATUS_SUCCESS && n1 >= 4 * 6 + 2 * 2 * sizeof(double));
    EXPECT(get_workspace_size_delay(1 << 15, 4096, 1 << 15, 1, &n) == RNNT_STATUS_SUCCESS && n > (size_t(1) << 40));
    REFUSED(get_workspace_size_delay(0, 3, 2, 0, &n));
    REFUSED(get_workspace_size_delay(4, 0, 2, 0, &n));
    REFUSED(get_workspace_size_delay(4, 3, 0, 0, &n));
    REFUSED(get_workspace_size_delay(4, 3, 2, -1, &n));
    REFUSED(get_workspace_size_delay(4, 3, 2, 4, &n));
    REFUSED(get_workspace_size_delay(4, 3, 2, 0, nullptr));

    constexpr int N = 2, T = 4, U = 3, A = 7;
    std::vector<float> acts(N * T * U * A + 8), grads(N * T * U * A + 8), costs(N), scale(N, 1.0f);
    std::vector<int> labels(N * (U - 1)), lens(N, 1);
    EXPECT(get_workspace_size_delay(T, U, N, 1, &n) == RNNT_STATUS_SUCCESS);
    std::vector<char> ws(n);
    const rnntOptions ok = opts(T, U, 0);
    const float* a = acts.data();
    float *g = grads.data(), *c = costs.data();
    const int *l = labels.data(), *ln = lens.data();
    char* w = ws.data();
    std::vector<double> frames(N * (U - 1) + 2);                 // (wide enough for the fp64 lattice's values)
    double* e = frames.data();
    const float P = 0.25f;
    // the one-call entry: NULL pointers (gradients may be NULL: score only)
    REFUSED(compute_rnnt_loss_delay(nullptr, P, g, l, ln, ln, A, N, c, e, w, ok, 0));
    REFUSED(compute_rnnt_loss_delay(a, P, g, nullptr, ln, ln, A, N, c, e, w, ok, 0));
    REFUSED(compute_rnnt_loss_delay(a, P, g, l, nullptr, ln, A, N, c, e, w, ok, 0));
    REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, nullptr, A, N, c, e, w, ok, 0));
    REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, N, nullptr, e, w, ok, 0));
    REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, N, c, e, nullptr, ok, 0));
    // sizes, the CPU location, dtype codes
    REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, 0, N, c, e, w, ok, 0));
    REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, 0, c, e, w, ok, 0));
    REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, N, c, e, w, opts(0, U, 0), 0));
    REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, N, c, e, w, opts(T, 0, 0), 0));
    REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, N, c, e, w, opts(T, U, 0, RNNT_CPU), 0));
    for (int code : {-1, 4}) REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, N, c, e, w, ok, code));
    for (int code = 0; code <= 3; ++code) {
        // the limits: blank outside [0, A), A past 2^23, maxU past 4096, maxT maxU >= 2^25, 2^32 rows
        REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, N, c, e, w, opts(T, U, A), code));
        REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, N, c, e, w, opts(T, U, -1), code));
        REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, (1 << 23) + 1, N, c, e, w, ok, code));
        REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, N, c, e, w, opts(T, 4097, 0), code));
        REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, N, c, e, w, opts(1 << 13, 4096, 0), code));
        REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, 1 << 16, c, e, w, opts(1 << 12, 16, 0), code));
        // tensors off their element boundary; gradients that overlap the activations without being them
        REFUSED(compute_rnnt_loss_delay(reinterpret_cast<const char*>(a) + 1, P, g, l, ln, ln, A, N, c, e, w, ok, code));
        REFUSED(compute_rnnt_loss_delay(a, P, reinterpret_cast<char*>(g) + 1, l, ln, ln, A, N, c, e, w, ok, code));
        REFUSED(compute_rnnt_loss_delay(a, P, const_cast<float*>(a) + 4, l, ln, ln, A, N, c, e, w, ok, code));
    }
    // the penalty: NaN and both infinities are refused in every entry that takes one, before the dtype switch (a dtype code
    // that is itself refused changes nothing); emit_frames NULL or not
    for (float bad : {std::nanf(""), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()})
        for (double* ef : {e, static_cast<double*>(nullptr)})
            for (int code = -1; code <= 4; ++code) {
                REFUSED(compute_rnnt_loss_delay(a, bad, g, l, ln, ln, A, N, c, ef, w, ok, code));
                REFUSED(compute_rnnt_loss_delay(a, bad, nullptr, l, ln, ln, A, N, c, ef, w, ok, code));
                REFUSED(compute_rnnt_loss_delay_fwd(a, bad, l, ln, ln, A, N, c, ef, w, ok, code, 0));
                REFUSED(compute_rnnt_loss_delay_fwd(a, bad, l, ln, ln, A, N, c, ef, w, ok, code, 1));
            }
    // emit_frames: off its element boundary; inside the activations, the gradients, the workspace (its first and its last
    // bytes); for every dtype code, with and without gradients
    for (int code = 0; code <= 3; ++code) {
        const size_t lat = code == 1 ? 8 : 4, esz = code == 1 ? 8 : code == 0 ? 4 : 2;
        size_t wsz = 0;
        EXPECT(get_workspace_size_delay(T, U, N, code, &wsz) == RNNT_STATUS_SUCCESS && wsz <= ws.size());
        char* ac = reinterpret_cast<char*>(acts.data());
        char* gc = reinterpret_cast<char*>(grads.data());
        void* inside[] = {reinterpret_cast<char*>(e) + 1, ac, ac + N * T * U * A * esz - lat, gc + 8, w, w + wsz - lat};
        for (void* ef : inside) {
            REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, N, c, ef, w, ok, code));
            if (ef != gc + 8) REFUSED(compute_rnnt_loss_delay(a, P, nullptr, l, ln, ln, A, N, c, ef, w, ok, code));
            if (ef != gc + 8) REFUSED(compute_rnnt_loss_delay_fwd(a, P, l, ln, ln, A, N, c, ef, w, ok, code, 0));
        }
        // an array that ends where the activations begin overlaps nothing: only with maxU == 1 is the pointer not looked at
        REFUSED(compute_rnnt_loss_delay(a, P, g, l, ln, ln, A, N, c, ac + lat, w, opts(T, 2, 0), code));
    }
    // _fwd: the same refusals
    REFUSED(compute_rnnt_loss_delay_fwd(nullptr, P, l, ln, ln, A, N, c, e, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_delay_fwd(a, P, nullptr, ln, ln, A, N, c, e, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_delay_fwd(a, P, l, nullptr, ln, A, N, c, e, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_delay_fwd(a, P, l, ln, nullptr, A, N, c, e, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_delay_fwd(a, P, l, ln, ln, A, N, nullptr, e, w, ok, 0, 1));
    REFUSED(compute_rnnt_loss_delay_fwd(a, P, l, ln, ln, A, N, c, e, nullptr, ok, 0, 1));
    REFUSED(compute_rnnt_loss_delay_fwd(a, P, l, ln, ln, A, N, c, e, w, opts(T, U, 0, RNNT_CPU), 0, 1));
    REFUSED(compute_rnnt_loss_delay_fwd(a, P, l, ln, ln, A, N, c, e, w, opts(T, U, A), 0, 1));
    REFUSED(compute_rnnt_loss_delay_fwd(a, P, l, ln, ln, A, N, c, e, w, opts(T, 4097, 0), 0, 0));
    for (int code : {-1, 4}) REFUSED(compute_rnnt_loss_delay_fwd(a, P, l, ln, ln, A, N, c, e, w, ok, code, 1));
    // _bwd
    REFUSED(compute_rnnt_loss_delay_bwd(nullptr, g, scale.data(), A, N, w, ok, 0));
    REFUSED(compute_rnnt_loss_delay_bwd(a, nullptr, scale.data(), A, N, w, ok, 0));
    REFUSED(compute_rnnt_loss_delay_bwd(a, g, scale.data(), A, N, nullptr, ok, 0));
    REFUSED(compute_rnnt_loss_delay_bwd(a, g, scale.data(), 0, N, w, ok, 0));
    REFUSED(compute_rnnt_loss_delay_bwd(a, g, scale.data(), A, 0, w, ok, 0));
    REFUSED(compute_rnnt_loss_delay_bwd(a, g, scale.data(), A, N, w, opts(T, U, 0, RNNT_CPU), 0));
    REFUSED(compute_rnnt_loss_delay_bwd(a, g, scale.data(), A, N, w, opts(T, U, A), 0));
    REFUSED(compute_rnnt_loss_delay_bwd(a, const_cast<float*>(a) + 4, scale.data(), A, N, w, ok, 0));
    for (int code : {-1, 4}) REFUSED(compute_rnnt_loss_delay_bwd(a, g, scale.data(), A, N, w, ok, code));
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("delay-penalized loss argument checks: all refused as include/rnnt_delay.h says\n");
    return 0;
}
