// test_side_args.cpp -- the host drivers of the four side libraries (libwarprnnt_pruned.so, _tdt.so, _hat.so, _mblank.so)
// under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (`make side-asan` builds their twelve
// translation units with the sanitizers on the host side and links them with this file; it needs no GPU): the workspace
// arithmetic of every get_workspace_size_* and the argument refusals of the entries -- the shared checks of
// csrc/rnnt_side_host.h through each library's one-call, _fwd and _bwd entry, and each library's own set checks -- all of
// which return before anything is launched.  run_hat and run_pruned build their plan (make_plan) before the buffer checks;
// make_plan asks the device nothing, so those refusals are decided here as on a machine with a GPU.  Left out: what only a
// finished kernel can tell (the cost markers of device-side lengths that do not fit the tensor).
// The pointers handed over are never dereferenced on these paths; the duration and big-blank arrays are real host arrays,
// read by the checks.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/rnnt_hat.h"
#include "../../include/rnnt_mblank.h"
#include "../../include/rnnt_pruned.h"
#include "../../include/rnnt_tdt.h"

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

// The shapes of every call below and buffers that hold them (TDT's rows are A + D wide; + 4: the overlapping gradients).
constexpr int N = 2, T = 4, U = 3, A = 7;
static std::vector<float> acts(N * T * U * (A + 8) + 4), grads(N * T * U * (A + 8) + 4), costs(N);
static std::vector<int> labels(N * (U - 1)), lens(N, 1), ranges(N * T);
static std::vector<char> ws;

// The refusals of csrc/rnnt_side_host.h through one library.  loss(acts, grads, costs, workspace, options, dtype_code,
// minibatch), fwd(acts, costs, workspace, options, dtype_code, minibatch) and bwd(acts, grads, workspace, options,
// dtype_code, minibatch) call its three entries with otherwise valid arguments.
template <typename Loss, typename Fwd, typename Bwd> static void shared_checks(Loss loss, Fwd fwd, Bwd bwd) {
    const rnntOptions ok = opts(T, U, 0), cpu = opts(T, U, 0, RNNT_CPU);
    float *a = acts.data(), *g = grads.data(), *c = costs.data();
    char* w = ws.data();
    // NULL tensor, costs or workspace
    REFUSED(loss(nullptr, g, c, w, ok, 0, N));
    REFUSED(loss(a, g, nullptr, w, ok, 0, N));
    REFUSED(loss(a, g, c, nullptr, ok, 0, N));
    REFUSED(fwd(nullptr, c, w, ok, 0, N));
    REFUSED(fwd(a, nullptr, w, ok, 0, N));
    REFUSED(fwd(a, c, nullptr, ok, 0, N));
    REFUSED(bwd(nullptr, g, w, ok, 0, N));
    REFUSED(bwd(a, g, nullptr, ok, 0, N));
    // minibatch 0, the CPU location
    REFUSED(loss(a, g, c, w, ok, 0, 0));
    REFUSED(fwd(a, c, w, ok, 0, 0));
    REFUSED(bwd(a, g, w, ok, 0, 0));
    REFUSED(loss(a, g, c, w, cpu, 0, N));
    REFUSED(fwd(a, c, w, cpu, 0, N));
    REFUSED(bwd(a, g, w, cpu, 0, N));
    for (int code : {-1, 4}) {
        REFUSED(loss(a, g, c, w, ok, code, N));
        REFUSED(fwd(a, c, w, ok, code, N));
        REFUSED(bwd(a, g, w, ok, code, N));
    }
    // NULL gradients to _bwd; a gradient pointer misaligned by one byte; gradients that overlap the activations without
    // being them
    REFUSED(bwd(a, nullptr, w, ok, 0, N));
    float* odd = reinterpret_cast<float*>(reinterpret_cast<char*>(g) + 1);
    REFUSED(loss(a, odd, c, w, ok, 0, N));
    REFUSED(bwd(a, odd, w, ok, 0, N));
    REFUSED(loss(a, a + 4, c, w, ok, 0, N));
    REFUSED(bwd(a, a + 4, w, ok, 0, N));
}

// Refusals every get_workspace_size_* shares, and one accepted size per dtype code; size(maxT, maxU, minibatch, dtype_code,
// size_bytes) calls it with the library's own argument valid.
template <typename Size> static void size_checks(Size size) {
    size_t n = 0;
    for (int code = 0; code <= 3; ++code) EXPECT(size(150, 21, 128, code, &n) == RNNT_STATUS_SUCCESS && n > 0);
    REFUSED(size(0, U, N, 0, &n));
    REFUSED(size(T, 0, N, 0, &n));
    REFUSED(size(T, U, 0, 0, &n));
    REFUSED(size(T, U, N, -1, &n));
    REFUSED(size(T, U, N, 4, &n));
    REFUSED(size(T, U, N, 0, nullptr));
}

static void pruned_checks() {
    size_checks([](int mt, int mu, int mb, int code, size_t* n) { return get_workspace_size_pruned(mt, mu, mb, code, n); });
    const int S = 2;
    int* r = ranges.data();
    const int *l = labels.data(), *ln = lens.data();
    shared_checks(
        [&](const void* a, void* g, void* c, void* w, rnntOptions o, int code, int mb) {
            return compute_rnnt_loss_pruned(a, g, r, S, l, ln, ln, A, mb, c, w, o, code);
        },
        [&](const void* a, void* c, void* w, rnntOptions o, int code, int mb) {
            return compute_rnnt_loss_pruned_fwd(a, r, S, l, ln, ln, A, mb, c, w, o, code, 1);
        },
        [&](const void* a, void* g, void* w, rnntOptions o, int code, int mb) {
            return compute_rnnt_loss_pruned_bwd(a, g, nullptr, S, A, mb, w, o, code);
        });
    // its own: NULL ranges, S outside [1, maxU]; the ranges entry: S outside [2, maxU], NULL prediction activations, no fp64
    const rnntOptions ok = opts(T, U, 0);
    float *a = acts.data(), *g = grads.data(), *c = costs.data();
    char* w = ws.data();
    REFUSED(compute_rnnt_loss_pruned(a, g, nullptr, S, l, ln, ln, A, N, c, w, ok, 0));
    REFUSED(compute_rnnt_loss_pruned_fwd(a, nullptr, S, l, ln, ln, A, N, c, w, ok, 0, 1));
    for (int s : {0, -1, U + 1}) {
        REFUSED(compute_rnnt_loss_pruned(a, g, r, s, l, ln, ln, A, N, c, w, ok, 0));
        REFUSED(compute_rnnt_loss_pruned_fwd(a, r, s, l, ln, ln, A, N, c, w, ok, 0, 1));
        REFUSED(compute_rnnt_loss_pruned_bwd(a, g, nullptr, s, A, N, w, ok, 0));
    }
    for (int s : {1, U + 1}) REFUSED(compute_rnnt_prune_ranges_add(a, g, l, ln, ln, A, N, s, r, w, ok, 0));
    REFUSED(compute_rnnt_prune_ranges_add(a, nullptr, l, ln, ln, A, N, S, r, w, ok, 0));
    REFUSED(compute_rnnt_prune_ranges_add(a, g, l, ln, ln, A, N, S, nullptr, w, ok, 0));
    for (int code : {-1, 1, 4}) REFUSED(compute_rnnt_prune_ranges_add(a, g, l, ln, ln, A, N, S, r, w, ok, code));
    REFUSED(compute_rnnt_prune_ranges_add(a, g, l, ln, ln, A, N, S, r, w, opts(T, U, 0, RNNT_CPU), 0));
}

static void tdt_checks() {
    size_checks([](int mt, int mu, int mb, int code, size_t* n) { return get_workspace_size_tdt(mt, mu, mb, 4, code, n); });
    size_t n = 0;
    REFUSED(get_workspace_size_tdt(T, U, N, 0, 0, &n));
    REFUSED(get_workspace_size_tdt(T, U, N, 9, 0, &n));
    const int durs[3] = {0, 1, 2};
    const int *l = labels.data(), *ln = lens.data();
    shared_checks(
        [&](const void* a, void* g, void* c, void* w, rnntOptions o, int code, int mb) {
            return compute_tdt_loss(a, g, durs, 3, 0.0f, l, ln, ln, A, mb, c, w, o, code);
        },
        [&](const void* a, void* c, void* w, rnntOptions o, int code, int mb) {
            return compute_tdt_loss_fwd(a, durs, 3, 0.0f, l, ln, ln, A, mb, c, w, o, code, 1);
        },
        [&](const void* a, void* g, void* w, rnntOptions o, int code, int mb) {
            return compute_tdt_loss_bwd(a, g, nullptr, durs, 3, A, mb, w, o, code);
        });
    // its own: the duration set -- 1 <= D <= 8, strictly increasing, non-negative, largest in [1, 64]; a NaN sigma
    struct Bad { std::vector<int> d; int D; };
    const std::vector<Bad> bad = {{{0, 1, 2}, 0}, {{0, 1, 2, 3, 4, 5, 6, 7, 8}, 9}, {{0, 1, 2}, -1}, {{0, 2, 2}, 3},
                                  {{0, 2, 1}, 3}, {{-1, 1, 2}, 3}, {{0}, 1}, {{0, 1, 65}, 3}};
    const rnntOptions ok = opts(T, U, 0);
    float *a = acts.data(), *g = grads.data(), *c = costs.data();
    char* w = ws.data();
    for (const Bad& b : bad) {
        REFUSED(compute_tdt_loss(a, g, b.d.data(), b.D, 0.0f, l, ln, ln, A, N, c, w, ok, 0));
        REFUSED(compute_tdt_loss_fwd(a, b.d.data(), b.D, 0.0f, l, ln, ln, A, N, c, w, ok, 0, 1));
        REFUSED(compute_tdt_loss_bwd(a, g, nullptr, b.d.data(), b.D, A, N, w, ok, 0));
    }
    REFUSED(compute_tdt_loss(a, g, nullptr, 3, 0.0f, l, ln, ln, A, N, c, w, ok, 0));
    REFUSED(compute_tdt_loss(a, g, durs, 3, __builtin_nanf(""), l, ln, ln, A, N, c, w, ok, 0));
    REFUSED(compute_tdt_loss(a, g, durs, 3, 0.0f, l, ln, ln, A, N, c, w, opts(T, U, A), 0));       // the blank outside [0, A)
}

static void hat_checks() {
    size_checks([](int mt, int mu, int mb, int code, size_t* n) { return get_workspace_size_hat(mt, mu, mb, code, n); });
    size_t n = 0;
    REFUSED(get_workspace_size_hat(T, 1025, N, 0, &n));
    const int *l = labels.data(), *ln = lens.data();
    shared_checks(
        [&](const void* a, void* g, void* c, void* w, rnntOptions o, int code, int mb) {
            return compute_hat_loss(a, g, l, ln, ln, A, mb, c, w, o, code);
        },
        [&](const void* a, void* c, void* w, rnntOptions o, int code, int mb) {
            return compute_hat_loss_fwd(a, l, ln, ln, A, mb, c, w, o, code, 1);
        },
        [&](const void* a, void* g, void* w, rnntOptions o, int code, int mb) {
            return compute_hat_loss_bwd(a, g, nullptr, A, mb, w, o, code);
        });
    // its own: a label column besides the blank, the blank inside [0, A), maxU <= 1024
    float *a = acts.data(), *g = grads.data(), *c = costs.data();
    char* w = ws.data();
    REFUSED(compute_hat_loss(a, g, l, ln, ln, 1, N, c, w, opts(T, U, 0), 0));
    REFUSED(compute_hat_loss(a, g, l, ln, ln, A, N, c, w, opts(T, U, A), 0));
    REFUSED(compute_hat_loss(a, g, l, ln, ln, A, N, c, w, opts(T, U, -1), 0));
    REFUSED(compute_hat_loss(a, g, l, ln, ln, A, N, c, w, opts(T, 1025, 0), 0));
}

// The multi-blank library: its workspace sizes, its big-blank set and the shared checks through its entries.
static void mblank_checks() {
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
}

int main() {
    // a workspace that holds the largest layout of the four at these shapes (fp64 lattice)
    size_t n = 0, need = 1 << 16;
    EXPECT(get_workspace_size_pruned(T, U, N, 1, &n) == RNNT_STATUS_SUCCESS);
    need = n > need ? n : need;
    EXPECT(get_workspace_size_hat(T, U, N, 1, &n) == RNNT_STATUS_SUCCESS);
    need = n > need ? n : need;
    ws.resize(need);
    pruned_checks();
    tdt_checks();
    hat_checks();
    mblank_checks();
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("side-library argument checks: all refused as include/rnnt_{pruned,tdt,hat,mblank}.h say\n");
    return 0;
}
