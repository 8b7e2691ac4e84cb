// test_joiner_args.cpp -- the host driver of libwarprnnt_joiner.so under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// program of its own (`make side-asan` builds the library's three translation units with the sanitizers on the host side and
// links them with this file; it needs no GPU): the workspace arithmetic of get_workspace_size_joiner and every refusal of
// include/rnnt_joiner.h, all of which return before anything is launched.  The pointers handed over are never dereferenced
// on these paths.
#include <cstdio>
#include <vector>

#include "../../include/rnnt_joiner.h"

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)
#define REFUSED(call) EXPECT((call) == RNNT_STATUS_INVALID_VALUE)

static rnntOptions opts(rnntComputeLocation loc = RNNT_GPU) {
    rnntOptions o{};
    o.loc = loc;
    o.batch_first = true;
    return o;
}

int main() {
    // sizes: the flags alone where the walk is not split (c3: N = 128 samples of 8 column slices are 1024 workgroups); the
    // partial sums of the shares where N and H give too few (one sample: 8 shares of T = 150); none past the single pass's
    // reach (U > 256 of fp32); fp64 partial sums are twice the fp32 ones, 16-bit storage sums in fp32
    size_t n = 0, c3 = 0, one = 0, one64 = 0;
    EXPECT(get_workspace_size_joiner(150, 21, 0, 512, 128, 0, 0, &c3) == RNNT_STATUS_SUCCESS && c3 >= 128 * 4 && c3 <= 128 * 4 + 512);
    EXPECT(get_workspace_size_joiner(150, 21, 0, 512, 1, 0, 0, &one) == RNNT_STATUS_SUCCESS);
    EXPECT(one >= size_t(8) * 21 * 512 * 4 && one <= size_t(8) * 21 * 512 * 4 + 1024);
    EXPECT(get_workspace_size_joiner(150, 21, 0, 512, 1, 0, 1, &one64) == RNNT_STATUS_SUCCESS && one64 >= 2 * (one - 1024));
    EXPECT(get_workspace_size_joiner(150, 21, 0, 512, 1, 1, 2, &n) == RNNT_STATUS_SUCCESS && n == one);
    EXPECT(get_workspace_size_joiner(150, 21, 5, 512, 1, 2, 3, &n) == RNNT_STATUS_SUCCESS && n == one);
    EXPECT(get_workspace_size_joiner(3, 600, 0, 8, 1, 0, 0, &n) == RNNT_STATUS_SUCCESS && n <= 1024);
    EXPECT(get_workspace_size_joiner(16, 21, 0, 512, 1, 0, 0, &n) == RNNT_STATUS_SUCCESS && n <= 1024);        // T too short to share
    REFUSED(get_workspace_size_joiner(0, 3, 0, 8, 2, 0, 0, &n));
    REFUSED(get_workspace_size_joiner(4, 0, 0, 8, 2, 0, 0, &n));
    REFUSED(get_workspace_size_joiner(4, 3, 0, 0, 2, 0, 0, &n));
    REFUSED(get_workspace_size_joiner(4, 3, 0, 8, 0, 0, 0, &n));
    REFUSED(get_workspace_size_joiner(4, 3, 0, 8, 2, -1, 0, &n));
    REFUSED(get_workspace_size_joiner(4, 3, 0, 8, 2, 3, 0, &n));
    REFUSED(get_workspace_size_joiner(4, 3, 0, 8, 2, 0, -1, &n));
    REFUSED(get_workspace_size_joiner(4, 3, 0, 8, 2, 0, 4, &n));
    REFUSED(get_workspace_size_joiner(4, 3, 0, 8, 2, 2, 0, &n));          // layout 2: S = 0
    REFUSED(get_workspace_size_joiner(4, 3, 4, 8, 2, 2, 0, &n));          // S > U
    REFUSED(get_workspace_size_joiner(4, 3, 2, 8, 2, 2, 0, nullptr));

    // host buffers stand in for device memory: no refused call reads or writes them
    const int N = 2, T = 4, U = 3, S = 2, H = 8;
    std::vector<float> f(N * T * H), g(N * U * H), out(N * T * U * H), dout(N * T * U * H), df(N * T * H), dg(N * U * H);
    std::vector<int> ranges(N * T), xl(N, T), yl(N, U - 1);
    std::vector<long long> offs(N + 1);
    std::vector<char> ws(4096);
    const rnntOptions o = opts();
#define FWD(f_, g_, out_, layout, act, rg, s, of, yl_, xl_, t, u, h, n_, ws_, o_, code) \
    compute_rnnt_joiner_fwd(f_, g_, out_, layout, act, rg, s, of, yl_, xl_, t, u, h, n_, ws_, o_, code)
#define BWD(out_, dout_, df_, dg_, layout, act, rg, s, of, yl_, xl_, t, u, h, n_, ws_, o_, code) \
    compute_rnnt_joiner_bwd(out_, dout_, df_, dg_, layout, act, rg, s, of, yl_, xl_, t, u, h, n_, ws_, o_, code)
    float *F = f.data(), *G = g.data(), *O = out.data(), *DO = dout.data(), *DF = df.data(), *DG = dg.data();
    int *RG = ranges.data(), *XL = xl.data(), *YL = yl.data();
    long long* OF = offs.data();
    void* WS = ws.data();

    // forward: NULL where a pointer is required
    REFUSED(FWD(nullptr, G, O, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(FWD(F, nullptr, O, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(FWD(F, G, nullptr, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(FWD(F, G, O, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, nullptr, o, 0));
    REFUSED(FWD(F, G, O, 2, 2, nullptr, S, nullptr, nullptr, XL, T, U, H, N, WS, o, 0));          // layout 2 without ranges
    REFUSED(FWD(F, G, O, 1, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));               // layout 1 without offsets
    REFUSED(FWD(F, G, O, 1, 2, nullptr, 0, OF, nullptr, XL, T, U, H, N, WS, o, 0));               // ... without label lengths
    REFUSED(FWD(F, G, O, 1, 2, nullptr, 0, OF, YL, nullptr, T, U, H, N, WS, o, 0));               // ... without input lengths
    // a layout, act or dtype outside the set
    for (int bad : {-1, 3, 7}) {
        REFUSED(FWD(F, G, O, bad, 2, RG, S, OF, YL, XL, T, U, H, N, WS, o, 0));
        REFUSED(FWD(F, G, O, 0, bad, RG, S, OF, YL, XL, T, U, H, N, WS, o, 0));
        REFUSED(BWD(O, DO, DF, DG, bad, 2, RG, S, OF, YL, XL, T, U, H, N, WS, o, 0));
        REFUSED(BWD(O, DO, DF, DG, 0, bad, RG, S, OF, YL, XL, T, U, H, N, WS, o, 0));
    }
    for (int bad : {-1, 4}) {
        REFUSED(FWD(F, G, O, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, bad));
        REFUSED(BWD(O, DO, DF, DG, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, bad));
    }
    // S outside [1, U] in layout 2
    for (int bad : {0, -1, U + 1}) {
        REFUSED(FWD(F, G, O, 2, 2, RG, bad, nullptr, nullptr, XL, T, U, H, N, WS, o, 0));
        REFUSED(BWD(O, DO, DF, DG, 2, 2, RG, bad, nullptr, nullptr, XL, T, U, H, N, WS, o, 0));
    }
    // non-positive sizes
    for (int bad : {0, -3}) {
        REFUSED(FWD(F, G, O, 0, 2, nullptr, 0, nullptr, YL, XL, bad, U, H, N, WS, o, 0));
        REFUSED(FWD(F, G, O, 0, 2, nullptr, 0, nullptr, YL, XL, T, bad, H, N, WS, o, 0));
        REFUSED(FWD(F, G, O, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, bad, N, WS, o, 0));
        REFUSED(FWD(F, G, O, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, bad, WS, o, 0));
        REFUSED(BWD(O, DO, DF, DG, 0, 2, nullptr, 0, nullptr, YL, XL, bad, U, H, N, WS, o, 0));
        REFUSED(BWD(O, DO, DF, DG, 0, 2, nullptr, 0, nullptr, YL, XL, T, bad, H, N, WS, o, 0));
        REFUSED(BWD(O, DO, DF, DG, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, bad, N, WS, o, 0));
        REFUSED(BWD(O, DO, DF, DG, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, bad, WS, o, 0));
    }
    // more rows than an int holds
    REFUSED(FWD(F, G, O, 0, 2, nullptr, 0, nullptr, YL, XL, 1 << 15, 1 << 10, H, 1 << 6, WS, o, 0));
    // the CPU location
    REFUSED(FWD(F, G, O, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, opts(RNNT_CPU), 0));
    REFUSED(BWD(O, DO, DF, DG, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, opts(RNNT_CPU), 0));
    // backward: NULL where a pointer is required; out may be NULL for the identity only
    REFUSED(BWD(nullptr, DO, DF, DG, 0, 1, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(BWD(nullptr, DO, DF, DG, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(BWD(O, nullptr, DF, DG, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(BWD(O, DO, nullptr, DG, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(BWD(O, DO, DF, nullptr, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(BWD(O, DO, DF, DG, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, nullptr, o, 0));
    REFUSED(BWD(O, DO, DF, DG, 2, 2, nullptr, S, nullptr, nullptr, XL, T, U, H, N, WS, o, 0));
    REFUSED(BWD(O, DO, DF, DG, 1, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    // dout overlapping df or dg (first byte, last byte), df overlapping dg
    REFUSED(BWD(O, DO, DO, DG, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(BWD(O, DO, DF, DO, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(BWD(O, DO, DO + N * T * U * H - 1, DG, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(BWD(O, DO + N * U * H - 1, DF, DO, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(BWD(O, DO, DF, DF, 0, 2, nullptr, 0, nullptr, YL, XL, T, U, H, N, WS, o, 0));
    REFUSED(BWD(O, DO, DO, DG, 1, 2, nullptr, 0, OF, YL, XL, T, U, H, N, WS, o, 0));               // packed: the first row of dout
    REFUSED(BWD(O, DO, DF, DO + H - 1, 1, 2, nullptr, 0, OF, YL, XL, T, U, H, N, WS, o, 0));

    if (failures == 0) std::printf("test_joiner_args: all refused\n");
    return failures == 0 ? 0 : 1;
}
