// test_bestpath_args.cpp -- the host driver of libwarprnnt_bestpath.so under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// program of its own (`make side-asan` builds the library's three translation units with the sanitizers on the host side and
// links them with this file; it needs no GPU): the argument refusals of the two entries of include/rnnt_bestpath.h, all of
// which return before anything is launched.  Left out: what only a finished kernel can tell (a boundary outside the
// tensor).  The pointers handed over are never dereferenced on these paths.
#include <cstdio>
#include <vector>

#include "../../include/rnnt_bestpath.h"

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)
#define REFUSED(call) EXPECT((call) == RNNT_STATUS_INVALID_VALUE)

static rnntOptions opts(rnntComputeLocation loc = RNNT_GPU) {
    rnntOptions o{};
    o.loc = loc;
    return o;
}

int main() {
    constexpr int B = 2, S = 3, T = 4, W = 1;                      // W = ceil((T + 1) / 64) words of a row of back
    std::vector<double> px(B * S * (T + 1) + 4), py(B * (S + 1) * T + 4), ex(B * S * (T + 1) + 4), ey(B * (S + 1) * T + 4);
    std::vector<double> scores(B + 1), scale(B, 1.0);
    std::vector<long long> bd(B * 4, 0);
    std::vector<int> frames(B * S + 2);
    std::vector<unsigned long long> back(B * (S + 1) * W + 2);
    const rnntOptions ok = opts();
    const void *x = px.data(), *y = py.data(), *b = bd.data();
    void *dx = ex.data(), *dy = ey.data(), *sc = scores.data(), *bk = back.data();
    int* fr = frames.data();
    for (int mod = 0; mod <= 1; ++mod) {
        // NULL pointers (boundary may be NULL; both indicators may be NULL)
        REFUSED(compute_rnnt_bestpath(nullptr, y, b, S, T, B, mod, sc, fr, bk, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath(x, nullptr, b, S, T, B, mod, sc, fr, bk, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, nullptr, fr, bk, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, nullptr, bk, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, nullptr, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath(x, y, nullptr, S, T, B, mod, sc, fr, nullptr, nullptr, nullptr, ok, 0));
        // one indicator array without the other
        REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bk, dx, nullptr, ok, 0));
        REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bk, nullptr, dy, ok, 0));
        // sizes, the CPU location, dtype codes
        REFUSED(compute_rnnt_bestpath(x, y, b, -1, T, B, mod, sc, fr, bk, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath(x, y, b, S, 0, B, mod, sc, fr, bk, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath(x, y, b, S, T, 0, mod, sc, fr, bk, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath(x, y, b, S, T, -3, mod, sc, fr, bk, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bk, dx, dy, opts(RNNT_CPU), 0));
        for (int code : {-1, 4}) REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bk, dx, dy, ok, code));
        for (int code = 0; code <= 3; ++code) {
            const size_t esz = code == 1 ? 8 : code == 0 ? 4 : 2;
            // the limits: S + 1 past 4096, (T + 1) (S + 1) >= 2^25, B (T + 1) (S + 1) >= 2^32
            REFUSED(compute_rnnt_bestpath(x, y, b, 4096, T, B, mod, sc, fr, bk, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, 4095, (1 << 13) - 1, B, mod, sc, fr, bk, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, 15, (1 << 12) - 1, 1 << 16, mod, sc, fr, bk, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), 4096, T, B, mod, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), 15, (1 << 12) - 1, 1 << 16, mod, dx, dy, ok, code));
            // buffers off their element boundary
            const char *xc = reinterpret_cast<const char*>(x), *yc = reinterpret_cast<const char*>(y);
            char *dxc = reinterpret_cast<char*>(dx), *dyc = reinterpret_cast<char*>(dy), *scc = reinterpret_cast<char*>(sc);
            char *bkc = reinterpret_cast<char*>(bk), *frc = reinterpret_cast<char*>(fr);
            REFUSED(compute_rnnt_bestpath(xc + 1, y, b, S, T, B, mod, sc, fr, bk, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, yc + 1, b, S, T, B, mod, sc, fr, bk, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, reinterpret_cast<const char*>(b) + 4, S, T, B, mod, sc, fr, bk, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, scc + 4, fr, bk, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, reinterpret_cast<int*>(frc + 2), bk, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bkc + 4, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bk, dxc + 1, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bk, dx, dyc + 1, ok, code));
            REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), S, T, B, mod, dxc + 1, dy, ok, code));
            REFUSED(compute_rnnt_bestpath_edges(fr, scc + 4, b, scale.data(), S, T, B, mod, dx, dy, ok, code));
            // outputs that overlap an input (its first and its last element), the boundary or each other
            const size_t xbytes = size_t(B) * S * (mod ? T : T + 1) * esz, ybytes = size_t(B) * (S + 1) * T * esz;
            void* inside[] = {const_cast<char*>(xc), const_cast<char*>(xc) + xbytes - esz, const_cast<char*>(yc),
                              const_cast<char*>(yc) + ybytes - esz, bd.data(),
                              reinterpret_cast<char*>(bd.data()) + B * 4 * sizeof(long long) - 8};
            for (void* g : inside) {
                REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bk, g, dy, ok, code));
                REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bk, dx, g, ok, code));
                REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, g, fr, bk, dx, dy, ok, code));
                REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, static_cast<int*>(g), bk, dx, dy, ok, code));
                REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, g, dx, dy, ok, code));
                REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, g, nullptr, nullptr, ok, code));
            }
            REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bk, dx, dxc + xbytes - esz, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bk, dyc + ybytes - esz, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, sc, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, bkc + 8, fr, bk, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, frc + 8, dx, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bk, bk, dy, ok, code));
            REFUSED(compute_rnnt_bestpath(x, y, b, S, T, B, mod, sc, fr, bk, dx, fr, ok, code));
            // the edges entry: an output inside frames, the scores, the boundary, the scale or the other output
            REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), S, T, B, mod, fr, dy, ok, code));
            REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), S, T, B, mod, dx, sc, ok, code));
            REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), S, T, B, mod, bd.data(), dy, ok, code));
            REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), S, T, B, mod, dx, scale.data(), ok, code));
            REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), S, T, B, mod, dx, dxc + esz, ok, code));
        }
        // the edges entry: NULL pointers (boundary and scale may be NULL), sizes, location, dtype codes
        REFUSED(compute_rnnt_bestpath_edges(nullptr, sc, b, scale.data(), S, T, B, mod, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath_edges(fr, nullptr, b, scale.data(), S, T, B, mod, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), S, T, B, mod, nullptr, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), S, T, B, mod, dx, nullptr, ok, 0));
        REFUSED(compute_rnnt_bestpath_edges(fr, sc, nullptr, nullptr, S, T, B, mod, nullptr, nullptr, ok, 0));
        REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), -1, T, B, mod, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), S, 0, B, mod, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), S, T, 0, mod, dx, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), S, T, B, mod, dx, dy, opts(RNNT_CPU), 0));
        for (int code : {-1, 4}) REFUSED(compute_rnnt_bestpath_edges(fr, sc, b, scale.data(), S, T, B, mod, dx, dy, ok, code));
        // S == 0: px, frames and px_path are not looked at, the other pointers are
        REFUSED(compute_rnnt_bestpath(nullptr, nullptr, b, 0, T, B, mod, sc, nullptr, bk, nullptr, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath(nullptr, y, b, 0, T, B, mod, sc, nullptr, nullptr, nullptr, dy, ok, 0));
        REFUSED(compute_rnnt_bestpath_edges(nullptr, sc, b, nullptr, 0, T, B, mod, nullptr, nullptr, ok, 0));
    }
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("best path on px / py argument checks: all refused as include/rnnt_bestpath.h says\n");
    return 0;
}
