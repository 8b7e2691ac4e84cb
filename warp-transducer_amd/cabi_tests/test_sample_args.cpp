// test_sample_args.cpp -- the host driver of libwarprnnt_sample.so under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// program of its own (`make side-asan` builds the library's three translation units with the sanitizers on the host side and
// links them with this file; it needs no GPU): the argument refusals of the four entries of include/rnnt_sample.h, all of
// which return before anything is launched.  Left out: what only a finished kernel can tell (a boundary outside the
// tensor, a row of frames that is no path).  The pointers handed over are never dereferenced on these paths.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/rnnt_sample.h"

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
    constexpr int B = 2, S = 3, T = 4, K = 5;
    const size_t nx = B * S * (T + 1) + 4, ny = B * (S + 1) * T + 4;
    std::vector<double> px(nx), py(ny), ax(nx), ay(ny);
    std::vector<double> scores(B + 2), alpha(B * (S + 1) * (T + 1) + 2), weights(B * K + 2), coeff(B * K + 2);
    std::vector<float> uni(B * K * (S + T) + 2);
    std::vector<int> frames(B * K * S + 2);
    std::vector<long long> bd(B * 4, 0);
    const rnntOptions ok = opts();
    const void *x = px.data(), *y = py.data(), *b = bd.data(), *cf = coeff.data();
    const float* u = uni.data();
    int* fr = frames.data();
    void *sc = scores.data(), *al = alpha.data(), *w = weights.data(), *gx = ax.data(), *gy = ay.data();
    for (int mod = 0; mod <= 1; ++mod) {
        // NULL pointers (boundary and coeff may be NULL)
        REFUSED(compute_rnnt_sample(nullptr, y, b, u, S, T, B, K, mod, sc, al, fr, w, ok, 0));
        REFUSED(compute_rnnt_sample(x, nullptr, b, u, S, T, B, K, mod, sc, al, fr, w, ok, 0));
        REFUSED(compute_rnnt_sample(x, y, b, nullptr, S, T, B, K, mod, sc, al, fr, w, ok, 0));
        REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, nullptr, al, fr, w, ok, 0));
        REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, nullptr, fr, w, ok, 0));
        REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, al, nullptr, w, ok, 0));
        REFUSED(compute_rnnt_sample(x, y, nullptr, u, S, T, B, K, mod, sc, al, fr, nullptr, ok, 0));
        REFUSED(compute_rnnt_sample_walk(nullptr, y, b, al, sc, u, S, T, B, K, mod, fr, w, ok, 0));
        REFUSED(compute_rnnt_sample_walk(x, nullptr, b, al, sc, u, S, T, B, K, mod, fr, w, ok, 0));
        REFUSED(compute_rnnt_sample_walk(x, y, b, nullptr, sc, u, S, T, B, K, mod, fr, w, ok, 0));
        REFUSED(compute_rnnt_sample_walk(x, y, b, al, nullptr, u, S, T, B, K, mod, fr, w, ok, 0));
        REFUSED(compute_rnnt_sample_walk(x, y, b, al, sc, nullptr, S, T, B, K, mod, fr, w, ok, 0));
        REFUSED(compute_rnnt_sample_walk(x, y, b, al, sc, u, S, T, B, K, mod, nullptr, w, ok, 0));
        REFUSED(compute_rnnt_sample_walk(x, y, nullptr, al, sc, u, S, T, B, K, mod, fr, nullptr, ok, 0));
        REFUSED(compute_rnnt_path_weights(nullptr, y, b, fr, S, T, B, K, mod, w, ok, 0));
        REFUSED(compute_rnnt_path_weights(x, nullptr, b, fr, S, T, B, K, mod, w, ok, 0));
        REFUSED(compute_rnnt_path_weights(x, y, b, nullptr, S, T, B, K, mod, w, ok, 0));
        REFUSED(compute_rnnt_path_weights(x, y, nullptr, fr, S, T, B, K, mod, nullptr, ok, 0));
        REFUSED(compute_rnnt_path_edges(nullptr, cf, b, S, T, B, K, mod, gx, gy, ok, 0));
        REFUSED(compute_rnnt_path_edges(fr, cf, b, S, T, B, K, mod, nullptr, gy, ok, 0));
        REFUSED(compute_rnnt_path_edges(fr, nullptr, nullptr, S, T, B, K, mod, gx, nullptr, ok, 0));
        // sizes, K, the CPU location, dtype codes
        const int bad_dims[][4] = {{-1, T, B, K}, {S, 0, B, K}, {S, T, 0, K}, {S, T, -3, K}, {S, T, B, 0}, {S, T, B, -1},
                                   {S, T, B, 1025}, {1024, T, B, K}, {1023, (1 << 15) - 1, B, K}, {15, (1 << 12) - 1, 1 << 16, 1},
                                   {1000, 4, 4096, 1024}, {0, 1, 1 << 22, 1024}};
        for (const auto& d : bad_dims) {
            for (int code = 0; code <= 3; ++code) {
                REFUSED(compute_rnnt_sample(x, y, b, u, d[0], d[1], d[2], d[3], mod, sc, al, fr, w, ok, code));
                REFUSED(compute_rnnt_sample_walk(x, y, b, al, sc, u, d[0], d[1], d[2], d[3], mod, fr, w, ok, code));
                REFUSED(compute_rnnt_path_weights(x, y, b, fr, d[0], d[1], d[2], d[3], mod, w, ok, code));
                REFUSED(compute_rnnt_path_edges(fr, cf, b, d[0], d[1], d[2], d[3], mod, gx, gy, ok, code));
            }
        }
        REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, al, fr, w, opts(RNNT_CPU), 0));
        REFUSED(compute_rnnt_sample_walk(x, y, b, al, sc, u, S, T, B, K, mod, fr, w, opts(RNNT_CPU), 0));
        REFUSED(compute_rnnt_path_weights(x, y, b, fr, S, T, B, K, mod, w, opts(RNNT_CPU), 0));
        REFUSED(compute_rnnt_path_edges(fr, cf, b, S, T, B, K, mod, gx, gy, opts(RNNT_CPU), 0));
        for (int code : {-1, 4}) {
            REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, al, fr, w, ok, code));
            REFUSED(compute_rnnt_sample_walk(x, y, b, al, sc, u, S, T, B, K, mod, fr, w, ok, code));
            REFUSED(compute_rnnt_path_weights(x, y, b, fr, S, T, B, K, mod, w, ok, code));
            REFUSED(compute_rnnt_path_edges(fr, cf, b, S, T, B, K, mod, gx, gy, ok, code));
        }
        for (int code = 0; code <= 3; ++code) {
            const size_t esz = code == 1 ? 8 : code == 0 ? 4 : 2;
            // buffers off their element boundary
            const char *xc = reinterpret_cast<const char*>(x), *yc = reinterpret_cast<const char*>(y);
            const char *bc = reinterpret_cast<const char*>(b), *uc = reinterpret_cast<const char*>(u);
            char *scc = reinterpret_cast<char*>(sc), *alc = reinterpret_cast<char*>(al), *wc = reinterpret_cast<char*>(w);
            char *frc = reinterpret_cast<char*>(fr), *gxc = reinterpret_cast<char*>(gx), *gyc = reinterpret_cast<char*>(gy);
            REFUSED(compute_rnnt_sample(xc + 1, y, b, u, S, T, B, K, mod, sc, al, fr, w, ok, code));
            REFUSED(compute_rnnt_sample(x, yc + 1, b, u, S, T, B, K, mod, sc, al, fr, w, ok, code));
            REFUSED(compute_rnnt_sample(x, y, bc + 4, u, S, T, B, K, mod, sc, al, fr, w, ok, code));
            REFUSED(compute_rnnt_sample(x, y, b, reinterpret_cast<const float*>(uc + 2), S, T, B, K, mod, sc, al, fr, w, ok, code));
            REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, scc + 4, al, fr, w, ok, code));
            REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, alc + 4, fr, w, ok, code));
            REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, al, reinterpret_cast<int*>(frc + 2), w, ok, code));
            REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, al, fr, wc + 4, ok, code));
            REFUSED(compute_rnnt_sample_walk(x, y, b, alc + 4, sc, u, S, T, B, K, mod, fr, w, ok, code));
            REFUSED(compute_rnnt_sample_walk(x, y, b, al, scc + 4, u, S, T, B, K, mod, fr, w, ok, code));
            REFUSED(compute_rnnt_path_weights(x, y, b, reinterpret_cast<const int*>(frc + 2), S, T, B, K, mod, w, ok, code));
            REFUSED(compute_rnnt_path_weights(x, y, b, fr, S, T, B, K, mod, wc + 4, ok, code));
            REFUSED(compute_rnnt_path_edges(fr, reinterpret_cast<const char*>(cf) + 4, b, S, T, B, K, mod, gx, gy, ok, code));
            REFUSED(compute_rnnt_path_edges(fr, cf, b, S, T, B, K, mod, gxc + 1, gy, ok, code));
            REFUSED(compute_rnnt_path_edges(fr, cf, b, S, T, B, K, mod, gx, gyc + 1, ok, code));
            // outputs that overlap an input (its first and its last element) or each other
            const size_t xbytes = size_t(B) * S * (mod ? T : T + 1) * esz, ybytes = size_t(B) * (S + 1) * T * esz;
            const size_t ubytes = size_t(B) * K * (S + T) * 4;
            void* inside[] = {const_cast<char*>(xc), const_cast<char*>(xc) + xbytes - 8, const_cast<char*>(yc),
                              const_cast<char*>(yc) + ybytes - 8, bd.data(), const_cast<char*>(bc) + B * 4 * sizeof(long long) - 8,
                              const_cast<char*>(uc), const_cast<char*>(uc) + ubytes - 8};
            for (void* g : inside) {
                REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, g, al, fr, w, ok, code));
                REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, g, fr, w, ok, code));
                REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, al, static_cast<int*>(g), w, ok, code));
                REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, al, fr, g, ok, code));
                REFUSED(compute_rnnt_sample_walk(x, y, b, al, sc, u, S, T, B, K, mod, static_cast<int*>(g), w, ok, code));
                REFUSED(compute_rnnt_sample_walk(x, y, b, al, sc, u, S, T, B, K, mod, fr, g, ok, code));
            }
            REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, sc, fr, w, ok, code));
            REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, al, fr, sc, ok, code));
            REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, al, reinterpret_cast<int*>(w), w, ok, code));
            REFUSED(compute_rnnt_sample(x, y, b, u, S, T, B, K, mod, sc, al, fr, alc + 8, ok, code));
            REFUSED(compute_rnnt_sample_walk(x, y, b, al, sc, u, S, T, B, K, mod, fr, al, ok, code));
            REFUSED(compute_rnnt_sample_walk(x, y, b, al, sc, u, S, T, B, K, mod, fr, sc, ok, code));
            REFUSED(compute_rnnt_sample_walk(x, y, b, al, sc, u, S, T, B, K, mod, reinterpret_cast<int*>(w), w, ok, code));
            REFUSED(compute_rnnt_path_weights(x, y, b, fr, S, T, B, K, mod, fr, ok, code));
            REFUSED(compute_rnnt_path_weights(x, y, b, fr, S, T, B, K, mod, const_cast<void*>(x), ok, code));
            REFUSED(compute_rnnt_path_weights(x, y, b, fr, S, T, B, K, mod, const_cast<char*>(yc) + ybytes - 8, ok, code));
            REFUSED(compute_rnnt_path_weights(x, y, b, fr, S, T, B, K, mod, bd.data(), ok, code));
            REFUSED(compute_rnnt_path_edges(fr, cf, b, S, T, B, K, mod, fr, gy, ok, code));
            REFUSED(compute_rnnt_path_edges(fr, cf, b, S, T, B, K, mod, gx, const_cast<void*>(cf), ok, code));
            REFUSED(compute_rnnt_path_edges(fr, cf, b, S, T, B, K, mod, bd.data(), gy, ok, code));
            REFUSED(compute_rnnt_path_edges(fr, cf, b, S, T, B, K, mod, gx, gx, ok, code));
            REFUSED(compute_rnnt_path_edges(fr, cf, b, S, T, B, K, mod, gx, gxc + xbytes - esz, ok, code));
        }
        // S == 0: px, px_acc, frames and uniforms are not looked at, the other pointers are
        REFUSED(compute_rnnt_sample(nullptr, nullptr, b, nullptr, 0, T, B, K, mod, sc, al, nullptr, w, ok, 0));
        REFUSED(compute_rnnt_sample(nullptr, y, b, nullptr, 0, T, B, K, mod, sc, nullptr, nullptr, w, ok, 0));
        REFUSED(compute_rnnt_sample_walk(nullptr, y, b, al, sc, nullptr, 0, T, B, K, mod, nullptr, nullptr, ok, 0));
        REFUSED(compute_rnnt_path_weights(nullptr, y, b, nullptr, 0, T, B, K, mod, nullptr, ok, 0));
        REFUSED(compute_rnnt_path_edges(nullptr, cf, b, 0, T, B, K, mod, nullptr, nullptr, ok, 0));
    }
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("alignment sampling on px / py argument checks: all refused as include/rnnt_sample.h says\n");
    return 0;
}
