// test_expect_args.cpp -- the host driver of libwarprnnt_expect.so under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// program of its own (`make side-asan` builds the library's three translation units with the sanitizers on the host side and
// links them with this file; it needs no GPU): the argument refusals of the three entries of include/rnnt_expect.h, all of
// which return before anything is launched.  Left out: what only a finished kernel can tell (a boundary outside the
// tensor).  The pointers handed over are never dereferenced on these paths.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/rnnt_expect.h"

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
    constexpr int B = 2, S = 3, T = 4;
    const size_t nx = B * S * (T + 1) + 4, ny = B * (S + 1) * T + 4;
    std::vector<double> px(nx), py(ny), cx(nx), cy(ny), gx(nx), gy(ny), hx(nx), hy(ny);
    std::vector<double> scores(B + 2), expect(B + 2), ge(B, 1.0), gs(B, 0.0);
    std::vector<double> nodes(B * (S + 1) * (T + 1) * 2 + 4);
    std::vector<long long> bd(B * 4, 0);
    const rnntOptions ok = opts();
    const void *x = px.data(), *y = py.data(), *kx = cx.data(), *ky = cy.data(), *b = bd.data();
    void *dx = gx.data(), *dy = gy.data(), *ex = hx.data(), *ey = hy.data(), *sc = scores.data(), *ec = expect.data();
    // the pair (a, A) is the element of nodes: a 16-byte boundary
    char* ndc = reinterpret_cast<char*>(nodes.data());
    ndc += (16 - reinterpret_cast<uintptr_t>(ndc) % 16) % 16;
    void* nd = ndc;
    const double *e1 = ge.data(), *s1 = gs.data();
    for (int mod = 0; mod <= 1; ++mod) {
        // NULL pointers (boundary may be NULL; the four gradients may all be NULL, the cost gradients may both be NULL)
        REFUSED(compute_rnnt_expect(nullptr, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, nullptr, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, nullptr, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, nullptr, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, nullptr, ec, nd, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, nullptr, nd, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nullptr, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, ky, nullptr, S, T, B, mod, sc, ec, nullptr, nullptr, nullptr, nullptr, nullptr, ok, 0));
        // one gradient of a pair without the other; cost gradients without weight gradients
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, nullptr, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, nullptr, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, nullptr, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, nullptr, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, nullptr, nullptr, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, ex, nullptr, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, nullptr, ey, ok, 0));
        // sizes, the CPU location, dtype codes
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, -1, T, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, 0, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, 0, mod, sc, ec, nd, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, -3, mod, sc, ec, nd, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, ey, opts(RNNT_CPU), 0));
        REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, opts(RNNT_CPU), 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, ex, ey, opts(RNNT_CPU), 0));
        for (int code : {-1, 4}) {
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, ex, ey, ok, code));
        }
        for (int code = 0; code <= 3; ++code) {
            const size_t esz = code == 1 ? 8 : code == 0 ? 4 : 2;
            // the limits: S + 1 past 1024, (T + 1) (S + 1) >= 2^25, B (T + 1) (S + 1) >= 2^32
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, 1024, T, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, 1023, (1 << 15) - 1, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, 15, (1 << 12) - 1, 1 << 16, mod, sc, ec, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, 1024, T, B, mod, sc, ec, nd, ok, code));
            REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, 15, (1 << 12) - 1, 1 << 16, mod, sc, ec, nd, ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, 1024, T, B, mod, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, 1023, (1 << 15) - 1, B, mod, dx, dy, ex, ey, ok, code));
            // buffers off their element boundary
            const char *xc = reinterpret_cast<const char*>(x), *yc = reinterpret_cast<const char*>(y);
            const char *kxc = reinterpret_cast<const char*>(kx), *kyc = reinterpret_cast<const char*>(ky);
            char *dxc = reinterpret_cast<char*>(dx), *dyc = reinterpret_cast<char*>(dy), *exc = reinterpret_cast<char*>(ex);
            char *eyc = reinterpret_cast<char*>(ey), *scc = reinterpret_cast<char*>(sc), *ecc = reinterpret_cast<char*>(ec);
            REFUSED(compute_rnnt_expect(xc + 1, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, yc + 1, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kxc + 1, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, kyc + 1, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, reinterpret_cast<const char*>(b) + 4, S, T, B, mod, sc, ec, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, scc + 4, ec, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ecc + 4, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, ndc + 8, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dxc + 1, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dyc + 1, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, exc + 1, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, eyc + 1, ok, code));
            REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, S, T, B, mod, sc, ec, ndc + 8, ok, code));
            REFUSED(compute_rnnt_expect_fwd(xc + 1, y, kx, ky, b, S, T, B, mod, sc, ec, nd, ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, ndc + 8, sc, ec, e1, s1, S, T, B, mod, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, scc + 4, ec, e1, s1, S, T, B, mod, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, reinterpret_cast<const char*>(e1) + 4, s1, S, T, B, mod, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dxc + 1, dy, ex, ey, ok, code));
            // outputs that overlap an input (its first and its last element), the boundary or each other
            const size_t xbytes = size_t(B) * S * (mod ? T : T + 1) * esz, ybytes = size_t(B) * (S + 1) * T * esz;
            void* inside[] = {const_cast<char*>(xc), const_cast<char*>(xc) + xbytes - esz, const_cast<char*>(yc),
                              const_cast<char*>(yc) + ybytes - esz, const_cast<char*>(kxc), const_cast<char*>(kxc) + xbytes - esz,
                              const_cast<char*>(kyc), const_cast<char*>(kyc) + ybytes - esz, bd.data(),
                              reinterpret_cast<char*>(bd.data()) + B * 4 * sizeof(long long) - 8};
            for (void* g : inside) {
                REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, g, dy, ex, ey, ok, code));
                REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, g, ex, ey, ok, code));
                REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, g, ey, ok, code));
                REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, g, ok, code));
                REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, g, ec, nd, dx, dy, ex, ey, ok, code));
                REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, g, nd, dx, dy, ex, ey, ok, code));
                REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, S, T, B, mod, g, ec, nd, ok, code));
                REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, g, dy, ex, ey, ok, code));
                REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, ex, g, ok, code));
            }
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, const_cast<double*>(px.data()), dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dxc + xbytes - esz, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, dxc, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, dx, dy, ex, dyc + ybytes - esz, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, sc, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, scc + 8, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, nd, ec, nd, dx, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect(x, y, kx, ky, b, S, T, B, mod, sc, ec, nd, nd, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, S, T, B, mod, sc, sc, nd, ok, code));
            REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, S, T, B, mod, sc, ec, sc, ok, code));
            // the backward entry: an output inside nodes, the scalars, the scales or another output
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, nd, dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, sc, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, ec, ey, ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, ex, ge.data(), ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, gs.data(), dy, ex, ey, ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, dx, ey, ok, code));
            REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, ex, dyc + esz, ok, code));
        }
        // the forward and backward entries: NULL pointers (boundary and the scales may be NULL)
        REFUSED(compute_rnnt_expect_fwd(nullptr, y, kx, ky, b, S, T, B, mod, sc, ec, nd, ok, 0));
        REFUSED(compute_rnnt_expect_fwd(x, nullptr, kx, ky, b, S, T, B, mod, sc, ec, nd, ok, 0));
        REFUSED(compute_rnnt_expect_fwd(x, y, nullptr, ky, b, S, T, B, mod, sc, ec, nd, ok, 0));
        REFUSED(compute_rnnt_expect_fwd(x, y, kx, nullptr, b, S, T, B, mod, sc, ec, nd, ok, 0));
        REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, S, T, B, mod, nullptr, ec, nd, ok, 0));
        REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, S, T, B, mod, sc, nullptr, nd, ok, 0));
        REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, nullptr, S, T, B, mod, sc, ec, nullptr, ok, 0));
        REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, -1, T, B, mod, sc, ec, nd, ok, 0));
        REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, S, 0, B, mod, sc, ec, nd, ok, 0));
        REFUSED(compute_rnnt_expect_fwd(x, y, kx, ky, b, S, T, 0, mod, sc, ec, nd, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(nullptr, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, nullptr, kx, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, nullptr, ky, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, kx, nullptr, b, nd, sc, ec, e1, s1, S, T, B, mod, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nullptr, sc, ec, e1, s1, S, T, B, mod, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, nullptr, ec, e1, s1, S, T, B, mod, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, nullptr, e1, s1, S, T, B, mod, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, nullptr, nd, sc, ec, nullptr, nullptr, S, T, B, mod, nullptr, dy, nullptr, nullptr, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, nullptr, nd, sc, ec, nullptr, nullptr, S, T, B, mod, dx, nullptr, nullptr, nullptr, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, -1, T, B, mod, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, 0, B, mod, dx, dy, ex, ey, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(x, y, kx, ky, b, nd, sc, ec, e1, s1, S, T, 0, mod, dx, dy, ex, ey, ok, 0));
        // S == 0: px, cx and their gradients are not looked at, the other pointers are
        REFUSED(compute_rnnt_expect(nullptr, nullptr, nullptr, ky, b, 0, T, B, mod, sc, ec, nd, nullptr, dy, nullptr, ey, ok, 0));
        REFUSED(compute_rnnt_expect(nullptr, y, nullptr, nullptr, b, 0, T, B, mod, sc, ec, nd, nullptr, dy, nullptr, ey, ok, 0));
        REFUSED(compute_rnnt_expect(nullptr, y, nullptr, ky, b, 0, T, B, mod, sc, ec, nullptr, nullptr, dy, nullptr, ey, ok, 0));
        REFUSED(compute_rnnt_expect(nullptr, y, nullptr, ky, b, 0, T, B, mod, sc, ec, nd, nullptr, nullptr, nullptr, ey, ok, 0));
        REFUSED(compute_rnnt_expect_bwd(nullptr, y, nullptr, ky, b, nd, sc, ec, e1, s1, 0, T, B, mod, nullptr, nullptr, nullptr, nullptr, ok, 0));
    }
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("expected cost on px / py argument checks: all refused as include/rnnt_expect.h says\n");
    return 0;
}
