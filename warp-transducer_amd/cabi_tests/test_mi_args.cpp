// test_mi_args.cpp -- the host driver of libwarprnnt_mi.so under AddressSanitizer + UndefinedBehaviorSanitizer, as a program
// of its own (`make side-asan` builds the library's three translation units with the sanitizers on the host side and links
// them with this file; it needs no GPU): the workspace arithmetic of get_workspace_size_mi and the argument refusals of the
// three compute entries of include/rnnt_mi.h, all of which return before anything is launched.  Left out: what only a
// finished kernel can tell (a boundary outside the tensor).  The pointers handed over are never dereferenced on these
// paths.
#include <cstdio>
#include <vector>

#include "../../include/rnnt_mi.h"

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
    // sizes: one per dtype code and type; the fp64 lattice needs more than the fp32 one, 16-bit storage the fp32 lattice's;
    // the regular type's table has T + 1 node columns and an offset per diagonal, the modified type's T and one per frame
    size_t n = 0, r32 = 0, r64 = 0, m32 = 0, n1 = 0;
    EXPECT(get_workspace_size_mi(20, 150, 128, 0, 0, &r32) == RNNT_STATUS_SUCCESS && r32 > 0);
    EXPECT(get_workspace_size_mi(20, 150, 128, 0, 1, &r64) == RNNT_STATUS_SUCCESS && r64 > r32);
    EXPECT(get_workspace_size_mi(20, 150, 128, 0, 2, &n) == RNNT_STATUS_SUCCESS && n == r32);
    EXPECT(get_workspace_size_mi(20, 150, 128, 0, 3, &n) == RNNT_STATUS_SUCCESS && n == r32);
    EXPECT(get_workspace_size_mi(20, 150, 128, 1, 0, &m32) == RNNT_STATUS_SUCCESS && m32 < r32);
    EXPECT(get_workspace_size_mi(20, 150, 128, 7, 0, &n) == RNNT_STATUS_SUCCESS && n == m32);      // any nonzero: modified
    const size_t slack = 12 * 256 + 128 * 64;                       // thirteen aligned arrays and the base's alignment
    {
        const size_t cells = size_t(128) * 151 * 21, offs = size_t(128) * (151 + 21) * 2 * sizeof(double);
        const size_t own = 128 * (4 * sizeof(int) + 3 * sizeof(double));           // lengths, origins; ll, costs, scores
        EXPECT(r32 >= cells * 4 * (4 + 1 + 1) + offs + own && r32 < cells * 4 * (4 + 1 + 1) + offs + own + 128 * 4 + slack);
        EXPECT(r64 >= cells * 8 * (4 + 1 + 1) + offs + own);
    }
    {
        const size_t cells = size_t(128) * 150 * 21, offs = size_t(128) * (150 + 1) * 2 * sizeof(double);
        EXPECT(m32 >= cells * 4 * (4 + 1 + 1) + offs && m32 < cells * 4 * (4 + 1 + 1) + offs + 128 * 48 + slack);
    }
    EXPECT(get_workspace_size_mi(20, 151, 128, 0, 0, &n) == RNNT_STATUS_SUCCESS && n > r32);
    EXPECT(get_workspace_size_mi(21, 150, 128, 0, 0, &n) == RNNT_STATUS_SUCCESS && n > r32);
    EXPECT(get_workspace_size_mi(20, 150, 129, 0, 0, &n) == RNNT_STATUS_SUCCESS && n > r32);
    EXPECT(get_workspace_size_mi(0, 1, 1, 0, 0, &n1) == RNNT_STATUS_SUCCESS && n1 >= 2 * 4 * 6 + 3 * 2 * sizeof(double));
    EXPECT(get_workspace_size_mi(0, 1, 1, 1, 0, &n) == RNNT_STATUS_SUCCESS && n > 0 && n <= n1);
    EXPECT(get_workspace_size_mi(4095, 1 << 15, 1 << 15, 0, 1, &n) == RNNT_STATUS_SUCCESS && n > (size_t(1) << 40));
    REFUSED(get_workspace_size_mi(-1, 3, 2, 0, 0, &n));
    REFUSED(get_workspace_size_mi(4, 0, 2, 0, 0, &n));
    REFUSED(get_workspace_size_mi(4, 3, 0, 0, 0, &n));
    REFUSED(get_workspace_size_mi(4, 3, 2, 0, -1, &n));
    REFUSED(get_workspace_size_mi(4, 3, 2, 0, 4, &n));
    REFUSED(get_workspace_size_mi(4, 3, 2, 0, 0, nullptr));

    constexpr int B = 2, S = 3, T = 4;
    std::vector<double> px(B * S * (T + 1) + 4), py(B * (S + 1) * T + 4), gx(B * S * (T + 1) + 4), gy(B * (S + 1) * T + 4);
    std::vector<double> scores(B), scale(B, 1.0);
    std::vector<long long> bd(B * 4, 0);
    EXPECT(get_workspace_size_mi(S, T, B, 0, 1, &n) == RNNT_STATUS_SUCCESS);
    std::vector<char> ws(n);
    const rnntOptions ok = opts();
    const void *x = px.data(), *y = py.data(), *b = bd.data();
    void *dx = gx.data(), *dy = gy.data(), *sc = scores.data(), *w = ws.data();
    for (int mod = 0; mod <= 1; ++mod) {
        // the one-call entry: NULL pointers (boundary may be NULL; both gradients may be NULL: score only)
        REFUSED(compute_rnnt_mi(nullptr, y, b, S, T, B, mod, sc, dx, dy, w, ok, 0));
        REFUSED(compute_rnnt_mi(x, nullptr, b, S, T, B, mod, sc, dx, dy, w, ok, 0));
        REFUSED(compute_rnnt_mi(x, y, b, S, T, B, mod, nullptr, dx, dy, w, ok, 0));
        REFUSED(compute_rnnt_mi(x, y, b, S, T, B, mod, sc, dx, dy, nullptr, ok, 0));
        // one gradient without the other
        REFUSED(compute_rnnt_mi(x, y, b, S, T, B, mod, sc, dx, nullptr, w, ok, 0));
        REFUSED(compute_rnnt_mi(x, y, b, S, T, B, mod, sc, nullptr, dy, w, ok, 0));
        // sizes, the CPU location, dtype codes
        REFUSED(compute_rnnt_mi(x, y, b, -1, T, B, mod, sc, dx, dy, w, ok, 0));
        REFUSED(compute_rnnt_mi(x, y, b, S, 0, B, mod, sc, dx, dy, w, ok, 0));
        REFUSED(compute_rnnt_mi(x, y, b, S, T, 0, mod, sc, dx, dy, w, ok, 0));
        REFUSED(compute_rnnt_mi(x, y, b, S, T, B, mod, sc, dx, dy, w, opts(RNNT_CPU), 0));
        for (int code : {-1, 4}) REFUSED(compute_rnnt_mi(x, y, b, S, T, B, mod, sc, dx, dy, w, ok, code));
        for (int code = 0; code <= 3; ++code) {
            const size_t esz = code == 1 ? 8 : code == 0 ? 4 : 2;
            // the limits: S + 1 past 4096, (T + 1) (S + 1) >= 2^25, B (T + 1) (S + 1) >= 2^32
            REFUSED(compute_rnnt_mi(x, y, b, 4096, T, B, mod, sc, dx, dy, w, ok, code));
            REFUSED(compute_rnnt_mi(x, y, b, 4095, (1 << 13) - 1, B, mod, sc, dx, dy, w, ok, code));
            REFUSED(compute_rnnt_mi(x, y, b, 15, (1 << 12) - 1, 1 << 16, mod, sc, dx, dy, w, ok, code));
            REFUSED(compute_rnnt_mi_fwd(x, y, b, 4096, T, B, mod, sc, w, ok, code, 1));
            REFUSED(compute_rnnt_mi_bwd(dx, dy, nullptr, 4096, T, B, mod, w, ok, code));
            // tensors off their element boundary
            const char *xc = reinterpret_cast<const char*>(x), *yc = reinterpret_cast<const char*>(y);
            char *dxc = reinterpret_cast<char*>(dx), *dyc = reinterpret_cast<char*>(dy);
            REFUSED(compute_rnnt_mi(xc + 1, y, b, S, T, B, mod, sc, dx, dy, w, ok, code));
            REFUSED(compute_rnnt_mi(x, yc + 1, b, S, T, B, mod, sc, dx, dy, w, ok, code));
            REFUSED(compute_rnnt_mi(x, y, b, S, T, B, mod, sc, dxc + 1, dy, w, ok, code));
            REFUSED(compute_rnnt_mi(x, y, b, S, T, B, mod, sc, dx, dyc + 1, w, ok, code));
            REFUSED(compute_rnnt_mi(x, y, reinterpret_cast<const char*>(b) + 4, S, T, B, mod, sc, dx, dy, w, ok, code));
            // gradients that overlap an input (its first and its last element), each other, the boundary or the workspace
            const size_t xbytes = size_t(B) * S * (mod ? T : T + 1) * esz, ybytes = size_t(B) * (S + 1) * T * esz;
            size_t wsz = 0;
            EXPECT(get_workspace_size_mi(S, T, B, mod, code, &wsz) == RNNT_STATUS_SUCCESS && wsz <= ws.size());
            char* wc = reinterpret_cast<char*>(w);
            void* inside[] = {const_cast<char*>(xc), const_cast<char*>(xc) + xbytes - esz, const_cast<char*>(yc),
                              const_cast<char*>(yc) + ybytes - esz, wc, wc + wsz - esz, bd.data(),
                              reinterpret_cast<char*>(bd.data()) + B * 4 * sizeof(long long) - esz};
            for (void* g : inside) {
                REFUSED(compute_rnnt_mi(x, y, b, S, T, B, mod, sc, g, dy, w, ok, code));
                REFUSED(compute_rnnt_mi(x, y, b, S, T, B, mod, sc, dx, g, w, ok, code));
            }
            REFUSED(compute_rnnt_mi(x, y, b, S, T, B, mod, sc, dx, dxc + xbytes - esz, w, ok, code));
            REFUSED(compute_rnnt_mi(x, y, b, S, T, B, mod, sc, dyc + ybytes - esz, dy, w, ok, code));
            REFUSED(compute_rnnt_mi_bwd(wc + 64, dy, scale.data(), S, T, B, mod, w, ok, code));
            REFUSED(compute_rnnt_mi_bwd(dx, wc + wsz - esz, scale.data(), S, T, B, mod, w, ok, code));
            REFUSED(compute_rnnt_mi_bwd(dx, dxc + esz, scale.data(), S, T, B, mod, w, ok, code));
        }
        // _fwd: the same refusals
        REFUSED(compute_rnnt_mi_fwd(nullptr, y, b, S, T, B, mod, sc, w, ok, 0, 1));
        REFUSED(compute_rnnt_mi_fwd(x, nullptr, b, S, T, B, mod, sc, w, ok, 0, 1));
        REFUSED(compute_rnnt_mi_fwd(x, y, b, S, T, B, mod, nullptr, w, ok, 0, 1));
        REFUSED(compute_rnnt_mi_fwd(x, y, b, S, T, B, mod, sc, nullptr, ok, 0, 0));
        REFUSED(compute_rnnt_mi_fwd(x, y, b, S, 0, B, mod, sc, w, ok, 0, 1));
        REFUSED(compute_rnnt_mi_fwd(x, y, b, S, T, B, mod, sc, w, opts(RNNT_CPU), 0, 1));
        for (int code : {-1, 4}) REFUSED(compute_rnnt_mi_fwd(x, y, b, S, T, B, mod, sc, w, ok, code, 1));
        // _bwd
        REFUSED(compute_rnnt_mi_bwd(nullptr, dy, scale.data(), S, T, B, mod, w, ok, 0));
        REFUSED(compute_rnnt_mi_bwd(dx, nullptr, scale.data(), S, T, B, mod, w, ok, 0));
        REFUSED(compute_rnnt_mi_bwd(dx, dy, scale.data(), S, T, B, mod, nullptr, ok, 0));
        REFUSED(compute_rnnt_mi_bwd(dx, dy, scale.data(), -1, T, B, mod, w, ok, 0));
        REFUSED(compute_rnnt_mi_bwd(dx, dy, scale.data(), S, T, 0, mod, w, ok, 0));
        REFUSED(compute_rnnt_mi_bwd(dx, dy, scale.data(), S, T, B, mod, w, opts(RNNT_CPU), 0));
        for (int code : {-1, 4}) REFUSED(compute_rnnt_mi_bwd(dx, dy, scale.data(), S, T, B, mod, w, ok, code));
    }
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("lattice primitive on px / py argument checks: all refused as include/rnnt_mi.h says\n");
    return 0;
}
