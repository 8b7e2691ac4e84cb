// test_ranges_args.cpp -- the host driver of libwarprnnt_ranges.so under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// program of its own (`make side-asan` builds the library's three translation units with the sanitizers on the host side and
// links them with this file; it needs no GPU): the argument refusals of the two entries of include/rnnt_ranges.h, all of
// which return before anything is launched.  The pointers handed over are never dereferenced on these paths.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/rnnt_ranges.h"

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
    constexpr int B = 2, S = 3, T = 4, R = 3, ST = 2;
    const size_t nx = B * S * (T + 1) + 4, ny = B * (S + 1) * T + 4;
    std::vector<double> px(nx), py(ny), kept(B * T + 2);
    std::vector<int> ranges(B * T + 2);
    std::vector<long long> bd(B * 4, 0);
    const rnntOptions ok = opts();
    const void *x = px.data(), *y = py.data(), *b = bd.data();
    int* rg = ranges.data();
    double* kp = kept.data();
    for (int mod = 0; mod <= 1; ++mod) {
        // NULL pointers (boundary may be NULL)
        REFUSED(compute_rnnt_prune_ranges_occ(nullptr, y, b, S, T, B, mod, R, ST, rg, ok, 0));
        REFUSED(compute_rnnt_prune_ranges_occ(x, nullptr, b, S, T, B, mod, R, ST, rg, ok, 0));
        REFUSED(compute_rnnt_prune_ranges_occ(x, y, nullptr, S, T, B, mod, R, ST, nullptr, ok, 0));
        REFUSED(compute_rnnt_range_coverage(nullptr, y, b, rg, S, T, B, mod, R, kp, ok, 0));
        REFUSED(compute_rnnt_range_coverage(x, nullptr, b, rg, S, T, B, mod, R, kp, ok, 0));
        REFUSED(compute_rnnt_range_coverage(x, y, b, nullptr, S, T, B, mod, R, kp, ok, 0));
        REFUSED(compute_rnnt_range_coverage(x, y, nullptr, rg, S, T, B, mod, R, nullptr, ok, 0));
        // S == 0: px_grad is not looked at, the other pointers are
        REFUSED(compute_rnnt_prune_ranges_occ(nullptr, nullptr, b, 0, T, B, mod, 1, 1, rg, ok, 0));
        REFUSED(compute_rnnt_prune_ranges_occ(nullptr, y, b, 0, T, B, mod, 1, 1, nullptr, ok, 0));
        REFUSED(compute_rnnt_range_coverage(nullptr, y, b, rg, 0, T, B, mod, 1, nullptr, ok, 0));
        // sizes and mi's limits: S + 1 <= 4096, (T + 1) (S + 1) < 2^25, B (T + 1) (S + 1) < 2^32
        const int bad_dims[][3] = {{-1, T, B}, {S, 0, B}, {S, -2, B}, {S, T, 0}, {S, T, -3}, {4096, T, B}, {4095, (1 << 13) - 1, B},
                                   {0, (1 << 25) - 1, 1}, {15, (1 << 12) - 1, 1 << 16}, {3, 1, 1 << 29}};
        for (const auto& d : bad_dims) {
            for (int code = 0; code <= 3; ++code) {
                REFUSED(compute_rnnt_prune_ranges_occ(x, y, b, d[0], d[1], d[2], mod, 1, 1, rg, ok, code));
                REFUSED(compute_rnnt_range_coverage(x, y, b, rg, d[0], d[1], d[2], mod, 1, kp, ok, code));
            }
        }
        // R outside [1, S + 1]; step outside [1, max(1, R - 1)]
        for (int r : {0, -1, S + 2, 1 << 20}) {
            REFUSED(compute_rnnt_prune_ranges_occ(x, y, b, S, T, B, mod, r, 1, rg, ok, 0));
            REFUSED(compute_rnnt_range_coverage(x, y, b, rg, S, T, B, mod, r, kp, ok, 0));
        }
        const int bad_steps[][2] = {{R, 0}, {R, -1}, {R, R}, {R, 1 << 20}, {1, 2}, {1, 0}, {2, 2}, {S + 1, S + 1}};
        for (const auto& rs : bad_steps) REFUSED(compute_rnnt_prune_ranges_occ(x, y, b, S, T, B, mod, rs[0], rs[1], rg, ok, 0));
        // the CPU location, dtype codes
        REFUSED(compute_rnnt_prune_ranges_occ(x, y, b, S, T, B, mod, R, ST, rg, opts(RNNT_CPU), 0));
        REFUSED(compute_rnnt_range_coverage(x, y, b, rg, S, T, B, mod, R, kp, opts(RNNT_CPU), 0));
        for (int code : {-1, 4}) {
            REFUSED(compute_rnnt_prune_ranges_occ(x, y, b, S, T, B, mod, R, ST, rg, ok, code));
            REFUSED(compute_rnnt_range_coverage(x, y, b, rg, S, T, B, mod, R, kp, ok, code));
        }
        for (int code = 0; code <= 3; ++code) {
            const size_t esz = code == 1 ? 8 : code == 0 ? 4 : 2;
            // buffers off their element boundary
            const char *xc = reinterpret_cast<const char*>(x), *yc = reinterpret_cast<const char*>(y);
            const char* bc = reinterpret_cast<const char*>(b);
            char *rc = reinterpret_cast<char*>(rg), *kc = reinterpret_cast<char*>(kp);
            REFUSED(compute_rnnt_prune_ranges_occ(xc + 1, y, b, S, T, B, mod, R, ST, rg, ok, code));
            REFUSED(compute_rnnt_prune_ranges_occ(x, yc + 1, b, S, T, B, mod, R, ST, rg, ok, code));
            REFUSED(compute_rnnt_prune_ranges_occ(x, y, bc + 4, S, T, B, mod, R, ST, rg, ok, code));
            REFUSED(compute_rnnt_prune_ranges_occ(x, y, b, S, T, B, mod, R, ST, reinterpret_cast<int*>(rc + 2), ok, code));
            REFUSED(compute_rnnt_range_coverage(xc + 1, y, b, rg, S, T, B, mod, R, kp, ok, code));
            REFUSED(compute_rnnt_range_coverage(x, yc + 1, b, rg, S, T, B, mod, R, kp, ok, code));
            REFUSED(compute_rnnt_range_coverage(x, y, bc + 4, rg, S, T, B, mod, R, kp, ok, code));
            REFUSED(compute_rnnt_range_coverage(x, y, b, reinterpret_cast<const int*>(rc + 2), S, T, B, mod, R, kp, ok, code));
            REFUSED(compute_rnnt_range_coverage(x, y, b, rg, S, T, B, mod, R, reinterpret_cast<double*>(kc + 4), ok, code));
            // an output that overlaps an input: its first and its last element
            const size_t xbytes = size_t(B) * S * (mod ? T : T + 1) * esz, ybytes = size_t(B) * (S + 1) * T * esz;
            void* inside[] = {const_cast<char*>(xc), const_cast<char*>(xc) + xbytes - 8, const_cast<char*>(yc),
                              const_cast<char*>(yc) + ybytes - 8, bd.data(), const_cast<char*>(bc) + B * 4 * sizeof(long long) - 8};
            for (void* g : inside) {
                REFUSED(compute_rnnt_prune_ranges_occ(x, y, b, S, T, B, mod, R, ST, static_cast<int*>(g), ok, code));
                REFUSED(compute_rnnt_range_coverage(x, y, b, rg, S, T, B, mod, R, static_cast<double*>(g), ok, code));
            }
            REFUSED(compute_rnnt_range_coverage(x, y, b, rg, S, T, B, mod, R, reinterpret_cast<double*>(rg), ok, code));
            REFUSED(compute_rnnt_range_coverage(x, y, b, rg, S, T, B, mod, R, reinterpret_cast<double*>(rc + B * T * 4 - 8), ok, code));
            // ... and ends just before it
            REFUSED(compute_rnnt_prune_ranges_occ(x, y, b, S, T, B, mod, R, ST,
                                                  reinterpret_cast<int*>(const_cast<char*>(yc) - B * T * 4 + 4), ok, code));
        }
    }
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("prune ranges from occupations argument checks: all refused as include/rnnt_ranges.h says\n");
    return 0;
}
