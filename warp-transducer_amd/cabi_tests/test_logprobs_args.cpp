// test_logprobs_args.cpp -- the host driver of libwarprnnt_logprobs.so under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// program of its own (`make side-asan` builds the library's three translation units with the sanitizers on the host side and
// links them with this file; it needs no GPU): every refusal of include/rnnt_logprobs.h, all of which return before anything
// is launched.  The pointers handed over are never dereferenced on these paths.
#include <cstdio>
#include <vector>

#include "../../include/rnnt_logprobs.h"

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)
#define REFUSED(call) EXPECT((call) == RNNT_STATUS_INVALID_VALUE)

static rnntOptions opts(rnntComputeLocation loc = RNNT_GPU, int blank = 0) {
    rnntOptions o{};
    o.loc = loc;
    o.blank_label = blank;
    o.batch_first = true;
    return o;
}

int main() {
    // host buffers stand in for device memory: no refused call reads or writes them
    const int B = 2, T = 4, U = 3, K = 2, C = 8;
    std::vector<float> z(B * T * U * C), dz(B * T * U * C), px(B * (U - 1) * (T + 1)), py(B * U * T), lse(B * T * U);
    std::vector<float> gx(B * (U - 1) * (T + 1)), gy(B * U * T), gl(B * T * U);
    std::vector<int> sym(B * (U - 1)), rg(B * T);
    std::vector<long long> bd(B * 4);
    const rnntOptions o = opts();
    float *Z = z.data(), *DZ = dz.data(), *PX = px.data(), *PY = py.data(), *L = lse.data(), *GX = gx.data(), *GY = gy.data(),
          *GL = gl.data();
    int *SY = sym.data(), *RG = rg.data();
    long long* BD = bd.data();
#define FWD(z_, sy, rg_, k, bd_, ty, t, u, c, b, px_, py_, l_, o_, code) \
    compute_rnnt_logprobs_fwd(z_, sy, rg_, k, bd_, ty, t, u, c, b, px_, py_, l_, o_, code)
#define BWD(z_, l_, sy, rg_, k, bd_, ty, gx_, gy_, gl_, t, u, c, b, dz_, o_, code) \
    compute_rnnt_logprobs_bwd(z_, l_, sy, rg_, k, bd_, ty, gx_, gy_, gl_, t, u, c, b, dz_, o_, code)

    // forward: NULL where a pointer is required (boundary may be NULL; ranges only when K = 0)
    REFUSED(FWD(nullptr, SY, nullptr, 0, BD, 0, T, U, C, B, PX, PY, L, o, 0));
    REFUSED(FWD(Z, nullptr, nullptr, 0, BD, 0, T, U, C, B, PX, PY, L, o, 0));
    REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, B, nullptr, PY, L, o, 0));
    REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, B, PX, nullptr, L, o, 0));
    REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, B, PX, PY, nullptr, o, 0));
    REFUSED(FWD(Z, SY, nullptr, K, BD, 0, T, U, C, B, PX, PY, L, o, 0));                       // K > 0 without ranges
    // backward: the same, and the gradients
    REFUSED(BWD(nullptr, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, DZ, o, 0));
    REFUSED(BWD(Z, nullptr, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, DZ, o, 0));
    REFUSED(BWD(Z, L, nullptr, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, DZ, o, 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, nullptr, GY, GL, T, U, C, B, DZ, o, 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, nullptr, GL, T, U, C, B, DZ, o, 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, nullptr, o, 0));
    REFUSED(BWD(Z, L, SY, nullptr, K, BD, 0, GX, GY, GL, T, U, C, B, DZ, o, 0));
    // K outside {0} and [1, U]
    for (int bad : {-1, U + 1, 100}) {
        REFUSED(FWD(Z, SY, RG, bad, BD, 0, T, U, C, B, PX, PY, L, o, 0));
        REFUSED(BWD(Z, L, SY, RG, bad, BD, 0, GX, GY, GL, T, U, C, B, DZ, o, 0));
    }
    // an rnnt_type or dtype code outside its set
    for (int bad : {-1, 2, 7}) {
        REFUSED(FWD(Z, SY, nullptr, 0, BD, bad, T, U, C, B, PX, PY, L, o, 0));
        REFUSED(BWD(Z, L, SY, nullptr, 0, BD, bad, GX, GY, GL, T, U, C, B, DZ, o, 0));
    }
    for (int bad : {-1, 4}) {
        REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, B, PX, PY, L, o, bad));
        REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, DZ, o, bad));
    }
    // non-positive sizes
    for (int bad : {0, -3}) {
        REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, bad, U, C, B, PX, PY, L, o, 0));
        REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, bad, C, B, PX, PY, L, o, 0));
        REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, bad, B, PX, PY, L, o, 0));
        REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, bad, PX, PY, L, o, 0));
        REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, bad, U, C, B, DZ, o, 0));
        REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, bad, C, B, DZ, o, 0));
        REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, bad, B, DZ, o, 0));
        REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, bad, DZ, o, 0));
    }
    // the blank outside [0, C)
    REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, B, PX, PY, L, opts(RNNT_GPU, C), 0));
    REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, B, PX, PY, L, opts(RNNT_GPU, -1), 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, DZ, opts(RNNT_GPU, C), 0));
    // more rows than an int holds: B T U joint, B T K pruned
    REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, 1 << 15, 1 << 10, C, 1 << 6, PX, PY, L, o, 0));
    REFUSED(FWD(Z, SY, RG, 1 << 10, BD, 0, 1 << 15, 1 << 11, C, 1 << 6, PX, PY, L, o, 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, 1 << 15, 1 << 10, C, 1 << 6, DZ, o, 0));
    // the CPU location
    REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, B, PX, PY, L, opts(RNNT_CPU), 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, DZ, opts(RNNT_CPU), 0));
    // px, py and lse overlapping one another (same start; last byte on first byte)
    REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, B, PX, PX, L, o, 0));
    REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, B, PX, PY, PX, o, 0));
    REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, B, PX, PY, PY, o, 0));
    REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, B, PX, PX + B * (U - 1) * (T + 1) - 1, L, o, 0));
    REFUSED(FWD(Z, SY, nullptr, 0, BD, 0, T, U, C, B, PX, PY, PY + B * U * T - 1, o, 0));
    // dlogits overlapping anything but logits exactly
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, Z + 1, o, 0));
    REFUSED(BWD(Z + 1, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, Z, o, 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, L, o, 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, GX, o, 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, GY, o, 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, GL, o, 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, DZ + B * T * U * C - 1, T, U, C, B, DZ, o, 0));
    REFUSED(BWD(Z, L, SY, RG, K, BD, 0, GX, GY, GL, T, U, C, B, reinterpret_cast<float*>(RG), o, 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, reinterpret_cast<float*>(BD), o, 0));
    REFUSED(BWD(Z, L, SY, nullptr, 0, BD, 0, GX, GY, GL, T, U, C, B, reinterpret_cast<float*>(SY), o, 0));

    if (failures == 0) std::printf("test_logprobs_args: all refused\n");
    return failures == 0 ? 0 : 1;
}
