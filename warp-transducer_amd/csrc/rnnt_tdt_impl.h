// rnnt_tdt_impl.h -- host driver of libwarprnnt_tdt.so (include/rnnt_tdt.h): the Token-and-Duration Transducer loss
// (run_tdt<Tag>).  One instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_tdt.hip   F32 (+ every C entry point)     rnnt_tdt_f64.hip   F64     rnnt_tdt_h16.hip   BF16, F16
// Every kernel is rnnt_tdt_kernels.h's; rnnt_host.h contributes only helpers (workspace alignment, the tuning constants,
// the argument checks).
#pragma once
#include "rnnt_host.h"
#include "rnnt_tdt_kernels.h"
#include "../../include/rnnt_tdt.h"

namespace rnnt {

// Workspace: the cell table (stats, then the gradient records in place), alpha, beta, the per-diagonal offsets of both
// directions, log P, the costs of the host-costs entry and the poison flags.  lat = bytes of one lattice value.
struct TdtLayout { size_t tab, alpha, beta, offa, offb, ll, costs, poison, total; };
static inline TdtLayout tdt_layout(int maxT, int maxU, int N, int D, size_t lat) {
    const size_t cells = static_cast<size_t>(N) * maxT * maxU;
    const size_t diags = static_cast<size_t>(N) * tdt_diags(maxT, maxU);
    TdtLayout l;
    size_t o = 0;
    l.tab = o; o = align_up(o + cells * tdt_rec_stride(D) * lat);
    l.alpha = o; o = align_up(o + cells * lat);
    l.beta = o; o = align_up(o + cells * lat);
    l.offa = o; o = align_up(o + diags * sizeof(double));
    l.offb = o; o = align_up(o + diags * sizeof(double));
    l.ll = o; o = align_up(o + static_cast<size_t>(N) * sizeof(double));
    l.costs = o; o = align_up(o + static_cast<size_t>(N) * sizeof(double));     // (host costs: the device copy)
    l.poison = o; o = align_up(o + static_cast<size_t>(N) * sizeof(int));
    l.total = o + kAlign;                                  // slack to align the caller's base pointer
    return l;
}

// The duration set: 1 <= D <= 8, strictly increasing, non-negative, largest in [1, 64].
static inline bool tdt_durations(const int* durations, int D, TdtDurations& out) {
    if (durations == nullptr || D < 1 || D > kTdtMaxDurations) return false;
    out.n = D;
    for (int j = 0; j < kTdtMaxDurations; ++j) out.d[j] = j < D ? durations[j] : 0;
    if (out.d[0] < 0) return false;
    for (int j = 1; j < D; ++j)
        if (out.d[j] <= out.d[j - 1]) return false;
    return out.d[D - 1] >= 1 && out.d[D - 1] <= kTdtMaxDuration;
}

// Problem limits shared by every entry: blank inside the token columns, maxU <= kTdtMaxU, the statistics kernel's int row
// count, fewer than 2^32 rows (the gradient stream decodes rows in 32-bit arithmetic).
static inline bool tdt_shape_ok(int A, int D, int N, int maxT, int maxU, int blank) {
    if (A < 1 || N < 1 || maxT < 1 || maxU < 1 || maxU > kTdtMaxU || blank < 0 || blank >= A) return false;
    if (static_cast<long long>(A) + D > (1 << 23)) return false;
    if (static_cast<long long>(maxT) * maxU * 64 >= 0x7fffffffLL) return false;
    return static_cast<unsigned long long>(N) * maxT * maxU < (1ull << 32);
}

// Stage 1: G lanes per row, the smallest group that keeps a lane's share of the token packets at a few rounds
template <typename Tag>
static bool launch_tdt_stats(const typename Tag::store* acts, const int* labels, const int* xlen, const int* ylen,
                             typename Tag::comp* tab, int* poison, int N, int maxT, int maxU, int A, int D, int blank,
                             float sigma, hipStream_t s) {
    using C = typename Tag::comp;
    const size_t row_bytes = static_cast<size_t>(A) * sizeof(typename Tag::store);
    const int G = row_bytes <= 256 ? 4 : row_bytes <= 2048 ? 16 : 64;
    const long long rows = static_cast<long long>(maxT) * maxU;
    const unsigned gx = static_cast<unsigned>((rows * G + 255) / 256);
    const C sigma2 = static_cast<C>(static_cast<double>(sigma) * kLog2e);
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid(gx, N - b0 < kGridSamples ? N - b0 : kGridSamples);
#define RNNT_TSTATS(GG)                                                                                              \
        hipLaunchKernelGGL((tdt_stats_kernel<Tag, GG>), grid, dim3(256), 0, s, acts, labels, xlen, ylen, tab, maxT,  \
                           maxU, A, D, blank, sigma2, b0, poison)
        if (G == 4) RNNT_TSTATS(4); else if (G == 16) RNNT_TSTATS(16); else RNNT_TSTATS(64);
#undef RNNT_TSTATS
    }
    return hipGetLastError() == hipSuccess;
}

// Stage 4: the flat packet stream when both tensors sit on 16-byte boundaries, else element by element
template <typename Tag>
static bool launch_tdt_grad(const typename Tag::store* acts, typename Tag::store* grads, const typename Tag::comp* tab,
                            const typename Tag::comp* grad_scale, int N, int maxT, int maxU, int A, int D, int blank,
                            hipStream_t s) {
    constexpr int V = Vec<Tag>::N;
    const int W = A + D, RS = tdt_rec_stride(D);
    const unsigned rps = static_cast<unsigned>(maxT) * static_cast<unsigned>(maxU);
    const unsigned long long E = static_cast<unsigned long long>(N) * rps * W;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(acts), pg = reinterpret_cast<uintptr_t>(grads);
    if (((pa | pg) & 15u) == 0) {
        const FlatGrid fg = flat_grid(E / V, 2, V);                    // (tdt_grad_kernel: PPT = 2)
        hipLaunchKernelGGL((tdt_grad_kernel<Tag>), dim3(fg.grid), dim3(256), 0, s, acts, grads, tab, grad_scale, E, W, A, RS,
                           blank, rps, 1.0f / static_cast<float>(W), fg.stride / W, static_cast<int>(fg.stride % W));
    } else {
        const unsigned long long blocks = (E + 255) / 256;
        const unsigned grid = static_cast<unsigned>(blocks < 65536 ? (blocks ? blocks : 1) : 65536);
        hipLaunchKernelGGL((tdt_grad_elem_kernel<Tag>), dim3(grid), dim3(256), 0, s, acts, grads, tab, grad_scale, E, W, A,
                           RS, blank, rps);
    }
    return hipGetLastError() == hipSuccess;
}

// The TDT loss.  phases: bit 0 = forward (statistics, lattice, and with want_grad the gradient records), bit 1 = gradient
// stream from the workspace a forward call left.  costs_host != nullptr: the one-call entry with costs in host memory
// (copied behind the last kernel, the stream synchronised, the cost markers answered with RNNT_STATUS_INVALID_VALUE).
template <typename Tag>
rnntStatus_t run_tdt(const typename Tag::store* acts, typename Tag::store* grads, const typename Tag::comp* grad_scale,
                     const int* durations, int D, float sigma, const int* labels, const int* label_lengths,
                     const int* input_lengths, int A, int N, typename Tag::comp* costs_device, typename Tag::comp* costs_host,
                     void* workspace, const rnntOptions& opt, int phases, bool want_grad) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    (void)hipGetLastError();                           // a stale error of an unrelated earlier HIP call is not ours
    TdtDurations dur;
    if (!tdt_durations(durations, D, dur)) return RNNT_STATUS_INVALID_VALUE;
    const int maxT = opt.maxT, maxU = opt.maxU, blank = opt.blank_label;
    if (!tdt_shape_ok(A, D, N, maxT, maxU, blank) || !(sigma - sigma == 0.0f)) return RNNT_STATUS_INVALID_VALUE;
    const bool do_fwd = (phases & 1) != 0, do_bwd = (phases & 2) != 0 && want_grad;
    if (do_bwd && grads == nullptr) return RNNT_STATUS_INVALID_VALUE;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(acts), pg = reinterpret_cast<uintptr_t>(grads);
    if (pa % sizeof(St) != 0 || (grads != nullptr && pg % sizeof(St) != 0)) return RNNT_STATUS_INVALID_VALUE;
    if (do_bwd && pg != pa) {                          // in place, or not overlapping at all
        const unsigned long long bytes =
            static_cast<unsigned long long>(N) * maxT * maxU * static_cast<unsigned long long>(A + D) * sizeof(St);
        if ((pg > pa ? pg - pa : pa - pg) < bytes) return RNNT_STATUS_INVALID_VALUE;
    }
    const TdtLayout l = tdt_layout(maxT, maxU, N, D, sizeof(C));
    char* ws = reinterpret_cast<char*>(align_up(reinterpret_cast<size_t>(workspace)));
    C* tab = reinterpret_cast<C*>(ws + l.tab);
    C* alpha = reinterpret_cast<C*>(ws + l.alpha);
    C* beta = reinterpret_cast<C*>(ws + l.beta);
    double* offa = reinterpret_cast<double*>(ws + l.offa);
    double* offb = reinterpret_cast<double*>(ws + l.offb);
    double* ll = reinterpret_cast<double*>(ws + l.ll);
    int* poison = reinterpret_cast<int*>(ws + l.poison);
    if (costs_device == nullptr) costs_device = reinterpret_cast<C*>(ws + l.costs);
    hipStream_t s = reinterpret_cast<hipStream_t>(opt.stream);
    bool ok = true;

    if (do_fwd) {
        ok = ok && hipMemsetAsync(poison, 0, sizeof(int) * N, s) == hipSuccess;
        ok = ok && launch_tdt_stats<Tag>(acts, labels, input_lengths, label_lengths, tab, poison, N, maxT, maxU, A, D, blank,
                                         sigma, s);
        // lattice: a block per (sample, direction), a thread per cell of the widest diagonal (up to 1024)
        const int threads = maxU >= 1024 ? 1024 : (maxU + 63) / 64 * 64;
        for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
            hipLaunchKernelGGL((tdt_lattice_kernel<C>), dim3(N - b0 < kGridSamples ? N - b0 : kGridSamples, 2), dim3(threads),
                               0, s, tab, alpha, beta, offa, offb, ll, input_lengths, label_lengths, poison, costs_device,
                               dur, maxT, maxU, b0);
            ok = hipGetLastError() == hipSuccess;
        }
        if (want_grad) {
            const unsigned gx = static_cast<unsigned>((static_cast<long long>(maxT) * maxU + 255) / 256);
            for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
                hipLaunchKernelGGL((tdt_coef_kernel<C>), dim3(gx, N - b0 < kGridSamples ? N - b0 : kGridSamples), dim3(256), 0,
                                   s, tab, alpha, beta, offa, offb, ll, input_lengths, label_lengths, labels, poison, dur,
                                   maxT, maxU, A, blank, b0);
                ok = hipGetLastError() == hipSuccess;
            }
        }
    }
    if (do_bwd && ok) ok = launch_tdt_grad<Tag>(acts, grads, tab, grad_scale, N, maxT, maxU, A, D, blank, s);
    if (!ok) return RNNT_STATUS_EXECUTION_FAILED;
    return costs_host != nullptr ? finish_host_costs(costs_host, costs_device, N, s) : RNNT_STATUS_SUCCESS;
}

}  // namespace rnnt

namespace rnnt {
#define RNNT_TDT_DECLARE(TAG, ST, CT)                                                                                     \
    extern template rnntStatus_t run_tdt<TAG>(const ST*, ST*, const CT*, const int*, int, float, const int*, const int*,   \
                                              const int*, int, int, CT*, CT*, void*, const rnntOptions&, int, bool);
#ifndef RNNT_TDT_INSTANTIATE_F32
RNNT_TDT_DECLARE(F32, float, float)
#endif
#ifndef RNNT_TDT_INSTANTIATE_F64
RNNT_TDT_DECLARE(F64, double, double)
#endif
#ifndef RNNT_TDT_INSTANTIATE_H16
RNNT_TDT_DECLARE(BF16, uint16_t, float)
RNNT_TDT_DECLARE(F16, uint16_t, float)
#endif
#undef RNNT_TDT_DECLARE
}  // namespace rnnt
