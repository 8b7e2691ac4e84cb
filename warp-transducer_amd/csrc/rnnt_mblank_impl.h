// rnnt_mblank_impl.h -- host driver of libwarprnnt_mblank.so (include/rnnt_mblank.h): the multi-blank transducer loss
// (run_mblank<Tag>).  One instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_mblank.hip   F32 (+ every C entry point)     rnnt_mblank_f64.hip   F64     rnnt_mblank_h16.hip   BF16, F16
// Every kernel is rnnt_mblank_kernels.h's; rnnt_host.h contributes only helpers (workspace alignment, the tuning
// constants, the argument checks).
#pragma once
#include "rnnt_host.h"
#include "rnnt_mblank_kernels.h"
#include "../../include/rnnt_mblank.h"

namespace rnnt {

// Workspace: the cell table (stats, then the gradient records in place), alpha, beta, the per-diagonal offsets of both
// directions, log P, the costs of the host-costs entry and the poison flags.  lat = bytes of one lattice value.
struct MbLayout { size_t tab, alpha, beta, offa, offb, ll, costs, poison, total; };
static inline MbLayout mblank_layout(int maxT, int maxU, int N, int K, size_t lat) {
    const size_t cells = static_cast<size_t>(N) * maxT * maxU;
    const size_t diags = static_cast<size_t>(N) * tdt_diags(maxT, maxU);
    MbLayout l;
    size_t o = 0;
    l.tab = o; o = align_up(o + cells * mblank_rec_stride(K) * lat);
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

// Problem limits shared by every entry: blank inside the columns, maxU <= kMbMaxU, labels exact as lattice values
// (A <= 2^23), the statistics kernel's int row count, fewer than 2^32 rows (the gradient stream decodes rows in 32-bit
// arithmetic).
static inline bool mblank_shape_ok(int A, int N, int maxT, int maxU, int blank) {
    if (A < 1 || A > (1 << 23) || N < 1 || maxT < 1 || maxU < 1 || maxU > kMbMaxU || blank < 0 || blank >= A) return false;
    if (static_cast<long long>(maxT) * maxU * 64 >= 0x7fffffffLL) return false;
    return static_cast<unsigned long long>(N) * maxT * maxU < (1ull << 32);
}

// The big blanks: 0 <= K <= 8, columns distinct, inside [0, A) and not the standard blank; durations strictly increasing
// inside [2, 64].  Call after mblank_shape_ok (blank inside [0, A)).
static inline bool mblank_blanks(const int* columns, const int* durations, int K, int A, int blank, MbBlanks& out) {
    if (K < 0 || K > kMbMaxBig || (K > 0 && (columns == nullptr || durations == nullptr))) return false;
    out.n = K;
    out.blank = out.lo = out.hi = blank;
    for (int j = 0; j < kMbMaxBig; ++j) {
        out.col[j] = j < K ? columns[j] : -1;
        out.dur[j] = j < K ? durations[j] : 0;
    }
    for (int j = 0; j < K; ++j) {
        const int c = out.col[j], d = out.dur[j];
        if (c < 0 || c >= A || c == blank || d < 2 || d > kMbMaxDuration) return false;
        if (j > 0 && d <= out.dur[j - 1]) return false;
        for (int i = 0; i < j; ++i)
            if (out.col[i] == c) return false;
        out.lo = c < out.lo ? c : out.lo;
        out.hi = c > out.hi ? c : out.hi;
    }
    return true;
}

// Stage 1: G lanes per row, the smallest group that keeps a lane's share of the row's packets at a few rounds
template <typename Tag>
static bool launch_mblank_stats(const typename Tag::store* acts, const int* labels, const int* xlen, const int* ylen,
                                typename Tag::comp* tab, int* poison, int N, int maxT, int maxU, int A,
                                const MbBlanks& bb, float sigma, hipStream_t s) {
    using C = typename Tag::comp;
    const size_t row_bytes = static_cast<size_t>(A) * sizeof(typename Tag::store);
    const int G = row_bytes <= 256 ? 4 : row_bytes <= 2048 ? 16 : 64;
    const long long rows = static_cast<long long>(maxT) * maxU;
    const unsigned gx = static_cast<unsigned>((rows * G + 255) / 256);
    const C sigma2 = static_cast<C>(static_cast<double>(sigma) * kLog2e);
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid(gx, N - b0 < kGridSamples ? N - b0 : kGridSamples);
#define RNNT_MSTATS(GG)                                                                                                \
        hipLaunchKernelGGL((mblank_stats_kernel<Tag, GG>), grid, dim3(256), 0, s, acts, labels, xlen, ylen, tab, maxT, \
                           maxU, A, bb, sigma2, b0, poison)
        if (G == 4) RNNT_MSTATS(4); else if (G == 16) RNNT_MSTATS(16); else RNNT_MSTATS(64);
#undef RNNT_MSTATS
    }
    return hipGetLastError() == hipSuccess;
}

// Stage 4: the flat packet stream when both tensors sit on 16-byte boundaries, else element by element
template <typename Tag>
static bool launch_mblank_grad(const typename Tag::store* acts, typename Tag::store* grads, const typename Tag::comp* tab,
                               const typename Tag::comp* grad_scale, int N, int maxT, int maxU, int A, const MbBlanks& bb,
                               hipStream_t s) {
    constexpr int V = Vec<Tag>::N;
    const int RS = mblank_rec_stride(bb.n);
    const unsigned rps = static_cast<unsigned>(maxT) * static_cast<unsigned>(maxU);
    const unsigned long long E = static_cast<unsigned long long>(N) * rps * A;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(acts), pg = reinterpret_cast<uintptr_t>(grads);
    if (((pa | pg) & 15u) == 0) {
        const FlatGrid fg = flat_grid(E / V, 2, V);                    // (mblank_grad_kernel: PPT = 2)
        hipLaunchKernelGGL((mblank_grad_kernel<Tag>), dim3(fg.grid), dim3(256), 0, s, acts, grads, tab, grad_scale, E, A, RS,
                           bb, rps, 1.0f / static_cast<float>(A), fg.stride / A, static_cast<int>(fg.stride % A));
    } else {
        const unsigned long long blocks = (E + 255) / 256;
        const unsigned grid = static_cast<unsigned>(blocks < 65536 ? (blocks ? blocks : 1) : 65536);
        hipLaunchKernelGGL((mblank_grad_elem_kernel<Tag>), dim3(grid), dim3(256), 0, s, acts, grads, tab, grad_scale, E, A,
                           RS, bb, rps);
    }
    return hipGetLastError() == hipSuccess;
}

// The multi-blank loss.  phases: bit 0 = forward (statistics, lattice, and with want_grad the gradient records), bit 1 =
// gradient stream from the workspace a forward call left.  costs_host != nullptr: the one-call entry with costs in host
// memory (copied behind the last kernel, the stream synchronised, the cost markers answered with
// RNNT_STATUS_INVALID_VALUE).
template <typename Tag>
rnntStatus_t run_mblank(const typename Tag::store* acts, typename Tag::store* grads, const typename Tag::comp* grad_scale,
                        const int* columns, const int* durations, int K, float sigma, const int* labels,
                        const int* label_lengths, const int* input_lengths, int A, int N, typename Tag::comp* costs_device,
                        typename Tag::comp* costs_host, void* workspace, const rnntOptions& opt, int phases,
                        bool want_grad) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    (void)hipGetLastError();                           // a stale error of an unrelated earlier HIP call is not ours
    const int maxT = opt.maxT, maxU = opt.maxU, blank = opt.blank_label;
    if (!mblank_shape_ok(A, N, maxT, maxU, blank) || !(sigma - sigma == 0.0f)) return RNNT_STATUS_INVALID_VALUE;
    MbBlanks bb;
    if (!mblank_blanks(columns, durations, K, A, blank, bb)) return RNNT_STATUS_INVALID_VALUE;
    const bool do_fwd = (phases & 1) != 0, do_bwd = (phases & 2) != 0 && want_grad;
    if (do_bwd && grads == nullptr) return RNNT_STATUS_INVALID_VALUE;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(acts), pg = reinterpret_cast<uintptr_t>(grads);
    if (pa % sizeof(St) != 0 || (grads != nullptr && pg % sizeof(St) != 0)) return RNNT_STATUS_INVALID_VALUE;
    if (do_bwd && pg != pa) {                          // in place, or not overlapping at all
        const unsigned long long bytes =
            static_cast<unsigned long long>(N) * maxT * maxU * static_cast<unsigned long long>(A) * sizeof(St);
        if ((pg > pa ? pg - pa : pa - pg) < bytes) return RNNT_STATUS_INVALID_VALUE;
    }
    const MbLayout l = mblank_layout(maxT, maxU, N, K, sizeof(C));
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
        ok = ok && launch_mblank_stats<Tag>(acts, labels, input_lengths, label_lengths, tab, poison, N, maxT, maxU, A, bb,
                                            sigma, s);
        // lattice: a block per (sample, direction), a thread per cell of the widest diagonal (up to 1024)
        const int threads = maxU >= 1024 ? 1024 : (maxU + 63) / 64 * 64;
        for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
            hipLaunchKernelGGL((mblank_lattice_kernel<C>), dim3(N - b0 < kGridSamples ? N - b0 : kGridSamples, 2),
                               dim3(threads), 0, s, tab, alpha, beta, offa, offb, ll, input_lengths, label_lengths, poison,
                               costs_device, bb, maxT, maxU, b0);
            ok = hipGetLastError() == hipSuccess;
        }
        if (want_grad) {
            const unsigned gx = static_cast<unsigned>((static_cast<long long>(maxT) * maxU + 255) / 256);
            for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
                hipLaunchKernelGGL((mblank_coef_kernel<C>), dim3(gx, N - b0 < kGridSamples ? N - b0 : kGridSamples), dim3(256),
                                   0, s, tab, alpha, beta, offa, offb, ll, input_lengths, label_lengths, labels, poison, bb,
                                   maxT, maxU, A, b0);
                ok = hipGetLastError() == hipSuccess;
            }
        }
    }
    if (do_bwd && ok) ok = launch_mblank_grad<Tag>(acts, grads, tab, grad_scale, N, maxT, maxU, A, bb, s);
    if (!ok) return RNNT_STATUS_EXECUTION_FAILED;
    return costs_host != nullptr ? finish_host_costs(costs_host, costs_device, N, s) : RNNT_STATUS_SUCCESS;
}

}  // namespace rnnt

namespace rnnt {
#define RNNT_MBLANK_DECLARE(TAG, ST, CT)                                                                                  \
    extern template rnntStatus_t run_mblank<TAG>(const ST*, ST*, const CT*, const int*, const int*, int, float, const int*, \
                                                 const int*, const int*, int, int, CT*, CT*, void*, const rnntOptions&,    \
                                                 int, bool);
#ifndef RNNT_MBLANK_INSTANTIATE_F32
RNNT_MBLANK_DECLARE(F32, float, float)
#endif
#ifndef RNNT_MBLANK_INSTANTIATE_F64
RNNT_MBLANK_DECLARE(F64, double, double)
#endif
#ifndef RNNT_MBLANK_INSTANTIATE_H16
RNNT_MBLANK_DECLARE(BF16, uint16_t, float)
RNNT_MBLANK_DECLARE(F16, uint16_t, float)
#endif
#undef RNNT_MBLANK_DECLARE
}  // namespace rnnt
