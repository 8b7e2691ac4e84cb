// rnnt_hat_impl.h -- host driver of libwarprnnt_hat.so (include/rnnt_hat.h): the Hybrid Autoregressive Transducer loss
// (run_hat<Tag>).  One instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_hat.hip   F32 (+ every C entry point)     rnnt_hat_f64.hip   F64     rnnt_hat_h16.hip   BF16, F16
// Statistics and gradient kernels are rnnt_hat_kernels.h's.  The workspace (make_layout: the record table overlaying the
// per-sample lattice blocks), the plan, the lattice stage with its selection rule (launch_lattice) and the coefficient
// stage (launch_coef) are rnnt_host.h's and rnnt_kernels.h's, instantiated here: HAT's lattice is the plain RNN-T lattice.
#pragma once
#include "rnnt_host.h"
#include "rnnt_hat_kernels.h"
#include "../../include/rnnt_hat.h"

namespace rnnt {

// Limits on top of make_plan's (maxU <= 1024, maxT maxU < 2^29, one sample's skewed array < 2 GB): a label column besides
// the blank, the gradient stream's 32-bit row arithmetic and reciprocal division.
static inline bool hat_shape_ok(int A, int N, int maxT, int maxU) {
    if (A < 2 || A > (1 << 23) || N < 1 || maxT < 1 || maxU < 1) return false;
    return static_cast<unsigned long long>(N) * maxT * maxU < (1ull << 32);
}

// Stage 1: G lanes per row, the smallest group that keeps a lane's share of the row at a few rounds of four packets
// (rows of 2 to 4 KB -- bf16 vocabularies of 1025 -- stay with 16 lanes: 64 would hold two packets each, one round trip
// per row with nothing behind it)
static inline int hat_stats_group(size_t row_bytes) { return row_bytes <= 256 ? 4 : row_bytes <= 4096 ? 16 : 64; }
template <typename Tag>
static void launch_hat_stats(Plan<typename Tag::comp>& p, const typename Tag::store* acts) {
    const int G = hat_stats_group(static_cast<size_t>(p.A) * sizeof(typename Tag::store));
    const unsigned gx = static_cast<unsigned>((static_cast<long long>(p.cells_per_sample) * G + 255) / 256);
    for (int b0 = 0; b0 < p.N; b0 += kGridSamples) {
        const dim3 grid(gx, p.N - b0 < kGridSamples ? p.N - b0 : kGridSamples);
#define RNNT_HSTATS(GG)                                                                                                \
        hipLaunchKernelGGL((hat_stats_kernel<Tag, GG>), grid, dim3(256), 0, p.stream, acts, p.labels, p.input_lengths, \
                           p.label_lengths, p.lp2, p.logz, p.maxT, p.maxU, p.Up, p.A, p.blank, b0, p.poison)
        if (G == 4) RNNT_HSTATS(4); else if (G == 16) RNNT_HSTATS(16); else RNNT_HSTATS(64);
#undef RNNT_HSTATS
    }
    p.check();
}

// Stage 4: the flat packet stream when both tensors sit on 16-byte boundaries, else element by element
template <typename Tag>
static void launch_hat_grad(Plan<typename Tag::comp>& p, const typename Tag::store* acts, typename Tag::store* grads,
                            const typename Tag::comp* grad_scale) {
    constexpr int V = Vec<Tag>::N;
    const unsigned TU = static_cast<unsigned>(p.cells_per_sample);
    const unsigned R = static_cast<unsigned>(static_cast<unsigned long long>(p.N) * TU);
    const unsigned long long E = static_cast<unsigned long long>(R) * p.A;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(acts), pg = reinterpret_cast<uintptr_t>(grads);
    if (((pa | pg) & 15u) == 0) {
        const FlatGrid fg = flat_grid(E / V, 2, V);                    // (hat_grad_kernel: PPT = 2)
        hipLaunchKernelGGL((hat_grad_kernel<Tag>), dim3(fg.grid), dim3(256), 0, p.stream, acts, grads, p.rowtab, grad_scale, E,
                           R, p.A, p.blank, TU, 1.0f / static_cast<float>(p.A), fg.stride / p.A,
                           static_cast<int>(fg.stride % p.A), p.padflag);
    } else {
        const unsigned long long blocks = (E + 255) / 256;
        const unsigned grid = static_cast<unsigned>(blocks < 65536 ? (blocks ? blocks : 1) : 65536);
        hipLaunchKernelGGL((hat_grad_elem_kernel<Tag>), dim3(grid), dim3(256), 0, p.stream, acts, grads, p.rowtab,
                           grad_scale, E, p.A, p.blank, TU);
    }
    p.check();
}

// The HAT loss.  phases: bit 0 = forward (statistics, lattice, and with want_grad the gradient records), bit 1 = gradient
// stream from the workspace a forward call left.  costs_host != nullptr: the one-call entry with costs in host memory
// (copied behind the last kernel, the stream synchronised, the cost markers answered with RNNT_STATUS_INVALID_VALUE).
template <typename Tag>
rnntStatus_t run_hat(const typename Tag::store* acts, typename Tag::store* grads, const typename Tag::comp* grad_scale,
                     const int* labels, const int* label_lengths, const int* input_lengths, int A, int N,
                     typename Tag::comp* costs_device, typename Tag::comp* costs_host, void* workspace,
                     const rnntOptions& opt, int phases, bool want_grad) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    if (!hat_shape_ok(A, N, opt.maxT, opt.maxU)) return RNNT_STATUS_INVALID_VALUE;
    Plan<C> p;
    if (!make_plan(p, A, N, opt, workspace, labels, label_lengths, input_lengths, costs_device))
        return RNNT_STATUS_INVALID_VALUE;
    const bool do_fwd = (phases & 1) != 0, do_bwd = (phases & 2) != 0 && want_grad;
    if (do_bwd && grads == nullptr) return RNNT_STATUS_INVALID_VALUE;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(acts), pg = reinterpret_cast<uintptr_t>(grads);
    if (pa % sizeof(St) != 0 || (grads != nullptr && pg % sizeof(St) != 0)) return RNNT_STATUS_INVALID_VALUE;
    if (do_bwd && pg != pa) {                          // in place, or not overlapping at all
        const unsigned long long bytes =
            static_cast<unsigned long long>(N) * p.cells_per_sample * static_cast<unsigned long long>(A) * sizeof(St);
        if ((pg > pa ? pg - pa : pa - pg) < bytes) return RNNT_STATUS_INVALID_VALUE;
    }
    if (do_fwd) {
        launch_hat_stats<Tag>(p, acts);
        if (!p.failed) launch_lattice(p, want_grad);
        if (!p.failed && want_grad) launch_coef(p);
    }
    if (do_bwd && !p.failed) launch_hat_grad<Tag>(p, acts, grads, grad_scale);
    if (p.failed) return RNNT_STATUS_EXECUTION_FAILED;
    return costs_host != nullptr ? finish_host_costs(costs_host, p.costs_dev, N, p.stream) : RNNT_STATUS_SUCCESS;
}

}  // namespace rnnt

namespace rnnt {
#define RNNT_HAT_DECLARE(TAG, ST, CT)                                                                                  \
    extern template rnntStatus_t run_hat<TAG>(const ST*, ST*, const CT*, const int*, const int*, const int*, int, int, \
                                              CT*, CT*, void*, const rnntOptions&, int, bool);
#ifndef RNNT_HAT_INSTANTIATE_F32
RNNT_HAT_DECLARE(F32, float, float)
#endif
#ifndef RNNT_HAT_INSTANTIATE_F64
RNNT_HAT_DECLARE(F64, double, double)
#endif
#ifndef RNNT_HAT_INSTANTIATE_H16
RNNT_HAT_DECLARE(BF16, uint16_t, float)
RNNT_HAT_DECLARE(F16, uint16_t, float)
#endif
#undef RNNT_HAT_DECLARE
}  // namespace rnnt
