// rnnt_hat_impl.h -- host driver of libwarprnnt_hat.so (include/rnnt_hat.h): the Hybrid Autoregressive Transducer loss
// (run_hat<Tag>).  One instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_hat.hip   F32 (+ every C entry point)     rnnt_hat_f64.hip   F64     rnnt_hat_h16.hip   BF16, F16
// Statistics and gradient kernels are rnnt_hat_kernels.h's.  The workspace (make_layout: the record table overlaying the
// per-sample lattice blocks), the plan, the lattice stage with its selection rule (launch_lattice) and the coefficient
// stage (launch_coef) are rnnt_host.h's and rnnt_kernels.h's, instantiated here: HAT's lattice is the plain RNN-T lattice.
// The call record, its buffer checks and the launch arithmetic are rnnt_side_host.h's.
#pragma once
#include "rnnt_side_host.h"
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
constexpr size_t kHatWideRowBytes = 4096;
template <typename Tag>
static void launch_hat_stats(Plan<typename Tag::comp>& p, const typename Tag::store* acts) {
    const StatsGrid sg = stats_grid(static_cast<size_t>(p.A) * sizeof(typename Tag::store), p.cells_per_sample, kHatWideRowBytes);
    for (int b0 = 0; b0 < p.N; b0 += kGridSamples) {
        const dim3 grid(sg.gx, grid_samples(p.N, b0));
        stats_dispatch(sg.G, [&](auto g) {
            hipLaunchKernelGGL((hat_stats_kernel<Tag, decltype(g)::value>), grid, dim3(256), 0, p.stream,
                               acts, p.labels, p.input_lengths, p.label_lengths, p.lp2, p.logz, p.maxT, p.maxU, p.Up, p.A,
                               p.blank, b0, p.poison);
        });
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
    if (packets_aligned(acts, grads)) {
        const FlatGrid fg = flat_grid(E / V, 2, V);                    // (hat_grad_kernel: PPT = 2)
        hipLaunchKernelGGL((hat_grad_kernel<Tag>), dim3(fg.grid), dim3(256), 0, p.stream, acts, grads, p.rowtab, grad_scale, E,
                           R, p.A, p.blank, TU, 1.0f / static_cast<float>(p.A), fg.stride / p.A,
                           static_cast<int>(fg.stride % p.A), p.padflag);
    } else {
        hipLaunchKernelGGL((hat_grad_elem_kernel<Tag>), dim3(elem_grid(E)), dim3(256), 0, p.stream, acts, grads, p.rowtab,
                           grad_scale, E, p.A, p.blank, TU);
    }
    p.check();
}

// The HAT loss of call `c` (SideCall: phases, host or device costs).
template <typename Tag>
rnntStatus_t run_hat(const SideCall& c) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const St* acts = static_cast<const St*>(c.acts);
    St* grads = static_cast<St*>(c.grads);
    if (!hat_shape_ok(c.A, c.N, c.opt.maxT, c.opt.maxU)) return RNNT_STATUS_INVALID_VALUE;
    Plan<C> p;
    if (!make_plan(p, c.A, c.N, c.opt, c.workspace, c.labels, c.label_lengths, c.input_lengths, static_cast<C*>(c.costs_dev)))
        return RNNT_STATUS_INVALID_VALUE;
    bool do_fwd, do_bwd;
    if (!side_buffers_ok(c, sizeof(St), static_cast<unsigned long long>(c.N) * p.cells_per_sample * c.A, do_fwd, do_bwd))
        return RNNT_STATUS_INVALID_VALUE;
    if (do_fwd) {
        launch_hat_stats<Tag>(p, acts);
        if (!p.failed) launch_lattice(p, c.want_grad);
        if (!p.failed && c.want_grad) launch_coef(p);
    }
    if (do_bwd && !p.failed) launch_hat_grad<Tag>(p, acts, grads, static_cast<const C*>(c.grad_scale));
    if (p.failed) return RNNT_STATUS_EXECUTION_FAILED;
    return c.costs_host != nullptr ? finish_host_costs(static_cast<C*>(c.costs_host), p.costs_dev, c.N, p.stream)
                                   : RNNT_STATUS_SUCCESS;
}

#ifndef RNNT_HAT_INSTANTIATE_F32
extern template rnntStatus_t run_hat<F32>(const SideCall&);
#endif
#ifndef RNNT_HAT_INSTANTIATE_F64
extern template rnntStatus_t run_hat<F64>(const SideCall&);
#endif
#ifndef RNNT_HAT_INSTANTIATE_H16
extern template rnntStatus_t run_hat<BF16>(const SideCall&);
extern template rnntStatus_t run_hat<F16>(const SideCall&);
#endif

}  // namespace rnnt
