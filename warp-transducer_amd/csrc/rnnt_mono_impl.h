// rnnt_mono_impl.h -- host driver of libwarprnnt_mono.so (include/rnnt_mono.h): the monotonic (one label per frame)
// transducer loss (run_mono<Tag>).  One instantiation per storage type, each in a translation unit -- a code object -- of
// its own:
//     rnnt_mono.hip   F32 (+ every C entry point)     rnnt_mono_f64.hip   F64     rnnt_mono_h16.hip   BF16, F16
// Stages 1 to 3 are rnnt_mono_kernels.h's.  Stage 4 is the multi-blank gradient stream with K = 0 (launch_mblank_grad,
// rnnt_mblank_impl.h: the gradient record is the same four words), and the shape limits are multi-blank's
// (mblank_shape_ok).  The call record, its buffer checks, the cell-table workspace and the launch arithmetic are
// rnnt_side_host.h's.
#pragma once
#include "rnnt_mblank_impl.h"
#include "rnnt_mono_kernels.h"
#include "../../include/rnnt_mono.h"

namespace rnnt {

// Workspace: the cell table of rnnt_side_host.h with records of kMonoRec lattice values and maxT + 1 offsets per sample
// and direction (one per frame and the terminal row's).
static inline CellTableLayout mono_layout(int maxT, int maxU, int N, size_t lat) {
    return cell_table_layout(maxT, maxU, N, kMonoRec, mono_offsets(maxT), lat);
}

// Stage 1: G lanes per row (stats_grid)
template <typename Tag>
static bool launch_mono_stats(const typename Tag::store* acts, const int* labels, const int* xlen, const int* ylen,
                              typename Tag::comp* tab, int* poison, int N, int maxT, int maxU, int A, int blank,
                              hipStream_t s) {
    const StatsGrid sg = stats_grid(static_cast<size_t>(A) * sizeof(typename Tag::store), static_cast<long long>(maxT) * maxU);
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid(sg.gx, grid_samples(N, b0));
        stats_dispatch(sg.G, [&](auto g) {
            hipLaunchKernelGGL((mono_stats_kernel<Tag, decltype(g)::value>), grid, dim3(256), 0, s, acts,
                               labels, xlen, ylen, tab, maxT, maxU, A, blank, b0, poison);
        });
    }
    return hipGetLastError() == hipSuccess;
}

// Stage 2, the release rule: up to kMonoWaveMaxU lattice columns one wavefront per (sample, direction) keeps the sweep in
// registers; wider lattices take a block per (sample, direction), a thread per column up to 1024.
template <typename C>
static bool launch_mono_lattice(const CellTable<C>& w, const int* xlen, const int* ylen, int N, int maxT, int maxU,
                                hipStream_t s) {
    const bool wave = maxU <= kMonoWaveMaxU;
    const int threads = wave ? 64 : (maxU >= 1024 ? 1024 : (maxU + 63) / 64 * 64);
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid(grid_samples(N, b0), 2);
        if (wave)
            hipLaunchKernelGGL((mono_lattice_wave_kernel<C>), grid, dim3(threads), 0, s, w.tab, w.alpha, w.beta, w.offa, w.offb,
                               w.ll, xlen, ylen, w.poison, w.costs, maxT, maxU, b0);
        else
            hipLaunchKernelGGL((mono_lattice_block_kernel<C>), grid, dim3(threads), 0, s, w.tab, w.alpha, w.beta, w.offa, w.offb,
                               w.ll, xlen, ylen, w.poison, w.costs, maxT, maxU, b0);
    }
    return hipGetLastError() == hipSuccess;
}

// The monotonic loss of call `c` (SideCall: phases, host or device costs).
template <typename Tag>
rnntStatus_t run_mono(const SideCall& c) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const St* acts = static_cast<const St*>(c.acts);
    St* grads = static_cast<St*>(c.grads);
    const int *labels = c.labels, *label_lengths = c.label_lengths, *input_lengths = c.input_lengths;
    const int A = c.A, N = c.N, maxT = c.opt.maxT, maxU = c.opt.maxU, blank = c.opt.blank_label;
    (void)hipGetLastError();                           // a stale error of an unrelated earlier HIP call is not ours
    if (!mblank_shape_ok(A, N, maxT, maxU, blank)) return RNNT_STATUS_INVALID_VALUE;
    MbBlanks bb;                                       // K = 0: the standard blank alone
    if (!mblank_blanks(nullptr, nullptr, 0, A, blank, bb)) return RNNT_STATUS_INVALID_VALUE;
    bool do_fwd, do_bwd;
    if (!side_buffers_ok(c, sizeof(St), static_cast<unsigned long long>(N) * maxT * maxU * A, do_fwd, do_bwd))
        return RNNT_STATUS_INVALID_VALUE;
    const CellTable<C> w = carve_cell_table<C>(mono_layout(maxT, maxU, N, sizeof(C)), c.workspace, c.costs_dev);
    hipStream_t s = reinterpret_cast<hipStream_t>(c.opt.stream);
    bool ok = true;

    if (do_fwd) {
        ok = ok && hipMemsetAsync(w.poison, 0, sizeof(int) * N, s) == hipSuccess;
        ok = ok && launch_mono_stats<Tag>(acts, labels, input_lengths, label_lengths, w.tab, w.poison, N, maxT, maxU, A, blank, s);
        ok = ok && launch_mono_lattice<C>(w, input_lengths, label_lengths, N, maxT, maxU, s);
        if (c.want_grad) {
            const unsigned gx = static_cast<unsigned>((static_cast<long long>(maxT) * maxU + 255) / 256);
            for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
                hipLaunchKernelGGL((mono_coef_kernel<C>), dim3(gx, grid_samples(N, b0)), dim3(256), 0, s, w.tab, w.alpha,
                                   w.beta, w.offa, w.offb, w.ll, input_lengths, label_lengths, labels, w.poison, maxT, maxU,
                                   A, b0);
                ok = hipGetLastError() == hipSuccess;
            }
        }
    }
    if (do_bwd && ok)
        ok = launch_mblank_grad<Tag>(acts, grads, w.tab, static_cast<const C*>(c.grad_scale), N, maxT, maxU, A, bb, s);
    if (!ok) return RNNT_STATUS_EXECUTION_FAILED;
    return c.costs_host != nullptr ? finish_host_costs(static_cast<C*>(c.costs_host), w.costs, N, s) : RNNT_STATUS_SUCCESS;
}

#ifndef RNNT_MONO_INSTANTIATE_F32
extern template rnntStatus_t run_mono<F32>(const SideCall&);
#endif
#ifndef RNNT_MONO_INSTANTIATE_F64
extern template rnntStatus_t run_mono<F64>(const SideCall&);
#endif
#ifndef RNNT_MONO_INSTANTIATE_H16
extern template rnntStatus_t run_mono<BF16>(const SideCall&);
extern template rnntStatus_t run_mono<F16>(const SideCall&);
#endif

}  // namespace rnnt
