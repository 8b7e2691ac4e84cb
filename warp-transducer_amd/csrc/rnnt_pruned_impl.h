// rnnt_pruned_impl.h -- host driver of libwarprnnt_pruned.so (include/rnnt_pruned.h): the pruned loss (run_pruned<Tag>) and the
// prune ranges of the additive joint (run_prune_ranges<Tag>).  One instantiation per storage type, each in a translation unit
// -- a code object -- of its own, as in the main library:
//     rnnt_pruned.hip   F32 (+ every C entry point)     rnnt_pruned_f64.hip   F64     rnnt_pruned_h16.hip   BF16, F16
// The lattice, the coefficient stage and the additive joint's partition stage are the launchers of rnnt_host.h /
// rnnt_joint_impl.h, unchanged; the two streaming stages of the pruned loss and the ranges kernels are rnnt_pruned_kernels.h.
// The call record, its buffer checks and the launch arithmetic are rnnt_side_host.h's.
#pragma once
#include "rnnt_side_host.h"
#include "rnnt_joint_impl.h"
#include "rnnt_pruned_kernels.h"
#include "../../include/rnnt_pruned.h"

namespace rnnt {

// Workspace: the additive joint's layout (make_layout(joint = true): a plan carved from it serves the pruned loss, whose
// record table and lattice blocks are the materialised path's, and the ranges entry, which runs the joint's partition stage),
// then the per-frame windows and the per-sample "bad start" flags -- behind everything the record table can overlay.
struct PrunedLayout { size_t win, bad, total; };
static inline PrunedLayout pruned_layout(int maxT, int maxU, int N, size_t lat) {
    const Layout l = make_layout(maxT, maxU, N, lat, true);
    PrunedLayout pl;
    size_t o = l.total - kAlign;                       // (make_layout's end, aligned; its slack moves behind our arrays)
    pl.win = o; o = align_up(o + static_cast<size_t>(N) * maxT * sizeof(int2));
    pl.bad = o; o = align_up(o + static_cast<size_t>(N) * sizeof(int));
    pl.total = o + kAlign;
    return pl;
}

// Stage 1 of the pruned loss: G lanes per row (stats_grid)
template <typename Tag>
static void launch_pruned_stats(Plan<typename Tag::comp>& p, const typename Tag::store* acts, const int2* win, int S) {
    const StatsGrid sg = stats_grid(static_cast<size_t>(p.A) * sizeof(typename Tag::store), static_cast<long long>(p.maxT) * S);
    for (int b0 = 0; b0 < p.N; b0 += kGridSamples) {
        const dim3 grid(sg.gx, grid_samples(p.N, b0));
        stats_dispatch(sg.G, [&](auto g) {
            hipLaunchKernelGGL((pruned_stats_kernel<Tag, decltype(g)::value>), grid, dim3(256), 0, p.stream,
                               acts, win, p.labels, p.label_lengths, p.lp2, p.logz, p.maxT, p.maxU, p.Up, S, p.A, p.blank,
                               b0, p.poison);
        });
    }
    p.check();
}

// Stage 4 of the pruned loss: the flat packet stream when both tensors sit on 16-byte boundaries, else element by element
template <typename Tag>
static void launch_pruned_grad(Plan<typename Tag::comp>& p, const typename Tag::store* acts, typename Tag::store* grads,
                               const typename Tag::comp* grad_scale, const int2* win, int S) {
    constexpr int V = Vec<Tag>::N;
    const unsigned long long R = static_cast<unsigned long long>(p.N) * p.maxT * S;
    const unsigned long long E = R * p.A;
    if (packets_aligned(acts, grads) && p.A <= (1 << 23)) {
        const FlatGrid fg = flat_grid(E / V, 2, V);                    // (pruned_grad_kernel: PPT = 2)
        hipLaunchKernelGGL((pruned_grad_kernel<Tag>), dim3(fg.grid), dim3(256), 0, p.stream, acts, grads, p.rowtab, win,
                           grad_scale, E, p.A, p.blank, S, p.maxT, p.maxU, 1.0f / static_cast<float>(p.A), fg.stride / p.A,
                           static_cast<int>(fg.stride % p.A));
    } else {
        hipLaunchKernelGGL((pruned_grad_elem_kernel<Tag>), dim3(elem_grid(E)), dim3(256), 0, p.stream, acts, grads, p.rowtab,
                           win, grad_scale, E, p.A, p.blank, S, p.maxT, p.maxU);
    }
    p.check();
}

// The pruned loss of call `c` (SideCall: phases, host or device costs) over windows of S label positions per frame.
template <typename Tag>
rnntStatus_t run_pruned(const SideCall& c, const int* ranges, int S) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const St* acts = static_cast<const St*>(c.acts);
    St* grads = static_cast<St*>(c.grads);
    const int N = c.N;
    Plan<C> p;
    if (!make_plan(p, c.A, N, c.opt, c.workspace, c.labels, c.label_lengths, c.input_lengths, static_cast<C*>(c.costs_dev),
                   /*joint=*/true))
        return RNNT_STATUS_INVALID_VALUE;
    if (S < 1 || S > p.maxU) return RNNT_STATUS_INVALID_VALUE;
    // the gradient stream decodes rows in 32-bit arithmetic; the statistics kernel counts a sample's rows in an int
    const unsigned long long R = static_cast<unsigned long long>(N) * p.maxT * S;
    if (R >= (1ull << 32) || static_cast<long long>(p.maxT) * S * 64 >= 0x7fffffffLL) return RNNT_STATUS_INVALID_VALUE;
    bool do_fwd, do_bwd;
    if (!side_buffers_ok(c, sizeof(St), R * c.A, do_fwd, do_bwd)) return RNNT_STATUS_INVALID_VALUE;
    const PrunedLayout pl = pruned_layout(p.maxT, p.maxU, N, sizeof(C));
    char* ws = reinterpret_cast<char*>(align_up(reinterpret_cast<size_t>(c.workspace)));
    int2* win = reinterpret_cast<int2*>(ws + pl.win);
    int* bad = reinterpret_cast<int*>(ws + pl.bad);

    if (do_fwd) {
        for (int b0 = 0; b0 < N; b0 += kGridSamples)
            hipLaunchKernelGGL((pruned_prep_kernel<C>), dim3((p.maxT + 31) / 32, grid_samples(N, b0)), dim3(256), 0, p.stream,
                               ranges, c.input_lengths, c.label_lengths, p.lp2, p.logz, win, bad, p.maxT, p.maxU, p.Up, S, b0);
        p.check();
        launch_pruned_stats<Tag>(p, acts, win, S);
        launch_lattice(p, c.want_grad);
        hipLaunchKernelGGL((pruned_fix_kernel<C>), dim3((N + 255) / 256), dim3(256), 0, p.stream, bad, p.costs_dev, N);
        p.check();
        if (c.want_grad) launch_coef(p);
    }
    if (do_bwd) launch_pruned_grad<Tag>(p, acts, grads, static_cast<const C*>(c.grad_scale), win, S);
    if (p.failed) return RNNT_STATUS_EXECUTION_FAILED;
    return c.costs_host != nullptr ? finish_host_costs(static_cast<C*>(c.costs_host), p.costs_dev, N, p.stream)
                                   : RNNT_STATUS_SUCCESS;
}

// Prune ranges of the additive joint: its partition stage (row maxima, Z: lp2 / log Z of every cell), the lattice in both
// directions, then the window sums of the occupancy and the per-sample repair.  No coefficient stage: the record table
// overlays nothing.  Enqueue only.  Of `c` it reads the transcription activations (acts), the labels and lengths, A, N, the
// workspace and the options.
template <typename Tag>
rnntStatus_t run_prune_ranges(const SideCall& c, const void* pred_acts, int S, int* ranges) {
    const typename Tag::store* f = static_cast<const typename Tag::store*>(c.acts);
    const typename Tag::store* g = static_cast<const typename Tag::store*>(pred_acts);
    const int *label_lengths = c.label_lengths, *input_lengths = c.input_lengths;
    const int A = c.A, N = c.N;
    Plan<float> p;
    if (N > kGridSamples) return RNNT_STATUS_INVALID_VALUE;    // the partition kernels keep the samples on ONE grid dimension
    if (!make_plan(p, A, N, c.opt, c.workspace, c.labels, label_lengths, input_lengths, static_cast<float*>(nullptr),
                   /*joint=*/true))
        return RNNT_STATUS_INVALID_VALUE;
    if (S < 2 || S > p.maxU) return RNNT_STATUS_INVALID_VALUE;
    // (the partition stage's addressing limits, as run_gpu_joint checks them)
    if (static_cast<long long>(p.maxT > p.maxU ? p.maxT : p.maxU) * A >= (1LL << 31) ||
        static_cast<long long>(N) * (p.maxT + p.maxU) >= (1LL << 31))
        return RNNT_STATUS_INVALID_VALUE;
    launch_joint_partition<Tag>(p, f, g, /*training=*/false);
    launch_lattice(p, /*with_beta=*/true);
    const size_t lds = static_cast<size_t>(4) * p.maxU * sizeof(double);
    for (int b0 = 0; b0 < N; b0 += kGridSamples)
        hipLaunchKernelGGL(pruned_window_kernel<0>, dim3((p.maxT + 3) / 4, grid_samples(N, b0)), dim3(256), lds, p.stream,
                           p.alpha, p.beta, p.offa, p.offb, p.llf, input_lengths, label_lengths, ranges, p.maxT, p.maxU, p.Up, S, p.lat_w, p.lat_sh, b0);
    hipLaunchKernelGGL(pruned_ranges_kernel<0>, dim3((N + 63) / 64), dim3(64), 0, p.stream, input_lengths, label_lengths, ranges,
                       N, p.maxT, p.maxU, S);
    p.check();
    return p.failed ? RNNT_STATUS_EXECUTION_FAILED : RNNT_STATUS_SUCCESS;
}

#ifndef RNNT_PRUNED_INSTANTIATE_F32
extern template rnntStatus_t run_pruned<F32>(const SideCall&, const int*, int);
extern template rnntStatus_t run_prune_ranges<F32>(const SideCall&, const void*, int, int*);
#endif
#ifndef RNNT_PRUNED_INSTANTIATE_F64
extern template rnntStatus_t run_pruned<F64>(const SideCall&, const int*, int);
#endif
#ifndef RNNT_PRUNED_INSTANTIATE_H16
extern template rnntStatus_t run_pruned<BF16>(const SideCall&, const int*, int);
extern template rnntStatus_t run_pruned<F16>(const SideCall&, const int*, int);
extern template rnntStatus_t run_prune_ranges<BF16>(const SideCall&, const void*, int, int*);
extern template rnntStatus_t run_prune_ranges<F16>(const SideCall&, const void*, int, int*);
#endif

}  // namespace rnnt
