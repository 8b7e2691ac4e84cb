// rnnt_ar_impl.h -- host driver of libwarprnnt_ar.so (include/rnnt_ar.h): the alignment-restricted RNN-T loss
// (run_ar<Tag>).  One instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_ar.hip   F32 (+ every C entry point)     rnnt_ar_f64.hip   F64     rnnt_ar_h16.hip   BF16, F16
// Stages 0 to 3 are rnnt_ar_kernels.h's.  Stage 4 is the multi-blank gradient stream with K = 0 (launch_mblank_grad,
// rnnt_mblank_impl.h: the gradient record is the same four words), and the shape limits are multi-blank's
// (mblank_shape_ok).  The call record, its buffer checks, the cell-table workspace and the launch arithmetic are
// rnnt_side_host.h's.
#pragma once
#include "rnnt_mblank_impl.h"
#include "rnnt_ar_kernels.h"
#include "../../include/rnnt_ar.h"

namespace rnnt {

// Workspace: the cell table of rnnt_side_host.h with records of kArRec lattice values and maxT + maxU offsets per sample
// and direction (one per diagonal and the terminal one); behind it this library's own arrays: the band's bounds e and l
// ((N, maxU) int32 each) and the per-sample feasibility flag.
struct ArLayout { CellTableLayout cells; size_t e, l, ok, total; };
static inline ArLayout ar_layout(int maxT, int maxU, int N, size_t lat) {
    ArLayout a;
    a.cells = cell_table_layout(maxT, maxU, N, kArRec, ar_offsets(maxT, maxU), lat);
    const size_t bounds = static_cast<size_t>(N) * maxU * sizeof(int);
    size_t o = a.cells.total - kAlign;                     // (the table's arrays end here; its alignment slack moves behind ours)
    a.e = o; o = align_up(o + bounds);
    a.l = o; o = align_up(o + bounds);
    a.ok = o; o = align_up(o + static_cast<size_t>(N) * sizeof(int));
    a.total = o + kAlign;
    return a;
}
struct ArBounds { int *e, *l, *ok; };
static inline ArBounds carve_ar_bounds(const ArLayout& a, void* workspace) {
    char* ws = reinterpret_cast<char*>(align_up(reinterpret_cast<size_t>(workspace)));
    return {reinterpret_cast<int*>(ws + a.e), reinterpret_cast<int*>(ws + a.l), reinterpret_cast<int*>(ws + a.ok)};
}

// Stage 1: G lanes per row (stats_grid)
template <typename Tag>
static bool launch_ar_stats(const typename Tag::store* acts, const int* labels, const int* xlen, const int* ylen,
                            const ArBounds& bd, typename Tag::comp* tab, int* poison, int N, int maxT, int maxU, int A,
                            int blank, hipStream_t s) {
    const StatsGrid sg = stats_grid(static_cast<size_t>(A) * sizeof(typename Tag::store), static_cast<long long>(maxT) * maxU);
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid(sg.gx, grid_samples(N, b0));
        stats_dispatch(sg.G, [&](auto g) {
            hipLaunchKernelGGL((ar_stats_kernel<Tag, decltype(g)::value>), grid, dim3(256), 0, s, acts,
                               labels, xlen, ylen, bd.e, bd.l, bd.ok, tab, maxT, maxU, A, blank, b0, poison);
        });
    }
    return hipGetLastError() == hipSuccess;
}

// Stage 2, the release rule: up to kArWaveMaxU lattice columns one wavefront per (sample, direction) keeps the sweep in
// registers; wider lattices take a block per (sample, direction), a thread per column up to 1024.
template <typename C>
static bool launch_ar_lattice(const CellTable<C>& w, const int* xlen, const int* ylen, int N, int maxT, int maxU,
                              hipStream_t s) {
    const bool wave = maxU <= kArWaveMaxU;
    const int threads = wave ? 64 : (maxU >= 1024 ? 1024 : (maxU + 63) / 64 * 64);
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid(grid_samples(N, b0), 2);
        if (wave)
            hipLaunchKernelGGL((ar_lattice_wave_kernel<C>), grid, dim3(threads), 0, s, w.tab, w.alpha, w.beta, w.offa, w.offb,
                               w.ll, xlen, ylen, w.poison, w.costs, maxT, maxU, b0);
        else
            hipLaunchKernelGGL((ar_lattice_block_kernel<C>), grid, dim3(threads), 0, s, w.tab, w.alpha, w.beta, w.offa, w.offb,
                               w.ll, xlen, ylen, w.poison, w.costs, maxT, maxU, b0);
    }
    return hipGetLastError() == hipSuccess;
}

// The alignment-restricted loss of call `c` (SideCall: phases, host or device costs) under the windows emit_lo / emit_hi
// (the forward phase only: the gradient stream works from the records).
template <typename Tag>
rnntStatus_t run_ar(const SideCall& c, const int* emit_lo, const int* emit_hi) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const St* acts = static_cast<const St*>(c.acts);
    St* grads = static_cast<St*>(c.grads);
    const int *labels = c.labels, *label_lengths = c.label_lengths, *input_lengths = c.input_lengths;
    const int A = c.A, N = c.N, maxT = c.opt.maxT, maxU = c.opt.maxU, blank = c.opt.blank_label;
    (void)hipGetLastError();                           // a stale error of an unrelated earlier HIP call is not ours
    static_assert(kArMaxU == kMbMaxU, "the bounds kernel scans up to multi-blank's widest lattice");
    if (!mblank_shape_ok(A, N, maxT, maxU, blank)) return RNNT_STATUS_INVALID_VALUE;
    MbBlanks bb;                                       // K = 0: the standard blank alone
    if (!mblank_blanks(nullptr, nullptr, 0, A, blank, bb)) return RNNT_STATUS_INVALID_VALUE;
    bool do_fwd, do_bwd;
    if (!side_buffers_ok(c, sizeof(St), static_cast<unsigned long long>(N) * maxT * maxU * A, do_fwd, do_bwd))
        return RNNT_STATUS_INVALID_VALUE;
    const ArLayout lay = ar_layout(maxT, maxU, N, sizeof(C));
    const CellTable<C> w = carve_cell_table<C>(lay.cells, c.workspace, c.costs_dev);
    const ArBounds bd = carve_ar_bounds(lay, c.workspace);
    hipStream_t s = reinterpret_cast<hipStream_t>(c.opt.stream);
    bool ok = true;

    if (do_fwd) {
        ok = ok && hipMemsetAsync(w.poison, 0, sizeof(int) * N, s) == hipSuccess;
        for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
            hipLaunchKernelGGL((ar_bounds_kernel<C>), dim3(grid_samples(N, b0)), dim3(64), 0, s, emit_lo, emit_hi, input_lengths,
                               label_lengths, bd.e, bd.l, bd.ok, maxT, maxU, b0);
            ok = hipGetLastError() == hipSuccess;
        }
        ok = ok && launch_ar_stats<Tag>(acts, labels, input_lengths, label_lengths, bd, w.tab, w.poison, N, maxT, maxU, A, blank, s);
        ok = ok && launch_ar_lattice<C>(w, input_lengths, label_lengths, N, maxT, maxU, s);
        if (c.want_grad) {
            const unsigned gx = static_cast<unsigned>((static_cast<long long>(maxT) * maxU + 255) / 256);
            for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
                hipLaunchKernelGGL((ar_coef_kernel<C>), dim3(gx, grid_samples(N, b0)), dim3(256), 0, s, w.tab, w.alpha,
                                   w.beta, w.offa, w.offb, w.ll, input_lengths, label_lengths, labels, bd.e, bd.l, w.poison,
                                   maxT, maxU, A, b0);
                ok = hipGetLastError() == hipSuccess;
            }
        }
    }
    if (do_bwd && ok)
        ok = launch_mblank_grad<Tag>(acts, grads, w.tab, static_cast<const C*>(c.grad_scale), N, maxT, maxU, A, bb, s);
    if (!ok) return RNNT_STATUS_EXECUTION_FAILED;
    return c.costs_host != nullptr ? finish_host_costs(static_cast<C*>(c.costs_host), w.costs, N, s) : RNNT_STATUS_SUCCESS;
}

#ifndef RNNT_AR_INSTANTIATE_F32
extern template rnntStatus_t run_ar<F32>(const SideCall&, const int*, const int*);
#endif
#ifndef RNNT_AR_INSTANTIATE_F64
extern template rnntStatus_t run_ar<F64>(const SideCall&, const int*, const int*);
#endif
#ifndef RNNT_AR_INSTANTIATE_H16
extern template rnntStatus_t run_ar<BF16>(const SideCall&, const int*, const int*);
extern template rnntStatus_t run_ar<F16>(const SideCall&, const int*, const int*);
#endif

}  // namespace rnnt
