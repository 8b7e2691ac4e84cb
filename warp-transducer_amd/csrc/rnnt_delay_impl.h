// rnnt_delay_impl.h -- host driver of libwarprnnt_delay.so (include/rnnt_delay.h): the delay-penalized RNN-T loss and the
// expected emission frames (run_delay<Tag>).  One instantiation per storage type, each in a translation unit -- a code
// object -- of its own:
//     rnnt_delay.hip   F32 (+ every C entry point)     rnnt_delay_f64.hip   F64     rnnt_delay_h16.hip   BF16, F16
// Stages 1, 3 and 4 are rnnt_delay_kernels.h's, stage 2 the two lattice kernels of rnnt_ar_kernels.h (instantiated in this
// library's code objects), stage 5 the multi-blank gradient stream with K = 0 (launch_mblank_grad, rnnt_mblank_impl.h); the
// shape limits are multi-blank's (mblank_shape_ok).  The call record, its buffer checks, the cell-table workspace and the
// launch arithmetic are rnnt_side_host.h's.
#pragma once
#include <cmath>

#include "rnnt_mblank_impl.h"
#include "rnnt_delay_kernels.h"
#include "../../include/rnnt_delay.h"

namespace rnnt {

// Workspace: the cell table of rnnt_side_host.h with records of kArRec lattice values and maxT + maxU offsets per sample
// and direction (one per diagonal and the terminal one).  Nothing of this library's own lies behind it.
static inline CellTableLayout delay_layout(int maxT, int maxU, int N, size_t lat) {
    return cell_table_layout(maxT, maxU, N, kArRec, ar_offsets(maxT, maxU), lat);
}

// [p, p + n) and [q, q + m) share a byte
static inline bool delay_overlap(const void* p, unsigned long long n, const void* q, unsigned long long m) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + m && b < a + n;
}

// Stage 1: G lanes per row (stats_grid)
template <typename Tag>
static bool launch_delay_stats(const typename Tag::store* acts, const int* labels, const int* xlen, const int* ylen,
                               typename Tag::comp* tab, int* poison, int N, int maxT, int maxU, int A, int blank, float penalty,
                               hipStream_t s) {
    const StatsGrid sg = stats_grid(static_cast<size_t>(A) * sizeof(typename Tag::store), static_cast<long long>(maxT) * maxU);
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid(sg.gx, grid_samples(N, b0));
        stats_dispatch(sg.G, [&](auto g) {
            hipLaunchKernelGGL((delay_stats_kernel<Tag, decltype(g)::value>), grid, dim3(256), 0, s, acts,
                               labels, xlen, ylen, tab, maxT, maxU, A, blank, penalty, b0, poison);
        });
    }
    return hipGetLastError() == hipSuccess;
}

// Stage 2, the release rule of the alignment-restricted loss (launch_ar_lattice, rnnt_ar_impl.h): up to kArWaveMaxU lattice
// columns one wavefront per (sample, direction) keeps the sweep in registers; wider lattices take a block per (sample,
// direction), a thread per column up to 1024.
template <typename C>
static bool launch_delay_lattice(const CellTable<C>& w, const int* xlen, const int* ylen, int N, int maxT, int maxU,
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

// Stage 4, the release rule: up to kDelayEmitNarrow label columns (maxU - 1 <= 64) a block is 32 lanes across u by
// kDelayEmitSlices slices of the frames -- with a thread per column alone a narrow lattice (maxU = 21) would leave most
// lanes of its one wavefront idle and the frames to a serial walk; wider lattices take a thread per column, 256 to a block,
// which reads whole runs of neighbouring records and has lanes enough.
template <typename C>
static bool launch_delay_emit(const C* tab, const int* xlen, const int* ylen, C* emit, int N, int maxT, int maxU,
                              hipStream_t s) {
    const int cols = maxU - 1;
    const bool narrow = cols <= kDelayEmitNarrow;
    const int lanes = narrow ? 256 / kDelayEmitSlices : 256;
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid((cols + lanes - 1) / lanes, grid_samples(N, b0));
        if (narrow)
            hipLaunchKernelGGL((delay_emit_kernel<C, kDelayEmitSlices>), grid, dim3(256), 0, s, tab, xlen, ylen, emit, maxT,
                               maxU, b0);
        else
            hipLaunchKernelGGL((delay_emit_kernel<C, 1>), grid, dim3(256), 0, s, tab, xlen, ylen, emit, maxT, maxU, b0);
    }
    return hipGetLastError() == hipSuccess;
}

// The delay-penalized loss of call `c` (SideCall: phases, host or device costs) at `penalty`, and with emit_frames != NULL
// the expected emission frames (both the forward phase only: the gradient stream works from the records).
template <typename Tag>
rnntStatus_t run_delay(const SideCall& c, float penalty, void* emit_frames) {
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
    const unsigned long long elems = static_cast<unsigned long long>(N) * maxT * maxU * A;
    if (!side_buffers_ok(c, sizeof(St), elems, do_fwd, do_bwd)) return RNNT_STATUS_INVALID_VALUE;
    const CellTableLayout lay = delay_layout(maxT, maxU, N, sizeof(C));
    C* emit = maxU > 1 ? static_cast<C*>(emit_frames) : nullptr;     // (maxU == 1: no element, the pointer is not looked at)
    if (emit != nullptr) {
        const unsigned long long eb = static_cast<unsigned long long>(N) * (maxU - 1) * sizeof(C);
        if (reinterpret_cast<uintptr_t>(emit) % sizeof(C) != 0 || delay_overlap(emit, eb, acts, elems * sizeof(St)) ||
            (grads != nullptr && delay_overlap(emit, eb, grads, elems * sizeof(St))) ||
            delay_overlap(emit, eb, c.workspace, lay.total))
            return RNNT_STATUS_INVALID_VALUE;
    }
    const CellTable<C> w = carve_cell_table<C>(lay, c.workspace, c.costs_dev);
    hipStream_t s = reinterpret_cast<hipStream_t>(c.opt.stream);
    bool ok = true;

    if (do_fwd) {
        ok = ok && hipMemsetAsync(w.poison, 0, sizeof(int) * N, s) == hipSuccess;
        ok = ok && launch_delay_stats<Tag>(acts, labels, input_lengths, label_lengths, w.tab, w.poison, N, maxT, maxU, A, blank,
                                           penalty, s);
        ok = ok && launch_delay_lattice<C>(w, input_lengths, label_lengths, N, maxT, maxU, s);
        if (c.want_grad || emit != nullptr) {
            const unsigned gx = static_cast<unsigned>((static_cast<long long>(maxT) * maxU + 255) / 256);
            for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
                hipLaunchKernelGGL((delay_coef_kernel<C>), dim3(gx, grid_samples(N, b0)), dim3(256), 0, s, w.tab, w.alpha,
                                   w.beta, w.offa, w.offb, w.ll, input_lengths, label_lengths, labels, w.poison, maxT, maxU, A,
                                   b0);
                ok = hipGetLastError() == hipSuccess;
            }
        }
        if (emit != nullptr) ok = ok && launch_delay_emit<C>(w.tab, input_lengths, label_lengths, emit, N, maxT, maxU, s);
    }
    if (do_bwd && ok)
        ok = launch_mblank_grad<Tag>(acts, grads, w.tab, static_cast<const C*>(c.grad_scale), N, maxT, maxU, A, bb, s);
    if (!ok) return RNNT_STATUS_EXECUTION_FAILED;
    return c.costs_host != nullptr ? finish_host_costs(static_cast<C*>(c.costs_host), w.costs, N, s) : RNNT_STATUS_SUCCESS;
}

#ifndef RNNT_DELAY_INSTANTIATE_F32
extern template rnntStatus_t run_delay<F32>(const SideCall&, float, void*);
#endif
#ifndef RNNT_DELAY_INSTANTIATE_F64
extern template rnntStatus_t run_delay<F64>(const SideCall&, float, void*);
#endif
#ifndef RNNT_DELAY_INSTANTIATE_H16
extern template rnntStatus_t run_delay<BF16>(const SideCall&, float, void*);
extern template rnntStatus_t run_delay<F16>(const SideCall&, float, void*);
#endif

}  // namespace rnnt
