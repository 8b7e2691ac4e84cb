// rnnt_pstream_impl.h -- host driver of libwarprnnt_pstream.so (include/rnnt_pstream.h): the pruned RNN-T loss with k2's
// two lattice types and delay_penalty (run_pstream<Tag>).  One instantiation per storage type, each in a translation unit --
// a code object -- of its own:
//     rnnt_pstream.hip   F32 (+ every C entry point)     rnnt_pstream_f64.hip   F64     rnnt_pstream_h16.hip   BF16, F16
// Stages 0, 1 and 3 and the closing kernel are rnnt_pstream_kernels.h's, stage 2 the lattice kernels of rnnt_ar_kernels.h
// (type 0) and rnnt_mono_kernels.h (type 1), instantiated in this library's code objects, stage 4 the multi-blank gradient
// stream with K = 0 over the compact (N, maxT, S) record table (launch_mblank_grad, rnnt_mblank_impl.h); the shape limits
// are multi-blank's (mblank_shape_ok).  The call record, its buffer checks, the cell-table workspace and the launch
// arithmetic are rnnt_side_host.h's.
#pragma once
#include <cmath>

#include "rnnt_mblank_impl.h"
#include "rnnt_pstream_kernels.h"
#include "../../include/rnnt_pstream.h"

namespace rnnt {

// Workspace: the cell table of rnnt_side_host.h over the natural-order maxT x maxU lattice (cell records of stage 1, alpha,
// beta, the offsets of either lattice); behind it this library's own arrays: the per-frame window words, the per-sample
// "bad start" flags and the compact (N, maxT, S) table of gradient records -- all the backward call reads.
struct PsLayout { CellTableLayout cells; size_t win, bad, coef, total; };
static inline PsLayout ps_layout(int maxT, int maxU, int S, int N, size_t lat) {
    PsLayout p;
    p.cells = cell_table_layout(maxT, maxU, N, kPsRec, ps_offsets(maxT, maxU), lat);
    size_t o = p.cells.total - kAlign;                     // (the table's arrays end here; its alignment slack moves behind ours)
    p.win = o; o = align_up(o + static_cast<size_t>(N) * maxT * sizeof(int2));
    p.bad = o; o = align_up(o + static_cast<size_t>(N) * sizeof(int));
    p.coef = o; o = align_up(o + static_cast<size_t>(N) * maxT * S * kPsRec * lat);
    p.total = o + kAlign;
    return p;
}

// Stage 1: G lanes per row (stats_grid)
template <typename Tag>
static bool launch_pstream_stats(const typename Tag::store* acts, const int2* win, const int* labels, const int* xlen,
                                 const int* ylen, typename Tag::comp* tab, int* poison, int N, int maxT, int maxU, int S, int A,
                                 int blank, int mod, float penalty, hipStream_t s) {
    const StatsGrid sg = stats_grid(static_cast<size_t>(A) * sizeof(typename Tag::store), static_cast<long long>(maxT) * S);
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid(sg.gx, grid_samples(N, b0));
        stats_dispatch(sg.G, [&](auto g) {
            hipLaunchKernelGGL((pstream_stats_kernel<Tag, decltype(g)::value>), grid, dim3(256), 0, s, acts,
                               win, labels, xlen, ylen, tab, maxT, maxU, S, A, blank, mod, penalty, b0, poison);
        });
    }
    return hipGetLastError() == hipSuccess;
}

// Stage 2, the release rule of both lattices restated (launch_ar_lattice, launch_mono_lattice): up to kArWaveMaxU ==
// kMonoWaveMaxU lattice columns one wavefront per (sample, direction) keeps the sweep in registers; wider lattices take a
// block per (sample, direction), a thread per column up to 1024.  dirs = 1: the forward sweep alone (a score-only call).
template <typename C>
static bool launch_pstream_lattice(const CellTable<C>& w, const int* xlen, const int* ylen, int N, int maxT, int maxU, int mod,
                                   int dirs, hipStream_t s) {
    static_assert(kArWaveMaxU == kMonoWaveMaxU, "one release rule for both lattices");
    const bool wave = maxU <= kArWaveMaxU;
    const dim3 threads(wave ? 64 : (maxU >= 1024 ? 1024 : (maxU + 63) / 64 * 64));
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid(grid_samples(N, b0), dirs);
#define RNNT_PSTREAM_LATTICE(KERNEL)                                                                                   \
        hipLaunchKernelGGL((KERNEL<C>), grid, threads, 0, s, w.tab, w.alpha, w.beta, w.offa, w.offb, w.ll, xlen, ylen, \
                           w.poison, w.costs, maxT, maxU, b0)
        if (mod != 0) {
            if (wave) RNNT_PSTREAM_LATTICE(mono_lattice_wave_kernel); else RNNT_PSTREAM_LATTICE(mono_lattice_block_kernel);
        } else {
            if (wave) RNNT_PSTREAM_LATTICE(ar_lattice_wave_kernel); else RNNT_PSTREAM_LATTICE(ar_lattice_block_kernel);
        }
#undef RNNT_PSTREAM_LATTICE
    }
    return hipGetLastError() == hipSuccess;
}

// The loss of call `c` (SideCall: phases, host or device costs) over windows of S label positions per frame; the forward
// phase takes the lattice type (0 regular, 1 modified) and the penalty, the gradient stream works from the records.
template <typename Tag>
rnntStatus_t run_pstream(const SideCall& c, const int* ranges, int S, int rnnt_type, float penalty) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const St* acts = static_cast<const St*>(c.acts);
    St* grads = static_cast<St*>(c.grads);
    const int *labels = c.labels, *label_lengths = c.label_lengths, *input_lengths = c.input_lengths;
    const int A = c.A, N = c.N, maxT = c.opt.maxT, maxU = c.opt.maxU, blank = c.opt.blank_label;
    (void)hipGetLastError();                           // a stale error of an unrelated earlier HIP call is not ours
    if (!mblank_shape_ok(A, N, maxT, maxU, blank) || S < 1 || S > maxU) return RNNT_STATUS_INVALID_VALUE;
    MbBlanks bb;                                       // K = 0: the standard blank alone
    if (!mblank_blanks(nullptr, nullptr, 0, A, blank, bb)) return RNNT_STATUS_INVALID_VALUE;
    bool do_fwd, do_bwd;
    const unsigned long long elems = static_cast<unsigned long long>(N) * maxT * S * A;
    if (!side_buffers_ok(c, sizeof(St), elems, do_fwd, do_bwd)) return RNNT_STATUS_INVALID_VALUE;
    if (do_fwd && (ranges == nullptr || (rnnt_type != 0 && rnnt_type != 1) || !std::isfinite(penalty)))
        return RNNT_STATUS_INVALID_VALUE;
    const PsLayout lay = ps_layout(maxT, maxU, S, N, sizeof(C));
    const CellTable<C> w = carve_cell_table<C>(lay.cells, c.workspace, c.costs_dev);
    char* ws = reinterpret_cast<char*>(align_up(reinterpret_cast<size_t>(c.workspace)));
    int2* win = reinterpret_cast<int2*>(ws + lay.win);
    int* bad = reinterpret_cast<int*>(ws + lay.bad);
    C* coef = reinterpret_cast<C*>(ws + lay.coef);
    hipStream_t s = reinterpret_cast<hipStream_t>(c.opt.stream);
    bool ok = true;

    if (do_fwd) {
        ok = ok && hipMemsetAsync(w.poison, 0, sizeof(int) * N, s) == hipSuccess;
        for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
            hipLaunchKernelGGL((pstream_prep_kernel<C>), dim3((maxT + kPsPrepFrames - 1) / kPsPrepFrames, grid_samples(N, b0)),
                               dim3(256), 0, s, ranges, input_lengths, label_lengths, w.tab, win, bad, maxT, maxU, S, rnnt_type,
                               b0);
            ok = hipGetLastError() == hipSuccess;
        }
        ok = ok && launch_pstream_stats<Tag>(acts, win, labels, input_lengths, label_lengths, w.tab, w.poison, N, maxT, maxU, S,
                                             A, blank, rnnt_type, penalty, s);
        ok = ok && launch_pstream_lattice<C>(w, input_lengths, label_lengths, N, maxT, maxU, rnnt_type, c.want_grad ? 2 : 1, s);
        if (ok) {
            hipLaunchKernelGGL((pstream_close_kernel<C>), dim3((N + 255) / 256), dim3(256), 0, s, bad, input_lengths,
                               label_lengths, w.ll, w.poison, w.costs, N, maxT, maxU, rnnt_type, penalty);
            ok = hipGetLastError() == hipSuccess;
        }
        if (c.want_grad) {
            const unsigned gx = static_cast<unsigned>((static_cast<long long>(maxT) * S + 255) / 256);
            for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
                hipLaunchKernelGGL((pstream_coef_kernel<C>), dim3(gx, grid_samples(N, b0)), dim3(256), 0, s, w.tab, coef,
                                   w.alpha, w.beta, w.offa, w.offb, w.ll, win, input_lengths, label_lengths, labels, w.poison,
                                   maxT, maxU, S, A, rnnt_type, b0);
                ok = hipGetLastError() == hipSuccess;
            }
        }
    }
    // the compact table is an (N, maxT, S) cell table: the multi-blank stream with S in the place of its maxU
    if (do_bwd && ok)
        ok = launch_mblank_grad<Tag>(acts, grads, coef, static_cast<const C*>(c.grad_scale), N, maxT, S, A, bb, s);
    if (!ok) return RNNT_STATUS_EXECUTION_FAILED;
    return c.costs_host != nullptr ? finish_host_costs(static_cast<C*>(c.costs_host), w.costs, N, s) : RNNT_STATUS_SUCCESS;
}

#ifndef RNNT_PSTREAM_INSTANTIATE_F32
extern template rnntStatus_t run_pstream<F32>(const SideCall&, const int*, int, int, float);
#endif
#ifndef RNNT_PSTREAM_INSTANTIATE_F64
extern template rnntStatus_t run_pstream<F64>(const SideCall&, const int*, int, int, float);
#endif
#ifndef RNNT_PSTREAM_INSTANTIATE_H16
extern template rnntStatus_t run_pstream<BF16>(const SideCall&, const int*, int, int, float);
extern template rnntStatus_t run_pstream<F16>(const SideCall&, const int*, int, int, float);
#endif

}  // namespace rnnt
