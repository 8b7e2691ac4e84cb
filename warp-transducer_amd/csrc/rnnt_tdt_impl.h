// rnnt_tdt_impl.h -- host driver of libwarprnnt_tdt.so (include/rnnt_tdt.h): the Token-and-Duration Transducer loss
// (run_tdt<Tag>).  One instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_tdt.hip   F32 (+ every C entry point)     rnnt_tdt_f64.hip   F64     rnnt_tdt_h16.hip   BF16, F16
// Every kernel is rnnt_tdt_kernels.h's; rnnt_host.h and rnnt_side_host.h contribute only helpers (workspace alignment, the
// tuning constants, the call record and its checks, the cell-table workspace, the launch arithmetic).
#pragma once
#include "rnnt_side_host.h"
#include "rnnt_tdt_kernels.h"
#include "../../include/rnnt_tdt.h"

namespace rnnt {

// Workspace: the cell table of rnnt_side_host.h with records of tdt_rec_stride(D) lattice values.
static inline CellTableLayout tdt_layout(int maxT, int maxU, int N, int D, size_t lat) {
    return cell_table_layout(maxT, maxU, N, tdt_rec_stride(D), tdt_diags(maxT, maxU), lat);
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

// Stage 1: G lanes per row (stats_grid; row_bytes: the token columns only)
template <typename Tag>
static bool launch_tdt_stats(const typename Tag::store* acts, const int* labels, const int* xlen, const int* ylen,
                             typename Tag::comp* tab, int* poison, int N, int maxT, int maxU, int A, int D, int blank,
                             float sigma, hipStream_t s) {
    using C = typename Tag::comp;
    const StatsGrid sg = stats_grid(static_cast<size_t>(A) * sizeof(typename Tag::store), static_cast<long long>(maxT) * maxU);
    const C sigma2 = static_cast<C>(static_cast<double>(sigma) * kLog2e);
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid(sg.gx, grid_samples(N, b0));
        stats_dispatch(sg.G, [&](auto g) {
            hipLaunchKernelGGL((tdt_stats_kernel<Tag, decltype(g)::value>), grid, dim3(256), 0, s, acts,
                               labels, xlen, ylen, tab, maxT, maxU, A, D, blank, sigma2, b0, poison);
        });
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
    if (packets_aligned(acts, grads)) {
        const FlatGrid fg = flat_grid(E / V, 2, V);                    // (tdt_grad_kernel: PPT = 2)
        hipLaunchKernelGGL((tdt_grad_kernel<Tag>), dim3(fg.grid), dim3(256), 0, s, acts, grads, tab, grad_scale, E, W, A, RS,
                           blank, rps, 1.0f / static_cast<float>(W), fg.stride / W, static_cast<int>(fg.stride % W));
    } else {
        hipLaunchKernelGGL((tdt_grad_elem_kernel<Tag>), dim3(elem_grid(E)), dim3(256), 0, s, acts, grads, tab, grad_scale, E,
                           W, A, RS, blank, rps);
    }
    return hipGetLastError() == hipSuccess;
}

// The TDT loss of call `c` (SideCall: phases, host or device costs) over the duration set.
template <typename Tag>
rnntStatus_t run_tdt(const SideCall& c, const int* durations, int D, float sigma) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const St* acts = static_cast<const St*>(c.acts);
    St* grads = static_cast<St*>(c.grads);
    const int *labels = c.labels, *label_lengths = c.label_lengths, *input_lengths = c.input_lengths;
    const int A = c.A, N = c.N, maxT = c.opt.maxT, maxU = c.opt.maxU, blank = c.opt.blank_label;
    (void)hipGetLastError();                           // a stale error of an unrelated earlier HIP call is not ours
    TdtDurations dur;
    if (!tdt_durations(durations, D, dur)) return RNNT_STATUS_INVALID_VALUE;
    if (!tdt_shape_ok(A, D, N, maxT, maxU, blank) || !(sigma - sigma == 0.0f)) return RNNT_STATUS_INVALID_VALUE;
    bool do_fwd, do_bwd;
    if (!side_buffers_ok(c, sizeof(St), static_cast<unsigned long long>(N) * maxT * maxU * (A + D), do_fwd, do_bwd))
        return RNNT_STATUS_INVALID_VALUE;
    const CellTable<C> w = carve_cell_table<C>(tdt_layout(maxT, maxU, N, D, sizeof(C)), c.workspace, c.costs_dev);
    hipStream_t s = reinterpret_cast<hipStream_t>(c.opt.stream);
    bool ok = true;

    if (do_fwd) {
        ok = ok && hipMemsetAsync(w.poison, 0, sizeof(int) * N, s) == hipSuccess;
        ok = ok && launch_tdt_stats<Tag>(acts, labels, input_lengths, label_lengths, w.tab, w.poison, N, maxT, maxU, A, D,
                                         blank, sigma, s);
        // lattice: a block per (sample, direction), a thread per cell of the widest diagonal (up to 1024)
        const int threads = maxU >= 1024 ? 1024 : (maxU + 63) / 64 * 64;
        for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
            hipLaunchKernelGGL((tdt_lattice_kernel<C>), dim3(grid_samples(N, b0), 2), dim3(threads), 0, s, w.tab, w.alpha,
                               w.beta, w.offa, w.offb, w.ll, input_lengths, label_lengths, w.poison, w.costs, dur, maxT, maxU,
                               b0);
            ok = hipGetLastError() == hipSuccess;
        }
        if (c.want_grad) {
            const unsigned gx = static_cast<unsigned>((static_cast<long long>(maxT) * maxU + 255) / 256);
            for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
                hipLaunchKernelGGL((tdt_coef_kernel<C>), dim3(gx, grid_samples(N, b0)), dim3(256), 0, s, w.tab, w.alpha,
                                   w.beta, w.offa, w.offb, w.ll, input_lengths, label_lengths, labels, w.poison, dur, maxT,
                                   maxU, A, blank, b0);
                ok = hipGetLastError() == hipSuccess;
            }
        }
    }
    if (do_bwd && ok)
        ok = launch_tdt_grad<Tag>(acts, grads, w.tab, static_cast<const C*>(c.grad_scale), N, maxT, maxU, A, D, blank, s);
    if (!ok) return RNNT_STATUS_EXECUTION_FAILED;
    return c.costs_host != nullptr ? finish_host_costs(static_cast<C*>(c.costs_host), w.costs, N, s) : RNNT_STATUS_SUCCESS;
}

#ifndef RNNT_TDT_INSTANTIATE_F32
extern template rnntStatus_t run_tdt<F32>(const SideCall&, const int*, int, float);
#endif
#ifndef RNNT_TDT_INSTANTIATE_F64
extern template rnntStatus_t run_tdt<F64>(const SideCall&, const int*, int, float);
#endif
#ifndef RNNT_TDT_INSTANTIATE_H16
extern template rnntStatus_t run_tdt<BF16>(const SideCall&, const int*, int, float);
extern template rnntStatus_t run_tdt<F16>(const SideCall&, const int*, int, float);
#endif

}  // namespace rnnt
