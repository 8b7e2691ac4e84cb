// rnnt_mblank_impl.h -- host driver of libwarprnnt_mblank.so (include/rnnt_mblank.h): the multi-blank transducer loss
// (run_mblank<Tag>).  One instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_mblank.hip   F32 (+ every C entry point)     rnnt_mblank_f64.hip   F64     rnnt_mblank_h16.hip   BF16, F16
// Every kernel is rnnt_mblank_kernels.h's; rnnt_host.h and rnnt_side_host.h contribute only helpers (workspace alignment,
// the tuning constants, the call record and its checks, the cell-table workspace, the launch arithmetic).
#pragma once
#include "rnnt_side_host.h"
#include "rnnt_mblank_kernels.h"
#include "../../include/rnnt_mblank.h"

namespace rnnt {

// Workspace: the cell table of rnnt_side_host.h with records of mblank_rec_stride(K) lattice values.
static inline CellTableLayout mblank_layout(int maxT, int maxU, int N, int K, size_t lat) {
    return cell_table_layout(maxT, maxU, N, mblank_rec_stride(K), tdt_diags(maxT, maxU), lat);
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

// Stage 1: G lanes per row (stats_grid)
template <typename Tag>
static bool launch_mblank_stats(const typename Tag::store* acts, const int* labels, const int* xlen, const int* ylen,
                                typename Tag::comp* tab, int* poison, int N, int maxT, int maxU, int A,
                                const MbBlanks& bb, float sigma, hipStream_t s) {
    using C = typename Tag::comp;
    const StatsGrid sg = stats_grid(static_cast<size_t>(A) * sizeof(typename Tag::store), static_cast<long long>(maxT) * maxU);
    const C sigma2 = static_cast<C>(static_cast<double>(sigma) * kLog2e);
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid(sg.gx, grid_samples(N, b0));
        stats_dispatch(sg.G, [&](auto g) {
            hipLaunchKernelGGL((mblank_stats_kernel<Tag, decltype(g)::value>), grid, dim3(256), 0, s, acts,
                               labels, xlen, ylen, tab, maxT, maxU, A, bb, sigma2, b0, poison);
        });
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
    if (packets_aligned(acts, grads)) {
        const FlatGrid fg = flat_grid(E / V, 2, V);                    // (mblank_grad_kernel: PPT = 2)
        hipLaunchKernelGGL((mblank_grad_kernel<Tag>), dim3(fg.grid), dim3(256), 0, s, acts, grads, tab, grad_scale, E, A, RS,
                           bb, rps, 1.0f / static_cast<float>(A), fg.stride / A, static_cast<int>(fg.stride % A));
    } else {
        hipLaunchKernelGGL((mblank_grad_elem_kernel<Tag>), dim3(elem_grid(E)), dim3(256), 0, s, acts, grads, tab, grad_scale,
                           E, A, RS, bb, rps);
    }
    return hipGetLastError() == hipSuccess;
}

// The multi-blank loss of call `c` (SideCall: phases, host or device costs) with K big blanks.
template <typename Tag>
rnntStatus_t run_mblank(const SideCall& c, const int* columns, const int* durations, int K, float sigma) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const St* acts = static_cast<const St*>(c.acts);
    St* grads = static_cast<St*>(c.grads);
    const int *labels = c.labels, *label_lengths = c.label_lengths, *input_lengths = c.input_lengths;
    const int A = c.A, N = c.N, maxT = c.opt.maxT, maxU = c.opt.maxU, blank = c.opt.blank_label;
    (void)hipGetLastError();                           // a stale error of an unrelated earlier HIP call is not ours
    if (!mblank_shape_ok(A, N, maxT, maxU, blank) || !(sigma - sigma == 0.0f)) return RNNT_STATUS_INVALID_VALUE;
    MbBlanks bb;
    if (!mblank_blanks(columns, durations, K, A, blank, bb)) return RNNT_STATUS_INVALID_VALUE;
    bool do_fwd, do_bwd;
    if (!side_buffers_ok(c, sizeof(St), static_cast<unsigned long long>(N) * maxT * maxU * A, do_fwd, do_bwd))
        return RNNT_STATUS_INVALID_VALUE;
    const CellTable<C> w = carve_cell_table<C>(mblank_layout(maxT, maxU, N, K, sizeof(C)), c.workspace, c.costs_dev);
    hipStream_t s = reinterpret_cast<hipStream_t>(c.opt.stream);
    bool ok = true;

    if (do_fwd) {
        ok = ok && hipMemsetAsync(w.poison, 0, sizeof(int) * N, s) == hipSuccess;
        ok = ok && launch_mblank_stats<Tag>(acts, labels, input_lengths, label_lengths, w.tab, w.poison, N, maxT, maxU, A, bb,
                                            sigma, s);
        // lattice: a block per (sample, direction), a thread per cell of the widest diagonal (up to 1024)
        const int threads = maxU >= 1024 ? 1024 : (maxU + 63) / 64 * 64;
        for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
            hipLaunchKernelGGL((mblank_lattice_kernel<C>), dim3(grid_samples(N, b0), 2), dim3(threads), 0, s, w.tab, w.alpha,
                               w.beta, w.offa, w.offb, w.ll, input_lengths, label_lengths, w.poison, w.costs, bb, maxT, maxU,
                               b0);
            ok = hipGetLastError() == hipSuccess;
        }
        if (c.want_grad) {
            const unsigned gx = static_cast<unsigned>((static_cast<long long>(maxT) * maxU + 255) / 256);
            for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
                hipLaunchKernelGGL((mblank_coef_kernel<C>), dim3(gx, grid_samples(N, b0)), dim3(256), 0, s, w.tab, w.alpha,
                                   w.beta, w.offa, w.offb, w.ll, input_lengths, label_lengths, labels, w.poison, bb, maxT,
                                   maxU, A, b0);
                ok = hipGetLastError() == hipSuccess;
            }
        }
    }
    if (do_bwd && ok)
        ok = launch_mblank_grad<Tag>(acts, grads, w.tab, static_cast<const C*>(c.grad_scale), N, maxT, maxU, A, bb, s);
    if (!ok) return RNNT_STATUS_EXECUTION_FAILED;
    return c.costs_host != nullptr ? finish_host_costs(static_cast<C*>(c.costs_host), w.costs, N, s) : RNNT_STATUS_SUCCESS;
}

#ifndef RNNT_MBLANK_INSTANTIATE_F32
extern template rnntStatus_t run_mblank<F32>(const SideCall&, const int*, const int*, int, float);
#endif
#ifndef RNNT_MBLANK_INSTANTIATE_F64
extern template rnntStatus_t run_mblank<F64>(const SideCall&, const int*, const int*, int, float);
#endif
#ifndef RNNT_MBLANK_INSTANTIATE_H16
extern template rnntStatus_t run_mblank<BF16>(const SideCall&, const int*, const int*, int, float);
extern template rnntStatus_t run_mblank<F16>(const SideCall&, const int*, const int*, int, float);
#endif

}  // namespace rnnt
