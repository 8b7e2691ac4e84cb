// rnnt_kd_impl.h -- host driver of libwarprnnt_kd.so (include/rnnt_kd.h): the transducer lattice distillation loss
// (run_kd<Tag>).  One instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_kd.hip   F32 (+ every C entry point)     rnnt_kd_f64.hip   F64     rnnt_kd_h16.hip   BF16, F16
// The kernels are rnnt_kd_kernels.h's.  There is no lattice, so neither the plan nor the workspace of rnnt_host.h is used:
// the layout below holds one record, one label word and one KL value per row, two values per sample and one word per batch.  The call record,
// the dtype switch and the launch arithmetic are rnnt_side_host.h's; the buffer check is its side_buffers_ok with the
// teacher as a third tensor.
#pragma once
#include <cmath>

#include "rnnt_side_host.h"
#include "rnnt_kd_kernels.h"
#include "../../include/rnnt_kd.h"

namespace rnnt {

// The limits of include/rnnt_kd.h: a column besides the blank, 32-bit row arithmetic inside a sample (and the statistics
// grid), the gradient stream's 32-bit row index and reciprocal division.
static inline bool kd_shape_ok(int A, int N, int maxT, int maxU) {
    if (A < 2 || A > (1 << 23) || N < 1 || maxT < 1 || maxU < 1) return false;
    if (static_cast<unsigned long long>(maxT) * maxU >= (1ull << 31)) return false;
    return static_cast<unsigned long long>(N) * maxT * maxU < (1ull << 32);
}
static inline bool kd_params_ok(int mode, float temperature) {
    return (mode == 0 || mode == 1) && std::isfinite(temperature) && temperature > 0.0f;
}

// ----------------------------------------------------------------------------- workspace
// Per row: the record (four values), the label word, the KL.  Per sample: the cost of the entries without a device cost
// array and the gradient multiplier; per batch the "some row is padding" word.  lat = bytes of one value (4 | 8).  The same
// for both modes.
struct KdLayout { size_t rec, lab, kl, costs, smul, padflag, total; };
static inline KdLayout kd_layout(int maxT, int maxU, int N, size_t lat) {
    const size_t rows = static_cast<size_t>(N) * maxT * maxU;
    KdLayout l;
    size_t o = 0;
    l.rec = o; o = align_up(o + rows * 4 * lat);
    l.lab = o; o = align_up(o + rows * sizeof(int));
    l.kl = o; o = align_up(o + rows * lat);
    l.costs = o; o = align_up(o + static_cast<size_t>(N) * sizeof(double));
    l.smul = o; o = align_up(o + static_cast<size_t>(N) * sizeof(double));
    l.padflag = o; o = align_up(o + sizeof(int));
    l.total = o + kAlign;                                  // slack to align the caller's base pointer
    return l;
}

// side_buffers_ok for three tensors: the teacher on an element boundary, the same tensor as the activations or apart from
// them, and never under the gradients.  `full`: mode 1, whose gradient stream reads the teacher; a backward-only call of
// collapsed mode does not, and may pass NULL for it.
static inline bool kd_buffers_ok(const SideCall& c, const void* teacher, bool full, size_t elem_size,
                                 unsigned long long elems, bool& do_fwd, bool& do_bwd) {
    if (!side_buffers_ok(c, elem_size, elems, do_fwd, do_bwd)) return false;
    if (teacher == nullptr) return !do_fwd && !full;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(c.acts), pg = reinterpret_cast<uintptr_t>(c.grads),
                    pt = reinterpret_cast<uintptr_t>(teacher);
    const unsigned long long bytes = elems * elem_size;
    if (pt % elem_size != 0) return false;
    if (pt != pa && (pt > pa ? pt - pa : pa - pt) < bytes) return false;
    if (do_bwd && (pg > pt ? pg - pt : pt - pg) < bytes) return false;
    return true;
}

// ----------------------------------------------------------------------------- launchers
// Stage 1: G lanes per row by stats_grid's rule at its default threshold: 4 lanes for rows up to 256 bytes, 16 up to 2048
// bytes, 64 beyond.  (HAT keeps rows up to 4096 bytes on 16 lanes; here a lane has the packets of TWO rows in flight, so the
// wider group starts at half that.)
constexpr size_t kKdWideRowBytes = 2048;
template <typename Tag, int Mode>
static bool launch_kd_stats(const SideCall& c, const typename Tag::store* acts, const typename Tag::store* teach,
                            Cell<typename Tag::comp>* rec, int* lab, typename Tag::comp* kl, int* padflag,
                            typename Tag::comp it) {
    const hipStream_t stream = reinterpret_cast<hipStream_t>(c.opt.stream);
    const long long TU = static_cast<long long>(c.opt.maxT) * c.opt.maxU;
    const StatsGrid sg = stats_grid(static_cast<size_t>(c.A) * sizeof(typename Tag::store), TU, kKdWideRowBytes);
    for (int b0 = 0; b0 < c.N; b0 += kGridSamples) {
        const dim3 grid(sg.gx, grid_samples(c.N, b0));
        stats_dispatch(sg.G, [&](auto g) {
            hipLaunchKernelGGL((kd_stats_kernel<Tag, decltype(g)::value, Mode>), grid, dim3(256), 0, stream,
                               acts, teach, c.labels, c.input_lengths, c.label_lengths, rec, lab, kl, padflag, c.opt.maxT,
                               c.opt.maxU, c.A, c.opt.blank_label, b0, it);
        });
    }
    return hipGetLastError() == hipSuccess;
}

// Stage 3: the flat packet stream when every tensor it touches sits on a 16-byte boundary (collapsed mode does not touch
// the teacher), else element by element
template <typename Tag, int Mode>
static bool launch_kd_grad(const SideCall& c, const typename Tag::store* acts, const typename Tag::store* teach,
                           typename Tag::store* grads, const Cell<typename Tag::comp>* rec, const int* lab,
                           const typename Tag::comp* smul, const int* padflag, typename Tag::comp it) {
    using C = typename Tag::comp;
    constexpr int V = Vec<Tag>::N;
    const hipStream_t stream = reinterpret_cast<hipStream_t>(c.opt.stream);
    const unsigned TU = static_cast<unsigned>(c.opt.maxT * c.opt.maxU);
    const unsigned R = static_cast<unsigned>(static_cast<unsigned long long>(c.N) * TU);
    const unsigned long long E = static_cast<unsigned long long>(R) * c.A;
    const C* scale = static_cast<const C*>(c.grad_scale);
    if (packets_aligned(acts, grads) && (Mode == 0 || packets_aligned(teach, grads))) {
        const FlatGrid fg = flat_grid(E / V, 2, V);                    // (kd_grad_kernel: PPT = 2)
        hipLaunchKernelGGL((kd_grad_kernel<Tag, Mode>), dim3(fg.grid), dim3(256), 0, stream, acts, teach, grads, rec, lab,
                           smul, padflag, scale, E, R, c.A, c.opt.blank_label, TU, 1.0f / static_cast<float>(c.A),
                           fg.stride / c.A, static_cast<int>(fg.stride % c.A), it);
    } else {
        hipLaunchKernelGGL((kd_grad_elem_kernel<Tag, Mode>), dim3(elem_grid(E)), dim3(256), 0, stream, acts, teach, grads, rec,
                           lab, smul, scale, E, c.A, c.opt.blank_label, TU, it);
    }
    return hipGetLastError() == hipSuccess;
}

// The distillation loss of call `c` (SideCall: phases, host or device costs) against `teacher`.
template <typename Tag, int Mode>
rnntStatus_t run_kd_mode(const SideCall& c, const void* teacher, float temperature) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const St* acts = static_cast<const St*>(c.acts);
    const St* teach = static_cast<const St*>(teacher);
    St* grads = static_cast<St*>(c.grads);
    bool do_fwd, do_bwd;
    if (!kd_buffers_ok(c, teacher, Mode == 1, sizeof(St),
                       static_cast<unsigned long long>(c.N) * c.opt.maxT * c.opt.maxU * c.A, do_fwd, do_bwd))
        return RNNT_STATUS_INVALID_VALUE;
    (void)hipGetLastError();                       // a stale error of an unrelated earlier HIP call is not ours
    const hipStream_t stream = reinterpret_cast<hipStream_t>(c.opt.stream);
    const KdLayout lay = kd_layout(c.opt.maxT, c.opt.maxU, c.N, sizeof(C));
    char* ws = reinterpret_cast<char*>(align_up(reinterpret_cast<size_t>(c.workspace)));
    Cell<C>* rec = reinterpret_cast<Cell<C>*>(ws + lay.rec);
    int* lab = reinterpret_cast<int*>(ws + lay.lab);
    C* kl = reinterpret_cast<C*>(ws + lay.kl);
    C* smul = reinterpret_cast<C*>(ws + lay.smul);
    int* padflag = reinterpret_cast<int*>(ws + lay.padflag);
    C* costs = c.costs_dev != nullptr ? static_cast<C*>(c.costs_dev) : reinterpret_cast<C*>(ws + lay.costs);
    const C it = C(1) / static_cast<C>(temperature);
    bool ok = true;
    if (do_fwd) {
        ok = launch_kd_stats<Tag, Mode>(c, acts, teach, rec, lab, kl, padflag, it);
        if (ok) {
            hipLaunchKernelGGL((kd_cost_kernel<C>), dim3(c.N), dim3(256), 0, stream, kl, c.input_lengths, c.label_lengths,
                               costs, smul, padflag, c.opt.maxT, c.opt.maxU);
            ok = hipGetLastError() == hipSuccess;
        }
    }
    if (do_bwd && ok) ok = launch_kd_grad<Tag, Mode>(c, acts, teach, grads, rec, lab, smul, padflag, it);
    if (!ok) return RNNT_STATUS_EXECUTION_FAILED;
    return c.costs_host != nullptr ? finish_host_costs(static_cast<C*>(c.costs_host), costs, c.N, stream)
                                   : RNNT_STATUS_SUCCESS;
}

template <typename Tag>
rnntStatus_t run_kd(const SideCall& c, const void* teacher, int mode, float temperature) {
    if (!kd_params_ok(mode, temperature) || !kd_shape_ok(c.A, c.N, c.opt.maxT, c.opt.maxU) || c.opt.blank_label < 0 ||
        c.opt.blank_label >= c.A)
        return RNNT_STATUS_INVALID_VALUE;
    return mode == 0 ? run_kd_mode<Tag, 0>(c, teacher, temperature) : run_kd_mode<Tag, 1>(c, teacher, temperature);
}

#ifndef RNNT_KD_INSTANTIATE_F32
extern template rnntStatus_t run_kd<F32>(const SideCall&, const void*, int, float);
#endif
#ifndef RNNT_KD_INSTANTIATE_F64
extern template rnntStatus_t run_kd<F64>(const SideCall&, const void*, int, float);
#endif
#ifndef RNNT_KD_INSTANTIATE_H16
extern template rnntStatus_t run_kd<BF16>(const SideCall&, const void*, int, float);
extern template rnntStatus_t run_kd<F16>(const SideCall&, const void*, int, float);
#endif

}  // namespace rnnt
