// rnnt_side_host.h -- what the host drivers of the side libraries share on top of rnnt_host.h (the four losses -- pruned,
// TDT, HAT, multi-blank -- all of it; the TDT alignment the dtype switch, the cell table and the launch arithmetic): the
// call record their C entry points fill (SideCall), the dtype switch (side_dispatch), the buffer checks of every run_X
// (side_buffers_ok), the buffer and lattice-size checks of the px / py libraries' C entries (SideBuf, side_bad_buffers,
// side_lattice_ok: bestpath, expect, sample, ranges), the cell-table workspace of TDT and multi-blank, and the launch
// arithmetic of the statistics and gradient launchers.  Host code only: no kernel is named here, so a library's code objects hold exactly the kernels its
// own rnnt_X_impl.h launches.
#pragma once
#include <type_traits>

#include "rnnt_host.h"

namespace rnnt {

// ----------------------------------------------------------------------------- the call record
// The arguments every side loss takes, untyped as they cross the C-ABI.  run_X<Tag>(call, <the library's own arguments>)
// casts acts / grads to Tag::store and grad_scale / costs_* to Tag::comp at its top.  phases: bit 0 = forward, bit 1 =
// gradient stream from the workspace a forward call left.  costs_host != nullptr: the one-call entry with costs in host
// memory; costs_dev == nullptr: the costs go to the workspace.
struct SideCall {
    const void* acts;
    void* grads;
    const void* grad_scale;
    void *costs_dev, *costs_host, *workspace;
    const int *labels, *label_lengths, *input_lengths;
    int A, N;
    rnntOptions opt;
    int phases;
    bool want_grad;
};

// The dtype codes of include/rnnt_*.h: run(tag) with tag an F32 / F64 / BF16 / F16 value, any other code refused.
template <typename F> static inline rnntStatus_t side_dispatch(int dtype_code, F&& run) {
    switch (dtype_code) {
        case 0: return run(F32{});
        case 1: return run(F64{});
        case 2: return run(BF16{});
        case 3: return run(F16{});
        default: return RNNT_STATUS_INVALID_VALUE;
    }
}

// The phases of a call and the checks on its two tensors of `elems` elements of `elem_size` bytes: gradients present when
// the gradient stream runs, both pointers on element boundaries, and the gradients either in place or not overlapping the
// activations at all.  false: the call is refused.
static inline bool side_buffers_ok(const SideCall& c, size_t elem_size, unsigned long long elems, bool& do_fwd,
                                   bool& do_bwd) {
    do_fwd = (c.phases & 1) != 0;
    do_bwd = (c.phases & 2) != 0 && c.want_grad;
    if (do_bwd && c.grads == nullptr) return false;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(c.acts), pg = reinterpret_cast<uintptr_t>(c.grads);
    if (pa % elem_size != 0 || (c.grads != nullptr && pg % elem_size != 0)) return false;
    if (do_bwd && pg != pa && (pg > pa ? pg - pa : pa - pg) < elems * elem_size) return false;
    return true;
}

// ----------------------------------------------------------------------------- the px / py libraries' checks
// (bestpath, expect, sample, ranges: no call record in common, no workspace; every array is an argument of its own)
// A buffer of a call: [p, p + bytes), `elem` the size its address must be a multiple of; p == nullptr: not given.
struct SideBuf { const void* p; unsigned long long bytes, elem; };

static inline bool side_overlap(const SideBuf& a, const SideBuf& b) {
    if (a.p == nullptr || b.p == nullptr || a.bytes == 0 || b.bytes == 0) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a.p), y = reinterpret_cast<uintptr_t>(b.p);
    return x < y + b.bytes && y < x + a.bytes;
}

// Every given buffer on an element boundary; no output sharing a byte with an input or another output (inputs may alias
// inputs).  true: refused.
static inline bool side_bad_buffers(const SideBuf* in, int nin, const SideBuf* out, int nout) {
    for (int i = 0; i < nin; ++i)
        if (in[i].p != nullptr && reinterpret_cast<uintptr_t>(in[i].p) % in[i].elem != 0) return true;
    for (int i = 0; i < nout; ++i) {
        if (out[i].p != nullptr && reinterpret_cast<uintptr_t>(out[i].p) % out[i].elem != 0) return true;
        for (int j = 0; j < nin; ++j)
            if (side_overlap(out[i], in[j])) return true;
        for (int j = i + 1; j < nout; ++j)
            if (side_overlap(out[i], out[j])) return true;
    }
    return false;
}

// The LIMITS of include/rnnt_{bestpath,expect,sample,ranges}.h on the lattice of a (B, S, T) call: S + 1 <= maxU,
// (T + 1) (S + 1) < 2^25, B (T + 1) (S + 1) < 2^32.
static inline bool side_lattice_ok(int S, int T, int N, int maxU) {
    if (S < 0 || T < 1 || N < 1 || S + 1 > maxU) return false;
    const unsigned long long nodes = static_cast<unsigned long long>(T + 1LL) * (S + 1LL);
    return nodes < (1ull << 25) && nodes * N < (1ull << 32);
}

// ----------------------------------------------------------------------------- entry points
// The common arguments of the three call forms into `c`; true: refused (RNNT_STATUS_INVALID_VALUE).  A library's own
// arguments (ranges, durations, big blanks) are checked by its entry or its run_X.
// One call: forward and, with gradients, the gradient stream; costs in device or in host memory.
static inline bool side_entry_loss(SideCall& c, const void* acts, void* grads, const int* labels, const int* label_lengths,
                                   const int* input_lengths, int A, int N, void* costs, void* workspace,
                                   const rnntOptions& o) {
    if (bad_args(acts, labels, label_lengths, input_lengths, costs, workspace, A, N, o) || loc_of(o) != RNNT_GPU) return true;
    const bool dev = is_device_pointer(costs);
    c = {acts, grads, nullptr, dev ? costs : nullptr, dev ? nullptr : costs, workspace, labels, label_lengths, input_lengths,
         A, N, o, 3, grads != nullptr};
    return false;
}

// _fwd: the forward phase, costs in device memory; prepare_backward leaves the gradient records for _bwd.
static inline bool side_entry_fwd(SideCall& c, const void* acts, const int* labels, const int* label_lengths,
                                  const int* input_lengths, int A, int N, void* costs_device, void* workspace,
                                  const rnntOptions& o, int prepare_backward) {
    if (bad_args(acts, labels, label_lengths, input_lengths, costs_device, workspace, A, N, o) || loc_of(o) != RNNT_GPU)
        return true;
    c = {acts, nullptr, nullptr, costs_device, nullptr, workspace, labels, label_lengths, input_lengths, A, N, o, 1,
         prepare_backward != 0};
    return false;
}

// _bwd: the gradient stream from the workspace of a _fwd call.
static inline bool side_entry_bwd(SideCall& c, const void* acts, void* grads, const void* grad_scale_device, int A, int N,
                                  void* workspace, const rnntOptions& o) {
    if (acts == nullptr || grads == nullptr || workspace == nullptr || A <= 0 || N <= 0 || o.maxT <= 0 || o.maxU <= 0 ||
        loc_of(o) != RNNT_GPU)
        return true;
    c = {acts, grads, grad_scale_device, nullptr, nullptr, workspace, nullptr, nullptr, nullptr, A, N, o, 2, true};
    return false;
}

// ----------------------------------------------------------------------------- the cell-table workspace (TDT, multi-blank)
// The cell table (stats, then the gradient records in place: rec_stride lattice values per cell), alpha, beta, the
// per-diagonal offsets of both directions (`diags` per sample), log P, the costs of the host-costs entry and the poison
// flags.  lat = bytes of one lattice value.
struct CellTableLayout { size_t tab, alpha, beta, offa, offb, ll, costs, poison, total; };
static inline CellTableLayout cell_table_layout(int maxT, int maxU, int N, int rec_stride, int diags, size_t lat) {
    const size_t cells = static_cast<size_t>(N) * maxT * maxU;
    const size_t ndiags = static_cast<size_t>(N) * diags;
    CellTableLayout l;
    size_t o = 0;
    l.tab = o; o = align_up(o + cells * rec_stride * lat);
    l.alpha = o; o = align_up(o + cells * lat);
    l.beta = o; o = align_up(o + cells * lat);
    l.offa = o; o = align_up(o + ndiags * sizeof(double));
    l.offb = o; o = align_up(o + ndiags * sizeof(double));
    l.ll = o; o = align_up(o + static_cast<size_t>(N) * sizeof(double));
    l.costs = o; o = align_up(o + static_cast<size_t>(N) * sizeof(double));     // (host costs: the device copy)
    l.poison = o; o = align_up(o + static_cast<size_t>(N) * sizeof(int));
    l.total = o + kAlign;                                  // slack to align the caller's base pointer
    return l;
}

// The arrays of a layout in the caller's workspace; costs: the caller's device array, or the workspace's.
template <typename C> struct CellTable { C *tab, *alpha, *beta; double *offa, *offb, *ll; int* poison; C* costs; };
template <typename C> static inline CellTable<C> carve_cell_table(const CellTableLayout& l, void* workspace, void* costs_dev) {
    char* ws = reinterpret_cast<char*>(align_up(reinterpret_cast<size_t>(workspace)));
    return {reinterpret_cast<C*>(ws + l.tab), reinterpret_cast<C*>(ws + l.alpha), reinterpret_cast<C*>(ws + l.beta),
            reinterpret_cast<double*>(ws + l.offa), reinterpret_cast<double*>(ws + l.offb),
            reinterpret_cast<double*>(ws + l.ll), reinterpret_cast<int*>(ws + l.poison),
            costs_dev != nullptr ? static_cast<C*>(costs_dev) : reinterpret_cast<C*>(ws + l.costs)};
}

// ----------------------------------------------------------------------------- launch arithmetic
// Samples of the launch that starts at sample b0: the batch goes over a grid dimension in chunks of kGridSamples.
static inline int grid_samples(int N, int b0) { return N - b0 < kGridSamples ? N - b0 : kGridSamples; }

// Statistics kernels: G lanes per row, the smallest group that keeps a lane's share of the row's packets at a few rounds
// (4 up to 256 bytes, 16 up to `wide_bytes`, else 64), and the blocks of 256 threads that cover `rows` rows of a sample.
struct StatsGrid { int G; unsigned gx; };
static inline StatsGrid stats_grid(size_t row_bytes, long long rows, size_t wide_bytes = 2048) {
    const int G = row_bytes <= 256 ? 4 : row_bytes <= wide_bytes ? 16 : 64;
    return {G, static_cast<unsigned>((rows * G + 255) / 256)};
}
// The group size as a template argument: launch(std::integral_constant<int, G>) for G = 4, 16, 64 (any other: 64).  The
// kernel and its hipLaunchKernelGGL stay in the library's callable.
template <typename F> static inline void stats_dispatch(int G, F&& launch) {
    if (G == 4) launch(std::integral_constant<int, 4>{});
    else if (G == 16) launch(std::integral_constant<int, 16>{});
    else launch(std::integral_constant<int, 64>{});
}

// Gradient kernels: the flat packet stream needs both tensors on 16-byte boundaries; the element-wise form takes a
// grid-stride loop of at most 65536 blocks of 256 threads over E elements.
static inline bool packets_aligned(const void* acts, const void* grads) {
    return ((reinterpret_cast<uintptr_t>(acts) | reinterpret_cast<uintptr_t>(grads)) & 15u) == 0;
}
static inline unsigned elem_grid(unsigned long long E) {
    const unsigned long long blocks = (E + 255) / 256;
    return static_cast<unsigned>(blocks < 65536 ? (blocks ? blocks : 1) : 65536);
}

}  // namespace rnnt
