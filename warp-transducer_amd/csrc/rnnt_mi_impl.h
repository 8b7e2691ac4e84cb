// rnnt_mi_impl.h -- host driver of libwarprnnt_mi.so (include/rnnt_mi.h): the lattice primitive on px / py edge
// log-probabilities (run_mi<Tag>).  One instantiation per storage type, each in a translation unit -- a code object -- of
// its own:
//     rnnt_mi.hip   F32 (+ every C entry point)     rnnt_mi_f64.hip   F64     rnnt_mi_h16.hip   BF16, F16
// Stages 1 and 3 and the score kernel are rnnt_mi_kernels.h's, stage 2 the lattice kernels of rnnt_ar_kernels.h (regular
// type) and rnnt_mono_kernels.h (modified type), instantiated in this library's code objects.  The dtype switch, the
// cell-table workspace and the launch arithmetic are rnnt_side_host.h's; the call record is this library's own (MiCall: it
// has two inputs, two gradients and no labels).
#pragma once
#include "rnnt_side_host.h"
#include "rnnt_mi_kernels.h"
#include "../../include/rnnt_mi.h"

namespace rnnt {

constexpr int kMiMaxU = 4096;           // S + 1 at most: the block form's thread-strided columns, as the other side libraries

// The arguments of every call form, untyped as they cross the C-ABI.  phases: bit 0 = forward, bit 1 = the gradients from
// the workspace a forward call left.  scores_host != nullptr: the one-call entry with scores in host memory.
struct MiCall {
    const void *px, *py, *boundary;
    void *px_grad, *py_grad;
    const void* grad_scale;
    void *scores_dev, *scores_host, *workspace;
    int S, T, N;
    bool modified;
    rnntOptions opt;
    int phases;
    bool want_grad;
};

static inline bool mi_shape_ok(int S, int T, int N) {
    if (S < 0 || T < 1 || N < 1 || S + 1 > kMiMaxU) return false;
    const unsigned long long nodes = static_cast<unsigned long long>(T + 1LL) * (S + 1LL);
    return nodes < (1ull << 25) && nodes * N < (1ull << 32);
}

// The table's frame axis: T + 1 node columns in the regular type (the last one's symbol edges are real), T in the modified.
static inline int mi_table_t(int T, bool modified) { return modified ? T : T + 1; }

// Workspace: the cell table of rnnt_side_host.h with four-word records and the offsets of the type's lattice (one per
// diagonal and the terminal one, or one per frame and the terminal row); behind it this library's own arrays: the derived
// lengths xlen, ylen, the rectangles' origins (s0, t0) and the scores of the host-scores entry (the table's own `costs`
// array takes what the lattice kernels close a sample with).
struct MiLayout { CellTableLayout cells; size_t xlen, ylen, org, scores, total; };
static inline MiLayout mi_layout(int S, int T, int N, bool modified, size_t lat) {
    const int maxTt = mi_table_t(T, modified), maxU = S + 1;
    MiLayout m;
    m.cells = cell_table_layout(maxTt, maxU, N, kMiRec, modified ? mono_offsets(maxTt) : ar_offsets(maxTt, maxU), lat);
    const size_t ints = static_cast<size_t>(N) * sizeof(int);
    size_t o = m.cells.total - kAlign;                     // (the table's arrays end here; its alignment slack moves behind ours)
    m.xlen = o; o = align_up(o + ints);
    m.ylen = o; o = align_up(o + ints);
    m.org = o; o = align_up(o + 2 * ints);
    m.scores = o; o = align_up(o + static_cast<size_t>(N) * sizeof(double));
    m.total = o + kAlign;
    return m;
}
struct MiArrays { int *xlen, *ylen, *org; void* scores; };
static inline MiArrays carve_mi_arrays(const MiLayout& m, void* workspace) {
    char* ws = reinterpret_cast<char*>(align_up(reinterpret_cast<size_t>(workspace)));
    return {reinterpret_cast<int*>(ws + m.xlen), reinterpret_cast<int*>(ws + m.ylen), reinterpret_cast<int*>(ws + m.org),
            ws + m.scores};
}

// [p, p + n) and [q, q + m) share a byte (an empty range shares none)
static inline bool mi_overlap(const void* p, unsigned long long n, const void* q, unsigned long long m) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return n != 0 && m != 0 && a < b + m && b < a + n;
}

// Stage 2, the release rule of both lattices restated (launch_ar_lattice, launch_mono_lattice): up to kArWaveMaxU ==
// kMonoWaveMaxU lattice columns one wavefront per (sample, direction) keeps the sweep in registers; wider lattices take a
// block per (sample, direction), a thread per column up to 1024.  dirs = 1: the forward sweep alone (a score-only call).
template <typename C>
static bool launch_mi_lattice(const CellTable<C>& w, const int* xlen, const int* ylen, int N, int maxTt, int maxU,
                              bool modified, int dirs, hipStream_t s) {
    static_assert(kArWaveMaxU == kMonoWaveMaxU, "one release rule for both lattices");
    const bool wave = maxU <= kArWaveMaxU;
    const dim3 threads(wave ? 64 : (maxU >= 1024 ? 1024 : (maxU + 63) / 64 * 64));
    for (int b0 = 0; b0 < N; b0 += kGridSamples) {
        const dim3 grid(grid_samples(N, b0), dirs);
#define RNNT_MI_LATTICE(KERNEL)                                                                                         \
        hipLaunchKernelGGL((KERNEL<C>), grid, threads, 0, s, w.tab, w.alpha, w.beta, w.offa, w.offb, w.ll, xlen, ylen,  \
                           w.poison, w.costs, maxTt, maxU, b0)
        if (modified) { if (wave) RNNT_MI_LATTICE(mono_lattice_wave_kernel); else RNNT_MI_LATTICE(mono_lattice_block_kernel); }
        else { if (wave) RNNT_MI_LATTICE(ar_lattice_wave_kernel); else RNNT_MI_LATTICE(ar_lattice_block_kernel); }
#undef RNNT_MI_LATTICE
    }
    return hipGetLastError() == hipSuccess;
}

// The call `c` (MiCall: phases, host or device scores).
template <typename Tag>
rnntStatus_t run_mi(const MiCall& c) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    const int S = c.S, T = c.T, N = c.N;
    (void)hipGetLastError();                               // a stale error of an unrelated earlier HIP call is not ours
    if (!mi_shape_ok(S, T, N)) return RNNT_STATUS_INVALID_VALUE;
    const bool mod = c.modified;
    const int maxTt = mi_table_t(T, mod), maxU = S + 1;
    const bool do_fwd = (c.phases & 1) != 0, do_bwd = (c.phases & 2) != 0 && c.want_grad;
    const unsigned long long xb = static_cast<unsigned long long>(N) * S * maxTt * sizeof(St);
    const unsigned long long yb = static_cast<unsigned long long>(N) * maxU * T * sizeof(St);
    const MiLayout lay = mi_layout(S, T, N, mod, sizeof(C));
    const auto off_element = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % sizeof(St) != 0; };
    if (do_fwd && ((S > 0 && (c.px == nullptr || off_element(c.px))) || c.py == nullptr || off_element(c.py) ||
                   (c.boundary != nullptr && reinterpret_cast<uintptr_t>(c.boundary) % sizeof(long long) != 0)))
        return RNNT_STATUS_INVALID_VALUE;
    if (do_bwd) {
        if ((S > 0 && (c.px_grad == nullptr || off_element(c.px_grad))) || c.py_grad == nullptr || off_element(c.py_grad))
            return RNNT_STATUS_INVALID_VALUE;
        const void* const in[] = {do_fwd ? c.px : nullptr, do_fwd ? c.py : nullptr, c.workspace};
        const unsigned long long inb[] = {xb, yb, lay.total};
        for (int i = 0; i < 3; ++i)
            if (in[i] != nullptr && (mi_overlap(c.px_grad, xb, in[i], inb[i]) || mi_overlap(c.py_grad, yb, in[i], inb[i])))
                return RNNT_STATUS_INVALID_VALUE;
        if (mi_overlap(c.px_grad, xb, c.py_grad, yb)) return RNNT_STATUS_INVALID_VALUE;
        if (do_fwd && c.boundary != nullptr) {
            const unsigned long long bb = static_cast<unsigned long long>(N) * 4 * sizeof(long long);
            if (mi_overlap(c.px_grad, xb, c.boundary, bb) || mi_overlap(c.py_grad, yb, c.boundary, bb))
                return RNNT_STATUS_INVALID_VALUE;
        }
    }
    const MiArrays m = carve_mi_arrays(lay, c.workspace);
    const CellTable<C> w = carve_cell_table<C>(lay.cells, c.workspace, nullptr);     // (costs: the workspace's own array)
    C* scores = c.scores_dev != nullptr ? static_cast<C*>(c.scores_dev) : static_cast<C*>(m.scores);
    hipStream_t s = reinterpret_cast<hipStream_t>(c.opt.stream);
    const unsigned tiles_u = (maxU + kMiTile - 1) / kMiTile, tiles_t = (maxTt + kMiTile - 1) / kMiTile;
    bool ok = true;

    if (do_fwd) {
        ok = ok && hipMemsetAsync(w.poison, 0, sizeof(int) * N, s) == hipSuccess;
        for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
            const dim3 grid(tiles_u * tiles_t, grid_samples(N, b0));
#define RNNT_MI_PACK(MOD)                                                                                               \
            hipLaunchKernelGGL((mi_pack_kernel<Tag, MOD>), grid, dim3(256), 0, s, static_cast<const St*>(c.px),          \
                               static_cast<const St*>(c.py), static_cast<const long long*>(c.boundary), w.tab, m.xlen,   \
                               m.ylen, m.org, w.poison, S, T, static_cast<int>(tiles_u), b0)
            if (mod) RNNT_MI_PACK(true); else RNNT_MI_PACK(false);
#undef RNNT_MI_PACK
            ok = hipGetLastError() == hipSuccess;
        }
        ok = ok && launch_mi_lattice<C>(w, m.xlen, m.ylen, N, maxTt, maxU, mod, c.want_grad ? 2 : 1, s);
        if (ok) {
            hipLaunchKernelGGL((mi_score_kernel<C>), dim3((N + 255) / 256), dim3(256), 0, s, w.ll, m.xlen, m.ylen, w.poison,
                               scores, N);
            ok = hipGetLastError() == hipSuccess;
        }
    }
    if (do_bwd) {
        for (int b0 = 0; b0 < N && ok; b0 += kGridSamples) {
            const dim3 grid(tiles_u * tiles_t, grid_samples(N, b0));
#define RNNT_MI_UNPACK(MOD)                                                                                             \
            hipLaunchKernelGGL((mi_unpack_kernel<Tag, MOD>), grid, dim3(256), 0, s, static_cast<St*>(c.px_grad),         \
                               static_cast<St*>(c.py_grad), static_cast<const C*>(c.grad_scale), w.tab, w.alpha, w.beta, \
                               w.offa, w.offb, w.ll, m.xlen, m.ylen, m.org, w.poison, S, T, static_cast<int>(tiles_u), b0)
            if (mod) RNNT_MI_UNPACK(true); else RNNT_MI_UNPACK(false);
#undef RNNT_MI_UNPACK
            ok = hipGetLastError() == hipSuccess;
        }
    }
    if (!ok) return RNNT_STATUS_EXECUTION_FAILED;
    return c.scores_host != nullptr ? finish_host_costs(static_cast<C*>(c.scores_host), scores, N, s) : RNNT_STATUS_SUCCESS;
}

#ifndef RNNT_MI_INSTANTIATE_F32
extern template rnntStatus_t run_mi<F32>(const MiCall&);
#endif
#ifndef RNNT_MI_INSTANTIATE_F64
extern template rnntStatus_t run_mi<F64>(const MiCall&);
#endif
#ifndef RNNT_MI_INSTANTIATE_H16
extern template rnntStatus_t run_mi<BF16>(const MiCall&);
extern template rnntStatus_t run_mi<F16>(const MiCall&);
#endif

}  // namespace rnnt
