// rnnt_row_lse.h -- what the statistics kernels (stage 1) of the side libraries share: the log-sum-exp of one row of
// logits by a group of G lanes (row_lse), and the label of a lattice row (row_label).  Device functions only: no kernel is
// named here, so a library's code objects hold exactly the kernels its own rnnt_X_kernels.h defines.  DESIGN.md 8s.
#pragma once

#include <type_traits>

#include "rnnt_kernels.h"             // absorb; through it rnnt_device.h

namespace rnnt {

// Label u of sample b from the (N, maxU - 1) label array, clamped into [0, A): an out-of-range label reads a column of its
// own row, never another row.
__device__ __forceinline__ int row_label(const int* __restrict__ labels, int b, int u, int maxU, int A) {
    const int lab = labels[static_cast<size_t>(b) * (maxU - 1) + u];
    return lab < 0 ? 0 : (lab >= A ? A - 1 : lab);
}

// What row_lse returns, on every lane of the group: sum of exp(x - shift) over the row, shift = max x (0 when every
// element is -inf, so that log() is -inf and not NaN).
template <typename C> struct RowLse {
    C shift, sum;
    __device__ __forceinline__ C log() const { return shift + acc_log(sum); }
};

struct RowNoHook {};                   // the default per-element hook: none, and no code for one

// The row `row` of A elements, reduced by the G lanes (G = 4, 16, 64; gl = this lane's index in its group, every lane of
// the group calls) to its log-normaliser.  The row may start anywhere: the aligned 16-byte packets that COVER it are
// loaded, `skip` elements of the first one and the tail of the last one belong to the neighbouring rows and are masked to
// -inf (one unsigned compare: column = stream index - skip, outside [0, A)).  A packet never leaves the 16-byte granule of
// an element of this row, so nothing outside the tensor's own allocation granules is touched.  Lane gl takes the packets
// gl, gl + G, ..., four per round, and ALL FOUR LOADS OF A ROUND ARE ISSUED BEFORE THE FIRST unpack: a load written behind
// the masking branch of the previous packet is a memory round trip of its own (rnnt_kernels.h, row_stats_kernel), four per
// round in place of one.  Then absorb<C, 4 * V> (one rescale per round) and the combine over the group: max-shuffle,
// shift, s * exp(m - shift), sum-shuffle.
//
// hook(col, x) -- optional -- is called for every element of the row with its column in [0, A) and its value; true
// excludes the element from the sum (HAT keeps the blank logit and masks it).  Without a hook there is no code for one.
// A hook that tests col against a column the caller knows to lie in [0, A) costs nothing either once the caller says so
// (__builtin_assume): the range gate in front of it folds away.  The gate and the hook stay two statements: as one ||
// the hook's store became a branch per element (hat_stats_kernel<BF16>: 124 VGPRs against 50).
template <typename Tag, int G, typename Hook = RowNoHook>
__device__ __forceinline__ RowLse<typename Tag::comp> row_lse(const typename Tag::store* row, int A, int gl,
                                                              Hook hook = Hook{}) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    constexpr int V = Vec<Tag>::N;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(row);
    const int skip = static_cast<int>((addr & 15u) / sizeof(St));                 // elements of the first packet before the row
    const u32x4* vp = reinterpret_cast<const u32x4*>(addr & ~static_cast<uintptr_t>(15));
    const int npk = (skip + A + V - 1) / V;
    C m = neg_inf<C>(), s = 0;
    for (int base = 0; base < npk; base += 4 * G) {
        uint4 raw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                                             // all loads of the round first
            const int i = base + gl + j * G;
            raw[j] = make_uint4(0, 0, 0, 0);
            if (i < npk) raw[j] = load_packet<true>(vp + i);
        }
        C v[4 * V];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = base + gl + j * G;
            unpack<Tag>(raw[j], v + j * V);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int col = i * V + e - skip;
                bool out = static_cast<unsigned>(col) >= static_cast<unsigned>(A);
                if constexpr (!std::is_same<Hook, RowNoHook>::value)
                    if (!out) out = hook(col, v[j * V + e]);
                if (out) v[j * V + e] = neg_inf<C>();
            }
        }
        absorb<C, 4 * V>(v, m, s);
    }
    C M = m;
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) M = vmax(M, __shfl_xor(M, off, kWave));
    const C shift = (M == neg_inf<C>()) ? C(0) : M;
    C sum = s * fast_exp(m - shift);
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, kWave);
    return {shift, sum};
}

}  // namespace rnnt
