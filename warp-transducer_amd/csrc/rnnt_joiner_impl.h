// rnnt_joiner_impl.h -- host driver of libwarprnnt_joiner.so (include/rnnt_joiner.h): run_joiner_fwd<Tag>, run_joiner_bwd<Tag>.
// One instantiation per storage type, each in a translation unit -- a code object -- of its own:
//     rnnt_joiner.hip   F32 (+ every C entry point)     rnnt_joiner_f64.hip   F64     rnnt_joiner_h16.hip   BF16, F16
//
// LAUNCH RULE (jn_plan; tests/joiner_forms.py restates it).  esz = bytes of a stored element, comp = 4 (8 for fp64).
//   VEC       H * esz is a multiple of 16 and every tensor of the call starts on a 16-byte boundary; else element-wise.
//   forward   joiner_fwd_kernel<Tag, VEC>: P = H / V accesses per row (V = 16 / esz, or 1), blocks of (PX, 256 / PX) threads,
//             PX = P rounded up to a power of two, at most 256; a grid-stride loop over the N T J rows of at most 2^20 blocks.
//   backward  accumulator group of a thread: Vb = 4 columns (2 of fp64) when VEC, else 1; Pb = H / Vb.
//             threads = the largest power of two <= min(256, 64 KiB / (U * Vb * comp)).
//             threads >= 64 and N <= 65535: SINGLE PASS, joiner_bwd_kernel<Tag, VEC> with CX = min(16, Pb rounded up to a
//               power of two) threads over the columns of a slice, TY = threads / CX frame groups, U * threads * Vb * comp
//               bytes of LDS, grid (ceil(Pb / CX), N, TZ), TZ = the shares of T:
//                   TZ = clamp(ceil(1024 / (N * ceil(H / 64))), 1, min(8, ceil(T / 16)))            (jn_shares)
//               -- enough workgroups for 256 CUs when N and H alone give too few.  TZ > 1: the shares' partial dg sums go to
//               the workspace and joiner_dg_sum_kernel<Tag> adds them in share order.
//             else the TWO-PASS FALLBACK: joiner_df_kernel<Tag, VEC> and joiner_dg_kernel<Tag, VEC>, arranged as the forward.
//             With VEC the fallback takes over at U > 64; element-wise at U > 256 (fp64: U > 128).
//   layout 2  joiner_prep_kernel first, in both calls: one block per sample writes the bad-start flags.
#pragma once
#include "rnnt_side_host.h"
#include "rnnt_joiner_kernels.h"
#include "../../include/rnnt_joiner.h"

namespace rnnt {

constexpr size_t kJnLdsBytes = 64 * 1024;      // what a workgroup of the single pass may allocate
constexpr int kJnBlocks = 1024;                // workgroups the shares of T aim for
constexpr int kJnMaxShares = 8;
constexpr long long kJnMaxGrid = 1 << 20;

// The arguments of both calls, untyped as they cross the C-ABI.
struct JoinerCall {
    const void *f, *g, *out, *dout;            // forward: f, g, out (written); backward: out (read), dout
    void *df, *dg;
    const int* ranges;
    const long long* offsets;
    const int *label_lengths, *input_lengths;
    int layout, act, S, T, U, H, N;
    void* workspace;
    hipStream_t stream;
};

static inline int jn_pow2_ceil(int x) { int p = 1; while (p < x) p <<= 1; return p; }
static inline int jn_pow2_floor(long long x) { int p = 1; while (2LL * p <= x) p <<= 1; return p; }

static inline int jn_shares(int N, int T, int H) {
    const long long base = static_cast<long long>(N) * ((H + 63) / 64);
    long long tz = (kJnBlocks + base - 1) / base;
    const int cap = (T + 15) / 16 < kJnMaxShares ? (T + 15) / 16 : kJnMaxShares;
    if (tz > cap) tz = cap;
    return tz < 1 ? 1 : static_cast<int>(tz);
}

// Workspace: the flags, then the partial sums of a split walk (sized for the element-wise form's reach, the wider one).
struct JnLayout { size_t flags, part, total; };
static inline JnLayout jn_layout(int T, int U, int H, int N, size_t comp) {
    JnLayout l;
    size_t o = 0;
    l.flags = o; o = align_up(o + static_cast<size_t>(N) * sizeof(int));
    l.part = o;
    const int tz = jn_shares(N, T, H);
    if (tz > 1 && static_cast<size_t>(U) * comp * 64 <= kJnLdsBytes)
        o = align_up(o + static_cast<size_t>(tz) * N * U * H * comp);
    l.total = o + kAlign;
    return l;
}

struct JnPlan { bool vec, single; int V, P, PX, Vb, Pb, CX, TY, TZ; size_t lds; };
static inline JnPlan jn_plan(const JoinerCall& c, size_t esz, size_t comp, bool aligned) {
    JnPlan p;
    p.vec = aligned && (static_cast<size_t>(c.H) * esz) % 16 == 0;
    p.V = p.vec ? static_cast<int>(16 / esz) : 1;
    p.P = c.H / p.V;
    p.PX = jn_pow2_ceil(p.P) < 256 ? jn_pow2_ceil(p.P) : 256;
    p.Vb = p.vec ? (esz == 8 ? 2 : 4) : 1;
    p.Pb = c.H / p.Vb;
    const long long fit = static_cast<long long>(kJnLdsBytes / (static_cast<size_t>(c.U) * p.Vb * comp));
    const int threads = fit < 1 ? 0 : jn_pow2_floor(fit < 256 ? fit : 256);
    p.single = threads >= 64 && c.N <= 65535;
    p.CX = jn_pow2_ceil(p.Pb) < 16 ? jn_pow2_ceil(p.Pb) : 16;
    p.TY = p.single ? threads / p.CX : 1;
    p.TZ = p.single ? jn_shares(c.N, c.T, c.H) : 1;
    p.lds = static_cast<size_t>(c.U) * threads * p.Vb * comp;
    return p;
}

static inline bool jn_aligned16(std::initializer_list<const void*> ps) {
    uintptr_t all = 0;
    for (const void* p : ps) all |= reinterpret_cast<uintptr_t>(p);
    return (all & 15u) == 0;
}

static inline unsigned jn_row_grid(long long rows, int per_block) {
    const long long blocks = (rows + per_block - 1) / per_block;
    return static_cast<unsigned>(blocks < kJnMaxGrid ? (blocks ? blocks : 1) : kJnMaxGrid);
}

static inline JnArgs jn_args(const JoinerCall& c, int* flags) {
    return {c.ranges, c.offsets, c.label_lengths, c.input_lengths, flags, c.layout, c.act, c.T, c.U,
            c.layout == 2 ? c.S : c.U, c.H, c.N};
}

static inline int* jn_flags(const JoinerCall& c) {
    return reinterpret_cast<int*>(align_up(reinterpret_cast<size_t>(c.workspace)));
}

template <typename Tag> static bool jn_prep(const JoinerCall& c) {
    if (c.layout != 2) return true;
    hipLaunchKernelGGL((joiner_prep_kernel<Tag>), dim3(c.N), dim3(256), 0, c.stream, c.ranges, c.input_lengths, jn_flags(c), c.T, c.U);
    return hipGetLastError() == hipSuccess;
}

template <typename Tag> rnntStatus_t run_joiner_fwd(const JoinerCall& c) {
    using St = typename Tag::store;
    (void)hipGetLastError();                           // a stale error of an unrelated earlier HIP call is not ours
    const JnPlan p = jn_plan(c, sizeof(St), sizeof(typename Tag::comp), jn_aligned16({c.f, c.g, c.out}));
    const JnArgs a = jn_args(c, jn_flags(c));
    bool ok = jn_prep<Tag>(c);
    const dim3 block(p.PX, 256 / p.PX);
    const dim3 grid(jn_row_grid(static_cast<long long>(c.N) * c.T * a.J, block.y));
    const St *f = static_cast<const St*>(c.f), *g = static_cast<const St*>(c.g);
    St* out = static_cast<St*>(const_cast<void*>(c.out));
    if (ok) {
        if (p.vec) hipLaunchKernelGGL((joiner_fwd_kernel<Tag, true>), grid, block, 0, c.stream, f, g, out, a, p.P);
        else hipLaunchKernelGGL((joiner_fwd_kernel<Tag, false>), grid, block, 0, c.stream, f, g, out, a, p.P);
        ok = hipGetLastError() == hipSuccess;
    }
    return ok ? RNNT_STATUS_SUCCESS : RNNT_STATUS_EXECUTION_FAILED;
}

template <typename Tag> rnntStatus_t run_joiner_bwd(const JoinerCall& c) {
    using St = typename Tag::store;
    using C = typename Tag::comp;
    (void)hipGetLastError();
    const JnPlan p = jn_plan(c, sizeof(St), sizeof(C), jn_aligned16({c.out, c.dout, c.df, c.dg}));
    const JnArgs a = jn_args(c, jn_flags(c));
    const St *out = static_cast<const St*>(c.out), *dout = static_cast<const St*>(c.dout);
    St *df = static_cast<St*>(c.df), *dg = static_cast<St*>(c.dg);
    bool ok = jn_prep<Tag>(c);
    if (!ok) return RNNT_STATUS_EXECUTION_FAILED;
    if (p.single) {
        const JnLayout lay = jn_layout(c.T, c.U, c.H, c.N, sizeof(C));
        C* part = reinterpret_cast<C*>(reinterpret_cast<char*>(jn_flags(c)) + lay.part);
        const dim3 block(p.CX, p.TY), grid((p.Pb + p.CX - 1) / p.CX, c.N, p.TZ);
        if (p.vec) hipLaunchKernelGGL((joiner_bwd_kernel<Tag, true>), grid, block, p.lds, c.stream, out, dout, df, dg, part, a, p.Pb);
        else hipLaunchKernelGGL((joiner_bwd_kernel<Tag, false>), grid, block, p.lds, c.stream, out, dout, df, dg, part, a, p.Pb);
        ok = hipGetLastError() == hipSuccess;
        if (ok && p.TZ > 1) {
            const long long E = static_cast<long long>(c.N) * c.U * c.H;
            hipLaunchKernelGGL((joiner_dg_sum_kernel<Tag>), dim3(jn_row_grid(E, 256)), dim3(256), 0, c.stream, part, dg, E, p.TZ);
            ok = hipGetLastError() == hipSuccess;
        }
    } else {
        const dim3 block(p.PX, 256 / p.PX);
        const dim3 gf(jn_row_grid(static_cast<long long>(c.N) * c.T, block.y)), gg(jn_row_grid(static_cast<long long>(c.N) * c.U, block.y));
        if (p.vec) {
            hipLaunchKernelGGL((joiner_df_kernel<Tag, true>), gf, block, 0, c.stream, out, dout, df, a, p.P);
            hipLaunchKernelGGL((joiner_dg_kernel<Tag, true>), gg, block, 0, c.stream, out, dout, dg, a, p.P);
        } else {
            hipLaunchKernelGGL((joiner_df_kernel<Tag, false>), gf, block, 0, c.stream, out, dout, df, a, p.P);
            hipLaunchKernelGGL((joiner_dg_kernel<Tag, false>), gg, block, 0, c.stream, out, dout, dg, a, p.P);
        }
        ok = hipGetLastError() == hipSuccess;
    }
    return ok ? RNNT_STATUS_SUCCESS : RNNT_STATUS_EXECUTION_FAILED;
}

#ifndef RNNT_JOINER_INSTANTIATE_F32
extern template rnntStatus_t run_joiner_fwd<F32>(const JoinerCall&);
extern template rnntStatus_t run_joiner_bwd<F32>(const JoinerCall&);
#endif
#ifndef RNNT_JOINER_INSTANTIATE_F64
extern template rnntStatus_t run_joiner_fwd<F64>(const JoinerCall&);
extern template rnntStatus_t run_joiner_bwd<F64>(const JoinerCall&);
#endif
#ifndef RNNT_JOINER_INSTANTIATE_H16
extern template rnntStatus_t run_joiner_fwd<BF16>(const JoinerCall&);
extern template rnntStatus_t run_joiner_bwd<BF16>(const JoinerCall&);
extern template rnntStatus_t run_joiner_fwd<F16>(const JoinerCall&);
extern template rnntStatus_t run_joiner_bwd<F16>(const JoinerCall&);
#endif

}  // namespace rnnt
