// rnnt_joiner_kernels.h -- the kernels of libwarprnnt_joiner.so (include/rnnt_joiner.h): out = act(f + g) in the padded,
// packed or pruned layout, and df / dg from dout.  All of them address rows through ONE row map (jn_row); the launch rule
// is rnnt_joiner_impl.h's.
//   joiner_prep_kernel      layout 2: the per-sample bad-start flags
//   joiner_fwd_kernel       one write of out; VEC: 16-byte packets, else element-wise
//   joiner_bwd_kernel       single pass: a workgroup owns (sample, column slice, share of T), df per frame in registers, dg in
//                           LDS accumulators indexed by u, private per thread, combined over the block's frame groups in a
//                           fixed order; VEC: 16-byte accumulator groups (4 columns; 2 of fp64)
//   joiner_dg_sum_kernel    the ordered second stage of a walk split over T: dg = sum over the shares' partial sums
//   joiner_df_kernel, joiner_dg_kernel    the two-pass fallback: each reads dout once
#pragma once
#include "rnnt_device.h"

namespace rnnt {

struct JnArgs {
    const int* ranges;          // layout 2
    const long long* offsets;   // layout 1
    const int *ylen, *xlen;     // label_lengths, input_lengths (either may be null)
    const int* bad;             // layout 2: the flags joiner_prep_kernel wrote
    int layout, act, T, U, J, H, N;   // J = rows per frame of the iteration space: U, or S in layout 2
};

template <typename Tag> __device__ __forceinline__ typename Tag::comp jn_comp(typename Tag::store v);
template <> __device__ __forceinline__ float jn_comp<F32>(float v) { return v; }
template <> __device__ __forceinline__ double jn_comp<F64>(double v) { return v; }
template <> __device__ __forceinline__ float jn_comp<BF16>(uint16_t v) { return bf16_to_f32(v); }
template <> __device__ __forceinline__ float jn_comp<F16>(uint16_t v) { return f16_to_f32(v); }
template <typename Tag> __device__ __forceinline__ typename Tag::store jn_store(typename Tag::comp v);
template <> __device__ __forceinline__ float jn_store<F32>(float v) { return v; }
template <> __device__ __forceinline__ double jn_store<F64>(double v) { return v; }
template <> __device__ __forceinline__ uint16_t jn_store<BF16>(float v) { return f32_to_bf16(v); }
template <> __device__ __forceinline__ uint16_t jn_store<F16>(float v) { return f32_to_f16(v); }

// V storage values as one access of V * sizeof(store) bytes (4, 8 or 16: the caller guarantees that alignment)
template <typename St, int V> struct alignas(sizeof(St) * V) JnPack { St v[V]; };
template <typename Tag, int V>
__device__ __forceinline__ void jn_load(const typename Tag::store* p, typename Tag::comp* x) {
    const JnPack<typename Tag::store, V> k = *reinterpret_cast<const JnPack<typename Tag::store, V>*>(p);
#pragma unroll
    for (int i = 0; i < V; ++i) x[i] = jn_comp<Tag>(k.v[i]);
}
template <typename Tag, int V>
__device__ __forceinline__ void jn_save(typename Tag::store* p, const typename Tag::comp* x) {
    JnPack<typename Tag::store, V> k;
#pragma unroll
    for (int i = 0; i < V; ++i) k.v[i] = jn_store<Tag>(x[i]);
    *reinterpret_cast<JnPack<typename Tag::store, V>*>(p) = k;
}

__device__ __forceinline__ float jn_tanh(float x) { return tanhf(x); }
__device__ __forceinline__ double jn_tanh(double x) { return tanh(x); }
template <typename C> __device__ __forceinline__ C jn_act(C x, int act) {
    return act == 0 ? x : act == 1 ? (x <= C(0) ? C(0) : x) : jn_tanh(x);     // (relu keeps a NaN, as torch's does)
}
// One term of the backward sums, e = dout * act'(out), from the stored values.  relu's is dout or 0, exact.  tanh's is formed
// in fp64 for every storage type, in the three roundings of the definition read left to right and never contracted --
// dout * (1 - out * out) -- so that a term is the fp64 definition's own value, rounded once to the accumulator's type: what
// is left between the sums and their definition is the summation alone.
template <typename C> __device__ __forceinline__ C jn_term(C d, C o, int act) {
#pragma clang fp contract(off)
    if (act == 1) return o > C(0) ? d : C(0);
    const double od = static_cast<double>(o);
    const double sq = od * od;
    const double slope = 1.0 - sq;
    return static_cast<C>(static_cast<double>(d) * slope);
}

// ----------------------------------------------------------------------------- the row map
// Frame (b, t), row j of the iteration space (label position u in layouts 0 and 1, window slot k in layout 2).
//   kind 0: no row (layout 1 outside the sample's lattice)      kind 1: a row of exact zeros      kind 2: a real row
//   row: the row of out / dout; gu: the row of g / dg it adds
struct JnRow { int kind; long long row; int gu; };
struct JnSample { int Tb, Lb, bad; };

__device__ __forceinline__ JnSample jn_sample(const JnArgs& a, int b) {
    JnSample s;
    s.Tb = a.xlen != nullptr ? min(max(a.xlen[b], 0), a.T) : a.T;
    s.Lb = a.ylen != nullptr && a.layout != 2 ? min(max(a.ylen[b], 0), a.U - 1) : a.U - 1;
    s.bad = a.layout == 2 ? a.bad[b] : 0;
    return s;
}

// start: ranges[b, t] of a live frame of layout 2 (else unused)
__device__ __forceinline__ JnRow jn_row(const JnArgs& a, const JnSample& s, int b, int t, int j, int start) {
    JnRow r;
    const long long bt = static_cast<long long>(b) * a.T + t;
    if (a.layout == 2) {
        r.row = bt * a.J + j;
        r.kind = (t < s.Tb && s.bad == 0) ? 2 : 1;
        r.gu = min(max(start + j, 0), a.U - 1);
    } else {
        const bool real = t < s.Tb && j <= s.Lb;
        r.gu = j;
        if (a.layout == 1) {
            r.row = a.offsets[b] + static_cast<long long>(t) * (s.Lb + 1) + j;
            r.kind = real ? 2 : 0;
        } else {
            r.row = bt * a.U + j;
            r.kind = real ? 2 : 1;
        }
    }
    return r;
}
__device__ __forceinline__ int jn_start(const JnArgs& a, const JnSample& s, int b, int t) {
    return (a.layout == 2 && t < s.Tb) ? a.ranges[static_cast<long long>(b) * a.T + t] : 0;
}

// ----------------------------------------------------------------------------- layout 2: bad-start flags
// One block per sample: flag[b] = some frame t < T_b starts outside [0, U - 1].  Every flag is written.  (A template so that
// each code object holds its own.)
template <typename Tag>
__global__ void __launch_bounds__(256) joiner_prep_kernel(const int* ranges, const int* xlen, int* flag, int T, int U) {
    const int b = blockIdx.x;
    const int Tb = xlen != nullptr ? min(max(xlen[b], 0), T) : T;
    int badv = 0;
    for (int t = threadIdx.x; t < Tb; t += blockDim.x) {
        const int s = ranges[static_cast<long long>(b) * T + t];
        badv |= (s < 0 || s > U - 1) ? 1 : 0;
    }
    badv = __syncthreads_or(badv);
    if (threadIdx.x == 0) flag[b] = badv != 0 ? 1 : 0;
}

// ----------------------------------------------------------------------------- forward
// blockDim = (PX, RY): RY rows per block step, PX threads over the P = H / V accesses of a row; grid-stride over rows.
template <typename Tag, bool VEC>
__global__ void __launch_bounds__(256) joiner_fwd_kernel(const typename Tag::store* __restrict__ f,
                                                         const typename Tag::store* __restrict__ g,
                                                         typename Tag::store* __restrict__ out, JnArgs a, int P) {
    using C = typename Tag::comp;
    constexpr int V = VEC ? 16 / sizeof(typename Tag::store) : 1;
    const long long rows = static_cast<long long>(a.N) * a.T * a.J;
    const int act = a.act;
    for (long long r = static_cast<long long>(blockIdx.x) * blockDim.y + threadIdx.y; r < rows;
         r += static_cast<long long>(gridDim.x) * blockDim.y) {
        const int j = static_cast<int>(r % a.J);
        const long long bt = r / a.J;
        const int t = static_cast<int>(bt % a.T), b = static_cast<int>(bt / a.T);
        const JnSample s = jn_sample(a, b);
        const JnRow m = jn_row(a, s, b, t, j, jn_start(a, s, b, t));
        if (m.kind == 0) continue;
        typename Tag::store* o = out + m.row * a.H;
        C x[V], y[V];
        if (m.kind == 1) {                                  // zeros, nothing read
#pragma unroll
            for (int i = 0; i < V; ++i) x[i] = C(0);
            for (int p = threadIdx.x; p < P; p += blockDim.x) jn_save<Tag, V>(o + static_cast<long long>(p) * V, x);
            continue;
        }
        const typename Tag::store* fr = f + bt * a.H;
        const typename Tag::store* gr = g + (static_cast<long long>(b) * a.U + m.gu) * a.H;
        for (int p = threadIdx.x; p < P; p += blockDim.x) {
            jn_load<Tag, V>(fr + static_cast<long long>(p) * V, x);
            jn_load<Tag, V>(gr + static_cast<long long>(p) * V, y);
#pragma unroll
            for (int i = 0; i < V; ++i) x[i] = jn_act<C>(x[i] + y[i], act);
            jn_save<Tag, V>(o + static_cast<long long>(p) * V, x);
        }
    }
}

// e = dout * act'(out) of V columns of one real row
template <typename Tag, int V>
__device__ __forceinline__ void jn_e(const typename Tag::store* out, const typename Tag::store* dout, long long at, int act,
                                     typename Tag::comp* e) {
    using C = typename Tag::comp;
    jn_load<Tag, V>(dout + at, e);
    if (act != 0) {
        C o[V];
        jn_load<Tag, V>(out + at, o);
#pragma unroll
        for (int i = 0; i < V; ++i) e[i] = jn_term<C>(e[i], o[i], act);
    }
}

// ----------------------------------------------------------------------------- backward, single pass
// grid = (column slices, N, TZ), blockDim = (CX, TY).  Thread (cx, ty) owns the V columns of access c = slice * CX + cx and
// the frames t0 + ty, t0 + ty + TY, ... of share z's [t0, t1).  LDS: acc[u][ty][cx][V] of Tag::comp, U * TY * CX * V values
// (dynamic).  TZ == 1: dg is written rounded; else the partial sums go to part[z][b][u][H] for joiner_dg_sum_kernel.
template <typename Tag, bool VEC>
__global__ void __launch_bounds__(256) joiner_bwd_kernel(const typename Tag::store* __restrict__ out,
                                                         const typename Tag::store* __restrict__ dout,
                                                         typename Tag::store* __restrict__ df,
                                                         typename Tag::store* __restrict__ dg,
                                                         typename Tag::comp* __restrict__ part, JnArgs a, int P) {
    using C = typename Tag::comp;
    constexpr int V = VEC ? (sizeof(typename Tag::store) == 8 ? 2 : 4) : 1;
    extern __shared__ __align__(16) unsigned char jn_smem[];
    C* acc = reinterpret_cast<C*>(jn_smem);
    const int CX = blockDim.x, TY = blockDim.y, cx = threadIdx.x, ty = threadIdx.y;
    const int b = blockIdx.y, z = blockIdx.z, TZ = gridDim.z;
    const int c = blockIdx.x * CX + cx;
    const bool live = c < P;
    const long long col = static_cast<long long>(c) * V;
    const int act = a.act;
    const JnSample s = jn_sample(a, b);
    C zero[V];
#pragma unroll
    for (int i = 0; i < V; ++i) zero[i] = C(0);
    C* mine = acc + (static_cast<size_t>(ty) * CX + cx) * V;            // + u * TY * CX * V
    const size_t ustride = static_cast<size_t>(TY) * CX * V;
    for (int u = 0; u < a.U; ++u) {
#pragma unroll
        for (int i = 0; i < V; ++i) mine[u * ustride + i] = C(0);
    }
    const int share = (a.T + TZ - 1) / TZ;
    const int t0 = z * share, t1 = min(a.T, t0 + share);
    if (live) {
        for (int t = t0 + ty; t < t1; t += TY) {
            C sum[V];
#pragma unroll
            for (int i = 0; i < V; ++i) sum[i] = C(0);
            if (t < s.Tb && s.bad == 0) {
                const int start = jn_start(a, s, b, t);
                const int jn = a.layout == 2 ? a.J : s.Lb + 1;
#pragma unroll 4
                for (int j = 0; j < jn; ++j) {
                    const JnRow m = jn_row(a, s, b, t, j, start);
                    C e[V];
                    jn_e<Tag, V>(out, dout, m.row * a.H + col, act, e);
                    C* d = mine + m.gu * ustride;
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        sum[i] += e[i];
                        d[i] += e[i];
                    }
                }
            }
            jn_save<Tag, V>(df + (static_cast<long long>(b) * a.T + t) * a.H + col, sum);
        }
    }
    __syncthreads();
    if (!live) return;
    for (int u = ty; u < a.U; u += TY) {
        C sum[V];
#pragma unroll
        for (int i = 0; i < V; ++i) sum[i] = C(0);
        const C* src = acc + u * ustride + static_cast<size_t>(cx) * V;
        for (int k = 0; k < TY; ++k) {
#pragma unroll
            for (int i = 0; i < V; ++i) sum[i] += src[static_cast<size_t>(k) * CX * V + i];
        }
        const long long at = (static_cast<long long>(b) * a.U + u) * a.H + col;
        if (TZ == 1) {
            jn_save<Tag, V>(dg + at, sum);
        } else {
            C* p = part + static_cast<long long>(z) * a.N * a.U * a.H + at;
#pragma unroll
            for (int i = 0; i < V; ++i) p[i] = sum[i];
        }
    }
}

// dg[i] = part[0][i] + part[1][i] + ... in that order, rounded once; E = N U H elements
template <typename Tag>
__global__ void __launch_bounds__(256) joiner_dg_sum_kernel(const typename Tag::comp* __restrict__ part,
                                                            typename Tag::store* __restrict__ dg, long long E, int TZ) {
    for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < E;
         i += static_cast<long long>(gridDim.x) * 256) {
        typename Tag::comp sum = 0;
        for (int z = 0; z < TZ; ++z) sum += part[z * E + i];
        dg[i] = jn_store<Tag>(sum);
    }
}

// ----------------------------------------------------------------------------- backward, two passes (the fallback)
// The forward kernel's thread arrangement over the rows of df (N T) / of dg (N U).
template <typename Tag, bool VEC>
__global__ void __launch_bounds__(256) joiner_df_kernel(const typename Tag::store* __restrict__ out,
                                                        const typename Tag::store* __restrict__ dout,
                                                        typename Tag::store* __restrict__ df, JnArgs a, int P) {
    using C = typename Tag::comp;
    constexpr int V = VEC ? 16 / sizeof(typename Tag::store) : 1;
    const long long rows = static_cast<long long>(a.N) * a.T;
    for (long long bt = static_cast<long long>(blockIdx.x) * blockDim.y + threadIdx.y; bt < rows;
         bt += static_cast<long long>(gridDim.x) * blockDim.y) {
        const int t = static_cast<int>(bt % a.T), b = static_cast<int>(bt / a.T);
        const JnSample s = jn_sample(a, b);
        const bool real = t < s.Tb && s.bad == 0;
        const int start = jn_start(a, s, b, t);
        const int jn = !real ? 0 : a.layout == 2 ? a.J : s.Lb + 1;
        for (int p = threadIdx.x; p < P; p += blockDim.x) {
            const long long col = static_cast<long long>(p) * V;
            C sum[V];
#pragma unroll
            for (int i = 0; i < V; ++i) sum[i] = C(0);
            for (int j = 0; j < jn; ++j) {
                C e[V];
                jn_e<Tag, V>(out, dout, jn_row(a, s, b, t, j, start).row * a.H + col, a.act, e);
#pragma unroll
                for (int i = 0; i < V; ++i) sum[i] += e[i];
            }
            jn_save<Tag, V>(df + bt * a.H + col, sum);
        }
    }
}

template <typename Tag, bool VEC>
__global__ void __launch_bounds__(256) joiner_dg_kernel(const typename Tag::store* __restrict__ out,
                                                        const typename Tag::store* __restrict__ dout,
                                                        typename Tag::store* __restrict__ dg, JnArgs a, int P) {
    using C = typename Tag::comp;
    constexpr int V = VEC ? 16 / sizeof(typename Tag::store) : 1;
    const long long rows = static_cast<long long>(a.N) * a.U;
    for (long long bu = static_cast<long long>(blockIdx.x) * blockDim.y + threadIdx.y; bu < rows;
         bu += static_cast<long long>(gridDim.x) * blockDim.y) {
        const int u = static_cast<int>(bu % a.U), b = static_cast<int>(bu / a.U);
        const JnSample s = jn_sample(a, b);
        const int tn = (s.bad != 0 || u > s.Lb) ? 0 : s.Tb;
        for (int p = threadIdx.x; p < P; p += blockDim.x) {
            const long long col = static_cast<long long>(p) * V;
            C sum[V];
#pragma unroll
            for (int i = 0; i < V; ++i) sum[i] = C(0);
            for (int t = 0; t < tn; ++t) {
                const int start = jn_start(a, s, b, t);
                // layout 2: the slots of this frame whose clamped position is u (several at u = U - 1); else slot u
                const int j0 = a.layout == 2 ? u - start : u;
                const int j1 = a.layout == 2 ? (u == a.U - 1 ? a.J : j0 + 1) : u + 1;
                for (int j = max(j0, 0); j < min(j1, a.J); ++j) {
                    C e[V];
                    jn_e<Tag, V>(out, dout, jn_row(a, s, b, t, j, start).row * a.H + col, a.act, e);
#pragma unroll
                    for (int i = 0; i < V; ++i) sum[i] += e[i];
                }
            }
            jn_save<Tag, V>(dg + bu * a.H + col, sum);
        }
    }
}

}  // namespace rnnt
