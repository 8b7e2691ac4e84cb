"""The fp64 definition of include/rnnt_joiner.h in numpy, with plain loops over (b, t, u): out = act(f + g) in the padded, packed
and pruned layouts, and df / dg from dout -- with, for every element of df and dg, the number of terms of its sum and the sum
of their absolute values, which the summation bounds of tests/test_gpu_joiner.py need."""
import numpy as np

PADDED, PACKED, PRUNED = 0, 1, 2
ACTS = ("identity", "relu", "tanh")


def act(x, name):
    return x if name == "identity" else np.maximum(x, 0.0) if name == "relu" else np.tanh(x)


def term(dout, out, name):
    """e = dout * act'(out), from the stored out."""
    if name == "identity":
        return dout
    if name == "relu":
        return dout * (out > 0)
    return dout * (1.0 - out * out)


def lengths(N, T, U, tl, ll):
    tl = np.full(N, T) if tl is None else np.clip(np.asarray(tl), 0, T)
    ll = np.full(N, U - 1) if ll is None else np.clip(np.asarray(ll), 0, U - 1)
    return tl, ll


def offsets(tl, ll):
    return np.concatenate([[0], np.cumsum(np.asarray(tl, np.int64) * (np.asarray(ll, np.int64) + 1))])


def bad_samples(ranges, tl, U):
    """Layout 2: the samples with a start outside [0, U - 1] in a frame t < T_b."""
    return np.array([bool(((ranges[b, :tl[b]] < 0) | (ranges[b, :tl[b]] > U - 1)).any()) for b in range(len(tl))])


def rows(layout, N, T, U, tl=None, ll=None, ranges=None, S=None):
    """[(b, t, u, index of the row in out)] of the real rows, in the order of the loops; out's index is a tuple (padded, pruned)
    or an int (packed).  u is the row of g."""
    if layout == PRUNED:
        tl, _ = lengths(N, T, U, tl, None)
        bad = bad_samples(ranges, tl, U)
        return [(b, t, min(int(ranges[b, t]) + k, U - 1), (b, t, k))
                for b in range(N) if not bad[b] for t in range(tl[b]) for k in range(S)]
    tl, ll = lengths(N, T, U, tl, ll)
    offs = offsets(tl, ll)
    return [(b, t, u, (b, t, u) if layout == PADDED else int(offs[b]) + t * (int(ll[b]) + 1) + u)
            for b in range(N) for t in range(tl[b]) for u in range(ll[b] + 1)]


def out_shape(layout, N, T, U, H, tl=None, ll=None, S=None):
    if layout == PADDED:
        return (N, T, U, H)
    if layout == PRUNED:
        return (N, T, S, H)
    tl, ll = lengths(N, T, U, tl, ll)
    return (int(offsets(tl, ll)[-1]), H)


def forward(f, g, layout, name, tl=None, ll=None, ranges=None, S=None):
    """out in fp64: zeros in every row that is not real."""
    f, g = np.asarray(f, np.float64), np.asarray(g, np.float64)
    (N, T, H), U = f.shape, g.shape[1]
    out = np.zeros(out_shape(layout, N, T, U, H, tl, ll, S))
    for b, t, u, at in rows(layout, N, T, U, tl, ll, ranges, S):
        out[at] = act(f[b, t] + g[b, u], name)
    return out


def backward(out, dout, layout, name, N, T, U, tl=None, ll=None, ranges=None, S=None):
    """df (N, T, H), dg (N, U, H) in fp64, and for each of the two the sums of |e| and the numbers of terms (same shapes; the
    counts without the H axis).  Rows that are not real are not touched (they may hold NaN)."""
    out, dout = np.asarray(out, np.float64), np.asarray(dout, np.float64)
    H = dout.shape[-1]
    df, dg = np.zeros((N, T, H)), np.zeros((N, U, H))
    af, ag = np.zeros((N, T, H)), np.zeros((N, U, H))
    nf, ng = np.zeros((N, T), int), np.zeros((N, U), int)
    for b, t, u, at in rows(layout, N, T, U, tl, ll, ranges, S):
        e = term(dout[at], out[at], name)
        df[b, t] += e
        dg[b, u] += e
        af[b, t] += np.abs(e)
        ag[b, u] += np.abs(e)
        nf[b, t] += 1
        ng[b, u] += 1
    return df, dg, af, ag, nf, ng


def real_mask(layout, shape, N, T, U, tl=None, ll=None, ranges=None, S=None):
    """bool over out's rows (out's shape without H): the real ones."""
    m = np.zeros(shape[:-1], bool)
    for _, _, _, at in rows(layout, N, T, U, tl, ll, ranges, S):
        m[at] = True
    return m
