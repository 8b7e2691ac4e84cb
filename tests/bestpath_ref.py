"""numpy fp64 reference of include/rnnt_bestpath.h: the max-plus recursion written out node by node with the SAME additions
the header defines (each candidate one IEEE addition of an fp64 p and the stored weight upcast to fp64), the strict tie rule,
the traceback, the sum along a path in path order and the edge indicators.  Because the additions are the same, the library
must give the same bits: the tests compare with np.array_equal.  It is given the STORED values of px / py as doubles and
reads nothing outside a rectangle's edge sets.  `strict=False` is the wrong library of the negative control: the symbol edge
on ties."""
import numpy as np

from tests.mi_ref import edge_masks, full_boundary                      # noqa: F401  (this module's names too)

NEG = float("-inf")
MARKER = np.array([0x7ff8dead00000000], np.uint64).view(np.float64)[0]  # cost_invalid<double>() of include/rnnt.h


def back_words(T):
    return (T + 64) // 64


def _valid(row, S, T):
    s0, t0, s1, t1 = (int(v) for v in row)
    return 0 <= s0 <= s1 <= S and 0 <= t0 <= t1 <= T


def sweep_one(X, Y, s0, t0, s1, t1, mod, strict=True):
    """(p, bit, bad) over the nodes of one rectangle, local coordinates (Sr + 1, Tr + 1).  X = px[b], Y = py[b] (whole rows,
    absolute indices).  bad: a NaN or +inf on an edge of the rectangle.  Vectorised over the nodes that do not depend on one
    another -- a frame column (modified type) or an anti-diagonal (regular type); every node still gets exactly the two
    additions of the definition."""
    Sr, Tr = s1 - s0, t1 - t0
    Xr, Yr = X[s0:s1, t0:(t1 if mod else t1 + 1)], Y[s0:s1 + 1, t0:t1]
    bad = bool((~(Xr < np.inf)).any() or (~(Yr < np.inf)).any())
    p = np.full((Sr + 1, Tr + 1), NEG)
    bit = np.zeros((Sr + 1, Tr + 1), bool)
    p[0, 0] = 0.0
    with np.errstate(invalid="ignore"):
        for d in range(1, (Tr if mod else Tr + Sr) + 1):
            if mod:
                i = np.arange(Sr + 1)
                j = np.full(Sr + 1, d)
            else:
                i = np.arange(max(0, d - Tr), min(Sr, d) + 1)
                j = d - i
            x, y = np.full(len(i), NEG), np.full(len(i), NEG)
            jx = j - 1 if mod else j
            ex = (i > 0) & (jx >= 0)
            x[ex] = p[i[ex] - 1, jx[ex]] + Xr[i[ex] - 1, jx[ex]]
            ey = j > 0
            y[ey] = p[i[ey], j[ey] - 1] + Yr[i[ey], j[ey] - 1]
            sym = (x > y) if strict else (x >= y)
            p[i, j] = np.where(sym, x, y)
            bit[i, j] = sym
    return p, bit, bad


def trace_one(bit, s0, t0, Sr, Tr, mod, frames_row):
    s, t = Sr, Tr
    while s > 0 and t >= 0:
        sym = t == 0 or bit[s, t]
        if sym:
            frames_row[s0 + s - 1] = t0 + (t - 1 if mod else t)
            s -= 1
            t -= 1 if mod else 0
        else:
            t -= 1


def best_path(px, py, bd=None, mod=None, strict=True):
    """-> scores (B,) float64, frames (B, S) int32, back (B, S + 1, ceil((T + 1) / 64)) uint64."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    B, S1, T = py.shape
    S = S1 - 1
    mod = (px.shape[2] == T) if mod is None else bool(mod)
    bd = full_boundary(B, S, T) if bd is None else np.asarray(bd, np.int64)
    scores = np.zeros(B)
    frames = np.full((B, S), -1, np.int32)
    back = np.zeros((B, S + 1, back_words(T)), np.uint64)
    for b in range(B):
        if not _valid(bd[b], S, T):
            scores[b] = MARKER
            continue
        s0, t0, s1, t1 = (int(v) for v in bd[b])
        p, bit, bad = sweep_one(px[b], py[b], s0, t0, s1, t1, mod, strict)
        for i, j in zip(*np.nonzero(bit)):
            t = t0 + int(j)
            back[b, s0 + int(i), t >> 6] |= np.uint64(1) << np.uint64(t & 63)
        scores[b] = np.nan if bad else p[-1, -1]
        if np.isfinite(scores[b]):
            trace_one(bit, s0, t0, s1 - s0, t1 - t0, mod, frames[b])
    return scores, frames, back


def rescore(px, py, bd, mod, frames):
    """(sum, n, sum |w|) per sample along the path `frames` describes, in path order, fp64; n = edges on the path."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    B, S1, T = py.shape
    bd = full_boundary(B, S1 - 1, T) if bd is None else np.asarray(bd, np.int64)
    out = np.zeros((B, 3))
    for b in range(B):
        s0, t0, s1, t1 = (int(v) for v in bd[b])
        path = []                                           # the weights of the path's edges, in path order
        t = t0
        for s in range(s0, s1 + 1):
            hi = t1 if s == s1 else int(frames[b, s])
            path += [py[b, s, tt] for tt in range(t, hi)]
            if s < s1:
                path.append(px[b, s, hi])
                t = hi + 1 if mod else hi
        acc = 0.0
        for w in path:
            acc = acc + w
        out[b] = (acc, len(path), sum(abs(w) for w in path))
    return out


def edges(frames, scores, bd, S, T, mod, scale=None):
    """px_path, py_path (float64) of the header: the indicator times scale[b]; NaN on the rectangle's edges of a sample with
    a NaN score (not the marker's sample: its boundary is invalid), zeros for one without a path."""
    B = len(scores)
    bd = full_boundary(B, S, T) if bd is None else np.asarray(bd, np.int64)
    ex = np.zeros((B, S, T if mod else T + 1))
    ey = np.zeros((B, S + 1, T))
    g = np.ones(B) if scale is None else np.asarray(scale, np.float64)
    for b in range(B):
        if not _valid(bd[b], S, T):
            continue
        s0, t0, s1, t1 = (int(v) for v in bd[b])
        if np.isnan(scores[b]):
            ex[b, s0:s1, t0:(t1 if mod else t1 + 1)] = np.nan
            ey[b, s0:s1 + 1, t0:t1] = np.nan
            continue
        if not np.isfinite(scores[b]):
            continue
        for s in range(s0, s1 + 1):
            lo = t0 if s == s0 else int(frames[b, s - 1]) + (1 if mod else 0)
            hi = t1 if s == s1 else int(frames[b, s])
            ey[b, s, lo:hi] = g[b]
            if s < s1:
                ex[b, s, hi] = g[b]
    return ex, ey


def brute(X, Y, s0, t0, s1, t1, mod):
    """Every path of one small rectangle: [(weight, frames tuple)] with the weight summed in path order."""
    out = []

    def walk(s, t, acc, fr):
        if s == s1 and t == t1:
            out.append((acc, tuple(fr)))
            return
        if t < t1:
            walk(s, t + 1, acc + Y[s, t], fr)
        if s < s1 and (t < t1 or not mod):
            walk(s + 1, t + 1 if mod else t, acc + X[s, t], fr + [t])

    walk(s0, t0, 0.0, [])
    return out
