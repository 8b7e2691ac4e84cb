"""numpy fp64 reference of include/rnnt_expect.h: the forward recursion of (a, A) and the backward recursion of (bt, Bc)
written out node by node as the header defines them, the four gradients for arbitrary per-sample scales from the header's
edge formulas (occ_e = exp(a[u] + w + bt[v] - score)), an enumeration of every path of a tiny lattice (`walk`, as
tests/bestpath_ref.py), and the same recursion run on |c| -- Eabs[b] and the per-edge E[|C| | e], the magnitudes the bounds
of tests/test_gpu_expect.py are made of.  It is given the STORED values of px / py / cx / cy as doubles and reads nothing
outside a rectangle's edge sets.  Independent of the library: no chunks, no shares, a plain logaddexp."""
import numpy as np

from tests.bestpath_ref import MARKER, _valid
from tests.mi_ref import edge_masks, full_boundary                      # noqa: F401  (this module's names too)

NEG = float("-inf")


def _combine(x, xc, y, yc):
    """(w, c) of a node from its candidates (arrays): w = logaddexp(x, y), c the convex combination of the header -- a
    candidate of -inf is selected out, its cost never looked at; both -inf: (-inf, 0)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nx, ny = x == NEG, y == NEG
        w = np.where(nx & ny, NEG, np.logaddexp(np.where(nx & ny, 0.0, x), np.where(nx & ny, 0.0, y)))
        r = np.exp(np.where(nx, 0.0, x) - np.where(nx & ny, 0.0, w))
        c = np.where(nx, np.where(ny, 0.0, yc), np.where(ny, xc, r * xc + (1.0 - r) * yc))
    return w, c


def _steps(Sr, Tr, mod):
    """The rows i and frames j of the nodes of every step but the first: a frame column (modified type) or an
    anti-diagonal (regular type) -- the nodes that do not depend on one another."""
    for d in range(1, (Tr if mod else Tr + Sr) + 1):
        if mod:
            yield np.arange(Sr + 1), np.full(Sr + 1, d)
        else:
            i = np.arange(max(0, d - Tr), min(Sr, d) + 1)
            yield i, d - i


def sweep_one(X, Y, CX, CY, s0, t0, s1, t1, mod):
    """-> dict(a, A, bt, Bc, bad, badc) over the nodes of one rectangle, local coordinates (Sr + 1, Tr + 1); X = px[b], ...
    whole arrays, absolute indices.  bad: a NaN or +inf weight on an edge of the rectangle; badc: a non-finite cost on a
    reachable edge of finite weight.  Every node gets exactly the recursion of the header."""
    Sr, Tr = s1 - s0, t1 - t0
    Xr, Yr = X[s0:s1, t0:(t1 if mod else t1 + 1)], Y[s0:s1 + 1, t0:t1]
    Cx, Cy = CX[s0:s1, t0:(t1 if mod else t1 + 1)], CY[s0:s1 + 1, t0:t1]
    bad = bool((~(Xr < np.inf)).any() or (~(Yr < np.inf)).any())
    a = np.full((Sr + 1, Tr + 1), NEG)
    A = np.zeros((Sr + 1, Tr + 1))
    bt = np.full((Sr + 1, Tr + 1), NEG)
    Bc = np.zeros((Sr + 1, Tr + 1))
    if bad:
        return dict(a=a, A=A, bt=bt, Bc=Bc, bad=True, badc=False)
    badc = False
    a[0, 0] = 0.0
    bt[Sr, Tr] = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for i, j in _steps(Sr, Tr, mod):
            n = len(i)
            x, xc, y, yc = np.full(n, NEG), np.zeros(n), np.full(n, NEG), np.zeros(n)
            jx = j - 1 if mod else j
            ex = (i > 0) & (jx >= 0)
            x[ex] = a[i[ex] - 1, jx[ex]] + Xr[i[ex] - 1, jx[ex]]
            xc[ex] = A[i[ex] - 1, jx[ex]] + Cx[i[ex] - 1, jx[ex]]
            ey = j > 0
            y[ey] = a[i[ey], j[ey] - 1] + Yr[i[ey], j[ey] - 1]
            yc[ey] = A[i[ey], j[ey] - 1] + Cy[i[ey], j[ey] - 1]
            badc = badc or bool(((x > NEG) & ~np.isfinite(xc)).any() or ((y > NEG) & ~np.isfinite(yc)).any())
            a[i, j], A[i, j] = _combine(x, xc, y, yc)
        for i, j in _steps(Sr, Tr, mod):                       # mirrored: node (Sr - i, Tr - j) from its out-edges
            i, j = Sr - i, Tr - j
            n = len(i)
            x, xc, y, yc = np.full(n, NEG), np.zeros(n), np.full(n, NEG), np.zeros(n)
            ex = (i < Sr) & ((j < Tr) if mod else (j <= Tr))
            vi, vj = i[ex] + 1, (j[ex] + 1 if mod else j[ex])
            x[ex] = Xr[i[ex], j[ex]] + bt[vi, vj]
            xc[ex] = Cx[i[ex], j[ex]] + Bc[vi, vj]
            ey = j < Tr
            y[ey] = Yr[i[ey], j[ey]] + bt[i[ey], j[ey] + 1]
            yc[ey] = Cy[i[ey], j[ey]] + Bc[i[ey], j[ey] + 1]
            bt[i, j], Bc[i, j] = _combine(x, xc, y, yc)
    return dict(a=a, A=A, bt=bt, Bc=Bc, bad=False, badc=badc)


def expected_cost(px, py, cx, cy, bd=None, mod=None, g_expect=None, g_score=None):
    """-> dict(scores (B,), expect (B,), nodes (B, S + 1, T + 1, 2), gx, gy, hx, hy (the gradients in px, py, cx, cy for
    the scales g_expect -- default 1 -- and g_score -- default 0 --), occx, occy (the occupations), Eabs (B,), nodes_abs
    (B, S + 1, T + 1) (the expected prefix |cost| of every node), magx, magy (occ_e (E[|C| | e] + Eabs[b]): the size of the
    terms px_grad / py_grad at g_expect = 1 are differences of))."""
    px, py, cx, cy = (np.asarray(v, np.float64) for v in (px, py, cx, cy))
    B, S1, T = py.shape
    S = S1 - 1
    mod = (px.shape[2] == T) if mod is None else bool(mod)
    bd = full_boundary(B, S, T) if bd is None else np.asarray(bd, np.int64)
    ge = np.ones(B) if g_expect is None else np.asarray(g_expect, np.float64)
    gs = np.zeros(B) if g_score is None else np.asarray(g_score, np.float64)
    out = dict(scores=np.zeros(B), expect=np.zeros(B), nodes=np.zeros((B, S + 1, T + 1, 2)), Eabs=np.zeros(B),
               nodes_abs=np.zeros((B, S + 1, T + 1)))
    out["nodes"][..., 0] = NEG
    for k, like in (("gx", px), ("gy", py), ("hx", px), ("hy", py), ("occx", px), ("occy", py), ("magx", px), ("magy", py)):
        out[k] = np.zeros(like.shape)
    for b in range(B):
        if not _valid(bd[b], S, T):
            out["scores"][b] = MARKER
            continue
        s0, t0, s1, t1 = (int(v) for v in bd[b])
        Sr, Tr = s1 - s0, t1 - t0
        sx = (b, slice(s0, s1), slice(t0, t1 if mod else t1 + 1))
        sy = (b, slice(s0, s1 + 1), slice(t0, t1))
        r = sweep_one(px[b], py[b], cx[b], cy[b], s0, t0, s1, t1, mod)
        if r["bad"]:
            out["scores"][b] = out["expect"][b] = np.nan
            for k in ("gx", "hx"):
                out[k][sx] = np.nan
            for k in ("gy", "hy"):
                out[k][sy] = np.nan
            continue
        out["nodes"][b, s0:s1 + 1, t0:t1 + 1, 0] = r["a"]
        out["nodes"][b, s0:s1 + 1, t0:t1 + 1, 1] = r["A"]
        sc = r["a"][Sr, Tr]
        out["scores"][b] = sc
        out["expect"][b] = np.nan if r["badc"] else (r["A"][Sr, Tr] if sc > NEG else 0.0)
        if not sc > NEG or r["badc"]:
            continue
        ec = r["A"][Sr, Tr]
        with np.errstate(invalid="ignore"):
            m = sweep_one(px[b], py[b], np.abs(cx[b]), np.abs(cy[b]), s0, t0, s1, t1, mod)
        out["Eabs"][b] = m["A"][Sr, Tr]
        out["nodes_abs"][b, s0:s1 + 1, t0:t1 + 1] = m["A"]
        a, A, bt, Bc = r["a"], r["A"], r["bt"], r["Bc"]
        # the edges u -> v of the rectangle: x edges u = (i, j), v = (i + 1, j | j + 1); y edges v = (i, j + 1)
        nx = Tr if mod else Tr + 1
        for X, Cc, key_g, key_h, key_o, key_m, sl, us, vs in (
                (px, cx, "gx", "hx", "occx", "magx", sx, (slice(0, Sr), slice(0, nx)),
                 (slice(1, Sr + 1), slice(1, nx + 1) if mod else slice(0, nx))),
                (py, cy, "gy", "hy", "occy", "magy", sy, (slice(0, Sr + 1), slice(0, Tr)), (slice(0, Sr + 1), slice(1, Tr + 1)))):
            w, c = X[sl], Cc[sl]
            with np.errstate(invalid="ignore", over="ignore"):
                occ = np.exp(a[us] + w + bt[vs] - sc)
                live = occ > 0
                dev = np.where(live, A[us] + np.where(live, c, 0.0) + Bc[vs] - ec, 0.0)
                mabs = np.where(live, m["A"][us] + np.where(live, np.abs(c), 0.0) + m["Bc"][vs], 0.0)
            occ = np.where(live, occ, 0.0)
            out[key_o][sl] = occ
            out[key_g][sl] = ge[b] * occ * dev + gs[b] * occ
            out[key_h][sl] = ge[b] * occ
            out[key_m][sl] = occ * (mabs + out["Eabs"][b])
    return out


def walk(X, Y, CX, CY, s0, t0, s1, t1, mod):
    """Every path of one small rectangle: [(weight, cost, [("x" | "y", s, t), ...])], absolute edge coordinates; paths
    through a -inf edge are left out (their costs are never looked at)."""
    out = []

    def go(s, t, w, c, edges):
        if w == NEG:
            return
        if s == s1 and t == t1:
            out.append((w, c, list(edges)))
            return
        if t < t1:
            wy = Y[s, t]
            go(s, t + 1, w + wy, c + (CY[s, t] if wy > NEG else 0.0), edges + [("y", s, t)])
        if s < s1 and (t < t1 or not mod):
            wx = X[s, t]
            go(s + 1, t + 1 if mod else t, w + wx, c + (CX[s, t] if wx > NEG else 0.0), edges + [("x", s, t)])

    go(s0, t0, 0.0, 0.0, [])
    return out


def enumerate_one(X, Y, CX, CY, bd_row, mod, ge=1.0, gs=0.0):
    """(score, expect, gx, gy, hx, hy) of one sample from its enumerated paths: p = softmax of the weights, expect =
    sum p C, d expect / d w_e = sum over the paths through e of p (C - expect), d expect / d c_e = d score / d w_e =
    sum over the paths through e of p."""
    s0, t0, s1, t1 = (int(v) for v in bd_row)
    paths = walk(X, Y, CX, CY, s0, t0, s1, t1, mod)
    gx, gy, hx, hy = np.zeros(X.shape), np.zeros(Y.shape), np.zeros(X.shape), np.zeros(Y.shape)
    if not paths:
        return NEG, 0.0, gx, gy, hx, hy
    w = np.array([p[0] for p in paths])
    c = np.array([p[1] for p in paths])
    score = float(np.logaddexp.reduce(w))
    p = np.exp(w - score)
    expect = float((p * c).sum())
    for pk, ck, (_, _, edges) in zip(p, c, paths):
        for kind, s, t in edges:
            g, h = (gx, hx) if kind == "x" else (gy, hy)
            g[s, t] += ge * pk * (ck - expect) + gs * pk
            h[s, t] += ge * pk
    return score, expect, gx, gy, hx, hy
