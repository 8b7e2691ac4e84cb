"""numpy fp64 reference of include/rnnt_sample.h: the log-sum sweep written out node by node as the header defines it (a
-inf candidate selected out), the walks back from the terminal with the header's one comparison u < r and its additions in
walk order, the weight of given paths in that same order, the rule that says whether a row of frames is a path, and the
accumulated edge indicators in ascending k.  It is given the STORED values of px / py as doubles and reads nothing outside a
rectangle's edge sets.  Independent of the library: no chunks, a plain np.logaddexp.  The walks of one sample advance together
as arrays over k; every walk still makes exactly the header's decisions and additions.

`margin(...)` is the bound on |r_device - r_reference| that tests/test_sample_cpu.py holds every decision of every case of
tests/sample_forms.py against; its derivation is in its docstring."""
import numpy as np

from tests.bestpath_ref import MARKER, _valid
from tests.mi_ref import edge_masks, full_boundary                      # noqa: F401  (this module's names too)

NEG = float("-inf")
EPS = 2.0 ** -52


def sweep_one(X, Y, s0, t0, s1, t1, mod):
    """(a, bad): a over the nodes of one rectangle, local coordinates (Sr + 1, Tr + 1); X = px[b], Y = py[b] whole arrays,
    absolute indices.  bad: a NaN or +inf on an edge of the rectangle."""
    Sr, Tr = s1 - s0, t1 - t0
    Xr, Yr = X[s0:s1, t0:(t1 if mod else t1 + 1)], Y[s0:s1 + 1, t0:t1]
    bad = bool((~(Xr < np.inf)).any() or (~(Yr < np.inf)).any())
    a = np.full((Sr + 1, Tr + 1), NEG)
    a[0, 0] = 0.0
    if bad:
        return a, True
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for d in range(1, (Tr if mod else Tr + Sr) + 1):
            if mod:
                i, j = np.arange(Sr + 1), np.full(Sr + 1, d)
            else:
                i = np.arange(max(0, d - Tr), min(Sr, d) + 1)
                j = d - i
            x, y = np.full(len(i), NEG), np.full(len(i), NEG)
            jx = j - 1 if mod else j
            ex = (i > 0) & (jx >= 0)
            x[ex] = a[i[ex] - 1, jx[ex]] + Xr[i[ex] - 1, jx[ex]]
            ey = j > 0
            y[ey] = a[i[ey], j[ey] - 1] + Yr[i[ey], j[ey] - 1]
            nx, ny = x == NEG, y == NEG
            both = np.logaddexp(np.where(nx, 0.0, x), np.where(ny, 0.0, y))
            a[i, j] = np.where(nx, y, np.where(ny, x, both))        # selected out: the other candidate bit for bit
    return a, False


def walk_one(X, Y, a, s0, t0, s1, t1, mod, U):
    """The K walks of one sample from its a (local coordinates): U (K, S + T) float32 -> frames (K, S) int32 with -1 outside
    the walk's symbol edges, W (K,), shares: the list of (u, r) arrays of every decision made."""
    K, S = U.shape[0], X.shape[0]
    frames = np.full((K, S), -1, np.int32)
    W = np.zeros(K)
    s, t = np.full(K, s1), np.full(K, t1)
    cur = np.full(K, a[s1 - s0, t1 - t0])
    ks = np.arange(K)
    shares = []
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range((s1 - s0) + (t1 - t0)):
            act = (s > s0) | (t > t0)
            if not act.any():
                break
            tp = t - 1 if mod else t
            hasx, hasy = act & (s > s0) & (tp >= t0), act & (t > t0)
            sx, tx = np.where(hasx, s - 1, s0), np.where(hasx, tp, t0)
            ax = np.where(hasx, a[sx - s0, tx - t0], NEG)
            wx = np.where(hasx, X[np.minimum(sx, max(S - 1, 0)), tx] if S else NEG, NEG)
            ty = np.where(hasy, t - 1, t0)
            ay = np.where(hasy, a[s - s0, ty - t0], NEG)
            wy = np.where(hasy, Y[s, np.minimum(ty, Y.shape[1] - 1)], NEG)
            dec = act & (s > s0)
            u = U[ks, np.where(dec, (s - s0) + (t - t0) - 1, 0)].astype(np.float64)
            r = np.exp(ax + wx - cur)
            sym = dec & (u < r)
            assert not (sym & ~hasx).any() and not (act & ~sym & ~hasy).any()        # a walk stays on the lattice
            shares.append((u[dec], r[dec]))
            frames[ks[sym], s[sym] - 1] = tp[sym]
            W = np.where(act, W + np.where(sym, wx, wy), W)
            cur = np.where(act, np.where(sym, ax, ay), cur)
            s, t = np.where(sym, s - 1, s), np.where(sym, tp, np.where(act, t - 1, t))
    assert ((s == s0) & (t == t0)).all()
    return frames, W, shares


def sample(px, py, uniforms, bd=None, mod=None):
    """Entry 1 -> dict(scores (B,), alpha (B, S + 1, T + 1), frames (B, K, S) int32, weights (B, K), gap (B,): the smallest
    |u - r| over the decisions of the sample's walks (inf without one), amax (B,): max |a| over the finite nodes)."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    B, S1, T = py.shape
    S = S1 - 1
    K = uniforms.shape[1]
    mod = (px.shape[2] == T) if mod is None else bool(mod)
    bd = full_boundary(B, S, T) if bd is None else np.asarray(bd, np.int64)
    out = dict(scores=np.zeros(B), alpha=np.full((B, S + 1, T + 1), NEG), frames=np.full((B, K, S), -1, np.int32),
               weights=np.full((B, K), np.nan), gap=np.full(B, np.inf), amax=np.zeros(B))
    for b in range(B):
        if not _valid(bd[b], S, T):
            out["scores"][b] = MARKER
            continue
        s0, t0, s1, t1 = (int(v) for v in bd[b])
        a, bad = sweep_one(px[b], py[b], s0, t0, s1, t1, mod)
        if bad:
            out["scores"][b] = np.nan                       # (alpha: unspecified)
            continue
        out["alpha"][b, s0:s1 + 1, t0:t1 + 1] = a
        sc = out["scores"][b] = a[-1, -1]
        fin = np.isfinite(a)
        out["amax"][b] = np.abs(a[fin]).max() if fin.any() else 0.0
        if sc == NEG:
            out["weights"][b] = NEG
            continue
        fr, W, shares = walk_one(px[b], py[b], a, s0, t0, s1, t1, mod, uniforms[b])
        out["frames"][b], out["weights"][b] = fr, W
        gaps = [np.abs(u - r).min() for u, r in shares if len(u)]
        out["gap"][b] = min(gaps) if gaps else np.inf
    return out


def margin(steps, amax):
    """A bound on |r_device - r_reference| of any decision of a lattice swept in `steps` steps with max |a| = amax.

    Each node of the sweep costs at most 8 fp64 roundings (the two candidates' additions, lo - hi, exp, 1 + e inside log1p,
    log1p, the final addition, and one of slack for the library functions' own last-place error), each of at most
    EPS (1 + amax) in absolute terms since every intermediate is bounded by 1 + amax; logaddexp does not expand errors
    (its partial derivatives are non-negative and sum to 1), so a node's error is at most steps 8 EPS (1 + amax), on the device
    and in this reference alike.  r = exp(a' + w - a) of an argument <= 0 (up to that error) has derivative <= 1: two such
    node errors, two roundings of the argument and two for exp (4 EPS (1 + amax) bounds them, r <= 1 and the argument below
    1 + amax in magnitude where r is not 0 to the last place).  Two computations that each err by that much differ by
    at most twice it."""
    return 2.0 * (2.0 * 8.0 * steps + 4.0) * EPS * (1.0 + amax)


def is_path(row, s0, t0, s1, t1, mod):
    """A row of frames is a path of its rectangle: include/rnnt_sample.h, GIVEN PATHS."""
    prev = t0 - 1 if mod else t0
    for s in range(s0, s1):
        f = int(row[s])
        if not (t0 <= f <= (t1 - 1 if mod else t1)) or (f <= prev if mod else f < prev):
            return False
        prev = f
    return True


def path_edges_of(X, Y, row, s0, t0, s1, t1, mod):
    """The weights of the path's edges in PATH order (source first)."""
    parts = []
    t = t0
    for s in range(s0, s1 + 1):
        hi = t1 if s == s1 else int(row[s])
        parts.append(Y[s, t:hi])
        if s < s1:
            parts.append(X[s, hi:hi + 1])
            t = hi + 1 if mod else hi
    return np.concatenate(parts) if parts else np.zeros(0)


def _as_bks(frames, B, S):
    """frames (B, K, S), or (B, S) for K = 1 (S may be 0: no reshape by -1)."""
    frames = np.asarray(frames)
    return frames.reshape(B, 1, S) if frames.ndim == 2 else frames.reshape(B, frames.shape[1], S)


def path_weights(px, py, frames, bd=None, mod=None):
    """Entries 1 and 3 -> (W (B, K), n (B, K), sumabs (B, K)): W added from 0.0 in WALK order (the terminal's in-edge
    first), one IEEE addition per edge (np.cumsum is sequential); NaN for a row that is no path or a bad boundary; n the
    number of edges, sumabs the sum of |w| over the finite ones."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    B, S1, T = py.shape
    S = S1 - 1
    frames = _as_bks(frames, B, S)
    K = frames.shape[1]
    mod = (px.shape[2] == T) if mod is None else bool(mod)
    bd = full_boundary(B, S, T) if bd is None else np.asarray(bd, np.int64)
    W, n, sa = np.full((B, K), np.nan), np.zeros((B, K), np.int64), np.zeros((B, K))
    for b in range(B):
        if not _valid(bd[b], S, T):
            continue
        rect = tuple(int(v) for v in bd[b])
        for k in range(K):
            if not is_path(frames[b, k], *rect, mod):
                continue
            w = path_edges_of(px[b], py[b], frames[b, k], *rect, mod)[::-1]
            with np.errstate(invalid="ignore"):
                W[b, k] = np.cumsum(w)[-1] if len(w) else 0.0
            n[b, k] = len(w)
            sa[b, k] = np.abs(w[np.isfinite(w)]).sum()
    return W, n, sa


def path_edges(frames, coeff, bd, S, T, mod):
    """Entry 4 -> (px_acc, py_acc) float64: sum over k ascending of coeff[b, k] 1[edge on path k]; rows that are no path are
    left out; zeros for a bad boundary."""
    frames = np.asarray(frames)
    B = frames.shape[0]
    frames = _as_bks(frames, B, S)
    K = frames.shape[1]
    bd = full_boundary(B, S, T) if bd is None else np.asarray(bd, np.int64)
    cf = np.ones((B, K)) if coeff is None else np.asarray(coeff, np.float64).reshape(B, K)
    ax, ay = np.zeros((B, S, T if mod else T + 1)), np.zeros((B, S + 1, T))
    for b in range(B):
        if not _valid(bd[b], S, T):
            continue
        s0, t0, s1, t1 = (int(v) for v in bd[b])
        for k in range(K):
            if not is_path(frames[b, k], s0, t0, s1, t1, mod):
                continue
            for s in range(s0, s1 + 1):
                lo = t0 if s == s0 else int(frames[b, k, s - 1]) + (1 if mod else 0)
                hi = t1 if s == s1 else int(frames[b, k, s])
                ay[b, s, lo:hi] += cf[b, k]
                if s < s1:
                    ax[b, s, hi] += cf[b, k]
    return ax, ay
