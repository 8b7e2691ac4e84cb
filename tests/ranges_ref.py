"""The fp64 reference of include/rnnt_ranges.h, written from the header in plain loops with its fixed order of additions (not
collected, not a conftest): the occupancy g, the window sums w(s), the raw starts, the repair passes as the SERIAL passes the
header states, and the coverage.  Python floats are IEEE fp64 and every sum here is one addition per element from 0.0 in
ascending u, so the device must return the same bits."""
import numpy as np


def tile(U):
    """Frames per tile of the kernels (rg_tile, csrc/rnnt_ranges_kernels.h) for U = S + 1 rows."""
    tf = 32
    while tf > 1 and tf * (U | 1) > 6144:
        tf >>= 1
    return tf


def lengths(boundary, B, S, T):
    """(S_b, T_b) per sample: columns 2 and 3 clamped into [0, S] and [0, T]; None: S and T."""
    if boundary is None:
        return [S] * B, [T] * B
    bd = np.asarray(boundary)
    return [int(min(max(v, 0), S)) for v in bd[:, 2]], [int(min(max(v, 0), T)) for v in bd[:, 3]]


def column(px, py, b, t, Sb):
    """g[0 .. S_b] of frame t as Python floats: double(py) + (u < S_b ? double(px) : 0.0).  Nothing else is read."""
    y = np.asarray(py[b, :Sb + 1, t], dtype=np.float64).tolist()
    x = np.asarray(px[b, :Sb, t], dtype=np.float64).tolist() + [0.0]
    return [a + c for a, c in zip(y, x)]


def window(g, s, R, Sb):
    w = 0.0
    for u in range(s, min(s + R - 1, Sb) + 1):
        w = w + g[u]
    return w


def raw_start(g, R, Sb):
    """(start, [w(0), ..., w(smax)]): the largest w(s) over s in [0, smax], the smallest s among equals; a NaN never wins."""
    smax = max(0, Sb + 1 - R)
    best, bs, have = 0.0, 0, False
    sums = []
    for s in range(smax + 1):
        w = window(g, s, R, Sb)
        sums.append(w)
        if w == w and (not have or w > best):
            best, bs, have = w, s, True
    return (bs if have else 0), sums


def repair(raw, Tb, Sb, R, step):
    """Steps 2 and 3 of the header on the raw starts of the frames t < T_b; returns the T_b starts."""
    smax = max(0, Sb + 1 - R)
    if Tb == 0:
        return []
    if smax > (Tb - 1) * step:
        return [min(t * step, smax) for t in range(Tb)]
    s = [min(max(int(raw[t]), max(0, smax - (Tb - 1 - t) * step)), min(smax, t * step)) for t in range(Tb)]
    for t in range(1, Tb):
        s[t] = max(s[t], s[t - 1])
    for t in range(Tb - 2, -1, -1):
        s[t] = max(s[t], s[t + 1] - step)
    return s


def ranges_from_gamma(gamma, Tb, Sb, R, step):
    """The whole rule on an fp64 occupancy gamma (T_b, S_b + 1) -- tests/pruned_ref.ranges_rule's argument."""
    raw = [raw_start([float(v) for v in gamma[t, :Sb + 1]], R, Sb)[0] for t in range(Tb)]
    return np.array(repair(raw, Tb, Sb, R, step), dtype=np.int64)


def prune_ranges(px, py, boundary, R, step):
    """ranges (B, T) int32 of entry 1.  px, py: numpy arrays of any float type (upcast exactly), px (B, S, T + 1) or (B, S, T)."""
    B, S1, T = py.shape
    S = S1 - 1
    Sbs, Tbs = lengths(boundary, B, S, T)
    out = np.zeros((B, T), np.int32)
    for b in range(B):
        Sb, Tb = Sbs[b], Tbs[b]
        raw = [raw_start(column(px, py, b, t, Sb), R, Sb)[0] for t in range(Tb)]
        out[b, :Tb] = repair(raw, Tb, Sb, R, step)
    return out


def coverage(px, py, boundary, ranges, R):
    """kept (B, T) float64 of entry 2."""
    B, S1, T = py.shape
    S = S1 - 1
    Sbs, Tbs = lengths(boundary, B, S, T)
    out = np.zeros((B, T), np.float64)
    with np.errstate(all="ignore"):
        for b in range(B):
            Sb, Tb = Sbs[b], Tbs[b]
            for t in range(Tb):
                g = column(px, py, b, t, Sb)
                w = window(g, min(max(int(ranges[b, t]), 0), Sb), R, Sb)
                c = 0.0
                for u in range(Sb + 1):
                    c = c + g[u]
                out[b, t] = 0.0 if c == 0.0 else float(np.float64(w) / np.float64(c))
    return out


def modified_path_exists(s, Tb, Sb, R):
    """Brute-force reachability in the MODIFIED lattice: from node (u, t) inside frame t's window the frame edge goes to
    (u, t + 1) and the symbol edge to (u + 1, t + 1); is (S_b, T_b) reached from (0, 0)?"""
    reach = np.zeros((Tb + 1, Sb + 1), bool)
    reach[0, 0] = True
    for t in range(Tb):
        for u in range(Sb + 1):
            if reach[t, u] and int(s[t]) <= u < int(s[t]) + R:
                reach[t + 1, u] = True
                if u < Sb:
                    reach[t + 1, u + 1] = True
    return bool(reach[Tb, Sb])


# ----------------------------------------------------------------------------- the additive joint's occupancy, end to end
# Seeds of additive_problem whose best and runner-up window sums differ by at least ADD_GAP relative in every frame of the
# fp64 reference (tests/test_ranges_cpu.py checks each; a seed that fails is replaced here, never skipped at run time).
ADD_SEEDS = (2, 3, 4, 7)                # (0, 1, 5, 6 and 8 .. 11 have a frame below the gap)
ADD_GAP = 1e-3


def additive_problem(seed):
    """A random additive joint f (B, T, A) + g (B, U, A) of float32 values with ragged lengths; px, py of its lattice in
    fp64 (log-softmax over the classes; blank 0), the boundary rows, and from the fp64 occupancy (pruned_ref.occupancy_add)
    the ranges of the rule at step = R - 1 and the smallest relative gap between best and runner-up window sums."""
    from tests import pruned_ref
    rng = np.random.default_rng([seed, 77])
    B, T, U, A, Rw = 3, 10, 7, 5, 3
    S = U - 1
    f = (rng.standard_normal((B, T, A)) * 2).astype(np.float32)
    g = (rng.standard_normal((B, U, A)) * 2).astype(np.float32)
    labels = rng.integers(1, A, (B, S)).astype(np.int32)
    T_b, L_b = np.array([T, 7, T], np.int32), np.array([S, 3, 2], np.int32)
    z = f[:, :, None, :].astype(np.float64) + g[:, None, :, :].astype(np.float64)
    mx = z.max(-1, keepdims=True)
    lp = z - (mx + np.log(np.exp(z - mx).sum(-1, keepdims=True)))          # (B, T, U, A)
    py = np.ascontiguousarray(lp[..., 0].transpose(0, 2, 1))                # (B, U, T)
    px = np.full((B, S, T + 1), -np.inf)
    for b in range(B):
        for u in range(S):
            px[b, u, :T] = lp[b, :, u, labels[b, u]]
    boundary = np.stack([np.zeros(B), np.zeros(B), L_b, T_b], 1).astype(np.int64)
    ranges, gap = np.zeros((B, T), np.int32), np.inf
    for b in range(B):
        Tb, Lb = int(T_b[b]), int(L_b[b])
        gamma = pruned_ref.occupancy_add(f[b], g[b], labels[b], Tb, Lb)
        ranges[b, :Tb] = ranges_from_gamma(gamma, Tb, Lb, Rw, Rw - 1)
        for t in range(Tb):
            sums = raw_start([float(v) for v in gamma[t, :Lb + 1]], Rw, Lb)[1]
            if len(sums) > 1:
                top = sorted(sums, reverse=True)[:2]
                gap = min(gap, (top[0] - top[1]) / top[0])
    return dict(f=f, g=g, labels=labels, T_b=T_b, L_b=L_b, R=Rw, px=px, py=py, boundary=boundary, ranges=ranges, gap=gap)
