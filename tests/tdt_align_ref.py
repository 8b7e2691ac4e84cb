"""Test infrastructure (no GPU) for the TDT best-path alignment (include/rnnt_tdt_align.h).  Everything is fp64 numpy on
log_softmax of the logits as handed over (the caller upcasts the stored ones).

  * best_path: the max-plus recursion over anti-diagonals with back-pointers and the header's tie rule (in-edges in the order
    duration index 0 .. D-1, blank before label, a candidate replaces the best only if strictly greater), vectorised over the
    cells of a diagonal;
  * rescore: the best path constrained to emit label u at frames[u] with duration durs[u] -- only the blank jumps between
    the labels are optimised (a shortest-path problem per lattice row); -inf if the labelling is infeasible;
  * brute: every path from (0, 0) to the terminal node enumerated one by one (tiny lattices only);
  * planted: the planted-path cases that tests/test_tdt_align_cpu.py and tests/test_gpu_tdt_align.py share.
"""
import numpy as np

NEG = -np.inf


def log_probs(x, A, sigma):
    """(token log-probs - sigma, duration log-probs) of logits (..., A + D), natural log."""
    def lsm(z):
        m = z.max(-1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        with np.errstate(divide="ignore"):
            return z - m - np.log(np.exp(z - m).sum(-1, keepdims=True))
    x = np.asarray(x, np.float64)
    return lsm(x[..., :A]) - sigma, lsm(x[..., A:])


def _weights(x, lab, T, L, A, blank, sigma):
    """lb (T, L + 1) blank weights, ll (T, L) label weights, dr (T, L + 1, D) duration weights of one sample."""
    tok, dr = log_probs(x[:T, :L + 1], A, sigma)
    lb = tok[..., blank]
    lab = np.clip(np.asarray(lab[:L], np.int64), 0, A - 1)
    ll = np.take_along_axis(tok[:, :L], lab[None, :, None], -1)[..., 0] if L > 0 else np.zeros((T, 0))
    return lb, ll, dr


def _best_sample(x, lab, T, L, durations, blank, sigma, maxL):
    D = len(durations)
    A = x.shape[-1] - D
    frames, durs = np.full(maxL, -1, np.int32), np.full(maxL, -1, np.int32)
    lb, ll, dr = _weights(x, lab, T, L, A, blank, sigma)
    V = np.full((T, L + 1), NEG)
    BP = np.full((T, L + 1), -1, np.int64)
    with np.errstate(invalid="ignore"):
        for n in range(T + L):
            us = np.arange(max(0, n - (T - 1)), min(n, L) + 1)
            ts = n - us
            best = np.full(len(us), 0.0 if n == 0 else NEG)
            arg = np.full(len(us), -1, np.int64)
            for j, d in enumerate(durations):
                src = ts - d
                sc = np.maximum(src, 0)
                if d > 0:                                                     # blank (t - d, u) -> (t, u)
                    cand = np.where(src >= 0, V[sc, us] + lb[sc, us] + dr[sc, us, j], NEG)
                    up = cand > best
                    best, arg = np.where(up, cand, best), np.where(up, 2 * j, arg)
                if L > 0:                                                     # label (t - d, u - 1) -> (t, u)
                    ok = (src >= 0) & (us >= 1)
                    um = np.maximum(us - 1, 0)
                    cand = np.where(ok, V[sc, um] + ll[sc, np.minimum(um, L - 1)] + dr[sc, um, j], NEG)
                    up = cand > best
                    best, arg = np.where(up, cand, best), np.where(up, 2 * j + 1, arg)
            V[ts, us], BP[ts, us] = best, arg
    score, jf = NEG, -1
    for j, d in enumerate(durations):                                         # the final blanks into the terminal node
        if d > 0 and T - d >= 0:
            cand = V[T - d, L] + lb[T - d, L] + dr[T - d, L, j]
            if cand > score:
                score, jf = cand, j
    if jf < 0 or not np.isfinite(score):
        return (score if np.isnan(score) else NEG), frames, durs
    t, u = T - durations[jf], L
    while (t, u) != (0, 0):
        e = int(BP[t, u])
        d = durations[e >> 1]
        t -= d
        if e & 1:
            u -= 1
            frames[u], durs[u] = t, d
    return score, frames, durs


def best_path(x, labels, tl, ll, durations, blank=0, sigma=0.0):
    """(score (N,) fp64, frames (N, U - 1) int32, durs (N, U - 1) int32) as include/rnnt_tdt_align.h defines them."""
    x = np.asarray(x, np.float64)
    N, _, U, _ = x.shape
    labels = np.asarray(labels).reshape(N, -1)
    durations = tuple(int(d) for d in durations)
    out = [_best_sample(x[b], labels[b], int(tl[b]), int(ll[b]), durations, blank, sigma, U - 1) for b in range(N)]
    return (np.array([o[0] for o in out]), np.stack([o[1] for o in out]).reshape(N, U - 1),
            np.stack([o[2] for o in out]).reshape(N, U - 1))


def _blank_run(lb, dr, u, t0, t1, durations):
    """The best chain of blank edges (t0, u) -> ... -> (t1, u) on row u (t1 may be T: the terminal node); 0 when t0 == t1."""
    g = np.full(t1 - t0 + 1, NEG)
    g[0] = 0.0
    for t in range(t0 + 1, t1 + 1):
        for j, d in enumerate(durations):
            if d > 0 and t - d >= t0:
                g[t - t0] = max(g[t - t0], g[t - d - t0] + lb[t - d, u] + dr[t - d, u, j])
    return g[-1]


def _rescore_sample(x, lab, T, L, durations, blank, sigma, frames, durs):
    D = len(durations)
    lb, ll, dr = _weights(x, lab, T, L, x.shape[-1] - D, blank, sigma)
    total, t = 0.0, 0
    for u in range(L):
        f, d = int(frames[u]), int(durs[u])
        if d not in durations or f < t or f + d >= T:
            return NEG
        total += _blank_run(lb, dr, u, t, f, durations) + ll[f, u] + dr[f, u, durations.index(d)]
        t = f + d
    return total + _blank_run(lb, dr, L, t, T, durations)


def rescore(x, labels, tl, ll, durations, blank, sigma, frames, durs):
    """(N,) fp64: the best path that emits label u at frames[b, u] with duration durs[b, u]; -inf if there is none."""
    x = np.asarray(x, np.float64)
    N = x.shape[0]
    labels = np.asarray(labels).reshape(N, -1)
    durations = tuple(int(d) for d in durations)
    with np.errstate(invalid="ignore"):
        return np.array([_rescore_sample(x[b], labels[b], int(tl[b]), int(ll[b]), durations, blank, sigma, frames[b], durs[b])
                         for b in range(N)])


def _brute_sample(x, lab, T, L, durations, blank, sigma):
    lb, ll, dr = _weights(x, lab, T, L, x.shape[-1] - len(durations), blank, sigma)
    best = [NEG, None]

    def walk(t, u, acc, emitted):
        for j, d in enumerate(durations):
            if d > 0 and (t + d < T or (t + d == T and u == L)):
                s = acc + lb[t, u] + dr[t, u, j]
                if t + d == T:
                    if s > best[0]:
                        best[0], best[1] = s, emitted
                else:
                    walk(t + d, u, s, emitted)
            if u < L and t + d < T:
                walk(t + d, u + 1, acc + ll[t, u] + dr[t, u, j], emitted + ((t, d),))

    walk(0, 0, 0.0, ())
    return best[0], best[1]


def brute(x, labels, tl, ll, durations, blank=0, sigma=0.0):
    """[(score, ((frame, duration), ...) or None)] per sample, by enumeration of every path."""
    x = np.asarray(x, np.float64)
    N = x.shape[0]
    labels = np.asarray(labels).reshape(N, -1)
    durations = tuple(int(d) for d in durations)
    return [_brute_sample(x[b], labels[b], int(tl[b]), int(ll[b]), durations, blank, sigma) for b in range(N)]


# ----------------------------------------------------------------------------- planted paths
PLANT = dict(N=3, T=12, U=5, A=17, durations=(0, 1, 2, 4), boost=12.0)


def _random_path(rng, T, L, durations):
    """A random path (0, 0) -> terminal: [(t, u, is_label, j)] of its edges; every step keeps the terminal reachable."""
    reach = np.zeros((T + 1, L + 1), bool)
    reach[T, L] = True
    for t in range(T - 1, -1, -1):
        for u in range(L, -1, -1):
            for d in durations:
                if d > 0 and (t + d < T or (t + d == T and u == L)) and reach[t + d, u]:
                    reach[t, u] = True
                if u < L and t + d < T and reach[t + d, u + 1]:
                    reach[t, u] = True
    assert reach[0, 0]
    path, t, u = [], 0, 0
    while t < T:
        moves = []
        for j, d in enumerate(durations):
            if d > 0 and (t + d < T or (t + d == T and u == L)) and reach[t + d, u]:
                moves.append((0, j))
            if u < L and t + d < T and reach[t + d, u + 1]:
                moves.append((1, j))
        is_label, j = moves[int(rng.integers(len(moves)))]
        path.append((t, u, is_label, j))
        t, u = t + durations[j], u + is_label
    return path


def planted(seed):
    """One planted case: N(0, 1) logits (N, T, U, A + D) fp64 with +boost on the token and the duration logit of every edge of
    a random path per sample -> (x, labels, tl, ll, frames, durs); frames / durs are the plant's.  blank = 0."""
    p = PLANT
    N, T, U, A, durations = p["N"], p["T"], p["U"], p["A"], p["durations"]
    rng = np.random.default_rng(7000 + seed)
    tl = np.array([T, int(rng.integers(4, T)), int(rng.integers(2, T))], np.int32)
    ll = np.array([U - 1, int(rng.integers(1, U - 1)), 0], np.int32)
    labels = rng.integers(1, A, size=(N, U - 1)).astype(np.int32)
    x = rng.standard_normal((N, T, U, A + len(durations)))
    frames, durs = np.full((N, U - 1), -1, np.int32), np.full((N, U - 1), -1, np.int32)
    for b in range(N):
        for t, u, is_label, j in _random_path(rng, int(tl[b]), int(ll[b]), durations):
            x[b, t, u, labels[b, u] if is_label else 0] += p["boost"]
            x[b, t, u, A + j] += p["boost"]
            if is_label:
                frames[b, u], durs[b, u] = t, durations[j]
    return x, labels, tl, ll, frames, durs
