"""The best-path alignment's numpy fp64 reference: a Viterbi with the tie rule of include/rnnt.h, and the score of a given path.
tests/test_align_cpu.py checks the Viterbi against brute-force enumeration of every path."""
import numpy as np


def viterbi_np(lp, labels, T, U, blank):
    """lp: (maxT, maxU, A) log-probs of one sample (fp64); U = number of labels.  Returns (score, frames[U]).
    Label predecessor (t, u-1) wins only when strictly better than the blank one (t-1, u)."""
    lp = np.asarray(lp, dtype=np.float64)
    if np.isnan(lp[:T, :U + 1, blank]).any() or (U and np.isnan(lp[np.arange(T)[:, None], np.arange(U)[None], labels[:U][None]]).any()):
        return float("nan"), [-1] * U
    v = np.full((T, U + 1), -np.inf)
    v[0, 0] = 0.0
    for t in range(T):
        for u in range(U + 1):
            if t == 0 and u == 0:
                continue
            stay = v[t - 1, u] + lp[t - 1, u, blank] if t > 0 else -np.inf
            emit = v[t, u - 1] + lp[t, u - 1, labels[u - 1]] if u > 0 else -np.inf
            v[t, u] = emit if emit > stay else stay
    s = v[T - 1, U] + lp[T - 1, U, blank]
    if not np.isfinite(s):
        return s, [-1] * U
    frames = [-1] * U
    t, u = T - 1, U
    while t > 0 or u > 0:
        label = u > 0 and (t == 0 or v[t, u - 1] + lp[t, u - 1, labels[u - 1]] > v[t - 1, u] + lp[t - 1, u, blank])
        if label:
            frames[u - 1] = t
            u -= 1
        else:
            t -= 1
    return s, frames


def path_score(lp, labels, T, U, blank, frames):
    """log-probability of the path that emits label u at frames[u] (fp64)."""
    lp = np.asarray(lp, dtype=np.float64)
    s, u = 0.0, 0
    for t in range(T):
        while u < U and frames[u] == t:
            s += lp[t, u, labels[u]]
            u += 1
        s += lp[t, u, blank]
    return s
