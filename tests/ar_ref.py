"""Test infrastructure (no GPU) for the alignment-restricted RNN-T loss (include/rnnt_ar.h).

  * ar_autograd: the loss written straight from the header's definition as an fp64 log-sum-exp recursion over the standard
    lattice, alpha(t, u) = lse(alpha(t - 1, u) + lp_blank(t - 1, u), alpha(t, u - 1) + lp_label(t, u - 1)) with the label
    edge of (t, u - 1) present only when lo_{u-1} <= t <= hi_{u-1}, differentiated by torch.autograd -- only the forward
    recursion is written down, as in tests/mblank_ref.py;
  * ar_brute: every path enumerated one by one (tiny lattices only), the same autograd;
  * ar_formula: the gradient by the header's closed formula from autograd's edge posteriors;
  * bounds: the header's e (prefix maximum of lo), l (suffix minimum of hi) and the feasibility statement;
  * band_mask: the rows a path can pass through (e_u <= t <= l_u; none for a sample without a path); in_lattice_mask:
    t < T_b, u <= L_b;
  * windows: a generator of feasible windows around a random non-decreasing alignment.
"""
import numpy as np
import torch

from tests.mblank_ref import NEG                      # "log zero": -inf would turn logsumexp's derivative into NaN
from tests.side_check import in_lattice_mask          # noqa: F401  (t < T_b, u <= L_b)

WIDE = 1 << 20                                         # a slack no utterance reaches: "unrestricted"


def bounds(T, L, lo, hi):
    """e (L + 1,), l (L + 1,) and feasible of one sample with T frames, L labels and the windows lo, hi (their first L
    entries): e_0 = 0, e_{u+1} = max(e_u, lo_u); l_L = T - 1, l_u = min(l_{u+1}, hi_u); feasible iff e_{u+1} <= l_u for
    every u < L."""
    T, L = int(T), int(L)
    e = np.zeros(L + 1, np.int64)
    l = np.full(L + 1, T - 1, np.int64)
    for u in range(L):
        e[u + 1] = max(e[u], int(lo[u]))
    for u in range(L - 1, -1, -1):
        l[u] = min(l[u + 1], int(hi[u]))
    return e, l, all(e[u + 1] <= l[u] for u in range(L))


def band_mask(shape, act_lens, label_lens, lo, hi):
    """(N, T, U) bool: the in-lattice rows with e_u <= t <= l_u; a sample without a path has none."""
    N, T, U = shape[:3]
    m = np.zeros((N, T, U), bool)
    for b in range(N):
        Tb, Lb = int(act_lens[b]), int(label_lens[b])
        e, l, ok = bounds(Tb, Lb, lo[b], hi[b])
        if not ok:
            continue
        for u in range(Lb + 1):
            for t in range(max(int(e[u]), 0), min(int(l[u]), Tb - 1) + 1):
                m[b, t, u] = True
    return m


def windows(rng, act_lens, label_lens, U, pinned=(), unrestricted=(), max_slack=3, wide=True):
    """(emit_lo, emit_hi, frames), int32 (N, U - 1): per sample a non-decreasing alignment in [0, T_b - 1] and per label a
    random left and right slack in [0, max_slack]; about a quarter of the labels get no slack at all and about a sixth an
    unrestricted window (lo far below 0 and hi far past T_b; none with wide=False).  Samples listed in `pinned` have every label pinned (a single
    path), those in `unrestricted` no restriction.  The alignment itself is a path, so every sample is feasible.  Entries
    behind a sample's labels are -1 (never looked at)."""
    N = len(act_lens)
    lo = np.full((N, max(U - 1, 0)), -1, np.int32)
    hi = np.full((N, max(U - 1, 0)), -1, np.int32)
    frames = np.full((N, max(U - 1, 0)), -1, np.int32)
    for b in range(N):
        T, L = int(act_lens[b]), int(label_lens[b])
        a = np.sort(rng.integers(0, T, size=L))
        left, right = rng.integers(0, max_slack + 1, size=L), rng.integers(0, max_slack + 1, size=L)
        kind = rng.integers(0, 12, size=L)
        left[kind < 3], right[kind < 3] = 0, 0
        if wide:
            left[kind >= 10], right[kind >= 10] = WIDE, WIDE
        if b in pinned:
            left[:], right[:] = 0, 0
        if b in unrestricted:
            left[:], right[:] = WIDE, WIDE
        frames[b, :L], lo[b, :L], hi[b, :L] = a, a - left, a + right
    return lo, hi, frames


def _edges(x, lab, T, L, lo, hi, blank, keep_edges):
    """x (T, L + 1, A) -> lp_blank (T, L + 1), lp_label (T, L) of the sample's labels (None without labels) and the (T, L)
    bool mask of the label edges the windows allow."""
    lp = torch.log_softmax(x, -1)
    lpb = lp[..., blank]
    lpl, allow = None, None
    if L > 0:
        labs = torch.as_tensor(np.asarray(lab[:L], dtype=np.int64))
        lpl = lp[:, :L].gather(-1, labs.view(1, L, 1).expand(T, L, 1)).squeeze(-1)
        t = np.arange(T)[:, None]
        allow = (t >= np.asarray(lo[:L], np.int64)[None]) & (t <= np.asarray(hi[:L], np.int64)[None])
    if keep_edges is not None:
        lpb = lpb.clone()                              # (a leaf per edge type: a label on the blank column keeps its own)
        lpb.retain_grad()
        if lpl is not None:
            lpl = lpl.clone()
            lpl.retain_grad()
        keep_edges.append((lpb, lpl))
    return lpb, lpl, allow


def _sample(x, lab, T, L, lo, hi, blank, keep_edges=None):
    """-log P of one sample: x (T, L + 1, A) fp64 logits (a view of the leaf), lab (L,) labels, lo / hi (L,) windows.  The
    recursion runs over anti-diagonals d = t + u (both predecessors of a cell lie on diagonal d - 1), a vector over u each."""
    lpb, lpl, allow = _edges(x, lab, T, L, lo, hi, blank, keep_edges)
    neg = torch.full((L + 1,), NEG, dtype=x.dtype)
    if L > 0:
        lplm = torch.where(torch.as_tensor(allow), lpl, torch.full((), NEG, dtype=x.dtype))
    u = torch.arange(L + 1)
    alpha = neg.clone()
    alpha[0] = 0.0
    for d in range(1, T + L):
        t = d - u
        cell = (t >= 0) & (t < T)
        stay = torch.where(cell & (t >= 1), alpha + lpb[(t - 1).clamp(0, T - 1), u], neg)
        if L > 0:
            left = torch.cat((neg[:1], alpha[:L] + lplm[t[1:].clamp(0, T - 1), u[:L]]))
            stay = torch.logsumexp(torch.stack((stay, torch.where(cell & (u >= 1), left, neg))), 0)
        alpha = torch.where(cell, stay, neg)
    return -(alpha[L] + lpb[T - 1, L])


def _sample_brute(x, lab, T, L, lo, hi, blank, keep_edges=None):
    lpb, lpl, allow = _edges(x, lab, T, L, lo, hi, blank, keep_edges)
    scores = []

    def walk(t, u, acc):
        if t == T - 1 and u == L:
            scores.append(acc + lpb[t, u])
            return
        if t + 1 < T:
            walk(t + 1, u, acc + lpb[t, u])
        if u < L and allow[t, u]:
            walk(t, u + 1, acc + lpl[t, u])

    walk(0, 0, torch.zeros((), dtype=x.dtype))
    if not scores:
        return None
    return -torch.logsumexp(torch.stack(scores), 0)


def _run(fn, logits, labels, act_lens, label_lens, lo, hi, blank, weights, keep_edges=None):
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    N = x.shape[0]
    labels = np.asarray(labels).reshape(N, -1)
    lo, hi = np.asarray(lo).reshape(N, -1), np.asarray(hi).reshape(N, -1)
    costs = []
    for b in range(N):
        T, L = int(act_lens[b]), int(label_lens[b])
        costs.append(fn(x[b, :T, :L + 1], labels[b], T, L, lo[b], hi[b], blank, keep_edges))
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    live = [c * float(w[i]) for i, c in enumerate(costs) if c is not None and c.item() < 1e29]
    if live:
        sum(live).backward()
    out = np.array([np.inf if c is None or c.item() > 1e29 else c.item() for c in costs])
    g = x.grad.numpy().copy() if x.grad is not None else np.zeros(x.shape)
    return out, g


def ar_autograd(logits, labels, act_lens, label_lens, lo, hi, blank=0, weights=None):
    """costs (N,) and d(sum_b w_b cost_b)/d(logits) (N, T, U, A) in fp64.  A sample without a path costs +inf (its gradient
    is left at zero here: the library's is NaN).  Padding rows: zero."""
    return _run(_sample, logits, labels, act_lens, label_lens, lo, hi, blank, weights)


def ar_brute(logits, labels, act_lens, label_lens, lo, hi, blank=0, weights=None):
    """ar_autograd by enumeration of every path (tiny lattices)."""
    return _run(_sample_brute, logits, labels, act_lens, label_lens, lo, hi, blank, weights)


def paths_through(T, L, lo, hi):
    """By enumeration: (T, L + 1) bool, the nodes some path passes through (all False: no path)."""
    T, L = int(T), int(L)
    seen = np.zeros((T, L + 1), bool)

    def walk(t, u, trail):
        trail = trail + [(t, u)]
        if t == T - 1 and u == L:
            for p in trail:
                seen[p] = True
            return
        if t + 1 < T:
            walk(t + 1, u, trail)
        if u < L and int(lo[u]) <= t <= int(hi[u]):
            walk(t, u + 1, trail)

    walk(0, 0, [])
    return seen


def ar_formula(logits, labels, act_lens, label_lens, lo, hi, blank=0):
    """The gradient by the header's formula: column k gets (cb + cl) softmax_k - [k == blank] cb - [k == y_u] cl, with the
    edge posteriors taken from autograd (d cost / d lp of the edge, negated)."""
    edges = []
    _run(_sample, logits, labels, act_lens, label_lens, lo, hi, blank, None, edges)
    x = np.asarray(logits, dtype=np.float64)
    N = x.shape[0]
    labels = np.asarray(labels).reshape(N, -1)
    g = np.zeros_like(x)
    for b, (lpb, lpl) in enumerate(edges):
        T, L = int(act_lens[b]), int(label_lens[b])
        z = x[b, :T, :L + 1]
        p = np.exp(z - z.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        cb = np.zeros(z.shape[:2]) if lpb.grad is None else -lpb.grad.numpy()
        cl = np.zeros(z.shape[:2])
        if L > 0 and lpl.grad is not None:
            cl[:, :L] = -lpl.grad.numpy()
        out = (cb + cl)[..., None] * p
        out[..., int(blank)] -= cb
        for u in range(L):
            out[:, u, int(labels[b, u])] -= cl[:, u]
        g[b, :T, :L + 1] = out
    return g
