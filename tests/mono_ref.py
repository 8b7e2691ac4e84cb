"""Test infrastructure (no GPU) for the monotonic transducer loss (include/rnnt_mono.h).

  * mono_autograd: the loss written straight from the header's definition as an fp64 log-sum-exp recursion over frames,
    alpha(t + 1, u) = lse(alpha(t, u) + lp_blank(t, u), alpha(t, u - 1) + lp_label(t, u - 1)), differentiated by
    torch.autograd -- only the forward recursion is written down, as in tests/mblank_ref.py;
  * mono_brute: every one of the C(T_b, L_b) paths enumerated one by one (tiny lattices only), the same autograd;
  * mono_formula: the gradient by the header's closed formula from autograd's edge posteriors;
  * band_mask: the rows a path can pass through (u <= t, L_b - u <= T_b - t); in_lattice_mask: t < T_b, u <= L_b.
"""
import numpy as np
import torch

from tests.mblank_ref import NEG                      # "log zero": -inf would turn logsumexp's derivative into NaN
from tests.side_check import in_lattice_mask          # noqa: F401  (t < T_b, u <= L_b)


def band_mask(shape, act_lens, label_lens):
    """(N, T, U) bool: the in-lattice rows inside the band u <= t, L_b - u <= T_b - t."""
    N, T, U = shape[:3]
    m = np.zeros((N, T, U), bool)
    for b in range(N):
        Tb, Lb = int(act_lens[b]), int(label_lens[b])
        for t in range(Tb):
            for u in range(Lb + 1):
                m[b, t, u] = u <= t and Lb - u <= Tb - t
    return m


def _edges(x, lab, L, blank, keep_edges):
    """x (T, L + 1, A) -> lp_blank (T, L + 1) and lp_label (T, L) of the sample's labels (None without labels)."""
    T = x.shape[0]
    lp = torch.log_softmax(x, -1)
    lpb = lp[..., blank]
    lpl = None
    if L > 0:
        labs = torch.as_tensor(np.asarray(lab[:L], dtype=np.int64))
        lpl = lp[:, :L].gather(-1, labs.view(1, L, 1).expand(T, L, 1)).squeeze(-1)
    if keep_edges is not None:
        lpb = lpb.clone()                              # (a leaf per edge type: a label on the blank column keeps its own)
        lpb.retain_grad()
        if lpl is not None:
            lpl = lpl.clone()
            lpl.retain_grad()
        keep_edges.append((lpb, lpl))
    return lpb, lpl


def _sample(x, lab, T, L, blank, keep_edges=None):
    """-log P of one sample: x (T, L + 1, A) fp64 logits (a view of the leaf), lab (L,) labels."""
    lpb, lpl = _edges(x, lab, L, blank, keep_edges)
    alpha = torch.full((L + 1,), NEG, dtype=x.dtype)
    alpha[0] = 0.0
    for t in range(T):
        stay = alpha + lpb[t]
        if L > 0:
            move = torch.cat((torch.full((1,), NEG, dtype=x.dtype), alpha[:L] + lpl[t]))
            alpha = torch.logsumexp(torch.stack((stay, move)), 0)
        else:
            alpha = stay
    return -alpha[L]                                   # the terminal node (T_b, L_b)


def _sample_brute(x, lab, T, L, blank, keep_edges=None):
    lpb, lpl = _edges(x, lab, L, blank, keep_edges)
    scores = []

    def walk(t, u, acc):
        if t == T:
            if u == L:
                scores.append(acc)
            return
        walk(t + 1, u, acc + lpb[t, u])
        if u < L:
            walk(t + 1, u + 1, acc + lpl[t, u])

    walk(0, 0, torch.zeros((), dtype=x.dtype))
    if not scores:
        return None
    return -torch.logsumexp(torch.stack(scores), 0)


def _run(fn, logits, labels, act_lens, label_lens, blank, weights, keep_edges=None):
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    N = x.shape[0]
    labels = np.asarray(labels).reshape(N, -1)
    costs = []
    for b in range(N):
        T, L = int(act_lens[b]), int(label_lens[b])
        costs.append(fn(x[b, :T, :L + 1], labels[b], T, L, blank, keep_edges))
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    live = [c * float(w[i]) for i, c in enumerate(costs) if c is not None and c.item() < 1e29]
    if live:
        sum(live).backward()
    out = np.array([np.inf if c is None or c.item() > 1e29 else c.item() for c in costs])
    g = x.grad.numpy().copy() if x.grad is not None else np.zeros(x.shape)
    return out, g


def mono_autograd(logits, labels, act_lens, label_lens, blank=0, weights=None):
    """costs (N,) and d(sum_b w_b cost_b)/d(logits) (N, T, U, A) in fp64.  A sample without a path (T_b < L_b) costs +inf
    (its gradient is left at zero here: the library's is NaN).  Padding rows: zero."""
    return _run(_sample, logits, labels, act_lens, label_lens, blank, weights)


def mono_brute(logits, labels, act_lens, label_lens, blank=0, weights=None):
    """mono_autograd by enumeration of every path (tiny lattices)."""
    return _run(_sample_brute, logits, labels, act_lens, label_lens, blank, weights)


def mono_formula(logits, labels, act_lens, label_lens, blank=0):
    """The gradient by the header's formula: column k gets (cb + cl) softmax_k - [k == blank] cb - [k == y_u] cl, with the
    edge posteriors taken from autograd (d cost / d lp of the edge, negated)."""
    edges = []
    _run(_sample, logits, labels, act_lens, label_lens, blank, None, edges)
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
