"""Test infrastructure (no GPU) for the multi-blank transducer loss (include/rnnt_mblank.h).

  * mblank_autograd: the loss written straight from the header's definition as an fp64 log-sum-exp recursion over frames,
    differentiated by torch.autograd -- only the forward recursion is written down, as in tests/tdt_ref.py.  The label
    edges stay inside a frame; they are a log-semiring prefix scan over u (logcumsumexp);
  * mblank_brute: every path from (0, 0) to the terminal node enumerated one by one (tiny lattices only), the same autograd;
  * mblank_formula: the gradient by the header's closed formula from autograd's edge posteriors;
  * in_lattice_mask: the rows the loss reads (t < T_b, u <= L_b).

Big blanks are given as `columns` and `durations` (two sequences of length K); K = 0 is the plain RNN-T loss.
"""
import numpy as np
import torch

from tests.side_check import in_lattice_mask          # noqa: F401  (the rows the loss reads: t < T_b, u <= L_b)

NEG = -1.0e30          # "log zero": -inf would turn logsumexp's derivative into NaN on nodes no path reaches


def _lse(terms):
    return torch.logsumexp(torch.stack(terms), 0)


def edge_log_probs(x, lab, L, columns, blank, sigma):
    """x (T, L + 1, A) -> [lp of the blank edges of duration d: (d, (T, L + 1))], standard blank first, and lp_label (T, L)
    of the sample's labels (None without labels)."""
    T = x.shape[0]
    lp = torch.log_softmax(x, -1) - sigma
    blanks = [lp[..., blank]] + [lp[..., int(c)] for c in columns]
    lpl = None
    if L > 0:
        labs = torch.as_tensor(np.asarray(lab[:L], dtype=np.int64))
        lpl = lp[:, :L].gather(-1, labs.view(1, L, 1).expand(T, L, 1)).squeeze(-1)
    return blanks, lpl


def _edges(x, lab, L, columns, blank, sigma, keep_edges):
    blanks, lpl = edge_log_probs(x, lab, L, columns, blank, sigma)
    if keep_edges is not None:
        blanks = [b.clone() for b in blanks]           # (a leaf per edge type: a column shared with a label keeps its own)
        for b in blanks:
            b.retain_grad()
        if lpl is not None:
            lpl = lpl.clone()
            lpl.retain_grad()
        keep_edges.append((blanks, lpl))
    return blanks, lpl


def _sample(x, lab, T, L, columns, durations, blank, sigma, keep_edges=None):
    """-log P of one sample: x (T, L + 1, A) fp64 logits (a view of the leaf), lab (L,) labels.  None without a path."""
    blanks, lpl = _edges(x, lab, L, columns, blank, sigma, keep_edges)
    durs = (1,) + tuple(durations)
    alpha = []
    for t in range(T):
        terms = []
        if t == 0:
            init = torch.full((L + 1,), NEG, dtype=x.dtype)
            init[0] = 0.0
            terms.append(init)
        for lpb, d in zip(blanks, durs):
            if t - d >= 0:
                terms.append(alpha[t - d] + lpb[t - d])                         # blank (t - d, u) -> (t, u)
        inc = _lse(terms) if len(terms) > 1 else terms[0]
        if L > 0:
            # alpha(t, u) = logsumexp(inc(u), alpha(t, u - 1) + lp_label(t, u - 1)): a prefix scan over u
            S = torch.cat((torch.zeros(1, dtype=x.dtype), torch.cumsum(lpl[t], 0)))
            inc = S + torch.logcumsumexp(inc - S, 0)
        alpha.append(inc)
    final = [alpha[T - d][L] + lpb[T - d, L] for lpb, d in zip(blanks, durs) if T - d >= 0]
    return -_lse(final)


def _sample_brute(x, lab, T, L, columns, durations, blank, sigma, keep_edges=None):
    blanks, lpl = _edges(x, lab, L, columns, blank, sigma, keep_edges)
    durs = (1,) + tuple(durations)
    scores = []

    def walk(t, u, acc):
        for lpb, d in zip(blanks, durs):
            if t + d < T:
                walk(t + d, u, acc + lpb[t, u])
            elif t + d == T and u == L:
                scores.append(acc + lpb[t, u])
        if u < L:
            walk(t, u + 1, acc + lpl[t, u])

    walk(0, 0, torch.zeros((), dtype=x.dtype))
    if not scores:
        return None
    return -_lse(scores)


def _run(fn, logits, labels, act_lens, label_lens, columns, durations, blank, sigma, weights, keep_edges=None):
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    N = x.shape[0]
    labels = np.asarray(labels).reshape(N, -1)
    columns, durations = tuple(int(c) for c in columns), tuple(int(d) for d in durations)
    assert len(columns) == len(durations)
    costs = []
    for b in range(N):
        T, L = int(act_lens[b]), int(label_lens[b])
        costs.append(fn(x[b, :T, :L + 1], labels[b], T, L, columns, durations, blank, sigma, keep_edges))
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    live = [c * float(w[i]) for i, c in enumerate(costs) if c is not None and c.item() < 1e29]
    if live:
        sum(live).backward()
    out = np.array([np.inf if c is None or c.item() > 1e29 else c.item() for c in costs])
    g = x.grad.numpy().copy() if x.grad is not None else np.zeros(x.shape)
    return out, g


def mblank_autograd(logits, labels, act_lens, label_lens, columns, durations, blank=0, sigma=0.0, weights=None):
    """costs (N,) and d(sum_b w_b cost_b)/d(logits) (N, T, U, A) in fp64.  A sample without a path costs +inf (its gradient
    is left at zero here: the library's is NaN).  Padding rows: zero."""
    return _run(_sample, logits, labels, act_lens, label_lens, columns, durations, blank, sigma, weights)


def mblank_brute(logits, labels, act_lens, label_lens, columns, durations, blank=0, sigma=0.0, weights=None):
    """mblank_autograd by enumeration of every path (tiny lattices)."""
    return _run(_sample_brute, logits, labels, act_lens, label_lens, columns, durations, blank, sigma, weights)


def mblank_formula(logits, labels, act_lens, label_lens, columns, durations, blank=0, sigma=0.0):
    """The gradient by the header's formula: column k gets c softmax_k - the posteriors of the row's out-edges that use
    column k, with the edge posteriors taken from autograd (d cost / d lp of the edge, negated)."""
    edges = []
    _run(_sample, logits, labels, act_lens, label_lens, columns, durations, blank, sigma, None, edges)
    x = np.asarray(logits, dtype=np.float64)
    N = x.shape[0]
    labels = np.asarray(labels).reshape(N, -1)
    cols = (int(blank),) + tuple(int(c) for c in columns)
    g = np.zeros_like(x)
    for b, (blanks, lpl) in enumerate(edges):
        T, L = int(act_lens[b]), int(label_lens[b])
        z = x[b, :T, :L + 1]
        p = np.exp(z - z.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        gam = [np.zeros(z.shape[:2]) if e.grad is None else -e.grad.numpy() for e in blanks]
        cl = np.zeros(z.shape[:2])
        if L > 0 and lpl.grad is not None:
            cl[:, :L] = -lpl.grad.numpy()
        c = sum(gam) + cl
        out = c[..., None] * p
        for col, ge in zip(cols, gam):
            out[..., col] -= ge
        for u in range(L):
            out[:, u, int(labels[b, u])] -= cl[:, u]
        g[b, :T, :L + 1] = out
    return g
