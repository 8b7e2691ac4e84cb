"""Test infrastructure (no GPU) for the Hybrid Autoregressive Transducer loss (include/rnnt_hat.h).

  * hat_autograd: the loss written straight from the header's definition -- log b = logsigmoid(z_blank), label log-probs
    logsigmoid(-z_blank) + log_softmax over the non-blank columns -- as an fp64 log-sum-exp recursion over frames,
    differentiated by torch.autograd: only the forward recursion is written down, as in tests/tdt_ref.py.
    `plain=True` leaves the blank column inside one softmax over all A columns: the ordinary RNN-T loss, the negative
    control of tests/test_gpu_hat.py;
  * hat_brute: every path from (0, 0) through the terminal blank enumerated one by one (tiny lattices only);
  * hat_formula: the gradient by the header's closed formula from autograd's edge posteriors;
  * in_lattice_mask: the rows the loss reads (t < T_b, u <= L_b).
"""
import numpy as np
import torch

from tests.side_check import in_lattice_mask          # noqa: F401  (the rows the loss reads: t < T_b, u <= L_b)

F = torch.nn.functional
NEG = -1.0e30          # "log zero": -inf would turn logsumexp's derivative into NaN on nodes no path reaches


def edge_log_probs(x, lab, L, blank, plain=False):
    """x (T, L + 1, A) -> lp_blank (T, L + 1), lp_label (T, L) of the sample's labels."""
    T, U, A = x.shape
    if plain:
        lp = torch.log_softmax(x, -1)
        lpb = lp[..., blank]
    else:
        keep = [k for k in range(A) if k != blank]
        zb = x[..., blank]
        lpb = F.logsigmoid(zb)
        lp = torch.full_like(x, NEG)
        lp = lp.index_copy(-1, torch.tensor(keep), F.logsigmoid(-zb).unsqueeze(-1) + torch.log_softmax(x[..., keep], -1))
    lpl = None
    if L > 0:
        labs = torch.as_tensor(np.asarray(lab[:L], dtype=np.int64))
        lpl = lp[:, :L].gather(-1, labs.view(1, L, 1).expand(T, L, 1)).squeeze(-1)
    return lpb, lpl


def _sample(x, lab, T, L, blank, plain=False, keep_edges=None):
    lpb, lpl = edge_log_probs(x, lab, L, blank, plain)
    if keep_edges is not None:
        lpb.retain_grad()
        if lpl is not None:
            lpl.retain_grad()
        keep_edges.append((lpb, lpl))
    alpha = None
    for t in range(T):
        # inc(u): what arrives from frame t - 1 by a blank; then the labels inside the frame, a prefix scan over u
        if t == 0:
            inc = torch.full((L + 1,), NEG, dtype=x.dtype)
            inc[0] = 0.0
        else:
            inc = alpha + lpb[t - 1]
        if L > 0:
            S = torch.cat((torch.zeros(1, dtype=x.dtype), torch.cumsum(lpl[t], 0)))
            inc = S + torch.logcumsumexp(inc - S, 0)
        alpha = inc
    return -(alpha[L] + lpb[T - 1, L])


def _sample_brute(x, lab, T, L, blank, plain=False, keep_edges=None):
    lpb, lpl = edge_log_probs(x, lab, L, blank, plain)
    scores = []

    def walk(t, u, acc):
        if t == T - 1 and u == L:
            scores.append(acc + lpb[t, u])
            return
        if t + 1 < T:
            walk(t + 1, u, acc + lpb[t, u])
        if u < L:
            walk(t, u + 1, acc + lpl[t, u])

    walk(0, 0, torch.zeros((), dtype=x.dtype))
    return -torch.logsumexp(torch.stack(scores), 0)


def _run(fn, logits, labels, act_lens, label_lens, blank, weights, plain=False, keep_edges=None):
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    N = x.shape[0]
    labels = np.asarray(labels).reshape(N, -1)
    costs = []
    for b in range(N):
        T, L = int(act_lens[b]), int(label_lens[b])
        costs.append(fn(x[b, :T, :L + 1], labels[b], T, L, blank, plain, keep_edges))
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    sum(c * float(w[i]) for i, c in enumerate(costs)).backward()
    return np.array([c.item() for c in costs]), x.grad.numpy().copy()


def hat_autograd(logits, labels, act_lens, label_lens, blank=0, weights=None, plain=False):
    """costs (N,) and d(sum_b w_b cost_b)/d(logits) (N, T, U, A) in fp64.  Padding rows: zero."""
    return _run(_sample, logits, labels, act_lens, label_lens, blank, weights, plain)


def hat_brute(logits, labels, act_lens, label_lens, blank=0, weights=None):
    """hat_autograd by enumeration of every path (tiny lattices)."""
    return _run(_sample_brute, logits, labels, act_lens, label_lens, blank, weights)


def hat_formula(logits, labels, act_lens, label_lens, blank=0):
    """The gradient by the header's formula: blank column c b - cb, column k != blank cl q_k - cl [k == y_u], with the edge
    posteriors cb, cl taken from autograd (d cost / d lp of the edge, negated)."""
    edges = []
    _run(_sample, logits, labels, act_lens, label_lens, blank, None, False, edges)
    x = np.asarray(logits, dtype=np.float64)
    N, _, _, A = x.shape
    labels = np.asarray(labels).reshape(N, -1)
    keep = [k for k in range(A) if k != blank]
    g = np.zeros_like(x)
    for b, (lpb, lpl) in enumerate(edges):
        T, L = int(act_lens[b]), int(label_lens[b])
        cb = -lpb.grad.numpy()
        cl = np.zeros_like(cb)
        if L > 0:
            cl[:, :L] = -lpl.grad.numpy()
        z = x[b, :T, :L + 1]
        bsig = 1.0 / (1.0 + np.exp(-z[..., blank]))
        zl = z[..., keep]
        q = np.exp(zl - zl.max(-1, keepdims=True))
        q /= q.sum(-1, keepdims=True)
        out = np.zeros_like(z)
        out[..., keep] = cl[..., None] * q
        for u in range(L):
            out[:, u, int(labels[b, u])] -= cl[:, u]
        out[..., blank] = (cb + cl) * bsig - cb
        g[b, :T, :L + 1] = out
    return g
