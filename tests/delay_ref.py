"""Test infrastructure (no GPU) for the delay-penalized RNN-T loss and the expected emission frames (include/rnnt_delay.h).

  * delay_autograd: the loss written straight from the header's definition as an fp64 log-sum-exp recursion over the standard
    lattice, alpha(t, u) = lse(alpha(t - 1, u) + lp_blank(t - 1, u), alpha(t, u - 1) + lp_label(t, u - 1)) with
    lp_label(t, u) = log_softmax[y_u] + delay_penalty * ((T_b - 1) / 2 - t), differentiated by torch.autograd -- only the
    forward recursion is written down, as in tests/ar_ref.py;
  * delay_brute: every path enumerated one by one (tiny lattices only), the same autograd;
  * emit_frames_ref: sum_t t * cl(t, u) with cl the label edge's posterior, taken from autograd (-d cost / d lp_label);
    delay_all: costs, gradients and emit_frames of one pass;
  * emit_frames_brute: the same expectation from the enumerated paths' weights, with no autograd in it;
  * f32_penalty: the value a penalty has behind the C-ABI's float.
"""
import numpy as np
import torch

from tests.mblank_ref import NEG                      # "log zero": -inf would turn logsumexp's derivative into NaN
from tests.side_check import in_lattice_mask          # noqa: F401  (t < T_b, u <= L_b)


def f32_penalty(p):
    """The penalty the library sees: the C entries take a float."""
    return float(np.float32(p))


def _edges(x, lab, T, L, blank, penalty, keep_edges):
    """x (T, L + 1, A) -> lp_blank (T, L + 1) and the biased lp_label (T, L) of the sample's labels (None without labels)."""
    lp = torch.log_softmax(x, -1)
    lpb = lp[..., blank]
    lpl = None
    if L > 0:
        labs = torch.as_tensor(np.asarray(lab[:L], dtype=np.int64))
        lpl = lp[:, :L].gather(-1, labs.view(1, L, 1).expand(T, L, 1)).squeeze(-1)
        bias = float(penalty) * (0.5 * (T - 1) - torch.arange(T, dtype=x.dtype))
        lpl = lpl + bias[:, None]
    if keep_edges is not None:
        lpb = lpb.clone()                              # (a leaf per edge type: a label on the blank column keeps its own)
        lpb.retain_grad()
        if lpl is not None:
            lpl = lpl.clone()
            lpl.retain_grad()
        keep_edges.append((lpb, lpl))
    return lpb, lpl


def _sample(x, lab, T, L, blank, penalty, keep_edges=None):
    """-log of the sample's path sum: x (T, L + 1, A) fp64 logits (a view of the leaf), lab (L,) labels.  The recursion runs
    over anti-diagonals d = t + u (both predecessors of a cell lie on diagonal d - 1), a vector over u each."""
    lpb, lpl = _edges(x, lab, T, L, blank, penalty, keep_edges)
    neg = torch.full((L + 1,), NEG, dtype=x.dtype)
    u = torch.arange(L + 1)
    alpha = neg.clone()
    alpha[0] = 0.0
    for d in range(1, T + L):
        t = d - u
        cell = (t >= 0) & (t < T)
        stay = torch.where(cell & (t >= 1), alpha + lpb[(t - 1).clamp(0, T - 1), u], neg)
        if L > 0:
            left = torch.cat((neg[:1], alpha[:L] + lpl[t[1:].clamp(0, T - 1), u[:L]]))
            stay = torch.logsumexp(torch.stack((stay, torch.where(cell & (u >= 1), left, neg))), 0)
        alpha = torch.where(cell, stay, neg)
    return -(alpha[L] + lpb[T - 1, L])


def _paths(lpb, lpl, T, L):
    """[(score, emission frames)] of every path."""
    out = []

    def walk(t, u, acc, frames):
        if t == T - 1 and u == L:
            out.append((acc + lpb[t, u], frames))
            return
        if t + 1 < T:
            walk(t + 1, u, acc + lpb[t, u], frames)
        if u < L:
            walk(t, u + 1, acc + lpl[t, u], frames + [t])

    walk(0, 0, torch.zeros((), dtype=lpb.dtype), [])
    return out


def _sample_brute(x, lab, T, L, blank, penalty, keep_edges=None):
    lpb, lpl = _edges(x, lab, T, L, blank, penalty, keep_edges)
    return -torch.logsumexp(torch.stack([s for s, _ in _paths(lpb, lpl, T, L)]), 0)


def _run(fn, logits, labels, act_lens, label_lens, blank, penalty, weights, keep_edges=None):
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    N = x.shape[0]
    labels = np.asarray(labels).reshape(N, -1)
    costs = []
    for b in range(N):
        T, L = int(act_lens[b]), int(label_lens[b])
        costs.append(fn(x[b, :T, :L + 1], labels[b], T, L, blank, penalty, keep_edges))
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    live = [c * float(w[i]) for i, c in enumerate(costs) if c.item() < 1e29]
    if live:
        sum(live).backward()
    out = np.array([np.inf if c.item() > 1e29 else c.item() for c in costs])
    g = x.grad.numpy().copy() if x.grad is not None else np.zeros(x.shape)
    return out, g


def delay_autograd(logits, labels, act_lens, label_lens, blank=0, delay_penalty=0.0, weights=None):
    """costs (N,) and d(sum_b w_b cost_b)/d(logits) (N, T, U, A) in fp64.  A sample without a path of positive probability
    costs +inf (its gradient is left at zero here: the library's is NaN).  Padding rows: zero."""
    return _run(_sample, logits, labels, act_lens, label_lens, blank, delay_penalty, weights)


def delay_brute(logits, labels, act_lens, label_lens, blank=0, delay_penalty=0.0, weights=None):
    """delay_autograd by enumeration of every path (tiny lattices)."""
    return _run(_sample_brute, logits, labels, act_lens, label_lens, blank, delay_penalty, weights)


def delay_all(logits, labels, act_lens, label_lens, blank=0, delay_penalty=0.0):
    """(costs, gradients, emit_frames) of one pass of delay_autograd: emit_frames (N, U - 1) fp64 = sum_t t * cl(t, u) for
    u < L_b, 0 behind a sample's labels; cl = the label edge's posterior under the tilted distribution
    = -d cost_b / d lp_label(t, u)."""
    edges = []
    c, g = _run(_sample, logits, labels, act_lens, label_lens, blank, delay_penalty, None, edges)
    N, U = np.asarray(logits).shape[0], np.asarray(logits).shape[2]
    out = np.zeros((N, U - 1))
    for b, (_, lpl) in enumerate(edges):
        T, L = int(act_lens[b]), int(label_lens[b])
        if L > 0 and lpl.grad is not None:
            out[b, :L] = (np.arange(T)[:, None] * -lpl.grad.numpy()).sum(0)
    return c, g, out


def emit_frames_ref(logits, labels, act_lens, label_lens, blank=0, delay_penalty=0.0):
    """The emit_frames of delay_all."""
    return delay_all(logits, labels, act_lens, label_lens, blank, delay_penalty)[2]


def emit_frames_brute(logits, labels, act_lens, label_lens, blank=0, delay_penalty=0.0):
    """The same expectation from the enumerated paths: sum_paths w(path) t_u(path) / sum_paths w(path)."""
    x = torch.tensor(np.asarray(logits, dtype=np.float64))
    N, U = x.shape[0], x.shape[2]
    labels = np.asarray(labels).reshape(N, -1)
    out = np.zeros((N, U - 1))
    for b in range(N):
        T, L = int(act_lens[b]), int(label_lens[b])
        lpb, lpl = _edges(x[b, :T, :L + 1], labels[b], T, L, blank, delay_penalty, None)
        paths = _paths(lpb, lpl, T, L)
        w = torch.softmax(torch.stack([s for s, _ in paths]), 0).numpy()
        for wi, (_, frames) in zip(w, paths):
            out[b, :L] += wi * np.asarray(frames, dtype=np.float64)
    return out
