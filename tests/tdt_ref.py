"""Test infrastructure (no GPU) for the Token-and-Duration Transducer loss (include/rnnt_tdt.h).

  * tdt_autograd: the loss written straight from the header's definition as an fp64 log-sum-exp recursion over frames,
    differentiated by torch.autograd -- only the forward recursion is written down, as in tests/autograd_ref.py.  The label
    edges of duration 0 stay inside a frame; they are a log-semiring prefix scan over u (logcumsumexp);
  * tdt_brute: every path from (0, 0) to the terminal node enumerated one by one (tiny lattices only), the same autograd;
  * in_lattice_mask: the rows the loss reads (t < T_b, u <= L_b).
"""
import numpy as np
import torch

from tests.side_check import in_lattice_mask          # noqa: F401  (the rows the loss reads: t < T_b, u <= L_b)

NEG = -1.0e30          # "log zero": -inf would turn logsumexp's derivative into NaN on nodes no path reaches


def _log_probs(x, A, blank, sigma):
    tok = torch.log_softmax(x[..., :A], -1) - sigma
    dur = torch.log_softmax(x[..., A:], -1)
    return tok, dur


def _lse(terms):
    return torch.logsumexp(torch.stack(terms), 0)


def _sample(x, lab, T, L, A, durations, blank, sigma):
    """-log P of one sample: x (T, L + 1, A + D) fp64 logits (a view of the leaf), lab (L,) labels."""
    tok, dur = _log_probs(x, A, blank, sigma)
    U = L + 1
    lb = tok[..., blank]                                                          # (T, U)
    labs = torch.as_tensor(np.asarray(lab[:L], dtype=np.int64))
    if L > 0:
        ll = tok[:, :L].gather(-1, labs.view(1, L, 1).expand(T, L, 1)).squeeze(-1)   # (T, L)
    zero = None
    if 0 in durations:
        zero = list(durations).index(0)
    alpha = []
    for t in range(T):
        terms = []
        if t == 0:
            init = torch.full((U,), NEG, dtype=x.dtype)
            init[0] = 0.0
            terms.append(init)
        for j, d in enumerate(durations):
            ts = t - d
            if d == 0 or ts < 0:
                continue
            terms.append(alpha[ts] + lb[ts] + dur[ts, :, j])                    # blank (ts, u) -> (t, u)
            if L > 0:
                lab_in = alpha[ts][:L] + ll[ts] + dur[ts, :L, j]                 # label (ts, u - 1) -> (t, u)
                terms.append(torch.cat((torch.full((1,), NEG, dtype=x.dtype), lab_in)))
        if not terms:                                                             # (no edge reaches frame t)
            inc = torch.full((U,), NEG, dtype=x.dtype)
        else:
            inc = _lse(terms) if len(terms) > 1 else terms[0]
        if zero is not None and L > 0:
            # alpha(t, u) = logsumexp(inc(u), alpha(t, u - 1) + c(u - 1)), c = label + duration 0 of the same frame
            c = ll[t] + dur[t, :L, zero]
            S = torch.cat((torch.zeros(1, dtype=x.dtype), torch.cumsum(c, 0)))
            inc = S + torch.logcumsumexp(inc - S, 0)
        alpha.append(inc)
    final = [alpha[T - d][L] + lb[T - d, L] + dur[T - d, L, j] for j, d in enumerate(durations) if d > 0 and T - d >= 0]
    if not final:
        return None
    return -_lse(final)


def _run(fn, logits, labels, act_lens, label_lens, durations, blank, sigma, weights):
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    N = x.shape[0]
    A = x.shape[3] - len(durations)
    labels = np.asarray(labels).reshape(N, -1)
    costs = []
    for b in range(N):
        T, L = int(act_lens[b]), int(label_lens[b])
        c = fn(x[b, :T, :L + 1], labels[b], T, L, A, tuple(int(d) for d in durations), blank, sigma)
        costs.append(c)
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    live = [c * float(w[i]) for i, c in enumerate(costs) if c is not None and c.item() < 1e29]
    if live:
        sum(live).backward()
    out = np.array([np.inf if c is None or c.item() > 1e29 else c.item() for c in costs])
    g = x.grad.numpy().copy() if x.grad is not None else np.zeros(x.shape)
    return out, g


def tdt_autograd(logits, labels, act_lens, label_lens, durations, blank=0, sigma=0.0, weights=None):
    """costs (N,) and d(sum_b w_b cost_b)/d(logits) (N, T, U, A + D) in fp64.  A sample without a path costs +inf (its
    gradient is left at zero here: the library's is NaN).  Padding rows: zero."""
    return _run(_sample, logits, labels, act_lens, label_lens, durations, blank, sigma, weights)


def _sample_brute(x, lab, T, L, A, durations, blank, sigma):
    tok, dur = _log_probs(x, A, blank, sigma)
    scores = []

    def walk(t, u, acc):
        for j, d in enumerate(durations):
            if d > 0 and (t + d < T or (t + d == T and u == L)):
                s = acc + tok[t, u, blank] + dur[t, u, j]
                if t + d == T:
                    scores.append(s)
                else:
                    walk(t + d, u, s)
            if u < L and t + d < T:
                walk(t + d, u + 1, acc + tok[t, u, int(lab[u])] + dur[t, u, j])

    walk(0, 0, torch.zeros((), dtype=x.dtype))
    if not scores:
        return None
    return -_lse(scores)


def tdt_brute(logits, labels, act_lens, label_lens, durations, blank=0, sigma=0.0, weights=None):
    """tdt_autograd by enumeration of every path (tiny lattices)."""
    return _run(_sample_brute, logits, labels, act_lens, label_lens, durations, blank, sigma, weights)
