"""Test infrastructure (no GPU) for the pruned RNN-T loss with k2's lattice types and delay_penalty (include/rnnt_pstream.h).

  * pstream_autograd: the loss written straight from the header's definition as an explicit fp64 log-sum-exp lattice over the
    windows, for both types, with the bias delay_penalty * ((T_b - 1) / 2 - t) added literally to the label edges (no gauge),
    differentiated by torch.autograd -- only the forward recursion is written down, as in tests/pruned_ref.py;
  * pstream_brute: every path enumerated one by one (tiny lattices only), the same autograd;
  * has_path: brute-force reachability of the terminal node through the windows, per type;
  * windows: window starts drawn AROUND a valid path, so that every sample has one; max_labels: the longest transcript a
    sample of T_b frames can have with windows of S states;
  * in_lattice_mask / read_mask: rows t < T_b, s_t + k <= L_b, and of those the rows the library reads (type 1: the band);
  * k2_px_py: px / py as k2's get_rnnt_logprobs_pruned is documented to build them, for the mapping test.
"""
import numpy as np
import torch

from tests.pruned_ref import NEG                     # "log zero": -inf would turn logaddexp's derivative into NaN

REGULAR, MODIFIED = 0, 1


def f32_penalty(p):
    """The penalty the library sees: the C entries take a float."""
    return float(np.float32(p))


def _edges(x, s, lab, T, L, blank, penalty):
    """x (T, S, A) -> pb, pl (T, L + 1): the blank and the biased label edge of every node, NEG where the node lies outside
    its frame's window (and pl at u = L)."""
    S, U = x.shape[1], L + 1
    lp = torch.log_softmax(x, -1)
    s = np.asarray(s[:T], dtype=np.int64)
    t_i, k_i = np.meshgrid(np.arange(T), np.arange(S), indexing="ij")
    u_i = s[:, None] + k_i
    inside = (u_i >= 0) & (u_i <= L)
    tt, kk, uu = (torch.as_tensor(a[inside]) for a in (t_i, k_i, u_i))
    pb = torch.full((T, U), NEG, dtype=x.dtype).index_put((tt, uu), lp[tt, kk, blank])
    pl = torch.full((T, U), NEG, dtype=x.dtype)
    has = uu < L
    if bool(has.any()):
        tl, kl, ul = tt[has], kk[has], uu[has]
        labs = torch.as_tensor(np.asarray(lab[:L], dtype=np.int64))
        bias = float(penalty) * (0.5 * (T - 1) - tl.to(x.dtype))
        pl = pl.index_put((tl, ul), lp[tl, kl, labs[ul]] + bias)
    return pb, pl


def _sample(x, s, lab, T, L, blank, penalty, rnnt_type):
    """-log of the sample's path sum: x (T, S, A) fp64 logits (a view of the leaf), s (T,) window starts, lab (L,) labels."""
    pb, pl = _edges(x, s, lab, T, L, blank, penalty)
    neg = torch.full((L + 1,), NEG, dtype=x.dtype)
    alpha = neg.clone()
    alpha[0] = 0.0
    if rnnt_type == MODIFIED:
        # over frames: alpha(t + 1, u) = lse(alpha(t, u) + pb(t, u), alpha(t, u - 1) + pl(t, u - 1)); the terminal node is
        # (T, L), and only it is taken of row T
        for t in range(T):
            stay = alpha + pb[t]
            diag = torch.cat((neg[:1], (alpha + pl[t])[:L]))
            alpha = torch.logaddexp(stay, diag)
        return -alpha[L]
    # over anti-diagonals d = t + u, a vector over u each (tests/delay_ref.py)
    u = torch.arange(L + 1)
    for d in range(1, T + L):
        t = d - u
        cell = (t >= 0) & (t < T)
        stay = torch.where(cell & (t >= 1), alpha + pb[(t - 1).clamp(0, T - 1), u], neg)
        if L > 0:
            left = torch.cat((neg[:1], alpha[:L] + pl[t[1:].clamp(0, T - 1), u[:L]]))
            stay = torch.logaddexp(stay, torch.where(cell & (u >= 1), left, neg))
        alpha = torch.where(cell, stay, neg)
    return -(alpha[L] + pb[T - 1, L])


def _sample_brute(x, s, lab, T, L, blank, penalty, rnnt_type):
    pb, pl = _edges(x, s, lab, T, L, blank, penalty)
    scores = []

    def walk(t, u, acc):
        if rnnt_type == MODIFIED:
            if t == T:
                if u == L:
                    scores.append(acc)
                return
            walk(t + 1, u, acc + pb[t, u])
            if u < L:
                walk(t + 1, u + 1, acc + pl[t, u])
        else:
            if t == T - 1 and u == L:
                scores.append(acc + pb[t, u])
                return
            if t + 1 < T:
                walk(t + 1, u, acc + pb[t, u])
            if u < L:
                walk(t, u + 1, acc + pl[t, u])

    walk(0, 0, torch.zeros((), dtype=x.dtype))
    if not scores:
        return torch.tensor(-2 * NEG, dtype=x.dtype)
    return -torch.logsumexp(torch.stack(scores), 0)


def _run(fn, logits, labels, ranges, act_lens, label_lens, blank, rnnt_type, penalty, weights):
    assert rnnt_type in (REGULAR, MODIFIED)
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    N = x.shape[0]
    labels = np.asarray(labels).reshape(N, -1)
    costs = []
    for b in range(N):
        T, L = int(act_lens[b]), int(label_lens[b])
        costs.append(fn(x[b, :T], np.asarray(ranges[b]), labels[b], T, L, blank, penalty, rnnt_type))
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    live = [c * float(w[i]) for i, c in enumerate(costs) if c.item() < 1e29 and c.requires_grad]
    if live:
        sum(live).backward()
    out = np.array([np.inf if c.item() > 1e29 else c.item() for c in costs])
    g = x.grad.numpy().copy() if x.grad is not None else np.zeros(x.shape)
    return out, g


def pstream_autograd(logits, labels, ranges, act_lens, label_lens, blank=0, rnnt_type=REGULAR, delay_penalty=0.0,
                     weights=None):
    """costs (N,) and d(sum_b w_b cost_b)/d(logits) (N, T, S, A) in fp64.  A sample without a path costs +inf (its gradient is
    left at zero here: the library's is NaN).  Rows never read: zero."""
    return _run(_sample, logits, labels, ranges, act_lens, label_lens, blank, rnnt_type, delay_penalty, weights)


def pstream_brute(logits, labels, ranges, act_lens, label_lens, blank=0, rnnt_type=REGULAR, delay_penalty=0.0, weights=None):
    """pstream_autograd by enumeration of every path (tiny lattices)."""
    return _run(_sample_brute, logits, labels, ranges, act_lens, label_lens, blank, rnnt_type, delay_penalty, weights)


# ----------------------------------------------------------------------------- windows
def has_path(s, T, L, S, rnnt_type):
    """Does a path from (0, 0) to the terminal node exist whose every node has its out-edge inside its frame's window?"""
    inside = lambda t, u: int(s[t]) <= u < int(s[t]) + S and u <= L                              # noqa: E731
    if rnnt_type == MODIFIED:
        reach = np.zeros((T + 1, L + 2), bool)
        reach[0, 0] = True
        for t in range(T):
            for u in range(L + 1):
                if reach[t, u] and inside(t, u):
                    reach[t + 1, u] = True
                    if u < L:
                        reach[t + 1, u + 1] = True
        return bool(reach[T, L])
    reach = np.zeros((T, L + 1), bool)
    reach[0, 0] = True
    for t in range(T):
        for u in range(L + 1):
            if not reach[t, u] or not inside(t, u):
                continue
            if u < L:
                reach[t, u + 1] = True
            if t + 1 < T:
                reach[t + 1, u] = True
    return bool(reach[T - 1, L] and inside(T - 1, L))


def max_labels(T, S, rnnt_type):
    """The longest transcript with a path through windows of S states over T frames: a regular frame holds at most S - 1
    label edges (their S nodes fill its window), a modified one a single label edge."""
    return T if rnnt_type == MODIFIED else T * (S - 1)


def windows(rng, T, L, S, rnnt_type, maxT, burst=False):
    """Window starts (maxT,) int32 of one sample, drawn around a valid path: first the path -- per frame a label step in
    {0, 1} (modified) or at most S - 1 labels (regular) --, then each frame's window placed at random around the nodes the
    path visits in that frame, the start clamped into [0, max(0, L + 1 - S)].  burst: the labels as early as the type allows
    and every window starting at the path's node, so that the starts jump by S - 1 (regular).  Frames past T get 0."""
    assert 0 <= L <= max_labels(T, S, rnnt_type), (T, L, S, rnnt_type)
    cap = 1 if rnnt_type == MODIFIED else S - 1
    counts = np.zeros(T, dtype=np.int64)
    if burst:
        left = L
        for t in range(T):
            counts[t] = min(cap, left)
            left -= counts[t]
    else:
        for _ in range(L):
            counts[rng.choice(np.nonzero(counts < cap)[0])] += 1
    s = np.zeros(maxT, dtype=np.int32)
    smax = max(0, L + 1 - S)
    u = 0
    for t in range(T):
        last = u if rnnt_type == MODIFIED else u + counts[t]          # the last node of frame t with an out-edge on the path
        lo, hi = last - (S - 1), u
        st = hi if burst else int(rng.integers(lo, hi + 1))
        s[t] = min(max(st, 0), smax)
        assert s[t] <= u and last < s[t] + S
        u += counts[t]
    assert u == L
    return s


def in_lattice_mask(shape, ranges, act_lens, label_lens):
    """(N, T, S) bool: rows t < T_b with ranges[b, t] + k <= L_b."""
    N, T, S = shape[:3]
    r = np.asarray(ranges)[:, :T, None] + np.arange(S)[None, None, :]
    t = np.arange(T)[None, :, None]
    return (t < np.asarray(act_lens)[:, None, None]) & (r <= np.asarray(label_lens)[:, None, None]) & (r >= 0)


def read_mask(shape, ranges, act_lens, label_lens, rnnt_type):
    """in_lattice_mask without the rows the modified type never reads: those outside the band u <= t, L_b - u <= T_b - t."""
    m = in_lattice_mask(shape, ranges, act_lens, label_lens)
    if rnnt_type == MODIFIED:
        N, T, S = shape[:3]
        u = np.asarray(ranges)[:, :T, None] + np.arange(S)[None, None, :]
        t = np.arange(T)[None, :, None]
        Tb, Lb = np.asarray(act_lens)[:, None, None], np.asarray(label_lens)[:, None, None]
        m = m & (u <= t) & (Lb - u <= Tb - t)
    return m


# ----------------------------------------------------------------------------- the k2 mapping
def k2_px_py(logits, labels, ranges, act_lens, label_lens, blank, rnnt_type, delay_penalty):
    """px (N, L, T + 1 | T) and py (N, L + 1, T) fp64 (L = maxU - 1) as k2's get_rnnt_logprobs_pruned is documented to build
    them from the pruned logits: log-softmax gathers of the label and of the blank at state ranges[b, t] + k, -inf outside
    the windows, and rnnt_loss_pruned's penalty = (T_b - 1) / 2 - t times delay_penalty added to px.  boundary (N, 4) =
    [0, 0, L_b, T_b]."""
    x = np.asarray(logits, dtype=np.float64)
    N, T, S, _ = x.shape
    L = np.asarray(labels).reshape(N, -1).shape[1]
    lp = torch.log_softmax(torch.tensor(x), -1).numpy()
    px = np.full((N, L, T if rnnt_type == MODIFIED else T + 1), -np.inf)
    py = np.full((N, L + 1, T), -np.inf)
    for b in range(N):
        Tb, Lb = int(act_lens[b]), int(label_lens[b])
        for t in range(Tb):
            for k in range(S):
                u = int(ranges[b][t]) + k
                if u > Lb:
                    continue
                py[b, u, t] = lp[b, t, k, blank]
                if u < Lb:
                    px[b, u, t] = lp[b, t, k, int(labels[b][u])] + delay_penalty * (0.5 * (Tb - 1) - t)
    boundary = np.stack([np.zeros(N), np.zeros(N), np.asarray(label_lens), np.asarray(act_lens)], 1).astype(np.int64)
    return px, py, boundary
