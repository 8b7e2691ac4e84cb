"""Test infrastructure (no GPU) for the pruned RNN-T loss and the prune ranges (include/rnnt_pruned.h).

  * pruned_autograd: the pruned loss as an explicit fp64 log-sum-exp lattice over the windows, differentiated by
    torch.autograd -- only the forward recursion is written down, as in tests/autograd_ref.py;
  * ranges_rule: the prune-ranges rule of rnnt_pruned.h in numpy, on an fp64 occupancy gamma (T_b, L_b + 1);
  * has_path: brute-force reachability of the final blank through the windows;
  * occupancy_add: gamma of the additive joint f + g from an fp64 forward-backward (for the GPU tests).
"""
import numpy as np
import torch

NEG = -1.0e30          # "log zero" of the reference lattice: -inf would turn logaddexp's derivative into NaN


def _sample_pruned(x, s, lab, T, L, blank):
    """-log P of one sample: x (T, S, A) fp64 logits (a view of the leaf), s (T,) window starts, lab (L,) labels."""
    S = x.shape[1]
    U = L + 1
    lp = torch.log_softmax(x, -1)
    pb = torch.full((T, U), NEG, dtype=x.dtype)
    pl = torch.full((T, U), NEG, dtype=x.dtype)
    labs = torch.as_tensor(np.asarray(lab, dtype=np.int64))
    for t in range(T):
        st = int(s[t])
        n = min(S, U - st)
        if n <= 0:
            continue
        pb[t, st:st + n] = lp[t, :n, blank]
        m = min(n, L - st)                                  # label edges: u < L
        if m > 0:
            pl[t, st:st + m] = lp[t, torch.arange(m), labs[st:st + m]]
    prev_lo, prev = 0, torch.zeros(1, dtype=x.dtype)
    for d in range(1, T + U - 1):
        lo, hi = max(0, d - (U - 1)), min(d, T - 1)
        t = torch.arange(lo, hi + 1)
        u = d - t
        top = torch.full((hi - lo + 1,), 2 * NEG, dtype=x.dtype)
        left = torch.full((hi - lo + 1,), 2 * NEG, dtype=x.dtype)
        m = t >= 1
        if m.any():
            top = torch.where(m, prev[(t - 1 - prev_lo).clamp(0, len(prev) - 1)] + pb[(t - 1).clamp(min=0), u], top)
        m = u >= 1
        if m.any():
            ti = (t - prev_lo).clamp(0, len(prev) - 1)
            left = torch.where(m, prev[ti] + pl[t, (u - 1).clamp(min=0)], left)
        prev_lo, prev = lo, torch.logaddexp(top, left)
    return -(prev[(T - 1) - prev_lo] + pb[T - 1, U - 1])


def pruned_autograd(logits, labels, ranges, act_lens, label_lens, blank=0, weights=None):
    """costs (N,) and d(sum_b w_b cost_b)/d(logits) (N, T, S, A) in fp64.  A sample without a path through its windows costs
    +inf (its gradient here is left as computed: the callers expect NaN from the library there).  Padding rows: zero."""
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    N = x.shape[0]
    labels = np.asarray(labels).reshape(N, -1)
    costs = []
    for b in range(N):
        T, L = int(act_lens[b]), int(label_lens[b])
        costs.append(_sample_pruned(x[b, :T], np.asarray(ranges[b]), labels[b], T, L, blank))
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    sum(c * float(w[i]) for i, c in enumerate(costs)).backward()
    out = np.array([c.item() for c in costs])
    out[out > 1e29] = np.inf
    return out, x.grad.numpy()


def in_lattice_mask(shape, ranges, act_lens, label_lens):
    """(N, T, S) bool: rows t < T_b with ranges[b, t] + k <= L_b."""
    N, T, S = shape[:3]
    m = np.zeros((N, T, S), bool)
    for b in range(N):
        for t in range(int(act_lens[b])):
            for k in range(S):
                m[b, t, k] = int(ranges[b][t]) + k <= int(label_lens[b])
    return m


def ranges_rule(gamma, T, L, S):
    """The rule of compute_rnnt_prune_ranges_add on an fp64 occupancy gamma (T, L + 1); returns s (T,) int."""
    step, smax = S - 1, max(0, L + 1 - S)
    if L > T * step:                                                 # no windows can hold a path
        return np.array([min(t * step, smax) for t in range(T)], dtype=np.int64)
    s = np.zeros(T, dtype=np.int64)
    for t in range(T):
        best, bs = -1.0, 0
        for c in range(smax + 1):
            v = float(np.sum(gamma[t, c:min(c + S, L + 1)]))
            if v > best:
                best, bs = v, c
        lo, hi = max(0, smax - (T - 1 - t) * step), min(smax, t * step)
        s[t] = min(max(bs, lo), hi)
    for t in range(1, T):
        s[t] = max(s[t], s[t - 1])
    for t in range(T - 2, -1, -1):
        s[t] = max(s[t], s[t + 1] - step)
    return s


def has_path(s, T, L, S):
    """Does a path from (0, 0) through the final blank at (T - 1, L) exist using only cells inside their frame's window?"""
    inside = lambda t, u: int(s[t]) <= u < int(s[t]) + S and u <= L
    reach = np.zeros((T, L + 1), bool)
    reach[0, 0] = True                                               # the start needs no edge; its edges need the window
    for t in range(T):
        for u in range(L + 1):
            if not reach[t, u] or not inside(t, u):
                continue
            if u < L:
                reach[t, u + 1] = True
            if t + 1 < T:
                reach[t + 1, u] = True
    return bool(reach[T - 1, L] and inside(T - 1, L))


def check_invariants(s, T, L, S):
    """The guarantees of the rule when L <= T (S - 1); a list of violated ones."""
    bad = []
    smax = max(0, L + 1 - S)
    if s[0] != 0:
        bad.append("s_0 = %d" % s[0])
    d = np.diff(np.asarray(s[:T], dtype=np.int64))
    if (d < 0).any() or (d > S - 1).any():
        bad.append("steps %s" % d)
    if s[T - 1] != smax:
        bad.append("s_last = %d, smax %d" % (s[T - 1], smax))
    if not has_path(s, T, L, S):
        bad.append("no path")
    return bad


def occupancy_add(f, g, labels, T, L, blank=0):
    """gamma (T, L + 1) of the additive joint f (T, A) + g (L + 1, A) in fp64 (forward-backward in the log domain)."""
    z = f[:T, None, :].astype(np.float64) + g[None, :L + 1, :].astype(np.float64)
    mx = z.max(-1, keepdims=True)
    lp = z - (mx + np.log(np.exp(z - mx).sum(-1, keepdims=True)))
    pb = lp[:, :, blank]
    pl = np.full((T, L + 1), -np.inf)
    for u in range(L):
        pl[:, u] = lp[:, u, int(labels[u])]
    a = np.full((T, L + 1), -np.inf)
    bt = np.full((T, L + 1), -np.inf)
    a[0, 0] = 0.0
    for t in range(T):
        for u in range(L + 1):
            if t == 0 and u == 0:
                continue
            x = -np.inf if t == 0 else a[t - 1, u] + pb[t - 1, u]
            y = -np.inf if u == 0 else a[t, u - 1] + pl[t, u - 1]
            a[t, u] = np.logaddexp(x, y)
    bt[T - 1, L] = pb[T - 1, L]
    for t in range(T - 1, -1, -1):
        for u in range(L, -1, -1):
            if t == T - 1 and u == L:
                continue
            x = -np.inf if t == T - 1 else bt[t + 1, u] + pb[t, u]
            y = -np.inf if u == L else bt[t, u + 1] + pl[t, u]
            bt[t, u] = np.logaddexp(x, y)
    return np.exp(a + bt - bt[0, 0])
