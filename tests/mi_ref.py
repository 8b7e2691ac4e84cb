"""fp64 reference of include/rnnt_mi.h: the recursion of `mutual_information_recursion` written out directly in torch --
one logaddexp per anti-diagonal (regular type) or per frame (modified type) of a sample's rectangle -- and torch autograd for
the edge occupations.  It is given the STORED values of px / py as doubles (the rounding of 16-bit inputs is the caller's),
honours -inf edges (a sample without a path scores -inf and has zero gradients) and reads nothing outside a rectangle's
edge sets: the rectangle is sliced out before anything is computed, so NaN elsewhere never reaches arithmetic.  Independent
of the library: no table, no base 2, no offsets."""
import numpy as np
import torch

NEG = float("-inf")


def _lae(a, b):
    """logaddexp with -inf as the additive zero and clean gradients: where both are -inf the result is a constant."""
    m = torch.maximum(a, b)
    dead = torch.isneginf(m)
    ms = torch.where(dead, torch.zeros_like(m), m)
    s = torch.exp(a - ms) + torch.exp(b - ms)
    s = torch.where(dead, torch.ones_like(s), s)
    return torch.where(dead, torch.full_like(m, NEG), ms + torch.log(s))


def _masked(v, mask):
    return torch.where(mask, v, torch.full_like(v, NEG))


def full_boundary(B, S, T):
    return np.tile(np.array([0, 0, S, T], np.int64), (B, 1))


def _closed(r):
    """A total of -inf is a constant: a sample without a path has zero gradients (k2's guard), also where its -inf came
    from a plain sum along a single chain of edges."""
    return torch.where(torch.isneginf(r), torch.full_like(r, NEG), r)


def score_one(X, Y, modified):
    """p[Sr, Tr] of one rectangle.  Y (Sr + 1, Tr): frame edges; X (Sr, Tr + 1) regular or (Sr, Tr) modified: symbol edges."""
    Sr, Tr = Y.shape[0] - 1, Y.shape[1]
    s = torch.arange(Sr + 1)
    p = _masked(torch.zeros(Sr + 1, dtype=torch.float64), s == 0)              # diagonal 0 / frame 0: p[0, 0] = 0
    if modified:
        for t in range(1, Tr + 1):                                             # p[., t] from p[., t - 1]
            stay = p + Y[:, t - 1]
            if Sr:
                move = torch.cat((torch.full((1,), NEG, dtype=torch.float64), p[:-1] + X[:, t - 1]))
                p = _lae(stay, move)
            else:
                p = stay
        return _closed(p[Sr])
    for d in range(1, Sr + Tr + 1):                                            # node (s, d - s) from diagonal d - 1
        t = d - s
        ty = (t >= 1) & (t <= Tr)                                              # the frame edge (s, t - 1) -> (s, t)
        stay = _masked(p + (Y[s, (t - 1).clamp(0, max(Tr - 1, 0))] if Tr else torch.zeros(Sr + 1, dtype=torch.float64)), ty)
        if Sr:
            tx = (t >= 0) & (t <= Tr) & (s >= 1)                               # the symbol edge (s - 1, t) -> (s, t)
            prev = torch.cat((torch.full((1,), NEG, dtype=torch.float64), p[:-1]))
            move = _masked(prev + X[(s - 1).clamp(0, Sr - 1), t.clamp(0, Tr)], tx)
            p = _lae(stay, move)
        else:
            p = stay
    return _closed(p[Sr])


def mi_autograd(px, py, boundary=None, weights=None):
    """(scores (B,), px_grad, py_grad) in fp64; the gradients are those of sum_b weights[b] * score[b]."""
    px = torch.tensor(np.asarray(px, np.float64), requires_grad=True)
    py = torch.tensor(np.asarray(py, np.float64), requires_grad=True)
    B, S1, T = py.shape
    S = S1 - 1
    modified = px.shape[2] == T
    assert px.shape[:2] == (B, S) and px.shape[2] in (T, T + 1)
    bd = full_boundary(B, S, T) if boundary is None else np.asarray(boundary, np.int64)
    w = np.ones(B) if weights is None else np.asarray(weights, np.float64)
    scores = []
    for b in range(B):
        s0, t0, s1, t1 = (int(v) for v in bd[b])
        assert 0 <= s0 <= s1 <= S and 0 <= t0 <= t1 <= T, bd[b]
        X = px[b, s0:s1, t0:(t1 if modified else t1 + 1)]
        Y = py[b, s0:s1 + 1, t0:t1]
        scores.append(score_one(X, Y, modified))
    scores = torch.stack(scores)
    total = (scores * torch.tensor(w)).sum()
    if total.requires_grad:
        total.backward()
    gx = px.grad.numpy() if px.grad is not None else np.zeros(px.shape)
    gy = py.grad.numpy() if py.grad is not None else np.zeros(py.shape)
    return scores.detach().numpy(), gx, gy


def edge_masks(B, S, T, modified, boundary=None):
    """(mask of px's shape, mask of py's shape): the rectangle's edges of every sample."""
    bd = full_boundary(B, S, T) if boundary is None else np.asarray(boundary, np.int64)
    mx = np.zeros((B, S, T if modified else T + 1), bool)
    my = np.zeros((B, S + 1, T), bool)
    for b in range(B):
        s0, t0, s1, t1 = (int(v) for v in bd[b])
        mx[b, s0:s1, t0:(t1 if modified else t1 + 1)] = True
        my[b, s0:s1 + 1, t0:t1] = True
    return mx, my


def mi_brute(X, Y, modified):
    """The score of one small rectangle by enumerating its paths (numpy arrays, finite or -inf)."""
    Sr, Tr = Y.shape[0] - 1, Y.shape[1]
    tot = []

    def walk(s, t, acc):
        if s == Sr and t == Tr:
            tot.append(acc)
            return
        if t < Tr:
            walk(s, t + 1, acc + Y[s, t])
        if s < Sr and (t < Tr or not modified):
            walk(s + 1, t + 1 if modified else t, acc + X[s, t])

    walk(0, 0, 0.0)
    fin = [v for v in tot if v > NEG]
    return float(np.logaddexp.reduce(fin)) if fin else NEG
