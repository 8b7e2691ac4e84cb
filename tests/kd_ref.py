"""fp64 reference of the transducer lattice distillation loss (include/rnnt_kd.h), no GPU: the loss written from the
definition with explicit class sums of probabilities and differentiated by torch autograd (kd_autograd), the gradient by the
header's closed formula in numpy (kd_formula), and the sizes of the terms the tests' bounds are relative to (cost_mag,
grad_mag).  mode: 0 collapsed, 1 full.  Padding rows may hold anything: they are replaced before anything is computed."""
import numpy as np
import torch

from tests.side_check import in_lattice_mask          # noqa: F401  (re-exported)


def class_labels(labels, label_lens, blank, A, U):
    """(N, U) int: the label column of row u (clamped into [0, A)), -1 where the row has two classes only (u >= L_b, or a
    label equal to the blank)."""
    N = len(label_lens)
    out = np.full((N, U), -1, np.int64)
    for b in range(N):
        for u in range(min(int(label_lens[b]), U - 1)):
            lab = min(max(int(labels[b, u]), 0), A - 1)
            out[b, u] = -1 if lab == blank else lab
    return out


def class_of_column(labels, label_lens, blank, shape, mode):
    """(N, 1, U, A) int: the class of every column -- collapsed 0 blank, 1 label, 2 rest; full: the column itself."""
    N, T, U, A = shape
    if mode == 1:
        return np.broadcast_to(np.arange(A), (N, 1, U, A)).copy()
    cls = np.full((N, 1, U, A), 2, np.int64)
    lab = class_labels(labels, label_lens, blank, A, U)
    for b in range(N):
        for u in range(U):
            if lab[b, u] >= 0:
                cls[b, 0, u, lab[b, u]] = 1
    cls[..., blank] = 0
    return cls


def _clean(x, mask):
    return np.where(mask[..., None], np.asarray(x, np.float64), 0.0)


def _class_sums(p, cls, K):
    """(N, T, U, K): sum of p over the columns of each class."""
    c = torch.as_tensor(cls)                                                             # (N, 1, U, A)
    return torch.stack([(p * (c == k)).sum(-1) for k in range(K)], -1)


def kd_autograd(z, w, labels, act_lens, label_lens, blank=0, mode=0, tau=1.0, weights=None, cls=None):
    """costs (N,), d sum_b weights_b cost_b / d z (N, T, U, A), numpy fp64."""
    shape = np.shape(z)
    N, T, U, A = shape
    mask = in_lattice_mask(shape, act_lens, label_lens)
    zt = torch.tensor(_clean(z, mask), requires_grad=True)
    wt = torch.tensor(_clean(w, mask))
    p, q = torch.softmax(zt / tau, -1), torch.softmax(wt / tau, -1)
    if mode == 0:
        cls = class_of_column(labels, label_lens, blank, shape, 0) if cls is None else cls
        P, Q = _class_sums(p, cls, 3), _class_sums(q, cls, 3)
    else:
        P, Q = p, q
    live = Q > 0
    one = torch.ones_like(P)
    rows = torch.where(live, Q * (torch.log(torch.where(live, Q, one)) - torch.log(torch.where(live, P, one))),
                       torch.zeros_like(P)).sum(-1)
    costs = (rows * torch.tensor(mask)).sum((1, 2))
    wts = torch.ones(N, dtype=torch.float64) if weights is None else torch.tensor(np.asarray(weights, np.float64))
    (costs * wts).sum().backward()
    return costs.detach().numpy(), zt.grad.numpy()


def _probs(z, w, labels, act_lens, label_lens, blank, mode, tau, cls=None):
    shape = np.shape(z)
    mask = in_lattice_mask(shape, act_lens, label_lens)
    p = torch.softmax(torch.tensor(_clean(z, mask)) / tau, -1).numpy()
    q = torch.softmax(torch.tensor(_clean(w, mask)) / tau, -1).numpy()
    cls = np.broadcast_to(class_of_column(labels, label_lens, blank, shape, mode) if cls is None else cls, shape)
    K = 3 if mode == 0 else shape[3]
    P, Q = np.zeros(shape[:3] + (K,)), np.zeros(shape[:3] + (K,))
    if mode == 0:
        for k in range(3):
            P[..., k] = np.where(cls == k, p, 0.0).sum(-1)
            Q[..., k] = np.where(cls == k, q, 0.0).sum(-1)
    else:
        P, Q = p, q
    return p, P, Q, cls, mask


def kd_formula(z, w, labels, act_lens, label_lens, blank=0, mode=0, tau=1.0, cls=None):
    """The header's gradient: (1 / tau) [p_v - p_v Q(c(v)) / P(c(v))], zero on padding."""
    p, P, Q, cls, mask = _probs(z, w, labels, act_lens, label_lens, blank, mode, tau, cls)
    Pc, Qc = np.take_along_axis(P, cls, -1), np.take_along_axis(Q, cls, -1)
    g = (p - p * Qc / np.where(Pc > 0, Pc, 1.0)) / tau
    return np.where(mask[..., None], g, 0.0)


def cost_mag(z, w, labels, act_lens, label_lens, blank=0, mode=0, tau=1.0, cls=None):
    """mag_b = sum over the in-lattice rows of sum_k Q(k) (|log Q(k)| + |log P(k)|): the size of the terms of cost_b."""
    p, P, Q, cls, mask = _probs(z, w, labels, act_lens, label_lens, blank, mode, tau, cls)
    live = Q > 0
    with np.errstate(divide="ignore"):
        terms = np.where(live, Q * (np.abs(np.log(np.where(live, Q, 1.0))) + np.abs(np.log(np.where(live, P, 1.0)))), 0.0)
    return (terms.sum(-1) * mask).sum((1, 2))


def grad_mag(z, w, labels, act_lens, label_lens, blank=0, mode=0, tau=1.0, cls=None):
    """The sum of the two terms' sizes of every gradient element: (p_v + p_v Q(c) / P(c)) / tau."""
    p, P, Q, cls, mask = _probs(z, w, labels, act_lens, label_lens, blank, mode, tau, cls)
    Pc, Qc = np.take_along_axis(P, cls, -1), np.take_along_axis(Q, cls, -1)
    return np.where(mask[..., None], (p + p * Qc / np.where(Pc > 0, Pc, 1.0)) / tau, 0.0)


def kd_rows(z, w, lab, blank=0, tau=1.0):
    """Collapsed mode on n separate rows z, w (n, A) with label columns lab (n,), -1 for a row of two classes: the rows' KL
    (n,), gradients (n, A), the size of each KL's terms (n,) and of each gradient element's (n, A).  Plain numpy from the
    definition and the header's closed formula, one pass (tests/test_kd_cpu.py holds it to kd_autograd): cheap enough for a
    few hundred rows of a large vocabulary."""
    n, A = np.shape(z)
    p = torch.softmax(torch.tensor(np.asarray(z, np.float64)) / tau, -1).numpy()
    q = torch.softmax(torch.tensor(np.asarray(w, np.float64)) / tau, -1).numpy()
    lab = np.asarray(lab)
    has = (lab >= 0) & (lab != blank)
    idx, lc = np.arange(n), np.where(has, lab, blank)

    def sums(x):                                                  # every class over its own columns
        rest = x.copy()
        rest[:, blank] = 0.0
        rest[idx[has], lc[has]] = 0.0
        return np.stack((x[:, blank], np.where(has, x[idx, lc], 0.0), rest.sum(1)), 1)
    P, Q = sums(p), sums(q)
    live = Q > 0
    lQ, lP = np.log(np.where(live, Q, 1.0)), np.log(np.where(live, P, 1.0))
    kl = np.where(live, Q * (lQ - lP), 0.0).sum(1)
    cmag = np.where(live, Q * (np.abs(lQ) + np.abs(lP)), 0.0).sum(1)
    ratio = Q / np.where(P > 0, P, 1.0)
    r = np.repeat(ratio[:, 2:3], A, 1)
    r[idx[has], lc[has]] = ratio[has, 1]
    r[:, blank] = ratio[:, 0]
    return kl, (p - p * r) / tau, cmag, (p + p * r) / tau
