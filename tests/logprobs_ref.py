"""The definition of libwarprnnt_logprobs.so (include/rnnt_logprobs.h) in numpy: the edge log-probabilities px, py and the
normaliser lse from joint (B, T, U, C) or pruned (B, T, K, C) logits, and the logit gradient from the three incoming gradients.
The inputs are taken as fp64 values and the arithmetic is numpy's long double (a 64-bit mantissa where the platform has one), so
that the reference's own error stays far below the fp64 kernels' bound -- gl - gx - gy and the sums of the special columns cancel.
Loops over the rows: the tests use tiny shapes."""
import numpy as np

NEG = -np.inf
LD = np.longdouble


def lengths(B, T, S, boundary):
    """(S_b, T_b) per sample: boundary columns 2 and 3 clamped into [0, S] and [0, T]; S and T without a boundary."""
    if boundary is None:
        return np.full(B, S, int), np.full(B, T, int)
    bd = np.asarray(boundary)
    return np.clip(bd[:, 2], 0, S).astype(int), np.clip(bd[:, 3], 0, T).astype(int)


def rows(B, T, U, K, ranges, boundary):
    """[(b, t, k, u)] of the real rows, in logits order: t < T_b and u <= S_b, u = k (K = 0) or clamp(ranges[b, t], 0, U - K) + k."""
    sb, tb = lengths(B, T, U - 1, boundary)
    out = []
    for b in range(B):
        for t in range(int(tb[b])):
            r = 0 if K == 0 else int(np.clip(ranges[b, t], 0, U - K))
            for k in range(U if K == 0 else K):
                if r + k <= sb[b]:
                    out.append((b, t, k, r + k))
    return out


def real_mask(B, T, U, K, ranges, boundary):
    m = np.zeros((B, T, U if K == 0 else K), bool)
    for b, t, k, _ in rows(B, T, U, K, ranges, boundary):
        m[b, t, k] = True
    return m


def row_lse(z):
    """logsumexp of one row; NaN for a row that is all -inf or holds a NaN or +inf."""
    z = np.asarray(z, LD)
    m = z.max()
    if not np.isfinite(m) or np.isnan(z).any():
        return np.nan
    return m + np.log(np.exp(z - m).sum())


def forward(logits, symbols, blank, K=0, ranges=None, boundary=None, modified=False, lse=None):
    """-> (px, py, lse), long double.  lse given: the stored normaliser is used in place of the row's own (for the backward's bound)."""
    z = np.asarray(logits, LD)
    B, T, Kp, C = z.shape
    S = symbols.shape[1]
    U = S + 1
    assert Kp == (U if K == 0 else K)
    sb, _ = lengths(B, T, S, boundary)
    px = np.full((B, S, T if modified else T + 1), NEG, LD)
    py = np.full((B, U, T), NEG, LD)
    out = np.zeros((B, T, Kp), LD)
    with np.errstate(invalid="ignore"):
        for b, t, k, u in rows(B, T, U, K, ranges, boundary):
            l = row_lse(z[b, t, k]) if lse is None else lse[b, t, k]
            out[b, t, k] = l
            py[b, u, t] = z[b, t, k, blank] - l
            if u < sb[b]:
                y = int(symbols[b, u])
                if 0 <= y < C:
                    px[b, u, t] = z[b, t, k, y] - l
    return px, py, out


def backward(logits, lse, symbols, blank, px_grad, py_grad, lse_grad=None, K=0, ranges=None, boundary=None, modified=False):
    """-> (dz, coef, gx, gy): dz[c] = gx [c == y_u] + gy [c == blank] + (gl - gx - gy) exp(z[c] - lse) on real rows, 0 elsewhere;
    coef = gl - gx - gy and the row's gx, gy as (B, T, K') arrays for the error bound."""
    z, lse = np.asarray(logits, LD), np.asarray(lse, LD)
    B, T, Kp, C = z.shape
    S = symbols.shape[1]
    U = S + 1
    sb, _ = lengths(B, T, S, boundary)
    dz = np.zeros_like(z)
    coef, gxs, gys = np.zeros((B, T, Kp), LD), np.zeros((B, T, Kp), LD), np.zeros((B, T, Kp), LD)
    with np.errstate(invalid="ignore", over="ignore"):
        for b, t, k, u in rows(B, T, U, K, ranges, boundary):
            gy = LD(py_grad[b, u, t])
            gl = LD(0) if lse_grad is None else LD(lse_grad[b, t, k])
            gx, y = LD(0), -1
            if u < sb[b] and 0 <= int(symbols[b, u]) < C:
                y = int(symbols[b, u])
                gx = LD(px_grad[b, u, t])
            c = gl - gx - gy
            row = c * np.exp(z[b, t, k] - lse[b, t, k])
            if y >= 0:
                row[y] += gx
            row[blank] += gy
            dz[b, t, k] = row
            coef[b, t, k], gxs[b, t, k], gys[b, t, k] = c, gx, gy
    return dz, coef, gxs, gys
