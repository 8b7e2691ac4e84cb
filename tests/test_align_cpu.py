"""Best-path alignment (compute_rnnt_align, warprnnt_pytorch.rnnt_align) on the CPU location, against a numpy fp64 Viterbi
with the tie rule of include/rnnt.h -- which is itself checked against brute-force enumeration of every path."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests.align_ref import path_score, viterbi_np
from warprnnt_pytorch import _lib, rnnt_align


# ----------------------------------------------------------------------------- numpy reference
def brute_force(lp, labels, T, U, blank):
    """Every path: every non-decreasing frame assignment of the U labels.  Best score, and the lexicographically
    smallest frames among the best (= the earliest emissions the tie rule asks for)."""
    best, arg = -np.inf, None
    for fr in itertools.combinations_with_replacement(range(T), U):
        s = path_score(lp, labels, T, U, blank, fr)
        if arg is None or s > best:
            best, arg = s, list(fr)
    return best, arg


def log_softmax_np(x):
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def test_numpy_viterbi_matches_brute_force():
    rng = np.random.default_rng(1)
    for T in range(1, 6):
        for U in range(0, 4):
            for trial in range(3):
                A = 4
                lp = log_softmax_np(rng.standard_normal((T, U + 1, A)) * 2)
                labels = rng.integers(1, A, size=U)
                s, fr = viterbi_np(lp, labels, T, U, 0)
                bs, bfr = brute_force(lp, labels, T, U, 0)
                assert abs(s - bs) < 1e-12, (T, U, s, bs)
                assert fr == bfr, (T, U, fr, bfr)
                assert abs(path_score(lp, labels, T, U, 0, fr) - s) < 1e-12


def test_numpy_viterbi_tie_rule_brute_force():
    for T in range(1, 6):
        for U in range(0, 4):
            lp = np.full((T, U + 1, 3), -np.log(3.0))
            labels = np.ones(U, dtype=np.int64)
            s, fr = viterbi_np(lp, labels, T, U, 0)
            assert fr == [0] * U
            assert fr == brute_force(lp, labels, T, U, 0)[1]


# ----------------------------------------------------------------------------- the C-ABI, CPU location
def cabi_align(lp, labels, act_lens, label_lens, blank=0):
    """compute_rnnt_align with RNNT_CPU on log-probs lp (N, maxT, maxU, A)."""
    lp = np.ascontiguousarray(lp)
    N, T, U, A = lp.shape
    code, esz = (_lib.DT_F64, 8) if lp.dtype == np.float64 else (_lib.DT_F32, 4)
    score = np.zeros(N, dtype=np.float64)
    frames = np.zeros((N, max(U - 1, 1)), dtype=np.int32)
    labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(N, U - 1) if U > 1 else np.zeros((N, 1), np.int32)
    xl = np.ascontiguousarray(act_lens, dtype=np.int32)
    yl = np.ascontiguousarray(label_lens, dtype=np.int32)
    ws = np.zeros(_lib.workspace_bytes(T, U, N, False, esz) // 8 + 1, dtype=np.float64)
    opt = _lib.rnntOptions(loc=_lib.RNNT_CPU, num_threads=0, stream=None, blank_label=blank, maxT=T, maxU=U,
                           batch_first=True)
    st = _lib.lib().compute_rnnt_align(lp.ctypes.data, labels.ctypes.data, yl.ctypes.data, xl.ctypes.data, A, N,
                                       score.ctypes.data, frames.ctypes.data, ws.ctypes.data, opt, code)
    return st, score, frames[:, :U - 1]


def check_batch(lp, labels, act_lens, label_lens, blank, score, frames, tol=1e-9):
    N = lp.shape[0]
    for b in range(N):
        T, U = int(act_lens[b]), int(label_lens[b])
        s, fr = viterbi_np(lp[b], labels[b], T, U, blank)
        if np.isnan(s):
            assert np.isnan(score[b]), (b, score[b])
        elif not np.isfinite(s):
            assert score[b] == s, (b, score[b], s)
        else:
            assert abs(score[b] - s) <= tol * max(1.0, abs(s)), (b, score[b], s)
        assert list(frames[b, :U]) == fr, (b, list(frames[b, :U]), fr)
        assert (frames[b, U:] == -1).all()


def make_batch(rng, N, T, U, A, blank=0, dtype=np.float64):
    acts = rng.standard_normal((N, T, U, A)) * 2
    lp = log_softmax_np(acts).astype(dtype)
    labels = rng.integers(0, A, size=(N, U - 1)).astype(np.int32)
    labels[labels == blank] = (blank + 1) % A
    act_lens = rng.integers(1, T + 1, size=N).astype(np.int32)
    label_lens = rng.integers(0, U, size=N).astype(np.int32)
    act_lens[0], label_lens[0] = T, U - 1
    return lp, labels, act_lens, label_lens


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("blank", [0, 3])
def test_cabi_cpu_padded_batch(dtype, blank):
    rng = np.random.default_rng(7)
    lp, labels, xl, yl = make_batch(rng, 6, 9, 5, 7, blank, dtype)
    yl[1] = 0                                        # U_b = 0: empty frame row, the sum of the blanks
    st, score, frames = cabi_align(lp, labels, xl, yl, blank)
    assert st == _lib.STATUS_SUCCESS
    check_batch(lp.astype(np.float64), labels, xl, yl, blank, score, frames, 1e-6 if dtype == np.float32 else 1e-12)
    assert abs(score[1] - lp[1, np.arange(xl[1]), 0, blank].astype(np.float64).sum()) < 1e-5
    assert (frames[1] == -1).all()


def test_cabi_cpu_label_equals_blank():
    rng = np.random.default_rng(3)
    lp, labels, xl, yl = make_batch(rng, 3, 6, 4, 5)
    labels[:] = 0                                    # the label IS the blank symbol: both moves read the same column
    st, score, frames = cabi_align(lp, labels, xl, yl, 0)
    assert st == 0
    check_batch(lp, labels, xl, yl, 0, score, frames)


def test_cabi_cpu_forbidden_cells_and_nan():
    rng = np.random.default_rng(4)
    lp, labels, xl, yl = make_batch(rng, 4, 6, 4, 5)
    xl[:] = 6
    yl[:] = 3
    lp[0, 2, 1, labels[0, 1]] = -np.inf              # sample 0: one label cell forbidden -- another path wins
    lp[1, :, :, 0] = -np.inf                         # sample 1: no blank anywhere -- no path at all
    lp[2, 3, 2, 0] = np.nan                          # sample 2: a NaN the lattice reads
    st, score, frames = cabi_align(lp, labels, xl, yl, 0)
    assert st == 0
    check_batch(lp, labels, xl, yl, 0, score, frames)
    assert np.isfinite(score[0]) and np.isfinite(score[3])
    assert score[1] == -np.inf and (frames[1] == -1).all()
    assert np.isnan(score[2]) and (frames[2] == -1).all()


def test_cabi_cpu_uniform_tie_all_frames_zero():
    N, T, U, A = 3, 7, 5, 6
    lp = np.full((N, T, U, A), -np.log(A))
    labels = np.full((N, U - 1), 2, np.int32)
    st, score, frames = cabi_align(lp, labels, np.full(N, T, np.int32), np.full(N, U - 1, np.int32))
    assert st == 0
    assert (frames == 0).all()
    assert np.allclose(score, -(T + U - 1) * np.log(A))


def test_cabi_invalid_arguments():
    lp, labels, xl, yl = make_batch(np.random.default_rng(0), 2, 4, 3, 5)
    lib = _lib.lib()
    N, T, U, A = lp.shape
    score = np.zeros(N)
    frames = np.zeros((N, U - 1), np.int32)
    ws = np.zeros(_lib.workspace_bytes(T, U, N, False, 8) // 8 + 1)
    opt = _lib.rnntOptions(loc=_lib.RNNT_CPU, num_threads=0, stream=None, blank_label=0, maxT=T, maxU=U, batch_first=True)
    args = [lp.ctypes.data, labels.ctypes.data, yl.ctypes.data, xl.ctypes.data, A, N, score.ctypes.data,
            frames.ctypes.data, ws.ctypes.data, opt, _lib.DT_F64]
    assert lib.compute_rnnt_align(*args) == 0
    for i in (0, 1, 2, 3, 6, 7, 8):                  # every pointer
        bad = list(args)
        bad[i] = None
        assert lib.compute_rnnt_align(*bad) == _lib.RNNT_STATUS_INVALID_VALUE, i
    for i, v in ((4, 0), (5, 0), (10, 2), (10, 7)):  # alphabet, minibatch, dtype (the CPU location: fp32 / fp64 only)
        bad = list(args)
        bad[i] = v
        assert lib.compute_rnnt_align(*bad) == _lib.RNNT_STATUS_INVALID_VALUE, (i, v)
    for field, v in (("blank_label", A), ("blank_label", -1), ("maxT", 0), ("maxU", 0), ("loc", 5)):
        o = _lib.rnntOptions(loc=_lib.RNNT_CPU, num_threads=0, stream=None, blank_label=0, maxT=T, maxU=U, batch_first=True)
        setattr(o, field, v)
        bad = list(args)
        bad[9] = o
        assert lib.compute_rnnt_align(*bad) == _lib.RNNT_STATUS_INVALID_VALUE, field
    xl_bad = xl.copy()
    xl_bad[1] = T + 1                                # lengths that do not fit the tensor
    bad = list(args)
    bad[3] = xl_bad.ctypes.data
    assert lib.compute_rnnt_align(*bad) == _lib.RNNT_STATUS_INVALID_VALUE
    # the additive entry is GPU only
    o = _lib.rnntOptions(loc=_lib.RNNT_CPU, num_threads=0, stream=None, blank_label=0, maxT=T, maxU=U, batch_first=True)
    assert lib.compute_rnnt_align_add(lp.ctypes.data, lp.ctypes.data, labels.ctypes.data, yl.ctypes.data,
                                      xl.ctypes.data, A, N, score.ctypes.data, frames.ctypes.data, ws.ctypes.data,
                                      o, 0) == _lib.RNNT_STATUS_INVALID_VALUE


# ----------------------------------------------------------------------------- the PyTorch function on CPU tensors
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rnnt_align_cpu_tensors(dtype):
    rng = np.random.default_rng(11)
    N, T, U, A, blank = 5, 8, 4, 6, 2
    acts = rng.standard_normal((N, T, U, A)) * 2
    labels = rng.integers(0, A, size=(N, U - 1)).astype(np.int32)
    xl = np.array([T, 3, 5, 1, T], np.int32)
    yl = np.array([U - 1, 0, 2, 1, U - 1], np.int32)
    x = torch.tensor(acts, dtype=dtype)
    score, frames = rnnt_align(x, torch.tensor(labels), torch.tensor(xl), torch.tensor(yl), blank=blank)
    assert score.dtype == torch.float64 and frames.dtype == torch.int32 and frames.shape == (N, U - 1)
    lp = torch.log_softmax(x, -1).double().numpy()
    check_batch(lp, labels, xl, yl, blank, score.numpy(), frames.numpy(), 1e-6 if dtype == torch.float32 else 1e-12)


def test_rnnt_align_cpu_no_labels_at_all():
    N, T, A = 2, 4, 3
    x = torch.randn(N, T, 1, A, dtype=torch.float64)
    score, frames = rnnt_align(x, torch.zeros((N, 0), dtype=torch.int32), torch.full((N,), T, dtype=torch.int32),
                               torch.zeros(N, dtype=torch.int32))
    assert frames.shape == (N, 0)
    assert torch.allclose(score, torch.log_softmax(x, -1)[:, :, 0, 0].sum(1))


def test_rnnt_align_checks_inputs():
    x = torch.randn(2, 4, 3, 5)
    lab = torch.ones((2, 2), dtype=torch.int32)
    with pytest.raises(ValueError):
        rnnt_align(x, lab, torch.tensor([3, 3], dtype=torch.int32), torch.tensor([2, 2], dtype=torch.int32))
    with pytest.raises(TypeError):
        rnnt_align(x, lab.long(), torch.tensor([4, 4], dtype=torch.int32), torch.tensor([2, 2], dtype=torch.int32))


# ----------------------------------------------------------------------------- workspace sizes are unchanged
# get_workspace_size / get_workspace_size_add as they were before the alignment entries existed (the align calls run in
# the same workspace): the layout arithmetic of the loss, restated here in the smallest form that pins the numbers.

@pytest.mark.parametrize("T,U,N", [(1, 1, 1), (2, 1, 3), (7, 5, 2), (50, 21, 16), (150, 41, 16), (200, 41, 64),
                                   (1500, 301, 64), (1000, 100, 8), (33, 600, 1), (9, 1024, 2)])
def test_workspace_sizes_unchanged(T, U, N):
    def size(gpu, esz):
        n = C.c_size_t(0)
        assert _lib.lib().get_workspace_size(T, U, N, gpu, C.byref(n), esz) == 0
        return n.value
    n = C.c_size_t(0)
    assert _lib.lib().get_workspace_size_add(T, U, N, C.byref(n)) == 0
    got = (size(True, 4), size(True, 8), size(True, 2), size(False, 4), size(False, 8), n.value)
    assert got == workspace_sizes_before(T, U, N)


def workspace_sizes_before(T, U, N):
    """make_layout() of csrc/rnnt_host.h as it stood when the alignment entries were added."""
    K = 256
    def al(x):
        return (x + K - 1) // K * K
    def layout(lat, joint):
        Dp = T + U - 1 + 32
        Up = (U + 7) & ~7
        W = (Up + 63) // 64
        block = ((5 * Dp * Up + Up + 64 + 63) & ~63) * lat
        rec1 = T * U * 4 * lat
        recs = rec1 * N
        head = recs
        if recs > (32 << 20):
            head = max((recs + 7) // 8, 32 << 20, rec1)
        head = al(head)
        o = al(head + block * N)
        rowscale = al(recs)
        if rowscale + T * U * N * lat > o:
            o = al(rowscale + T * U * N * lat)
        o = al(o + Dp * W * N * 8)
        o = al(o + (Dp * W * N + Dp) * 8)
        for _ in range(3):
            o = al(o + N * 8)
        o = al(o + 64 * N * 4)
        o = al(o + 16)
        o = al(o + N * 4)
        if joint:
            o = al(o + ((T + U) * N + 2) * 4)
            o = al(o + ((T + 2 * U) * N + N) * 4)
            o = al(o + 3 * T * ((U + 7) & ~7) * N * 4)
        return o + K
    return (layout(4, False), layout(8, False), layout(4, False), T * U * 4 * 4 * N, T * U * 4 * 8 * N, layout(4, True))
