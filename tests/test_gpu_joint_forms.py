"""-m gpu: every kernel form of the additive joint and of the alignment, one case per row of tests/joint_forms.py.  Each case
calls its C-ABI entry through warprnnt_pytorch._lib (compute_rnnt_loss_add, _add_fwd + _add_bwd, _add_fwd_dt + _add_bwd_dt,
_add_fwd_fastemit + _add_bwd, compute_rnnt_align_add, compute_rnnt_align) under torch.profiler, with f, g, df and dg placed at the
case's byte offsets from a 16-byte boundary, and the kernels recorded for each stage must be exactly the ones the release rules
predict (joint_forms.predict_joint, with this device's compute-unit count).  Costs, df = sum_u dz and dg = sum_t dz are compared
element by element with the fp64 oracle on the materialised joint z = f + g, at the bounds tests/test_gpu_add_network.py uses
for the same dtype and shape class; alignments with the numpy Viterbi of tests/align_ref.py.  Lengths are ragged (one
sample at T_b = 1, one at U_b = 1), and the padded rows of f (t >= T_b) and g (u >= U_b) hold NaN, which must never be read
(include/rnnt.h); the gradient buffers start as NaN and their padding must come back as exact zeros."""
import zlib

import numpy as np
import pytest
import torch

from tests import gpu_support as G
from tests import joint_forms as J
from tests.align_ref import path_score, viterbi_np
from tests.gpu_support import DEV, TORCH, assert_stages, options, place, profiled, ragged_lengths, stages_seen

pytestmark = pytest.mark.gpu


def _problem(case, cus):
    """f, g (fp32 numpy, before storage rounding), labels, lengths, blank for a case, with its data-dependent shape."""
    N, T, U, A = J.K.case_shape(case, cus)
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()))
    f = rng.standard_normal((N, T, A)) * 1.5
    g = rng.standard_normal((N, U, A)) * 1.5
    tl, ll = ragged_lengths(N, T, U, rng, pair_without_labels=True)
    blank = 0
    labels = rng.integers(1, A, size=(N, U - 1)) if A > 1 else np.zeros((N, U - 1), np.int64)
    data = case.get("data")
    if data == "guard":
        # Rows of sample 0 (f) and sample 1 (g) peak ~95 nats above their first 32 columns -- the sampled row reference -- far
        # beyond the guard (40 in base 2 = 27.7 nats).  Without the gated exact pass the Z kernel would sum exp(z - ref) with
        # z - ref > 88.7 = log(FLT_MAX): an infinite partition function, infinite costs and NaN gradients.
        f[0, ::3, 32 + A // 3] += 100.0
        g[min(1, N - 1), ::2, 32 + A // 2] += 100.0
    elif data == "masked32":
        # The first 32 columns of every row are -inf: the sampled reference is -inf, and without the exact pass every
        # z - ref would be +inf (NaN costs).  Blank and labels stay out of the masked columns.
        f[..., :32] = -np.inf
        g[..., :32] = -np.inf
        blank = 40
        labels = 41 + labels % (A - 41)
    elif data == "far":
        # Sample 1's best f column and best g column differ by 100+ nats (fp32: 120 / 150, the large-logit test; 16-bit: 70 / 70,
        # the 16-bit far-cell test): every one of its cells is a far cell, which the gradient GEMMs leave out (W = the far mark).
        # Their whole gradient comes from joint_far*_kernel: without it df[1] and dg[1] would miss O(1) mass per row.
        b = min(1, N - 1)
        big = (120.0, 150.0) if case["dtype"] == "f32" else (70.0, 70.0)
        f[b, :, 3] += big[0]
        g[b, :, 40 % A] += big[1]
    return f, g, labels.astype(np.int32), tl, ll, blank


def _nan_padding(x, lens, upto):
    """NaN in the rows t >= lens[b] (f) / u >= lens[b] + upto - 1 (g: upto = 2, u >= U_b)."""
    x = x.clone()
    for b in range(x.shape[0]):
        x[b, int(lens[b]) + upto - 1:] = float("nan")
    return x


def _scale(case, N):
    return (0.5 + 0.6 * (np.arange(N) % 5)).astype(np.float32) if case.get("scale") else None


def _check_stages(case, names, cus):
    assert_stages(case["name"], stages_seen(names, J.jstage_of, J.JSTAGES), J.predict_joint(case, cus))
    return sorted({n for n in names if J.jstage_of(n)})


# ----------------------------------------------------------------------------- the loss entries
def check_loss(case, oracle, fs, gs, labels, tl, ll, blank, sc, got_c, got_f, got_g):
    """Costs, df and dg of a loss case against the fp64 oracle on the materialised joint of the stored f and g (CPU tensors),
    at the module docstring's bounds; sc: the per-sample scale or None.  got_c None: gradients only (a backward call); got_f
    and got_g None: costs only.  -> the reference df."""
    N, T, A = fs.shape
    U = gs.shape[1]
    dt = fs.dtype
    lam = case.get("lam", 0.0)
    # the oracle on the materialised joint of the stored values
    fr, gr = fs.double().numpy(), gs.double().numpy()
    z = fr[:, :, None, :] + gr[:, None, :, :]
    if lam:
        lp = oracle.log_softmax(z)
        ref_c, g_lp = oracle.rnnt_logprobs(lp, labels, tl, ll, blank)
        for b in range(N):
            for u in range(ll[b]):
                g_lp[b, :tl[b], u, labels[b, u]] *= 1.0 + lam
        ref_gz = oracle.chain_rule_to_logits(lp, g_lp)
    else:
        ref_c, ref_gz = oracle.rnnt_logits(z, labels, tl, ll, blank)
    for b in range(N):
        ref_gz[b, tl[b]:] = 0
        ref_gz[b, :, ll[b] + 1:] = 0
    w = np.ones(N) if sc is None else sc.astype(np.float64)
    rdf = ref_gz.sum(axis=2) * w[:, None, None]
    rdg = ref_gz.sum(axis=1) * w[:, None, None]
    what = case["name"]
    if got_c is None:
        got_c = ref_c
    if got_f is None:
        got_f, got_g = rdf, rdg
    assert np.isfinite(got_c).all() and np.isfinite(got_f).all() and np.isfinite(got_g).all(), what
    for b in range(N):                                               # gradient padding: every element written, exactly zero
        assert not got_f[b, tl[b]:].any() and not got_g[b, ll[b] + 1:].any(), (what, b)
    big = max(1.0, np.abs(ref_c).max())
    scale = float(np.abs(w).max())
    data = case.get("data")
    if dt == torch.float32:
        if data is None:                                             # test_against_oracle_on_materialised_joint
            assert np.abs(got_c - ref_c).max() <= 1e-4 * big, (what, got_c, ref_c)
            edf = np.abs(got_f - rdf) - (2e-4 * scale * max(1.0, U / 32) + 5e-5 * np.abs(rdf))
            edg = np.abs(got_g - rdg) - (2e-4 * scale * max(1.0, T / 32) + 5e-5 * np.abs(rdg))
        else:                                                        # the guard / large-logit tests
            assert np.abs(got_c - ref_c).max() <= 2e-4 * big, (what, got_c, ref_c)
            edf = np.abs(got_f - rdf) - (5e-4 * scale + 1e-3 * np.abs(rdf))
            edg = np.abs(got_g - rdg) - (5e-4 * scale * (max(1.0, T / 32) if data != "far" else 1.0) + 1e-3 * np.abs(rdg))
    else:
        assert np.abs(got_c - ref_c).max() <= 1e-4 * big, (what, got_c, ref_c)
        if data == "far":                                            # test_sixteen_bit_far_cells_and_scale
            ulp = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10
            edf = np.abs(got_f - rdf) - (1e-3 * scale + ulp * (np.abs(rdf) + scale))
            edg = np.abs(got_g - rdg) - (1e-3 * scale + ulp * (np.abs(rdg) + scale))
        else:                                                        # test_sixteen_bit_activations / _bf16_case
            ulp = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
            edf = np.abs(got_f - rdf) - (2e-4 * scale * max(1.0, U / 32) + ulp * np.abs(rdf) + 1e-6)
            edg = np.abs(got_g - rdg) - (2e-4 * scale * max(1.0, T / 32) + ulp * np.abs(rdg) + 1e-6)
    assert edf.max() <= 0, (what, "df", edf.max(), np.unravel_index(edf.argmax(), edf.shape))
    assert edg.max() <= 0, (what, "dg", edg.max(), np.unravel_index(edg.argmax(), edg.shape))
    return rdf


def run_loss_case(case, oracle, cus):
    from warprnnt_pytorch import _lib
    lib = _lib.lib()
    N, T, U, A = J.K.case_shape(case, cus)
    dt = TORCH[case["dtype"]]
    f, g, labels, tl, ll, blank = _problem(case, cus)
    fs = torch.tensor(f, dtype=torch.float32).to(dt)                 # stored values: the oracle sees exactly these
    gs = torch.tensor(g, dtype=torch.float32).to(dt)
    off = dict({"f": 0, "g": 0, "df": 0, "dg": 0}, **case.get("off", {}))
    tf = place(_nan_padding(fs, tl, 1).to(DEV), off["f"], dt)
    tg = place(_nan_padding(gs, ll, 2).to(DEV), off["g"], dt)
    df = place(torch.full((N, T, A), float("nan"), dtype=dt), off["df"], dt)
    dg = place(torch.full((N, U, A), float("nan"), dtype=dt), off["dg"], dt)
    t_lab, t_tl, t_ll = (torch.tensor(v, device=DEV) for v in (labels, tl, ll))
    lab_ptr = t_lab.data_ptr() if t_lab.numel() else t_tl.data_ptr()
    costs = torch.full((N,), float("nan"), device=DEV)
    ws = torch.empty(_lib.workspace_bytes_add(T, U, N), dtype=torch.uint8, device=DEV)
    opt = options(T, U, blank)
    sc = _scale(case, N)
    t_sc = torch.tensor(sc, device=DEV) if sc is not None else None
    sc_ptr = t_sc.data_ptr() if t_sc is not None else None
    code = {"f32": _lib.DT_F32, "bf16": _lib.DT_BF16, "f16": _lib.DT_F16}[case["dtype"]]
    lam = case.get("lam", 0.0)
    p = (tf.data_ptr(), tg.data_ptr())
    entry = case["entry"]
    if entry == "add":
        assert sc is None and dt == torch.float32
        call = lambda: lib.compute_rnnt_loss_add(*p, df.data_ptr(), dg.data_ptr(), lab_ptr, t_ll.data_ptr(), t_tl.data_ptr(), A, N,
                                                 costs.data_ptr(), ws.data_ptr(), opt)
    elif entry in ("twophase", "fastemit"):
        assert dt == torch.float32

        def call():
            if entry == "fastemit":
                st = lib.compute_rnnt_loss_add_fwd_fastemit(*p, lab_ptr, t_ll.data_ptr(), t_tl.data_ptr(), A, N, costs.data_ptr(),
                                                            ws.data_ptr(), opt, 1, lam)
            else:
                st = lib.compute_rnnt_loss_add_fwd(*p, lab_ptr, t_ll.data_ptr(), t_tl.data_ptr(), A, N, costs.data_ptr(), ws.data_ptr(),
                                                   opt, 1)
            return st or lib.compute_rnnt_loss_add_bwd(*p, df.data_ptr(), dg.data_ptr(), sc_ptr, lab_ptr, t_ll.data_ptr(),
                                                       t_tl.data_ptr(), A, N, ws.data_ptr(), opt)
    else:
        assert entry == "dt"

        def call():
            st = lib.compute_rnnt_loss_add_fwd_dt(*p, lab_ptr, t_ll.data_ptr(), t_tl.data_ptr(), A, N, costs.data_ptr(), ws.data_ptr(),
                                                  opt, code, 1, 0.0)
            return st or lib.compute_rnnt_loss_add_bwd_dt(*p, df.data_ptr(), dg.data_ptr(), sc_ptr, lab_ptr, t_ll.data_ptr(),
                                                          t_tl.data_ptr(), A, N, ws.data_ptr(), opt, code)
    st, names = profiled(call)
    assert st == 0, (case["name"], st)
    reached = _check_stages(case, names, cus)

    rdf = check_loss(case, oracle, fs, gs, labels, tl, ll, blank, sc, costs.double().cpu().numpy(), df.double().cpu().numpy(),
                     dg.double().cpu().numpy())
    _check_data(case, fs.double().numpy(), gs.double().numpy(), rdf, tl)
    return reached


def _check_data(case, fr, gr, rdf, tl):
    """The stored inputs of a data-dependent case really carry the work its comment in _problem argues for."""
    data, A = case.get("data"), fr.shape[-1]
    if data == "guard":          # rows more than log(FLT_MAX) = 88.7 nats above their first 32 columns (the guard is 27.7)
        assert max((x.max(-1) - x[..., :32].max(-1)).max() for x in (fr, gr)) > 89.0, case["name"]
    elif data == "masked32":
        assert np.isneginf(fr[..., :32]).all() and np.isneginf(gr[..., :32]).all()
    elif data == "far":          # the far sample's gradient mass sits in its peak columns: O(1) per row, from the far cells only
        b = min(1, fr.shape[0] - 1)
        assert np.abs(rdf[b, :tl[b]][:, [3, 40 % A]]).max() > 0.5, case["name"]


# ----------------------------------------------------------------------------- the alignment entries
def _planted(N, T, U, A, rng, margin=4.0):
    """Logits whose best path beats every other by >= 1 nat per decision: a random monotone path gets +margin on the symbol it
    takes at each of its cells (tests/test_gpu_align.py)."""
    acts = np.zeros((N, T, U, A))
    labels = rng.integers(1, A, size=(N, U - 1))
    for b in range(N):
        fr = np.sort(rng.integers(0, T, size=U - 1))
        u = 0
        for t in range(T):
            while u < U - 1 and fr[u] == t:
                acts[b, t, u, labels[b, u]] = margin
                u += 1
            acts[b, t, u, 0] = margin
    return acts, labels.astype(np.int32)


def run_align_case(case, cus):
    from warprnnt_pytorch import _lib
    lib = _lib.lib()
    N, T, U, A = J.K.case_shape(case, cus)
    dt = TORCH[case["dtype"]]
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()))
    planted = case.get("data") == "planted"
    blank = 0
    if planted:
        acts, labels = _planted(N, T, U, A, rng)
        tl, ll = np.full(N, T, np.int32), np.full(N, U - 1, np.int32)
    else:
        tl, ll = ragged_lengths(N, T, U, rng, pair_without_labels=True)
        labels = rng.integers(1, A, size=(N, U - 1)).astype(np.int32)
    score = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
    frames = torch.full((N, max(U - 1, 1)), -7, dtype=torch.int32, device=DEV)
    t_lab, t_tl, t_ll = (torch.tensor(v, device=DEV) for v in (labels, tl, ll))
    opt = options(T, U, blank)
    code = {"f32": _lib.DT_F32, "f64": _lib.DT_F64, "bf16": _lib.DT_BF16, "f16": _lib.DT_F16}[case["dtype"]]
    if case["entry"] == "align_add":
        f = torch.tensor(rng.standard_normal((N, T, A)) * 1.5, dtype=torch.float32).to(dt)
        g = torch.tensor(rng.standard_normal((N, U, A)) * 1.5, dtype=torch.float32).to(dt)
        tf, tg = _nan_padding(f, tl, 1).to(DEV), _nan_padding(g, ll, 2).to(DEV)
        ws = torch.empty(_lib.workspace_bytes_add(T, U, N), dtype=torch.uint8, device=DEV)
        call = lambda: lib.compute_rnnt_align_add(tf.data_ptr(), tg.data_ptr(), t_lab.data_ptr(), t_ll.data_ptr(), t_tl.data_ptr(), A,
                                                  N, score.data_ptr(), frames.data_ptr(), ws.data_ptr(), opt, code)
        z = f.double().numpy()[:, :, None, :] + g.double().numpy()[:, None, :, :]
    else:
        assert not planted or dt in (torch.float32, torch.float64)
        x = torch.tensor(acts if planted else rng.standard_normal((N, T, U, A)), dtype=torch.float32).to(dt)
        xn = x.clone()
        for b in range(N):
            xn[b, tl[b]:] = float("nan")
            xn[b, :, ll[b] + 1:] = float("nan")
        xd = xn.to(DEV)
        esz = torch.finfo(dt).bits // 8
        ws = torch.empty(_lib.workspace_bytes(T, U, N, True, esz), dtype=torch.uint8, device=DEV)
        call = lambda: lib.compute_rnnt_align(xd.data_ptr(), t_lab.data_ptr(), t_ll.data_ptr(), t_tl.data_ptr(), A, N,
                                              score.data_ptr(), frames.data_ptr(), ws.data_ptr(), opt, code)
        z = x.double().numpy()
    st, names = profiled(call)
    assert st == 0, (case["name"], st)
    reached = _check_stages(case, names, cus)
    # no kernel of the additive joint's loss stages in an alignment call
    assert not [n for n in names if J.jstage_of(n) in ("lattice", "coef", "grad")], names

    got_s, got_f = score.cpu().numpy(), frames.cpu().numpy()
    for b in range(N):
        Tb, Ub = int(tl[b]), int(ll[b])
        lp = z[b, :Tb, :Ub + 1]
        lp = lp - lp.max(-1, keepdims=True)
        lp = lp - np.log(np.exp(lp).sum(-1, keepdims=True))          # fp64 log_softmax of the stored values
        s, fr = viterbi_np(lp, labels[b], Tb, Ub, blank)
        f = [int(v) for v in got_f[b, :Ub]]
        assert (got_f[b, Ub:U - 1] == -1).all(), (case["name"], b)
        tol = 1e-4 * max(1.0, abs(s))                                # tests/test_gpu_align.py
        assert np.isfinite(s) and abs(got_s[b] - s) <= tol, (case["name"], b, got_s[b], s)
        assert all(0 <= v < Tb for v in f) and all(f[i] <= f[i + 1] for i in range(Ub - 1)), (case["name"], b)
        assert abs(path_score(lp, labels[b], Tb, Ub, blank, f) - s) <= tol, (case["name"], b)
        if planted:
            assert f == fr, (case["name"], b, [i for i in range(Ub) if f[i] != fr[i]][:10])
    return reached


_REACHED = {}


@pytest.mark.parametrize("name", sorted(J.JCASES))
def test_joint_form(oracle, name):
    case = J.JCASES[name]
    cus = G.cus()
    if case["entry"] in ("align", "align_add"):
        _REACHED[name] = run_align_case(case, cus)
    else:
        _REACHED[name] = run_loss_case(case, oracle, cus)


def test_every_joint_row_reached_on_this_device():
    """Every row of the inventory: its case, run above, launched its kernel on this device (printed as the coverage table)."""
    if len(_REACHED) < len(J.JCASES):
        pytest.skip("needs the whole matrix in this session")
    lines = []
    for obj, kernel, case in J.FORMS:
        assert kernel in _REACHED[case], (kernel, case, _REACHED[case])
        lines.append("%-10s %-66s %s" % (obj, kernel, case))
    print("\n".join(lines))
