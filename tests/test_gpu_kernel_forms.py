"""-m gpu: every kernel form of the materialised path, one case per row of tests/kernel_forms.py.  Each case runs its entry
(one-call, async, two-phase, packed, packed two-phase) under torch.profiler, and the kernels recorded for each stage must be
exactly the one the release rules predict (kernel_forms.predict, with this device's compute-unit count).  Costs and
every gradient element are then compared with the fp64 oracle at the per-dtype bounds of oracle.grad_bound, and the
likelihoods kept in the workspace with the costs.  Lengths are ragged, one sample has T_b = 1 (U_b = 1 where the layout allows
it), and the padding of padded-layout activations holds NaN, which must never be read."""
import zlib

import numpy as np
import pytest
import torch

from tests import gpu_support as G
from tests import kernel_forms as K
from tests.gpu_support import CALL, TORCH, assert_stages, profiled, stages_seen

pytestmark = pytest.mark.gpu


def test_profiler_records_kernel_names():
    """The observation the matrix rests on: kineto on this build reports device kernels by name."""
    from warprnnt_pytorch import warp_rnnt
    dev = torch.device("cuda:0")
    x = torch.randn(2, 3, 3, 5, device=dev)
    lab = torch.ones(2, 2, dtype=torch.int32, device=dev)
    tl = torch.full((2,), 3, dtype=torch.int32, device=dev)
    ll = torch.full((2,), 2, dtype=torch.int32, device=dev)
    _, names = profiled(lambda: warp_rnnt.gpu_rnnt_async(x, lab, tl, ll, torch.zeros(2, device=dev), torch.zeros_like(x), 0))
    assert any(K.stage_of(n) == "lattice" for n in names), names


def _inputs(case, cus, rng):
    N, T, U, A = K.case_shape(case, cus)
    d = case["dtype"]
    x64 = rng.standard_normal((N, T, U, A))
    x = torch.tensor(x64, dtype=TORCH[d])                          # stored values; the oracle sees exactly these
    labels = rng.integers(1, A, size=(N, max(U - 1, 0))).astype(np.int32) if A > 1 else np.zeros((N, U - 1), np.int32)
    tl = rng.integers(1, T + 1, size=N).astype(np.int32)
    ll = rng.integers(0, U, size=N).astype(np.int32)
    tl[0], ll[0] = T, U - 1                                          # one full sample: maxT / maxU are used
    if N > 1:
        tl[1] = 1                                                    # T_b = 1
    if N > 2:
        ll[2] = 0                                                    # U_b = 1
    blank = 0
    return x, labels, tl, ll, blank


def _scale(case, N, dtype):
    if case.get("scale") is None:
        return None
    return (0.5 + 0.6 * (np.arange(N) % 5)).astype(np.float64 if dtype == torch.float64 else np.float32)   # non-uniform


def run_case(case, oracle, cus):
    from warprnnt_pytorch import _lib
    from warprnnt_pytorch.packed import pack_joint, row_offsets
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()))
    N, T, U, A = K.case_shape(case, cus)
    x, labels, tl, ll, blank = _inputs(case, cus, rng)
    dt = TORCH[case["dtype"]]
    code, esz = {torch.float32: (_lib.DT_F32, 4), torch.float64: (_lib.DT_F64, 8), torch.bfloat16: (_lib.DT_BF16, 2),
                 torch.float16: (_lib.DT_F16, 2)}[dt]
    cdt = torch.float64 if dt == torch.float64 else torch.float32
    sc = _scale(case, N, dt)
    xs = x.double().numpy()
    ref_c, ref_g, mag = oracle.rnnt_logits(xs, labels, tl, ll, blank=blank, want_mag=True)
    for b in range(N):                                               # the gradient of padding is 0
        ref_g[b, tl[b]:] = 0; ref_g[b, :, ll[b] + 1:] = 0
        mag[b, tl[b]:] = 0; mag[b, :, ll[b] + 1:] = 0
    t_lab, t_tl, t_ll = (torch.tensor(v, device=dev) for v in (labels, tl, ll))
    ws = torch.empty(_lib.workspace_bytes(T, U, N, True, esz), dtype=torch.uint8, device=dev)
    opt = _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=torch.cuda.current_stream(dev).cuda_stream, blank_label=blank,
                           maxT=T, maxU=U, batch_first=True)
    t_sc = torch.tensor(sc, device=dev) if sc is not None else None
    sc_ptr = t_sc.data_ptr() if t_sc is not None else None
    costs = torch.zeros(N, dtype=cdt, device=dev)
    entry = case["entry"]
    keep = []
    if case.get("layout") == "packed":
        xd = x.to(dev)
        p = pack_joint(xd, t_tl, t_ll).contiguous()
        offs = row_offsets(t_tl, t_ll)
        rows = p.shape[0]
        g = torch.full_like(p, float("nan"))
        if entry == "packed":
            call = lambda: lib.compute_rnnt_loss_packed(p.data_ptr(), g.data_ptr(), t_lab.data_ptr(), t_ll.data_ptr(), t_tl.data_ptr(),
                                                        offs.data_ptr(), rows, A, N, costs.data_ptr(), sc_ptr, ws.data_ptr(), opt, code, 0.0)
        else:
            def call():
                st = lib.compute_rnnt_loss_packed_fwd(p.data_ptr(), t_lab.data_ptr(), t_ll.data_ptr(), t_tl.data_ptr(), offs.data_ptr(),
                                                      rows, A, N, costs.data_ptr(), ws.data_ptr(), opt, code, 1, 0.0)
                return st or lib.compute_rnnt_loss_packed_bwd(p.data_ptr(), g.data_ptr(), sc_ptr, offs.data_ptr(), rows, A, N,
                                                              ws.data_ptr(), opt, code)
    else:
        xn = x.clone()
        for b in range(N):                                           # NaN in every padded row: must never be read
            xn[b, tl[b]:] = float("nan"); xn[b, :, ll[b] + 1:] = float("nan")
        xd = xn.to(dev)
        if case.get("misalign"):                                     # grads at another 16-byte phase than acts
            buf = torch.full((xd.numel() + 1,), float("nan"), dtype=dt, device=dev)
            g = buf[1:].view(xd.shape)
            assert (g.data_ptr() ^ xd.data_ptr()) & 15
        else:
            g = torch.full_like(xd, float("nan"))
        if entry == "call":
            assert sc is None
            host = np.zeros(N, dtype=np.float64 if dt == torch.float64 else np.float32)
            keep.append(host)

            def call():
                st = getattr(lib, CALL[case["dtype"]])(xd.data_ptr(), g.data_ptr(), t_lab.data_ptr(), t_ll.data_ptr(), t_tl.data_ptr(),
                                                         A, N, host.ctypes.data, ws.data_ptr(), opt)
                costs.copy_(torch.from_numpy(host))
                return st
        elif entry == "async":
            call = lambda: lib.compute_rnnt_loss_async(xd.data_ptr(), g.data_ptr(), t_lab.data_ptr(), t_ll.data_ptr(), t_tl.data_ptr(),
                                                       A, N, costs.data_ptr(), sc_ptr, ws.data_ptr(), opt, code)
        else:
            def call():
                st = lib.compute_rnnt_loss_fwd(xd.data_ptr(), t_lab.data_ptr(), t_ll.data_ptr(), t_tl.data_ptr(), A, N, costs.data_ptr(),
                                               ws.data_ptr(), opt, code, 1)
                return st or lib.compute_rnnt_loss_bwd(xd.data_ptr(), g.data_ptr(), sc_ptr, A, N, ws.data_ptr(), opt, code)
    from warprnnt_pytorch import warp_rnnt
    aux = torch.cuda.Stream(dev) if case.get("aux") else None
    if aux is not None:
        warp_rnnt.set_aux_stream(aux)
    try:
        st, names = profiled(call)
    finally:
        if aux is not None:
            warp_rnnt.set_aux_stream(None)
    assert st == 0, (case["name"], st)

    # 1. the forms that ran
    want = K.predict(case, cus)
    assert_stages(case["name"], stages_seen(names, K.stage_of, K.STAGES), want)
    ncoef = sum(1 for n in names if K.stage_of(n) == "coef")
    assert ncoef == K.coef_launches(case, cus) * (2 if case.get("aux") else 1) or not want.get("coef"), (case["name"], ncoef)

    # 2. costs and gradients against the oracle
    got_c = costs.double().cpu().numpy()
    ctol = 1e-9 if dt == torch.float64 else 1e-4
    assert np.abs(got_c - ref_c).max() <= ctol * max(1.0, np.abs(ref_c).max()), (case["name"], got_c, ref_c)
    if case.get("layout") == "packed":
        o = offs.cpu().numpy()
        gp = g.double().cpu()
        got = np.zeros_like(xs)
        for b in range(N):
            got[b, :tl[b], :ll[b] + 1] = gp[o[b]:o[b + 1]].view(int(tl[b]), int(ll[b]) + 1, A).numpy()
    else:
        got = g.double().cpu().numpy()
    s = np.ones(N) if sc is None else sc.astype(np.float64)
    rel = 1e-3 if esz == 2 and T + U - 1 > 500 else None          # (oracle.py: long lattices in 16-bit storage)
    oracle.assert_grads(got, ref_g * s[:, None, None, None], mag * s[:, None, None, None], dt, rel=rel, scale=float(s.max()),
                        what=case["name"])

    # 3. the likelihoods the workspace keeps
    llf, llb = np.zeros(N), np.zeros(N)
    assert lib.compute_rnnt_loss_likelihoods(ws.data_ptr(), N, opt, code, llf.ctypes.data, llb.ctypes.data) == 0
    big = max(1.0, np.abs(ref_c).max())
    assert np.abs(llf + got_c).max() <= ctol * big, (case["name"], llf, got_c)
    assert np.abs(llf - llb).max() <= (1e-9 if dt == torch.float64 else 1e-5) * big, (case["name"], llf, llb)
    return names


_REACHED = {}


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_form(oracle, name):
    case = K.CASES[name]
    cus = G.cus()
    names = run_case(case, oracle, cus)
    _REACHED[name] = sorted({n for n in names if K.stage_of(n)})


def test_every_row_reached_on_this_device():
    """Every row of the inventory: its case, run above, launched its kernel on this device (printed as the coverage table)."""
    if len(_REACHED) < len(K.CASES):
        pytest.skip("needs the whole matrix in this session")
    lines = []
    for obj, kernel, case in K.FORMS:
        assert kernel in _REACHED[case], (kernel, case, _REACHED[case])
        lines.append("%-4s %-58s %s" % (obj, kernel, case))
    print("\n".join(lines))
