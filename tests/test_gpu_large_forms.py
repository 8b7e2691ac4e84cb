"""-m gpu: every row of tests/large_forms.py -- the materialised path's statistics and gradient forms, the additive joint's
partition and gradient forms (f / df or g / dg past 2^31 elements, the W | CB | CL planes past 2^31 elements), the cell tables
and both alignments past 2^31 elements / 2^32 bytes.  Per row: the base block is generated on the host (small), copied to the device and
broadcast into the big tensor there; padded activations hold NaN in their padding, gradients start as NaN (every in-lattice
element must be written).  The call runs under torch.profiler and the kernels of each stage must be the predicted ones at this
device's compute-unit count.  Copy 0, every copy holding a boundary and the last copy are compared with the fp64 oracle (costs,
every gradient element at oracle.grad_bound; joint: df = sum_u dz and dg = sum_t dz of the oracle on z = f + g, at the bounds of
tests/test_gpu_joint_forms.py; alignments: the numpy Viterbi); every other copy must be bit-identical to copy 0
(costs, gradients, scores, frames: compared on the device, slab by slab; the joint's atomically accumulated df / dg: within
rounding, _close_to_copy0); gradient padding must be exact zeros and every row of
the whole (materialised) gradient tensor must sum to zero within oracle.rowsum_bound.  The block's period (2^p x odd bytes) makes a wrapped
32-bit offset read a different position of the block, which these comparisons see."""
import zlib

import numpy as np
import pytest
import torch

from tests import gpu_support as G
from tests import joint_forms as J
from tests import kernel_forms as K
from tests import large_forms as L
from tests.align_ref import path_score, viterbi_np
from tests.gpu_support import CALL, DEV, TORCH, assert_stages, profiled, stages_seen

pytestmark = pytest.mark.gpu

_INT = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16, torch.float16: torch.int16}
SLAB = 1 << 30                         # bytes of one device-side comparison slab


def _free():
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _block(row):
    """Host block: stored activations (K, T, U, A) with NaN padding, labels, lengths, per-sample scales."""
    k, T, U, A = row["K"], row["T"], row["U"], row["A"]
    rng = np.random.default_rng(zlib.crc32(row["name"].encode()) + 1)
    dt = TORCH[row["dtype"]]
    x = torch.tensor(rng.standard_normal((k, T, U, A)) * 1.5, dtype=torch.float32).to(dt)
    tl, ll = L.block_lengths(row)
    labels = rng.integers(1, A, size=(k, U - 1)).astype(np.int32)
    sc = None
    if row.get("scale"):
        sc = (0.5 + 0.6 * (np.arange(k) % 5)).astype(np.float64 if dt == torch.float64 else np.float32)
    return x, labels, tl, ll, sc


def _slabs(n, per_bytes):
    step = max(1, SLAB // per_bytes)
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def _same_as_copy0(t, copies, what):
    """Every copy of `t` (a contiguous (copies, ...) tensor) bit-identical to copy 0, compared on the device."""
    v = t.reshape(copies, -1)
    if v.is_floating_point():
        v = v.view(_INT[v.dtype])
    ref = v[0:1]
    for a, b in _slabs(copies, v.shape[1] * v.element_size()):
        bad = (v[a:b] != ref).any(dim=1)
        if bool(bad.any()):
            c = a + int(bad.nonzero()[0, 0])
            raise AssertionError("%s: copy %d differs from copy 0" % (what, c))


def _close_to_copy0(t, copies, what, scale, span):
    """Every copy of `t` within rounding of copy 0 (|x_c - x_0| <= r x (scale x max(1, span / 32) + |x_0|), r = 2e-5 for fp32,
    two storage ulps for 16-bit; a NaN anywhere fails), compared on the device: for the joint's df / dg, which joint_far*_kernel
    and the split contractions accumulate with unsafeAtomicAdd (rnnt_joint_kernels.h) -- the order of those additions, and so
    the last bits, can differ from run to run even for one copy (fp32 rows did: 8 of 16 on one MI355X).  A truncated offset
    reads another row of the block (an O(1) difference) or leaves the NaN sentinel."""
    v = t.reshape(copies, -1)
    ref = v[0:1].float()
    r = {torch.float32: 2e-5, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}[v.dtype]
    for a, b in _slabs(copies, v.shape[1] * 12):
        ok = (v[a:b].float() - ref).abs() <= r * (scale * max(1.0, span / 32) + ref.abs())
        bad = ~ok.all(dim=1)
        if bool(bad.any()):
            c = a + int(bad.nonzero()[0, 0])
            raise AssertionError("%s: copy %d differs from copy 0 beyond rounding" % (what, c))


def _rowsum_ratio(g, A, oracle, dt):
    """max over every row of the gradient tensor of |sum_v g_v| / oracle.rowsum_bound."""
    rows = g.reshape(-1, A)
    acc = torch.float64 if dt == torch.float64 else torch.float32
    worst = 0.0
    for a, b in _slabs(rows.shape[0], A * rows.element_size() * 4):
        r = rows[a:b].to(acc)
        worst = max(worst, (r.sum(-1).abs() / oracle.rowsum_bound(r.abs().sum(-1), dt, n_cols=A)).max().item())
    return worst


def _stages(row, names, cus):
    want = L.predicted(row, cus)
    assert_stages(row["name"], stages_seen(names, lambda n: K.stage_of(n) or J.jstage_of(n)), want)
    if want.get("coef"):    # the cell-per-thread kernel (maxU <= 48) runs in groups (launch_coef); the tiled one in one launch here
        ncoef = sum(1 for n in names if K.stage_of(n) == "coef")
        assert ncoef == (1 if row["U"] > 48 else K.coef_launches(L.case_of(row), cus)), (row["name"], ncoef)


def run_row(row, oracle, cus):
    from warprnnt_pytorch import _lib
    lib = _lib.lib()
    dt = TORCH[row["dtype"]]
    code, esz = {torch.float32: (_lib.DT_F32, 4), torch.float64: (_lib.DT_F64, 8), torch.bfloat16: (_lib.DT_BF16, 2),
                 torch.float16: (_lib.DT_F16, 2)}[dt]
    cdt = torch.float64 if dt == torch.float64 else torch.float32
    k, T, U, A, n = row["K"], row["T"], row["U"], row["A"], row["copies"]
    N = k * n
    ws_bytes = _lib.workspace_bytes(T, U, N, True, esz)
    need = L.peak_bytes(row, ws_bytes) + (2 << 30)
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < need:
        pytest.skip("%s needs %.1f GB, %.1f GB free" % (row["name"], need / 1e9, free / 1e9))
    x, labels, tl, ll, sc = _block(row)
    packed = row.get("layout") == "packed"
    entry = row["entry"]
    xb = x.clone()
    if not packed:
        for b in range(k):                                           # NaN in every padded row: must never be read
            xb[b, tl[b]:] = float("nan"); xb[b, :, ll[b] + 1:] = float("nan")
        blk = xb.reshape(-1)
    else:
        blk = torch.cat([x[b, :tl[b], :ll[b] + 1].reshape(-1) for b in range(k)])
    per = blk.numel()
    # the device tensors: the block broadcast copies times
    t_lab = torch.tensor(labels, device=DEV).repeat(n, 1)
    t_tl = torch.tensor(tl, device=DEV).repeat(n)
    t_ll = torch.tensor(ll, device=DEV).repeat(n)
    lab_ptr = t_lab.data_ptr()
    dblk = blk.to(DEV)
    misalign = row.get("misalign")
    xbuf = torch.empty(per * n, dtype=dt, device=DEV)
    xbuf.view(n, per).copy_(dblk.view(1, per).expand(n, per))
    del dblk
    if entry == "align":
        g = None
    elif row.get("inplace"):
        g = xbuf
    elif misalign:                                                   # grads at another 16-byte phase than acts
        gbuf = torch.full((per * n + 1,), float("nan"), dtype=dt, device=DEV)
        g = gbuf[1:]
        assert (g.data_ptr() ^ xbuf.data_ptr()) & 15
    else:
        g = torch.full_like(xbuf, float("nan"))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    opt = _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=torch.cuda.current_stream().cuda_stream, blank_label=0,
                           maxT=T, maxU=U, batch_first=True)
    t_sc = torch.tensor(np.tile(sc, n), device=DEV) if sc is not None else None
    sc_ptr = t_sc.data_ptr() if t_sc is not None else None
    costs = torch.zeros(N, dtype=cdt, device=DEV)
    xp, gp = xbuf.data_ptr(), (g.data_ptr() if g is not None else None)
    keep = []
    if entry == "align":
        score = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
        frames = torch.full((N, max(U - 1, 1)), -7, dtype=torch.int32, device=DEV)
        call = lambda: lib.compute_rnnt_align(xp, lab_ptr, t_ll.data_ptr(), t_tl.data_ptr(), A, N, score.data_ptr(),
                                              frames.data_ptr(), ws.data_ptr(), opt, code)
    elif packed:
        from warprnnt_pytorch.packed import row_offsets
        offs = row_offsets(t_tl, t_ll)
        rows = per * n // A
        assert int(offs[-1]) == rows
        if entry == "packed":
            call = lambda: lib.compute_rnnt_loss_packed(xp, gp, lab_ptr, t_ll.data_ptr(), t_tl.data_ptr(), offs.data_ptr(), rows, A, N,
                                                        costs.data_ptr(), sc_ptr, ws.data_ptr(), opt, code, 0.0)
        else:
            def call():
                st = lib.compute_rnnt_loss_packed_fwd(xp, lab_ptr, t_ll.data_ptr(), t_tl.data_ptr(), offs.data_ptr(), rows, A, N,
                                                      costs.data_ptr(), ws.data_ptr(), opt, code, 1, 0.0)
                return st or lib.compute_rnnt_loss_packed_bwd(xp, gp, sc_ptr, offs.data_ptr(), rows, A, N, ws.data_ptr(), opt, code)
    elif entry == "call":
        assert sc is None
        host = np.zeros(N, dtype=np.float64 if dt == torch.float64 else np.float32)
        keep.append(host)

        def call():
            st = getattr(lib, CALL[row["dtype"]])(xp, gp, lab_ptr, t_ll.data_ptr(), t_tl.data_ptr(), A, N, host.ctypes.data,
                                                   ws.data_ptr(), opt)
            costs.copy_(torch.from_numpy(host))
            return st
    elif entry == "async":
        call = lambda: lib.compute_rnnt_loss_async(xp, gp, lab_ptr, t_ll.data_ptr(), t_tl.data_ptr(), A, N, costs.data_ptr(), sc_ptr,
                                                   ws.data_ptr(), opt, code)
    else:
        assert entry == "twophase"

        def call():
            st = lib.compute_rnnt_loss_fwd(xp, lab_ptr, t_ll.data_ptr(), t_tl.data_ptr(), A, N, costs.data_ptr(), ws.data_ptr(), opt,
                                           code, 1)
            return st or lib.compute_rnnt_loss_bwd(xp, gp, sc_ptr, A, N, ws.data_ptr(), opt, code)
    st, names = profiled(call)
    assert st == 0, (row["name"], st)
    _stages(row, names, cus)
    del ws
    checked = L.checked_copies(row)
    xs = x.double().numpy()
    if entry == "align":
        _same_as_copy0(score, n, row["name"] + " score")
        _same_as_copy0(frames, n, row["name"] + " frames")
        got_s = score.view(n, k).cpu().numpy()
        got_f = frames.view(n, k, -1).cpu().numpy()
        for b in range(k):
            Tb, Ub = int(tl[b]), int(ll[b])
            lp = xs[b, :Tb, :Ub + 1]
            lp = lp - lp.max(-1, keepdims=True)
            lp = lp - np.log(np.exp(lp).sum(-1, keepdims=True))
            s, _ = viterbi_np(lp, labels[b], Tb, Ub, 0)
            tol = 1e-4 * max(1.0, abs(s))
            for c in checked:
                f = [int(v) for v in got_f[c, b, :Ub]]
                assert (got_f[c, b, Ub:U - 1] == -1).all(), (row["name"], c, b)
                assert abs(got_s[c, b] - s) <= tol, (row["name"], c, b, got_s[c, b], s)
                assert all(0 <= v < Tb for v in f) and all(f[i] <= f[i + 1] for i in range(Ub - 1)), (row["name"], c, b)
                assert abs(path_score(lp, labels[b], Tb, Ub, 0, f) - s) <= tol, (row["name"], c, b)
        return names
    # costs and gradients: every copy bit-identical to copy 0, the checked copies against the oracle
    _same_as_copy0(costs, n, row["name"] + " costs")
    _same_as_copy0(g.view(n, per), n, row["name"] + " grads")
    ref_c, ref_g, mag = oracle.rnnt_logits(xs, labels, tl, ll, want_mag=True)
    for b in range(k):
        ref_g[b, tl[b]:] = 0; ref_g[b, :, ll[b] + 1:] = 0
        mag[b, tl[b]:] = 0; mag[b, :, ll[b] + 1:] = 0
    s = np.ones(k) if sc is None else sc.astype(np.float64)
    ref_g *= s[:, None, None, None]
    mag *= s[:, None, None, None]
    got_c = costs.view(n, k).double().cpu().numpy()
    ctol = 1e-9 if dt == torch.float64 else 1e-4
    for c in checked:
        assert np.abs(got_c[c] - ref_c).max() <= ctol * max(1.0, np.abs(ref_c).max()), (row["name"], c, got_c[c], ref_c)
        gc_ = g.view(n, per)[c].double().cpu()
        if packed:
            got = np.zeros_like(xs)
            o = 0
            for b in range(k):
                r = int(tl[b]) * (int(ll[b]) + 1) * A
                got[b, :tl[b], :ll[b] + 1] = gc_[o:o + r].view(int(tl[b]), int(ll[b]) + 1, A).numpy()
                o += r
        else:
            got = gc_.view(k, T, U, A).numpy()
            for b in range(k):                                      # gradient padding: exact zeros
                assert not got[b, tl[b]:].any() and not got[b, :, ll[b] + 1:].any(), (row["name"], c, b)
        oracle.assert_grads(got, ref_g, mag, dt, scale=float(s.max()), what="%s copy %d" % (row["name"], c))
    worst = _rowsum_ratio(g, A, oracle, dt)
    assert worst <= 1.0, (row["name"], worst)
    return names


def _joint_view(blk, n, off, dt):
    """blk (host) repeated n times on the device, `off` bytes past a 16-byte boundary (a view into a slightly larger buffer)."""
    e = torch.finfo(dt).bits // 8
    m = blk.numel() * n
    buf = torch.empty(m + 32 // e, dtype=dt, device=DEV)
    base = (-buf.data_ptr() % 16) // e + off // e
    v = buf[base:base + m]
    assert v.data_ptr() % 16 == off
    dblk = blk.reshape(1, -1).to(DEV)
    v.view(n, -1).copy_(dblk.expand(n, -1))
    return v


def _viterbi_check(row, z, labels, tl, ll, got_s, got_f, checked):
    k, U = row["K"], row["U"]
    for b in range(k):
        Tb, Ub = int(tl[b]), int(ll[b])
        lp = z[b, :Tb, :Ub + 1]
        lp = lp - lp.max(-1, keepdims=True)
        lp = lp - np.log(np.exp(lp).sum(-1, keepdims=True))
        s, _ = viterbi_np(lp, labels[b], Tb, Ub, 0)
        tol = 1e-4 * max(1.0, abs(s))
        for c in checked:
            f = [int(v) for v in got_f[c, b, :Ub]]
            assert (got_f[c, b, Ub:U - 1] == -1).all(), (row["name"], c, b)
            assert abs(got_s[c, b] - s) <= tol, (row["name"], c, b, got_s[c, b], s)
            assert all(0 <= v < Tb for v in f) and all(f[i] <= f[i + 1] for i in range(Ub - 1)), (row["name"], c, b)
            assert abs(path_score(lp, labels[b], Tb, Ub, 0, f) - s) <= tol, (row["name"], c, b)


def run_joint_row(row, oracle, cus):
    from warprnnt_pytorch import _lib
    lib = _lib.lib()
    dt = TORCH[row["dtype"]]
    code = {"f32": _lib.DT_F32, "bf16": _lib.DT_BF16, "f16": _lib.DT_F16}[row["dtype"]]
    k, T, U, A, n = row["K"], row["T"], row["U"], row["A"], row["copies"]
    N = k * n
    need = L.joint_peak(row) + (2 << 30)
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < need:
        pytest.skip("%s needs %.1f GB, %.1f GB free" % (row["name"], need / 1e9, free / 1e9))
    rng = np.random.default_rng(zlib.crc32(row["name"].encode()) + 1)
    fs = torch.tensor(rng.standard_normal((k, T, A)) * 1.5, dtype=torch.float32).to(dt)    # stored values: the oracle's input
    gs = torch.tensor(rng.standard_normal((k, U, A)) * 1.5, dtype=torch.float32).to(dt)
    tl, ll = L.block_lengths(row)
    labels = rng.integers(1, A, size=(k, U - 1)).astype(np.int32)
    fn, gn = fs.clone(), gs.clone()
    for b in range(k):                                               # padded rows of f (t >= T_b) and g (u > U_b - 1): NaN
        fn[b, tl[b]:] = float("nan"); gn[b, ll[b] + 1:] = float("nan")
    off = dict({"f": 0, "g": 0, "df": 0, "dg": 0}, **row.get("off", {}))
    tf, tg = _joint_view(fn, n, off["f"], dt), _joint_view(gn, n, off["g"], dt)
    t_lab = torch.tensor(labels, device=DEV).repeat(n, 1)
    t_tl, t_ll = torch.tensor(tl, device=DEV).repeat(n), torch.tensor(ll, device=DEV).repeat(n)
    ws = torch.empty(_lib.workspace_bytes_add(T, U, N), dtype=torch.uint8, device=DEV)
    opt = _lib.rnntOptions(loc=_lib.RNNT_GPU, num_threads=0, stream=torch.cuda.current_stream().cuda_stream, blank_label=0,
                           maxT=T, maxU=U, batch_first=True)
    a = (tf.data_ptr(), tg.data_ptr())
    lens = (t_lab.data_ptr(), t_ll.data_ptr(), t_tl.data_ptr())
    z = fs.double().numpy()[:, :, None, :] + gs.double().numpy()[:, None, :, :]
    checked = L.checked_copies(row)
    entry = row["entry"]
    if entry == "align_add":
        score = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
        frames = torch.full((N, max(U - 1, 1)), -7, dtype=torch.int32, device=DEV)
        st, names = profiled(lambda: lib.compute_rnnt_align_add(*a, *lens, A, N, score.data_ptr(), frames.data_ptr(), ws.data_ptr(),
                                                                 opt, code))
        assert st == 0, (row["name"], st)
        _stages(row, names, cus)
        _same_as_copy0(score, n, row["name"] + " score")
        _same_as_copy0(frames, n, row["name"] + " frames")
        _viterbi_check(row, z, labels, tl, ll, score.view(n, k).cpu().numpy(), frames.view(n, k, -1).cpu().numpy(), checked)
        return names
    df = _joint_view(torch.full((k, T, A), float("nan"), dtype=dt), n, off["df"], dt)
    dg = _joint_view(torch.full((k, U, A), float("nan"), dtype=dt), n, off["dg"], dt)
    costs = torch.full((N,), float("nan"), device=DEV)
    sc = (0.5 + 0.6 * (np.arange(k) % 5)).astype(np.float32) if row.get("scale") else None
    t_sc = torch.tensor(np.tile(sc, n), device=DEV) if sc is not None else None
    sc_ptr = t_sc.data_ptr() if t_sc is not None else None
    g2 = (df.data_ptr(), dg.data_ptr())
    if entry == "add":
        assert sc is None and dt == torch.float32
        call = lambda: lib.compute_rnnt_loss_add(*a, *g2, *lens, A, N, costs.data_ptr(), ws.data_ptr(), opt)
    elif entry == "twophase":
        def call():
            st = lib.compute_rnnt_loss_add_fwd(*a, *lens, A, N, costs.data_ptr(), ws.data_ptr(), opt, 1)
            return st or lib.compute_rnnt_loss_add_bwd(*a, *g2, sc_ptr, *lens, A, N, ws.data_ptr(), opt)
    else:
        assert entry == "dt"

        def call():
            st = lib.compute_rnnt_loss_add_fwd_dt(*a, *lens, A, N, costs.data_ptr(), ws.data_ptr(), opt, code, 1, 0.0)
            return st or lib.compute_rnnt_loss_add_bwd_dt(*a, *g2, sc_ptr, *lens, A, N, ws.data_ptr(), opt, code)
    st, names = profiled(call)
    assert st == 0, (row["name"], st)
    _stages(row, names, cus)
    del ws
    _same_as_copy0(costs, n, row["name"] + " costs")
    wmax = 1.0 if sc is None else float(sc.max())      # df / dg are accumulated atomically: see _close_to_copy0
    _close_to_copy0(df.view(n, -1), n, row["name"] + " df", wmax, U)
    _close_to_copy0(dg.view(n, -1), n, row["name"] + " dg", wmax, T)
    ref_c, ref_gz = oracle.rnnt_logits(z, labels, tl, ll, 0)
    for b in range(k):
        ref_gz[b, tl[b]:] = 0
        ref_gz[b, :, ll[b] + 1:] = 0
    w = np.ones(k) if sc is None else sc.astype(np.float64)
    rdf = ref_gz.sum(axis=2) * w[:, None, None]
    rdg = ref_gz.sum(axis=1) * w[:, None, None]
    del ref_gz
    big = max(1.0, np.abs(ref_c).max())
    scale = float(np.abs(w).max())
    got_c = costs.view(n, k).double().cpu().numpy()
    for c in checked:                                    # the bounds of tests/test_gpu_joint_forms.py (plain random data)
        what = "%s copy %d" % (row["name"], c)
        got_f = df.view(n, k, T, A)[c].double().cpu().numpy()
        got_g = dg.view(n, k, U, A)[c].double().cpu().numpy()
        assert np.isfinite(got_c[c]).all() and np.isfinite(got_f).all() and np.isfinite(got_g).all(), what
        for b in range(k):                               # gradient padding: every element written, exactly zero
            assert not got_f[b, tl[b]:].any() and not got_g[b, ll[b] + 1:].any(), (what, b)
        assert np.abs(got_c[c] - ref_c).max() <= 1e-4 * big, (what, got_c[c], ref_c)
        ulp = 0.0 if dt == torch.float32 else 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
        rel, absf = (5e-5, 0.0) if dt == torch.float32 else (ulp, 1e-6)
        edf = np.abs(got_f - rdf) - (2e-4 * scale * max(1.0, U / 32) + rel * np.abs(rdf) + absf)
        edg = np.abs(got_g - rdg) - (2e-4 * scale * max(1.0, T / 32) + rel * np.abs(rdg) + absf)
        assert edf.max() <= 0, (what, "df", edf.max(), np.unravel_index(edf.argmax(), edf.shape))
        assert edg.max() <= 0, (what, "dg", edg.max(), np.unravel_index(edg.argmax(), edg.shape))
    return names


_REACHED = {}


@pytest.mark.parametrize("name", sorted(L.ROWS))
def test_large_form(oracle, name):
    row = L.ROWS[name]
    try:
        names = (run_joint_row if row.get("joint") else run_row)(row, oracle, G.cus())
    finally:
        _free()
    _REACHED[name] = sorted({n for n in names if K.stage_of(n) or J.jstage_of(n)})


def test_every_large_kernel_reached_on_this_device():
    """Every stats / grad (materialised) and partition / grad (joint) kernel of the inventory ran past 2^31 elements on this
    device (printed as the coverage table)."""
    if len(_REACHED) < len(L.ROWS):
        pytest.skip("needs the whole table in this session")
    lines = []
    for (obj, kernel), rows in sorted(L.covered(G.cus()).items()):
        assert any(kernel in _REACHED[r] for r in rows), (kernel, rows)
        lines.append("%-10s %-66s %s" % (obj, kernel, ", ".join(rows)))
    print("\n".join(lines))
