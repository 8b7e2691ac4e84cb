"""What the tests of the side libraries (pruned, TDT, HAT) hold a result to, without a GPU: the in-lattice mask, one
cost-and-gradient checker and the comparison of the kernels seen per stage with the predicted ones.  numpy only, so that
tests/test_side_check.py can plant faults and see each one refused; tests/gpu_support.py re-exports the names."""
import numpy as np

from oracle import oracle as O

COST_TOL = {"f64": 1e-9, "f32": 1e-5, "bf16": 1e-5, "f16": 1e-5}
_BOUND_DTYPE = {"f32": "float32", "f64": "float64", "bf16": "bfloat16", "f16": "float16"}     # oracle.grad_bound's names


def in_lattice_mask(shape, act_lens, label_lens):
    """(N, T, U) bool: rows t < T_b, u <= L_b."""
    N, T, U = shape[:3]
    m = np.zeros((N, T, U), bool)
    for b in range(N):
        m[b, :int(act_lens[b]), :int(label_lens[b]) + 1] = True
    return m


def check(dtype, got_c, got_g, ref_c, ref_g, mask, mag_of, scale=None, what="", infinite_ok=True, diagonals=0):
    """Costs and gradients of one call against the fp64 reference.

    +inf costs position for position (infinite_ok=False: the library has no sample without a path, a +inf in the reference
    fails and every cost goes through allclose); finite costs at COST_TOL; padding gradients exact zeros; a sample without a
    path all-NaN inside its lattice; every other sample per element at oracle.grad_bound.  mag_of(ref, b) -> the size of the
    terms of every element of ref = ref_g[b:b + 1] (scaled), the library's own rule.  diagonals = T + maxU - 1: 16-bit storage
    past ~500 of them passes rel=1e-3, the fp32 lattice's own error (oracle.py).  got_g None: costs only."""
    w = np.ones(len(ref_c)) if scale is None else np.asarray(scale, np.float64)
    fin = np.isfinite(ref_c)
    tol = COST_TOL[dtype]
    if fin.any():
        print(what, "max |dcost| = %.3e" % np.abs(got_c[fin] - ref_c[fin]).max())
    assert np.array_equal(np.isposinf(got_c), np.isposinf(ref_c)), (what, got_c, ref_c)
    assert infinite_ok or fin.all(), (what, ref_c)
    assert np.allclose(got_c[fin], ref_c[fin], rtol=tol, atol=tol), (what, got_c, ref_c)
    if got_g is None:
        return
    assert not got_g[~mask].any(), (what, "padding must be exact zeros")
    worst = 0.0
    for b in range(len(ref_c)):
        m = mask[b]
        if not fin[b]:
            assert np.isnan(got_g[b][m]).all(), (what, b, "no path: NaN in-lattice gradients")
            continue
        ref = ref_g[b:b + 1] * w[b]
        mag = mag_of(ref, b)[0][m]
        rel = 1e-3 if dtype in ("bf16", "f16") and diagonals > 500 else None
        r = O.grad_check(got_g[b][m], ref[0][m], mag, _BOUND_DTYPE[dtype], rel=rel)
        worst = max(worst, r["max_err_over_quantum"])
        assert r["passed"], ("%s sample %d" % (what, b), r)
    print(what, "max gradient error / bound = %.3f" % worst)


def stages_seen(names, stage_of, stages=()):
    """{stage: set of kernel names} of the recorded kernels `names`; every stage of `stages` is present, empty if unseen."""
    seen = {s: set() for s in stages}
    for n in names:
        s = stage_of(n)
        if s is not None:
            seen.setdefault(s, set()).add(n)
    return seen


def assert_stages(name, seen, want):
    """Exactly the predicted kernels ran, stage by stage, over every stage either side names."""
    for s in sorted(set(seen) | set(want)):
        assert seen.get(s, set()) == want.get(s, set()), (name, s, sorted(seen.get(s, ())), sorted(want.get(s, ())))
