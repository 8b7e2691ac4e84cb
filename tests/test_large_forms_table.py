"""The table of tests/large_forms.py, without a GPU: every statistics / gradient kernel of the materialised objects and every
partition / gradient kernel of the joint objects is taken past 2^31 elements by some row, or listed as unreachable there with the
arithmetic; every row crosses the boundaries it claims, with a block whose period is 2^p x an odd number of bytes; every row fits
the stated device-memory budget; the workspace figures the table uses agree with the library."""
from tests import kernel_forms as K
from tests import large_forms as L


def test_every_stats_and_grad_kernel_is_taken_past_2_31_elements():
    """Materialised stats / grad and joint partition / grad kernels: each reached past 2^31 elements by a row, or listed in
    UNREACHABLE_LARGE (joint inventory only), never both."""
    cov = L.covered()
    want = L.targets() | L.joint_targets()
    missing = sorted(k for k in want if k not in cov and k not in L.UNREACHABLE_LARGE)
    assert not missing, missing
    assert not set(L.UNREACHABLE_LARGE) & set(cov), sorted(set(L.UNREACHABLE_LARGE) & set(cov))
    assert set(L.UNREACHABLE_LARGE) <= L.joint_targets(), sorted(set(L.UNREACHABLE_LARGE) - L.joint_targets())
    assert len(L.joint_targets()) > 100 and len(L.targets()) > 70        # (both inventories are really there)
    # every row launches something
    for name, row in L.ROWS.items():
        st = L.predicted(row)
        assert st.get("stats") or st.get("partition"), name
    # and each dtype has a row in which one activation row straddles element 2^31 (A not a power of two)
    for d in K.STORES:
        assert any(L.straddles(r) for r in L.ROWS.values() if r["dtype"] == d and not r.get("joint")), d
    for d in ("f32", "bf16", "f16"):
        assert any(L.straddles(r) for r in L.ROWS.values() if r["dtype"] == d and r.get("joint")), d


def test_rows_cross_what_they_claim_with_odd_blocks():
    for name, row in L.ROWS.items():
        t = L.tensors(row)
        claimed = L.claimed(row)
        assert claimed, name
        crossed = {b[0] for b in L.boundaries(row)}
        for nm in claimed:
            assert nm in crossed, (name, nm)
        # the activations (and gradients) of every row pass 2^31 elements, except the cell-table row, whose claim is the
        # workspace: lp2 past 2^31 bytes, the record table past 2^32 bytes
        if row.get("joint"):
            assert L.crosses_elements(row, claimed), name
        elif "lp2" in claimed:
            per, el, n = t["lp2"]
            assert per * n > L.B31, name
            per, el, n = t["records"]
            assert per * n > L.B32, name
        else:
            assert L.crosses_elements(row, ("acts",)), name
        m = L.rule(row)
        assert set(m) == set(claimed), (name, m)
        for nm, v in m.items():
            assert isinstance(v, int) and v % 2 == 1 and v > 1, (name, nm, v)
        # the lengths of the block: one full sample, T_b = 1, U_b = 1
        assert row.get("pow2", 8) <= 13, name
        tl, ll = L.block_lengths(row)
        assert tl.max() == row["T"] and ll.max() <= row["U"] - 1 and tl.min() >= 1, name
        if row.get("layout") != "packed":
            assert tl[0] == row["T"] and ll[0] == row["U"] - 1, name
        if row["K"] >= 3:
            assert tl[1] == 1 and ll[2] == 0, name
        # the checked copies include every copy that holds a boundary of the activations
        for nm, what, c, smp, r in L.boundaries(row):
            if nm in ("acts", "f", "g"):
                assert c in L.checked_copies(row) and 0 <= c < row["copies"], (name, what, c)


def test_rows_fit_the_memory_budget():
    from warprnnt_pytorch import _lib
    worst = 0
    for name, row in L.ROWS.items():
        c = L.case_of(row)
        if row.get("joint"):
            peak = L.joint_peak(row)                   # (get_workspace_size_add)
        else:
            peak = L.peak_bytes(row, _lib.workspace_bytes(row["T"], row["U"], c["N"], True, L.esz(row)))
        assert peak <= L.BUDGET, (name, peak)
        worst = max(worst, peak)
    assert worst > 30e9            # (the f64 rows: the budget is not vacuous)


def test_cell_table_figures_match_the_library():
    """The lattice-block size the table uses (large_forms.lat_block_bytes, a restatement of rnnt_kernels.h) against the
    library: at large N (make_layout's head = the record table / 8 groups) get_workspace_size grows per sample by one lattice
    block, an eighth of the sample's records, its two offset arrays (2 x D x W doubles) and the same few per-sample words for
    every shape."""
    from warprnnt_pytorch import _lib
    rest = set()
    for T, U, lat in ((31, 48, 4), (33, 72, 4), (32, 9, 8), (1400, 8, 4)):
        n = 1 << 16
        d = _lib.workspace_bytes(T, U, 2 * n, True, lat) - _lib.workspace_bytes(T, U, n, True, lat)
        D, W = T + U - 1 + 2 * L.LAT_PAD, (K.lat_stride(U) + 63) // 64
        r = d - n * (L.lat_block_bytes(T, U, lat) + T * U * 4 * lat // 8 + 2 * D * W * 8)
        assert r % n == 0, (T, U, lat, r)
        rest.add(r // n)
    assert len(rest) == 1 and 0 < rest.pop() < 512
