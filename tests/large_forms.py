"""Kernel forms across the index-width boundaries: one row per large case, in the dict format of tests/kernel_forms.py (CASES)
and tests/joint_forms.py (JCASES), so that kernel_forms.predict / joint_forms.predict_joint give the kernels it launches.  The
materialised rows are written out; the additive joint's are found by _joint_rows (each partition / grad kernel of the joint
forms, grown from a case that reaches it into an f-heavy or g-heavy batch), and what no variant reaches within BUDGET is
UNREACHABLE_LARGE, with the arithmetic.
tests/test_large_forms_table.py checks the table without a GPU (coverage, the boundaries each row claims, the block-size rule,
the memory budget); tests/test_gpu_large_forms.py runs every row on the GPU.

A row is a batch of N = copies x K samples made by repeating a ragged base block of K samples (`block`: the lengths; sample 0
is full size, sample 1 has T_b = 1, sample 2 U_b = 1 where the layout has a U at all).  The block rule: every tensor a row puts
past a boundary repeats with a period of 2^p x m bytes, m odd and > 1, p = 8 (up to 13 where a vocabulary or a kernel's chunk
grid needs more: `pow2`).  A wrapped offset -- off mod 2^31 or 2^32, in elements or
bytes -- then lands on ANOTHER position of the block than the one it should have read: different data, so a truncated index
cannot pass the bit-identity check of copies by accident (a period dividing 2^32 would read an identical copy).  The phase of
every row against 16 bytes repeats too (2^p | period): the vector forms take the same path in every copy.

Per row: `boundaries(row)` lists which tensor crosses which of elements 2^31, bytes 2^31, bytes 2^32, and the copy / sample /
row that holds the boundary."""
import zlib

import numpy as np

from tests import joint_forms as J
from tests import kernel_forms as K

BUDGET = 48 * 10 ** 9                 # peak device bytes of one row: its tensors + get_workspace_size(_add)
E31, B31, B32 = 1 << 31, 1 << 31, 1 << 32
LAT_PAD = 16                           # kLatPad (rnnt_kernels.h)


def v2(x):
    return (x & -x).bit_length() - 1


# ----------------------------------------------------------------------------- lengths of the base block
def block_lengths(row):
    """(tl, ll) of the base block's K samples: deterministic from the row's name."""
    k, T, U = row["K"], row["T"], row["U"]
    rng = np.random.default_rng(zlib.crc32(row["name"].encode()))
    tl = rng.integers(1, T + 1, size=k).astype(np.int32)
    ll = rng.integers(0, U, size=k).astype(np.int32)
    tl[0], ll[0] = T, U - 1
    if k > 1:
        tl[1] = 1
    if k > 2:
        ll[2] = 0
    if row.get("layout") == "packed":
        # the packed block's row count sets its period: the last sample's lengths make it 2^j x odd (see rule())
        want = 8 - v2(row["A"] * esz(row))
        done = False
        for t in range(T, 0, -1):
            for l in range(U):
                tl[-1], ll[-1] = t, l
                if v2(int((tl.astype(np.int64) * (ll + 1)).sum())) == want:
                    done = True
                    break
            if done:
                break
    return tl, ll


def esz(row):
    return J.JSTORES[row["dtype"]][2] if row.get("joint") else K.STORES[row["dtype"]][3]


def case_of(row):
    """The kernel_forms / joint_forms case of a row (N = copies x K)."""
    c = {k: v for k, v in row.items() if k not in ("K", "copies", "joint", "heavy", "pow2", "cross", "src")}
    c["N"] = row["K"] * row["copies"]
    return c


# ----------------------------------------------------------------------------- the tensors of a row and their periods
def lat_block_bytes(T, U, lat):
    Up = K.lat_stride(U)
    vals = (5 * (T + U - 1 + 2 * LAT_PAD) * Up + Up + 64 + 63) & ~63
    return vals * lat


def tensors(row):
    """{name: (period in bytes, element bytes, copies)}: the tensors of the row that repeat with the block."""
    e = esz(row)
    k, T, U, A, n = row["K"], row["T"], row["U"], row["A"], row["copies"]
    out = {}
    if row.get("joint"):
        out["f"] = (k * T * A * e, e, n)
        out["g"] = (k * U * A * e, e, n)
        if row["entry"] != "align_add":
            out["df"], out["dg"] = out["f"], out["g"]
            out["wmat"] = (k * T * K.lat_stride(U) * 4, 4, 3 * n)     # W | CB | CL planes: (N, T, Upad) fp32 each
        return out
    lat = 8 if row["dtype"] == "f64" else 4
    if row.get("layout") == "packed":
        tl, ll = block_lengths(row)
        rows = int((tl.astype(np.int64) * (ll + 1)).sum())
        out["acts"] = (rows * A * e, e, n)
    else:
        out["acts"] = (k * T * U * A * e, e, n)
    if row["entry"] not in ("align",) and not row.get("inplace"):
        out["grads"] = out["acts"]
    out["lp2"] = (k * lat_block_bytes(T, U, lat), 2 * lat, n)
    if row["entry"] != "align":
        out["records"] = (k * T * U * 4 * lat, 4 * lat, n)
    return out


def boundaries(row):
    """[(tensor, boundary, copy, sample, row of the tensor)] for every boundary the row's tensors cross."""
    out = []
    for name, (per, el, n) in tensors(row).items():
        total = per * n
        for what, byte in (("elements 2^31", E31 * el), ("bytes 2^31", B31), ("bytes 2^32", B32)):
            if byte < total:
                c, inner = divmod(byte, per)
                if name in ("acts", "grads", "f", "df", "g", "dg"):
                    r = inner // (row["A"] * el)
                    cells = {"f": row["T"], "df": row["T"], "g": row["U"], "dg": row["U"]}.get(name, row["T"] * row["U"])
                    smp, rr = divmod(r, cells) if row.get("layout") != "packed" else (None, r)
                    out.append((name, what, c, smp, rr))
                else:
                    out.append((name, what, c, None, None))
    return out


def straddles(row):
    """Does one activation row hold both element 2^31 - 1 and element 2^31?"""
    A = row["A"]
    per, el, n = tensors(row)["f" if row.get("joint") else "acts"]
    return per * n > E31 * el and E31 % A != 0


def crosses_elements(row, names):
    t = tensors(row)
    return any(per * n > E31 * el for nm, (per, el, n) in t.items() if nm in names)


def claimed(row):
    """The tensors a row puts past a boundary on purpose (`cross`; default: the activations and gradients)."""
    t = tensors(row)
    default = {"f": ("f", "df"), "g": ("g", "dg")}[row["heavy"]] if row.get("joint") else ("acts", "grads")
    return tuple(n for n in row.get("cross", default) if n in t)


def rule(row):
    """{tensor: m} for the claimed tensors past a boundary: their period is 2^p x m bytes, m odd and > 1 (p = 8, or the row's
    `pow2` where a code path's phase must repeat too: still no divisor of 2^32)."""
    out = {}
    q = 1 << row.get("pow2", 8)
    for name, (per, el, n) in tensors(row).items():
        if name in claimed(row) and (per * n > B31 or per * n > E31 * el):
            out[name] = per // q if per % q == 0 else per / q
    return out


def checked_copies(row, names=("acts", "f", "g")):
    """Copy 0, every copy that holds a boundary of the row's activations, and the last copy."""
    cs = {0, row["copies"] - 1}
    for name, what, c, _, _ in boundaries(row):
        if name in names:
            cs.add(c)
    return sorted(cs)


# ----------------------------------------------------------------------------- the rows
def _copies(per_elems, over=E31 + 1):
    return -(-over // per_elems) + 1


def _mat(name, d, A, U, entry, kk=3, **kw):
    """A materialised row: T = 2^j x todd picked so that the block of K x T x U x A elements is 2^pow2 (256) x odd bytes."""
    e = K.STORES[d][3]
    j = kw.get("pow2", 8) - v2(A * e) - v2(U) - v2(kk)
    assert j >= 0, (name, A, U)
    T = (1 << j) * kw.pop("todd", 1)
    row = dict(name=name, dtype=d, T=T, U=U, A=A, entry=entry, K=kk, **kw)
    elems = kk * T * U * A
    if kw.get("layout") == "packed":
        row["copies"] = 1
        per = tensors(row)["acts"][0] // e
        row["copies"] = _copies(per)
    else:
        row["copies"] = _copies(elems)
    return row


# grad_flat_kernel<.., SCALE = 1, ..> writes a 4096-element chunk that spans two samples element by element (one scale per
# element), any other chunk packet by packet (one scale per chunk); in fp16 storage the two paths can round an element one
# ulp apart (seen: f16_block_s1p1 with A = 7001, sample 1's row (0, 0), element 2426 -- 6.3562e-4 in the copy where its chunk
# spans samples 0 and 1, 6.3515e-4 where it lies inside the row; both within oracle.grad_bound).  Bit-identity across copies
# needs the chunk grid to repeat with the block: a period of 2^13 x odd bytes (8192 = the chunk of 16-bit storage), which a
# 2^31 / 2^32 wrap still cannot hit.
_CHUNK_PHASE = {"f16": dict(pow2=13, A=7004, U=8)}


def _mat_rows():
    rows = []
    # stats form, grad form, entry per dtype; A chosen inside each form's row-size range (odd, or 2 x odd: not a power of two)
    A = {  # name: {dtype: A}
        "g1_s1p0": {"f32": 25, "f64": 15, "bf16": 51, "f16": 51},          # rb < 128: lane group 1, PADSKIP 0
        "t2d": {"f32": 30, "f64": 26, "bf16": 60, "f16": 60},             # rb % 8 == 0, <= 208, maxU >= 64
        "g2_s1p2": {"f32": 75, "f64": 51, "bf16": 151, "f16": 151},
        "g4_s0p2": {"f32": 150, "f64": 75, "bf16": 301, "f16": 301},
        "g8_packed_s": {"f32": 301, "f64": 151, "bf16": 601, "f16": 601},
        "g16_packed": {"f32": 601, "f64": 301, "bf16": 1201, "f16": 1201},
        "g32_inplace": {"f32": 901, "f64": 451, "bf16": 1801, "f16": 1801},
        "wave_s0p1": {"f32": 2501, "f64": 1251, "bf16": 5001, "f16": 5001},
        "block_s1p1": {"f32": 3501, "f64": 1751, "bf16": 7001, "f16": 7001},
        "rows": {"f32": 151, "f64": 75, "bf16": 301, "f16": 301},
        "rows_s": {"f32": 3001, "f64": 1501, "bf16": 6001, "f16": 6001},
    }
    for d in K.STORES:
        a = {k: v[d] for k, v in A.items()}
        ph = _CHUNK_PHASE.get(d)
        if ph:
            a["block_s1p1"] = ph["A"]
        rows += [
            # f64 at rb < 128: ~140 M cells of workspace; in place keeps the row inside the budget
            _mat(d + "_g1_s1p0", d, a["g1_s1p0"], 9, "async", scale="ragged", **({"inplace": True} if d == "f64" else {})),
            _mat(d + "_t2d", d, a["t2d"], 72, "call", kk=1, todd=49 if d == "f64" else 25),
            _mat(d + "_g2_s1p2", d, a["g2_s1p2"], 9, "twophase", scale="ragged"),
            _mat(d + "_g4_s0p2", d, a["g4_s0p2"], 5, "call"),
            _mat(d + "_g8_packed_s", d, a["g8_packed_s"], 5, "packed_twophase", kk=5, layout="packed", scale="ragged"),
            _mat(d + "_g16_packed", d, a["g16_packed"], 5, "packed", kk=5, layout="packed"),
            _mat(d + "_g32_inplace", d, a["g32_inplace"], 3, "async", inplace=True),
            _mat(d + "_wave_s0p1", d, a["wave_s0p1"], 3, "call"),
            _mat(d + "_block_s1p1", d, a["block_s1p1"], ph["U"] if ph else 3, "async", scale="ragged",
                 **({"pow2": ph["pow2"]} if ph else {})),
            _mat(d + "_rows", d, a["rows"], 5, "async", misalign=True),
            _mat(d + "_rows_s", d, a["rows_s"], 3, "twophase", misalign=True, scale="ragged"),
        ]
    # the cell tables: ~2^28 cells of a small vocabulary, maxU <= 48 (the cell-per-thread coefficient kernel in groups, the
    # record table overlaying lattice blocks): lp2 blocks past 2^31 bytes, the record table past 2^32 bytes
    # (T = 31: 3 x 31 x 48 cells and 3 lattice blocks of 415 x 256 bytes are both odd multiples of 256 bytes)
    r = dict(name="f32_cells", dtype="f32", T=31, U=48, A=4, entry="async", K=3, scale="ragged", cross=("acts", "grads", "lp2", "records"))
    r["copies"] = -(-(B32 + 1) // (3 * 31 * 48 * 16)) + 1
    rows.append(r)
    # best-path alignment on activations past 2^31 elements (materialised statistics stage + the max-plus lattice)
    rows += [_mat("f32_align", "f32", 25, 9, "align"), _mat("bf16_align", "bf16", 51, 9, "align")]
    return rows


# ----------------------------------------------------------------------------- the additive joint
JOINT_ENTRIES = ("add", "twophase", "dt")


def joint_targets():
    """{(object, kernel)} of the partition and grad stages the joint forms table holds."""
    return {(o, k) for (o, k) in J.predicted_rows() if J.jstage_of(k) in ("partition", "grad")}


def heavy_for(kernel):
    """Which tensors a joint kernel must see past 2^31 elements: DF kernels read f and write df ("f"), DG kernels g / dg ("g"),
    the row maxima, Z kernels and the far-cell epilogue read both (either)."""
    base = kernel.split("<")[0].split("::")[-1]
    return ("f",) if base.startswith("joint_df") else ("g",) if base.startswith("joint_dg") else ("f", "g")


def _joint_ws(T, U, N, _cache={}):
    if (T, U, N) not in _cache:
        from warprnnt_pytorch import _lib
        _cache[(T, U, N)] = _lib.workspace_bytes_add(T, U, N)
    return _cache[(T, U, N)]


def joint_peak(row):
    """Device bytes of a joint row: f, g, df, dg (+ the 16-byte slack of offset views), get_workspace_size_add, small arrays."""
    N, T, U, A, e = row["K"] * row["copies"], row["T"], row["U"], row["A"], esz(row)
    grads = 2 if row["entry"] != "align_add" else 1
    return grads * N * (T + U) * A * e + 64 + _joint_ws(T, U, N) + N * (32 + 4 * U)


_VOCAB_BASES = (2048, 4096, 8192, 16400, 17000, 20000, 40000, 66000, 70000)   # S = 4 / 8 past 2^31: few tiles, A > 16 K / 64 K
_ORACLE_MAX = 40 * 10 ** 6                                                      # elements of the block's z = f + g (host fp64)
_MAX_DIAGONALS = 600        # fp32 lattices up to the lengths at which tests/test_gpu_joint_forms.py sets its df / dg bounds


def _joint_variants(c, heavy):
    """Large variants of a joint case: its vocabulary or one near it (or a large one), K = 3 or 1 samples per block, and T
    (f-heavy) or U <= 1024 (g-heavy) = 2^j x odd, smallest first, so that the block is 2^p x odd bytes (p = 8, more where the
    vocabulary itself holds a larger power of two, at most 13) and N = K x copies <= 65535."""
    e = J.JSTORES[c["dtype"]][2]
    A0, T0, U0 = c["A"], c["T"], c["U"]
    cands = [A0 + d for d in sorted(range(-64, 65), key=abs)] + [b + d for b in _VOCAB_BASES for d in range(16)]
    for A in cands:
        if A < 2:
            continue
        for kk in (3, 1):
            p = max(8, v2(kk * A * e))
            if p > 13:
                continue
            j = p - v2(kk * A * e)
            for o in range(1, 1 << 16, 2):
                L_ = (1 << j) * o
                if L_ > (1024 if heavy == "g" else 65536):
                    break
                cop = -(-(E31 + 1) // (kk * L_ * A)) + 1
                if kk * cop > 65535:
                    continue
                if heavy == "f":
                    yield dict(A=A, K=kk, T=L_, U=U0, copies=cop, pow2=p)
                    if L_ > 4 * max(T0, 64) and L_ > 600:
                        break
                else:
                    for T in sorted({T0, 64, 72, 512, 520}):
                        yield dict(A=A, K=kk, T=T, U=L_, copies=cop, pow2=p)


def _joint_row(c, v, heavy):
    row = dict(name="", dtype=c["dtype"], entry=c["entry"], joint=True, heavy=heavy, src=c["name"], **v)
    for key in ("off", "scale"):
        if key in c:
            row[key] = c[key]
    N = v["K"] * v["copies"]
    if N * (v["T"] + v["U"]) >= E31 or max(v["T"], v["U"]) * v["A"] >= E31 or v["copies"] < 2:
        return None                                              # run_gpu_joint's host limits
    if v["K"] * v["T"] * v["U"] * v["A"] > _ORACLE_MAX:
        return None
    if v["T"] + v["U"] - 1 > _MAX_DIAGONALS:
        return None
    return row


def _joint_rows():
    """One row per joint target that no earlier row reaches: the first case of joint_forms that reaches it, grown by
    _joint_variants until the prediction still holds and the row fits BUDGET.  Targets no variant reaches are UNREACHABLE_LARGE."""
    rows = {}
    for o, k in sorted(joint_targets()):
        stage, heavies = J.jstage_of(k), heavy_for(k)
        if any(r["heavy"] in heavies and J.objects_of(r)[0] == o and k in J.predict_joint(case_of(r), 256)[stage]
               for r in rows.values()):
            continue
        if (o, k) in UNREACHABLE_LARGE:
            continue
        found = None
        for cname, c in sorted(J.JCASES.items()):
            if c["entry"] not in JOINT_ENTRIES or c.get("data") or J.objects_of(c)[0] != o or \
                    k not in J.predict_joint(c, 256)[stage]:
                continue
            for h in heavies:
                for v in _joint_variants(c, h):
                    row = _joint_row(c, v, h)
                    if row is None or k not in J.predict_joint(case_of(row), 256)[stage] or joint_peak(row) > BUDGET:
                        continue
                    found = row
                    break
                if found:
                    break
            if found:
                break
        if found:
            base = name = "j_%s_%sheavy" % (found["src"], found["heavy"])
            i = 2
            while name in rows:                                  # (another variant of the same case: A / T / U differ)
                name, i = "%s%d" % (base, i), i + 1
            found["name"] = name
            rows[name] = found
    return rows


def _joint_extra_rows():
    # the additive cell tables: the W | CB | CL planes (3 x N x T x Upad fp32) past 2^31 elements with a small vocabulary
    # (one-hot planes, the cell-per-thread coefficient kernel + joint_sums_kernel); T = 8 x 175: 3 x 1400 x 8 x 4 bytes =
    # 256 x 525 per copy
    cells = dict(name="j_f32_cells", dtype="f32", entry="add", joint=True, heavy="f", T=1400, U=8, A=9, K=3, cross=("wmat",))
    cells["copies"] = -(-(E31 + 1) // (3 * 3 * 1400 * 8)) + 1
    # best-path alignment of the additive joint, f past 2^31 elements (T = 64 x 3: 3 x 192 x 251 x 4 bytes = 256 x 2259)
    al = dict(name="j_f32_align_add", dtype="f32", entry="align_add", joint=True, heavy="f", T=192, U=9, A=251, K=3)
    al["copies"] = -(-(E31 + 1) // (3 * 192 * 251)) + 1
    al16 = dict(name="j_bf16_align_add", dtype="bf16", entry="align_add", joint=True, heavy="f", T=384, U=9, A=251, K=3)
    al16["copies"] = -(-(E31 + 1) // (3 * 384 * 251)) + 1
    return {r["name"]: r for r in (cells, al, al16)}


# Kernels of the joint's partition / grad stages that no row can take past 2^31 elements within BUDGET (the peaks: the smallest
# variant _joint_variants finds that still launches the kernel), with the arithmetic.  The materialised stages have none.
_SPLIT_F = ("split_f (maxU >= 64, at most two column groups: A <= 64 x NKf, fp32 <= 128) with f past 2^31 elements puts "
            "N x T x U >= 2^31 x 64 / 128 = 2^30 cells in the workspace: %.0f GB for the smallest variant, over the 48 GB budget")
_SPLIT_G = ("split_g (maxT >= 64 with at most two column groups, or maxT >= 512) with g past 2^31 elements puts N x T x U >= "
            "2^31 x 64 / A cells in the workspace and f = 2^31 x T / U elements beside it: %.0f GB for the smallest variant")
_Z4_VEC = ("S = 4 needs N x ceil(T/32) x ceil(U/32) < 4096, so N x T x A and N x U x A stay below 4096 x 32 x A, under 2^31 "
           "unless A > 16384; the vectorised non-matrix-core form needs 481 <= A <= 511 (A % 8 == 0 from 512 on takes "
           "joint_z16_kernel)")
UNREACHABLE_LARGE = {}
for _o, _tag in (("joint_f32", "F32"), ("joint_bf16", "BF16"), ("joint_f16", "F16")):
    gb = {"F32": (111, 100, 277, 185, 73), "BF16": (193, 90, 548, 149, 60), "F16": (193, 90, 548, 149, 60)}[_tag]
    UNREACHABLE_LARGE[(_o, "rnnt::joint_df_kernel<rnnt::%s, 1, true, true, true, true>" % _tag)] = _SPLIT_F % gb[0]
    UNREACHABLE_LARGE[(_o, "rnnt::joint_df_kernel<rnnt::%s, 2, true, true, true, true>" % _tag)] = _SPLIT_F % gb[1]
    UNREACHABLE_LARGE[(_o, "rnnt::joint_dg_kernel<rnnt::%s, 1, true, true>" % _tag)] = _SPLIT_G % gb[2]
    UNREACHABLE_LARGE[(_o, "rnnt::joint_dg_kernel<rnnt::%s, 2, true, true>" % _tag)] = _SPLIT_G % gb[3]
    UNREACHABLE_LARGE[(_o, "rnnt::joint_dg_kernel<rnnt::%s, 4, true, true>" % _tag)] = _SPLIT_G % gb[4]
    if _tag != "F32":
        UNREACHABLE_LARGE[(_o, "rnnt::joint_z_kernel<rnnt::%s, 4, true, false>" % _tag)] = _Z4_VEC
        UNREACHABLE_LARGE[(_o, "rnnt::joint_z_kernel<rnnt::%s, 4, true, true>" % _tag)] = _Z4_VEC


ROWS = {r["name"]: r for r in _mat_rows()}
ROWS.update(_joint_rows())
ROWS.update(_joint_extra_rows())


# ----------------------------------------------------------------------------- coverage
def targets():
    """{(object, kernel)} of the stats and grad stages the forms table holds for the materialised objects."""
    return {(o, k) for (o, k) in K.predicted_rows() if K.stage_of(k) in ("stats", "grad")}


def predicted(row, cus=256):
    """{stage: kernels} of a row."""
    if row.get("joint"):
        return {st: ks for st, ks in J.predict_joint(case_of(row), cus).items() if ks}
    if row["entry"] == "align":
        c = dict(case_of(row), entry="fwd_only", train=False)
        out = {"stats": K.predict(c, cus)["stats"]}
        out.update(J.predict_joint(case_of(row), cus))
        return out
    return K.predict(case_of(row), cus)


def covered(cus=256):
    """{(object, kernel): [rows]} of the stats / grad stages (materialised) and partition / grad stages (joint), for rows whose
    activations or gradients pass 2^31 elements (joint: the f / df or g / dg side the kernel reads, heavy_for)."""
    out = {}
    for name, row in ROWS.items():
        if row.get("joint"):
            if row["entry"] == "align_add" or not crosses_elements(row, claimed(row)):
                continue
            obj = J.objects_of(case_of(row))[0]
            for s, ks in predicted(row, cus).items():
                for k in ks:
                    if s in ("partition", "grad") and row["heavy"] in heavy_for(k):
                        out.setdefault((obj, k), []).append(name)
            continue
        if row["entry"] == "align" or not crosses_elements(row, ("acts", "grads")):
            continue
        obj = K.STORES[row["dtype"]][0]
        for s, ks in predicted(row, cus).items():
            if s in ("stats", "grad"):
                for k in ks:
                    out.setdefault((obj, k), []).append(name)
    return out


def peak_bytes(row, ws):
    """Device bytes of a row: activations, gradients (unless in place), the padding element of a misaligned view, the
    workspace `ws` (get_workspace_size), lengths, labels, costs and offsets."""
    per, el, n = tensors(row)["acts"]
    acts = per * n
    grads = 0 if row.get("inplace") or row["entry"] == "align" else acts + (el if row.get("misalign") else 0)
    N = row["K"] * row["copies"]
    small = N * (8 + 8 + 8 + 8 + 4 * row["U"])
    return acts + grads + ws + small
