"""The additive joint's kernel forms (rnnt_joint.hip, rnnt_joint_bf16.hip, rnnt_joint_fp16.hip) and the alignment kernels: which
kernels the release build holds, the release rules that pick them (a restatement of run_gpu_joint, csrc/rnnt_joint_impl.h, and of
launch_lattice / launch_coef, csrc/rnnt_host.h, where the joint reaches them), and one case per form that reaches it -- the
counterpart of tests/kernel_forms.py for the other half of the library.  tests/test_kernel_inventory.py checks the table
against the code objects of libwarprnnt.so (no GPU); tests/test_gpu_joint_forms.py runs every case through the C-ABI on the GPU,
checks that the predicted kernels of each stage -- and no others -- ran, and compares the results with the fp64 oracle on the
materialised joint z = f + g.

A case: dtype (f32 / bf16 / f16 storage of f, g, df, dg; f64 / ... for the materialised compute_rnnt_align rows), N, T, U, A,
entry (below), and `off`: the byte offset of f, g, df, dg from a 16-byte boundary (views into larger buffers), which the
vec / NKmax / 16-bit matrix-core gates read."""
import os
import re

from tests import kernel_forms as K

# ----------------------------------------------------------------------------- release constants
JOINT_Z_SMALL_A = 56               # kJointZSmallA (rnnt_joint_kernels.h)
SAMPLED_MIN_A = 64                 # sampled row references: A >= 64 (run_gpu_joint)
MFMA16_MIN_A = 512                 # z16 / df16 / dg16: A % 8 == 0 and A >= 512 (run_gpu_joint)
ROWMAX_BLOCK_BYTES = 12288         # joint_rowmax_kernel: a block per row from 12 KB on
ROWMAX_LANES_A = 64                # ... eight lanes per row up to 64 symbols
Z_TILES_ONE, Z_TILES_EIGHT = 4096, 1024     # vocabulary split S of the Z kernel: N * tiles against these ...
Z_CHUNKS_FOUR, Z_CHUNKS_EIGHT = 16, 32      # ... and ceil(A / 32) against these
COEF_CELL_MAX_U = 48               # coef_is_tiled: maxU > 48
SPLIT_MIN_U, SPLIT_MIN_T, SPLIT_LONG_T = 64, 64, 512   # split_f (maxU), split_g (maxT, and any vocabulary from maxT >= 512)
ALIGN_MAX_WAVES = 16               # kAlignMaxWaves (rnnt_align_kernels.h)
ALIGN_LDS_WORDS = 4096             # kAlignLdsWords: decision words staged per traceback chunk
# release Tune defaults the rules read (rnnt_host.h, struct Tune): a dev build's RNNT_TUNE is not what these tests run against
TUNE = {"jzs": 0, "jsamp": 1, "j16": 7, "j16pf": 1, "j16nt": 4, "jfnk": 0, "jgnk": 0, "jfpf": 1, "jgpf": 1, "joh": -1,
        "ctile": 1, "jfsum": 1, "jsplit": 1, "jnocb": 1, "latlin": 1, "lat2": -1}

# store type -> (object, store tag, element bytes); the materialised alignment rows add f64
JSTORES = {"f32": ("joint_f32", "rnnt::F32", 4), "bf16": ("joint_bf16", "rnnt::BF16", 2), "f16": ("joint_f16", "rnnt::F16", 2)}
JOBJECTS = {"joint_f32": "rnnt_joint.hip", "joint_bf16": "rnnt_joint_bf16.hip", "joint_f16": "rnnt_joint_fp16.hip"}
JSTAGES = ("partition", "lattice", "coef", "grad", "align")
# entries (C-ABI): add = compute_rnnt_loss_add; twophase = _add_fwd + _add_bwd (grad_scale); dt = _add_fwd_dt + _add_bwd_dt;
# fastemit = _add_fwd_fastemit + _add_bwd; align_add = compute_rnnt_align_add; align = compute_rnnt_align (materialised)
ENTRIES = ("add", "twophase", "dt", "fastemit", "align_add", "align")


def jstage_of(name):
    """Stage of a (demangled, argument-free) kernel name of the joint objects, or None."""
    base = name.split("<")[0].split("::")[-1]
    if base.startswith(("joint_rowmax", "joint_prep", "joint_z")):
        return "partition"
    if base.startswith("lattice_kernel") or base.startswith("lattice_lin_kernel"):
        return "lattice"
    if base.startswith("coef_") or base == "joint_sums_kernel":
        return "coef"
    if base.startswith(("joint_df", "joint_dg", "joint_far")):
        return "grad"
    if base.startswith("align_"):
        return "align"
    return None


def _b(x):
    return "true" if x else "false"


def planes_onehot(maxU):
    return 4 if ((maxU + 7) & ~7) <= 4 * maxU else 3


def predict_align(lat, U):
    """The alignment kernels of one call: one lattice type, and the wavefront count must fit launch_align."""
    assert K.lat_stride(U) <= 64 * ALIGN_MAX_WAVES
    return {"rnnt::align_lattice_kernel<%s>" % lat, "rnnt::align_traceback_kernel<%s>" % lat}


def predict_joint(case, cus):
    """{stage: set of kernel names} the release rules launch for `case` on a device with `cus` compute units."""
    N, T, U, A = K.case_shape(case, cus)
    entry = case["entry"]
    if entry == "align":                                 # the materialised statistics stage (kernel_forms) + the alignment
        return {"align": predict_align("double" if case["dtype"] == "f64" else "float", U)}
    obj, tag, esz = JSTORES[case["dtype"]]
    k16 = esz == 2
    off = dict({"f": 0, "g": 0, "df": 0, "dg": 0}, **case.get("off", {}))
    fg = off["f"] | off["g"]
    all4 = fg | off["df"] | off["dg"]
    out = {s: set() for s in JSTAGES}
    # partition: row maxima, Z
    vec = A % (16 // esz) == 0 and fg % 16 == 0
    tiles = ((T + 31) // 32) * ((U + 31) // 32)
    all_tiles, nchunk = N * tiles, (A + 31) // 32
    S = 1 if (all_tiles >= Z_TILES_ONE or nchunk < Z_CHUNKS_FOUR) else (8 if (all_tiles < Z_TILES_EIGHT and nchunk >= Z_CHUNKS_EIGHT) else 4)
    small = S == 1 and A <= JOINT_Z_SMALL_A
    sampled = not small and A >= SAMPLED_MIN_A
    z16 = k16 and not small and A % 8 == 0 and A >= MFMA16_MIN_A and fg % 16 == 0
    if A * esz >= ROWMAX_BLOCK_BYTES:
        rowmax = "rnnt::joint_rowmax_kernel<%s, %s, 4>" % (tag, _b(vec))
    elif A <= ROWMAX_LANES_A:
        rowmax = "rnnt::joint_rowmax_kernel<%s, false, 0>" % tag
    else:
        rowmax = "rnnt::joint_rowmax_kernel<%s, %s, 1>" % (tag, _b(vec))

    def z(samp):
        if z16:
            return "rnnt::joint_z16_kernel<%s, %d, %s>" % (tag, S, _b(samp))
        return "rnnt::joint_z_kernel<%s, %d, %s, %s>" % (tag, S, _b(vec), _b(samp))
    if sampled:        # the gated exact pair is enqueued in every call (it returns at once unless a row tripped the guard)
        out["partition"] = {"rnnt::joint_prep_kernel<0>", z(True), rowmax, z(False)}
    else:
        out["partition"] = {rowmax, "rnnt::joint_z_small_kernel<%s>" % tag if small else z(False)}
    if entry == "align_add":
        out["align"] = predict_align("float", U)
        return out
    # lattice (launch_lattice, fp32 lattice, both directions when training)
    up = K.lat_stride(U)
    if up <= 64 and N * 2 <= cus:
        out["lattice"] = {"rnnt::lattice_lin_kernel<0>"}
    elif up <= 64:
        out["lattice"] = {"rnnt::lattice_kernel<float, 1, 1>"}
    elif up <= 256:
        out["lattice"] = {"rnnt::lattice_kernel<float, 8, 1>"}
    elif up <= 512:
        out["lattice"] = {"rnnt::lattice_kernel<float, 4, 2>"}
    else:
        out["lattice"] = {"rnnt::lattice_kernel<float, 8, 2>"}
    # coefficients: the tiled kernel forms the correction sums itself; the cell-per-thread one leaves them to joint_sums_kernel
    tiled = U > COEF_CELL_MAX_U
    out["coef"] = {"rnnt::coef_kernel<float, true>"} if tiled else {"rnnt::coef_cell_kernel<float>", "rnnt::joint_sums_kernel<0>"}
    # gradient GEMMs
    onehot16 = A <= 64 and U >= 64 and planes_onehot(U) == 4 and tiled
    onehot = A <= 256 and (esz == 4 or onehot16)
    nkmax = (4 if (A % 4 == 0 and all4 % (4 * esz) == 0 and A >= 96) else
             2 if (A % 2 == 0 and all4 % (2 * esz) == 0 and A >= 48) else 1)
    nkf = nkg = nkmax
    if A <= 64 and U >= 64:
        nkf = min(nkf, 2)
    else:
        while nkf > 1 and 128 * nkf * (2 if k16 else 1) > A:
            nkf >>= 1
    groups = lambda nk: (A + 32 * nk - 1) // (32 * nk)
    nocb = onehot and planes_onehot(U) == 4 and tiled
    split_f = nkf <= 2 and U >= SPLIT_MIN_U and groups(nkf) <= 2
    split_g = T >= SPLIT_MIN_T and (groups(nkg) <= 2 or T >= SPLIT_LONG_T)
    pf_f, pf_g = (not k16) or nkf < 4, (not k16) or nkg < 4
    mfma = k16 and A % 8 == 0 and all4 % 16 == 0 and A >= MFMA16_MIN_A
    df = "rnnt::joint_df_kernel<%s, %d, %%s, %%s, %%s, %%s>" % (tag, nkf)
    if mfma:
        g_df = "rnnt::joint_df16_kernel<%s, 4, true>" % tag          # j16nt = 4, j16pf = 1
    elif split_f and onehot and nocb:
        g_df = df % ("true", "true", "true", "true")
    elif onehot and nocb:
        g_df = df % ("true", "true", "false", "true")
    elif split_f and onehot:
        g_df = df % ("true", "true", "true", "false")
    elif split_f:
        g_df = df % ("true", "false", "true", "false")
    elif onehot:
        g_df = df % ("true", "true", "false", "false")
    else:
        g_df = df % (_b(pf_f), "false", "false", "false")
    if mfma:
        g_dg = "rnnt::joint_dg16_kernel<%s, 4, true>" % tag
    elif split_g:
        g_dg = "rnnt::joint_dg_kernel<%s, %d, true, true>" % (tag, nkg)
    else:
        g_dg = "rnnt::joint_dg_kernel<%s, %d, %s, false>" % (tag, nkg, _b(pf_g))
    far = "rnnt::joint_far16_kernel<%s>" % tag if k16 else "rnnt::joint_far_kernel<%s>" % tag
    out["grad"] = {g_df, g_dg, far}
    return out


def objects_of(case):
    """The joint code objects whose kernels the case launches."""
    if case["entry"] == "align":
        return ["joint_f32"]                             # the alignment kernels live in rnnt_joint.hip only
    obj = JSTORES[case["dtype"]][0]
    return [obj]


def object_of_kernel(case, kernel):
    return "joint_f32" if kernel.split("<")[0].endswith(("align_lattice_kernel", "align_traceback_kernel")) else objects_of(case)[0]


# ----------------------------------------------------------------------------- the cases
def _case(name, dtype, N, T, U, A, entry, **kw):
    if entry == "add" and kw.get("scale"):               # (compute_rnnt_loss_add takes no grad_scale: the fp32 two-phase pair)
        entry = "twophase"
    return dict(name=name, dtype=dtype, N=N, T=T, U=U, A=A, entry=entry, **kw)


def _entry(d):
    return "add" if d == "f32" else "dt"


def _cases():
    cs = []
    for d in JSTORES:
        e = _entry(d)
        o1 = 4                                            # byte offset of a view: 4 (one fp32 / two 16-bit elements)
        cs += [
            # partition: the small-vocabulary Z kernel and its edge (A = 56 / 57), the exact-pass Z kernel without sampling
            # (57 .. 63), the sampled route from 64 on; row maxima per block (12 KB rows) / per lanes / per wavefront
            _case(d + "_a56", d, 3, 20, 9, 56, e),
            _case(d + "_a57", d, 3, 20, 9, 57, e, scale=True),
            _case(d + "_a63", d, 3, 33, 9, 63, e),
            _case(d + "_a64", d, 3, 33, 9, 64, e, scale=True),
            _case(d + "_a64_mis", d, 3, 20, 9, 64, e, off={"f": o1}),
            _case(d + "_a100", d, 3, 20, 7, 100, e),
            _case(d + "_a100_mis", d, 3, 20, 7, 100, e, off={"g": 8}),
            _case(d + "_block", d, 2, 5, 4, 12288 // JSTORES[d][2], e),
            _case(d + "_block_mis", d, 2, 5, 4, 12288 // JSTORES[d][2], e, off={"f": 8}),
            # the vocabulary split: ceil(A / 32) = 15 / 16 (S 1 -> 4) and 31 / 32 (S 4 -> 8), each with aligned and offset f
            _case(d + "_c15", d, 2, 9, 5, 480, e),
            _case(d + "_c16", d, 2, 9, 5, 488, e),
            _case(d + "_c16_mis", d, 2, 9, 5, 488, e, off={"f": 8}),
            _case(d + "_c31", d, 2, 9, 5, 992, e),
            _case(d + "_c32", d, 2, 9, 5, 1000, e, scale=True),
            _case(d + "_c32_mis", d, 2, 9, 5, 1000, e, off={"g": 8}),
            # ... and N * tiles on either side of 1024 (S 8 -> 4) and 4096 (S 4 -> 1): one-tile samples (T = U = 2)
            _case(d + "_t1023", d, 1023, 2, 2, 1024, e),
            _case(d + "_t1024", d, 1024, 2, 2, 1024, e),
            _case(d + "_t4095", d, 4095, 2, 2, 512, e),
            _case(d + "_t4096", d, 4096, 2, 2, 512, e),
            _case(d + "_t4096_mis", d, 4096, 2, 2, 520, e, off={"f": 8}),
            # lattice forms (linear chain / one-wavefront on either side of 2N vs the CU count; 8x1, 4x2, 8x2), coefficient
            # kernels either side of maxU = 48, the split DF / DG either side of maxU 64 and maxT 64 / 512
            _case(d + "_lat_lin", d, "cus//2", 3, 5, 9, e),
            _case(d + "_lat_11", d, "cus//2+1", 3, 5, 9, e),
            _case(d + "_u48", d, 2, 20, 48, 40, e),
            _case(d + "_u49", d, 2, 20, 49, 40, e),
            _case(d + "_u63", d, 2, 20, 63, 50, e, scale=True),
            _case(d + "_u64", d, 2, 20, 64, 50, e, scale=True),
            _case(d + "_t63", d, 2, 63, 9, 200, e),
            _case(d + "_t64", d, 2, 64, 9, 200, e),
            _case(d + "_t511", d, 2, 511, 5, 300, e),
            _case(d + "_t512", d, 2, 512, 5, 300, e),
            _case(d + "_lat_81", d, 2, 9, 130, 12, e),
            _case(d + "_lat_42", d, 2, 5, 300, 7, e),
            _case(d + "_lat_82", d, 2, 4, 600, 3, e),
            # columns per lane of DF / DG: NKmax from the alignment of all four pointers (4 / 2 / 1) and the vocabulary
            _case(d + "_nk_a256", d, 2, 70, 20, 256, e),
            _case(d + "_nk_a512", d, 2, 20, 20, 516, e),
            _case(d + "_nk_a1024", d, 2, 20, 20, 1028, e, scale=True),
            _case(d + "_nk_dg4", d, 2, 20, 20, 1028, e, off={"dg": 4}),
            _case(d + "_nk_df8", d, 2, 20, 20, 1028, e, off={"df": 8}),
            _case(d + "_nk_u64_dg4", d, 2, 70, 70, 50, e, off={"dg": 4}),
            _case(d + "_nk_u64_a96", d, 2, 70, 70, 96, e),
            _case(d + "_nk_u64_a96_f4", d, 2, 70, 70, 96, e, off={"f": 4}),
            _case(d + "_nk_u64_a200", d, 2, 20, 70, 200, e),
            _case(d + "_nk_u64_a200_g4", d, 2, 20, 70, 200, e, off={"g": 4}),
            _case(d + "_nk_a130", d, 2, 70, 20, 130, e),
            _case(d + "_nk_a130_odd", d, 2, 20, 20, 131, e),
            _case(d + "_split_g_a1028", d, 2, 600, 5, 1028, e),
            _case(d + "_nk_a256_u70", d, 2, 20, 70, 256, e),
            _case(d + "_nk_t70_a50", d, 2, 70, 20, 50, e),
            _case(d + "_nk_t70_a33", d, 2, 70, 9, 33, e),
            # data-dependent work: the exact pass behind the guard, -inf in the sampled columns, far cells
            _case(d + "_guard", d, 3, 37, 9, 200, e, data="guard"),
            _case(d + "_masked32", d, 3, 37, 9, 200, e, data="masked32"),
            _case(d + "_far", d, 3, 20, 9, 50, e, data="far", scale=True),
            _case(d + "_far_tiled", d, 3, 20, 70, 300, e, data="far"),
        ]
        if d != "f32":
            # 16-bit: the matrix-core gates either side of A = 512 (A % 8 == 0), and 16-byte alignment of all four pointers
            cs += [_case(d + "_m504", d, 2, 17, 9, 504, e, scale=True),
                   _case(d + "_m512", d, 2, 17, 9, 512, e, scale=True),
                   _case(d + "_m512_f8", d, 2, 17, 9, 512, e, off={"f": 8}),
                   _case(d + "_m512_df8", d, 2, 17, 9, 512, e, off={"df": 8}),
                   _case(d + "_m1024", d, 2, 40, 35, 1024, e),
                   _case(d + "_m512_s1", d, 4096, 2, 2, 512, e),
                   _case(d + "_m1024_s8", d, 2, 9, 5, 1024, e),
                   _case(d + "_m_guard", d, 2, 17, 9, 512, e, data="guard")]
        # alignment through the additive entry
        cs += [_case(d + "_al_add_u64", d, 3, 30, 64, 20, "align_add"),
               _case(d + "_al_add_u65", d, 3, 30, 65, 70, "align_add")]
    # the other fp32 entries: two-phase with a per-sample grad_scale, fastemit, the _dt entry with code 0
    cs += [_case("f32_twophase", "f32", 3, 21, 7, 130, "twophase", scale=True),
           _case("f32_twophase_u70", "f32", 3, 21, 70, 50, "twophase", scale=True),
           _case("f32_fastemit", "f32", 3, 23, 9, 130, "fastemit", lam=0.05),
           _case("f32_dt0", "f32", 3, 20, 9, 100, "dt", scale=True),
           _case("f32_dt0_mis", "f32", 3, 20, 9, 100, "dt", off={"f": 4, "df": 4})]
    # alignment: W = 1 / 2 (U 64 / 65), 8 wavefronts, W = 16 at U = 1024 (the make_plan limit) with a long T that needs several
    # traceback chunks (4096 / W = 256 diagonals per chunk); every dtype of the materialised entry, fp32 / 16-bit additive
    cs += [_case("f32_al_add_w8", "f32", 2, 40, 500, 6, "align_add"),
           _case("f32_al_add_w16", "f32", 1, 700, 1024, 5, "align_add"),
           _case("bf16_al_add_w16", "bf16", 1, 300, 1024, 8, "align_add")]
    for d in ("f32", "f64", "bf16", "f16"):
        cs += [_case(d + "_al_u64", d, 3, 30, 64, 6, "align"),
               _case(d + "_al_u65", d, 3, 30, 65, 6, "align"),
               _case(d + "_al_w8", d, 2, 40, 500, 4, "align")]
    cs += [_case("f32_al_w16", "f32", 1, 600, 1024, 3, "align"),
           _case("f64_al_w16", "f64", 1, 600, 1024, 3, "align"),
           _case("f32_al_w16_planted", "f32", 2, 400, 1024, 4, "align", data="planted"),
           _case("f64_al_w16_planted", "f64", 1, 400, 1024, 4, "align", data="planted")]
    return cs


JCASES = {c["name"]: c for c in _cases()}


def predicted_rows(cus=256):
    """{(object, kernel): [cases]} that the release rules reach with JCASES on a device of `cus` compute units."""
    rows = {}
    for name, c in JCASES.items():
        for ks in predict_joint(c, cus).values():
            for k in ks:
                rows.setdefault((object_of_kernel(c, k), k), []).append(name)
    return rows


# ----------------------------------------------------------------------------- the inventory
# One row per launched form: (object, kernel, the case that reaches it).  Written out, not derived: deleting a row, or a form
# the build gains or loses, fails tests/test_kernel_inventory.py.
FORMS = [
    ('joint_bf16', 'rnnt::coef_cell_kernel<float>', 'bf16_a56'),
    ('joint_bf16', 'rnnt::coef_kernel<float, true>', 'bf16_u49'),
    ('joint_bf16', 'rnnt::joint_df16_kernel<rnnt::BF16, 4, true>', 'bf16_block'),
    ('joint_bf16', 'rnnt::joint_df_kernel<rnnt::BF16, 1, true, false, false, false>', 'bf16_a56'),
    ('joint_bf16', 'rnnt::joint_df_kernel<rnnt::BF16, 1, true, true, true, true>', 'bf16_lat_81'),
    ('joint_bf16', 'rnnt::joint_df_kernel<rnnt::BF16, 2, true, false, false, false>', 'bf16_c32_mis'),
    ('joint_bf16', 'rnnt::joint_df_kernel<rnnt::BF16, 2, true, true, true, true>', 'bf16_u64'),
    ('joint_bf16', 'rnnt::joint_df_kernel<rnnt::BF16, 4, false, false, false, false>', 'bf16_block_mis'),
    ('joint_bf16', 'rnnt::joint_dg16_kernel<rnnt::BF16, 4, true>', 'bf16_block'),
    ('joint_bf16', 'rnnt::joint_dg_kernel<rnnt::BF16, 1, true, false>', 'bf16_a57'),
    ('joint_bf16', 'rnnt::joint_dg_kernel<rnnt::BF16, 1, true, true>', 'bf16_nk_t70_a33'),
    ('joint_bf16', 'rnnt::joint_dg_kernel<rnnt::BF16, 2, true, false>', 'bf16_a56'),
    ('joint_bf16', 'rnnt::joint_dg_kernel<rnnt::BF16, 2, true, true>', 'bf16_nk_u64_dg4'),
    ('joint_bf16', 'rnnt::joint_dg_kernel<rnnt::BF16, 4, false, false>', 'bf16_a100'),
    ('joint_bf16', 'rnnt::joint_dg_kernel<rnnt::BF16, 4, true, true>', 'bf16_t64'),
    ('joint_bf16', 'rnnt::joint_far16_kernel<rnnt::BF16>', 'bf16_a56'),
    ('joint_bf16', 'rnnt::joint_prep_kernel<0>', 'bf16_a64'),
    ('joint_bf16', 'rnnt::joint_rowmax_kernel<rnnt::BF16, false, 0>', 'bf16_a56'),
    ('joint_bf16', 'rnnt::joint_rowmax_kernel<rnnt::BF16, false, 1>', 'bf16_a100'),
    ('joint_bf16', 'rnnt::joint_rowmax_kernel<rnnt::BF16, false, 4>', 'bf16_block_mis'),
    ('joint_bf16', 'rnnt::joint_rowmax_kernel<rnnt::BF16, true, 1>', 'bf16_c15'),
    ('joint_bf16', 'rnnt::joint_rowmax_kernel<rnnt::BF16, true, 4>', 'bf16_block'),
    ('joint_bf16', 'rnnt::joint_sums_kernel<0>', 'bf16_a56'),
    ('joint_bf16', 'rnnt::joint_z16_kernel<rnnt::BF16, 1, false>', 'bf16_t4096'),
    ('joint_bf16', 'rnnt::joint_z16_kernel<rnnt::BF16, 1, true>', 'bf16_t4096'),
    ('joint_bf16', 'rnnt::joint_z16_kernel<rnnt::BF16, 4, false>', 'bf16_c31'),
    ('joint_bf16', 'rnnt::joint_z16_kernel<rnnt::BF16, 4, true>', 'bf16_c31'),
    ('joint_bf16', 'rnnt::joint_z16_kernel<rnnt::BF16, 8, false>', 'bf16_block'),
    ('joint_bf16', 'rnnt::joint_z16_kernel<rnnt::BF16, 8, true>', 'bf16_block'),
    ('joint_bf16', 'rnnt::joint_z_kernel<rnnt::BF16, 1, false, false>', 'bf16_a57'),
    ('joint_bf16', 'rnnt::joint_z_kernel<rnnt::BF16, 1, false, true>', 'bf16_a64_mis'),
    ('joint_bf16', 'rnnt::joint_z_kernel<rnnt::BF16, 1, true, false>', 'bf16_a64'),
    ('joint_bf16', 'rnnt::joint_z_kernel<rnnt::BF16, 1, true, true>', 'bf16_a64'),
    ('joint_bf16', 'rnnt::joint_z_kernel<rnnt::BF16, 4, false, false>', 'bf16_c16_mis'),
    ('joint_bf16', 'rnnt::joint_z_kernel<rnnt::BF16, 4, false, true>', 'bf16_c16_mis'),
    ('joint_bf16', 'rnnt::joint_z_kernel<rnnt::BF16, 4, true, false>', 'bf16_c16'),
    ('joint_bf16', 'rnnt::joint_z_kernel<rnnt::BF16, 4, true, true>', 'bf16_c16'),
    ('joint_bf16', 'rnnt::joint_z_kernel<rnnt::BF16, 8, false, false>', 'bf16_block_mis'),
    ('joint_bf16', 'rnnt::joint_z_kernel<rnnt::BF16, 8, false, true>', 'bf16_block_mis'),
    ('joint_bf16', 'rnnt::joint_z_small_kernel<rnnt::BF16>', 'bf16_a56'),
    ('joint_bf16', 'rnnt::lattice_kernel<float, 1, 1>', 'bf16_t1023'),
    ('joint_bf16', 'rnnt::lattice_kernel<float, 4, 2>', 'bf16_lat_42'),
    ('joint_bf16', 'rnnt::lattice_kernel<float, 8, 1>', 'bf16_lat_81'),
    ('joint_bf16', 'rnnt::lattice_kernel<float, 8, 2>', 'bf16_lat_82'),
    ('joint_bf16', 'rnnt::lattice_lin_kernel<0>', 'bf16_a56'),
    ('joint_f16', 'rnnt::coef_cell_kernel<float>', 'f16_a56'),
    ('joint_f16', 'rnnt::coef_kernel<float, true>', 'f16_u49'),
    ('joint_f16', 'rnnt::joint_df16_kernel<rnnt::F16, 4, true>', 'f16_block'),
    ('joint_f16', 'rnnt::joint_df_kernel<rnnt::F16, 1, true, false, false, false>', 'f16_a56'),
    ('joint_f16', 'rnnt::joint_df_kernel<rnnt::F16, 1, true, true, true, true>', 'f16_lat_81'),
    ('joint_f16', 'rnnt::joint_df_kernel<rnnt::F16, 2, true, false, false, false>', 'f16_c32_mis'),
    ('joint_f16', 'rnnt::joint_df_kernel<rnnt::F16, 2, true, true, true, true>', 'f16_u64'),
    ('joint_f16', 'rnnt::joint_df_kernel<rnnt::F16, 4, false, false, false, false>', 'f16_block_mis'),
    ('joint_f16', 'rnnt::joint_dg16_kernel<rnnt::F16, 4, true>', 'f16_block'),
    ('joint_f16', 'rnnt::joint_dg_kernel<rnnt::F16, 1, true, false>', 'f16_a57'),
    ('joint_f16', 'rnnt::joint_dg_kernel<rnnt::F16, 1, true, true>', 'f16_nk_t70_a33'),
    ('joint_f16', 'rnnt::joint_dg_kernel<rnnt::F16, 2, true, false>', 'f16_a56'),
    ('joint_f16', 'rnnt::joint_dg_kernel<rnnt::F16, 2, true, true>', 'f16_nk_u64_dg4'),
    ('joint_f16', 'rnnt::joint_dg_kernel<rnnt::F16, 4, false, false>', 'f16_a100'),
    ('joint_f16', 'rnnt::joint_dg_kernel<rnnt::F16, 4, true, true>', 'f16_t64'),
    ('joint_f16', 'rnnt::joint_far16_kernel<rnnt::F16>', 'f16_a56'),
    ('joint_f16', 'rnnt::joint_prep_kernel<0>', 'f16_a64'),
    ('joint_f16', 'rnnt::joint_rowmax_kernel<rnnt::F16, false, 0>', 'f16_a56'),
    ('joint_f16', 'rnnt::joint_rowmax_kernel<rnnt::F16, false, 1>', 'f16_a100'),
    ('joint_f16', 'rnnt::joint_rowmax_kernel<rnnt::F16, false, 4>', 'f16_block_mis'),
    ('joint_f16', 'rnnt::joint_rowmax_kernel<rnnt::F16, true, 1>', 'f16_c15'),
    ('joint_f16', 'rnnt::joint_rowmax_kernel<rnnt::F16, true, 4>', 'f16_block'),
    ('joint_f16', 'rnnt::joint_sums_kernel<0>', 'f16_a56'),
    ('joint_f16', 'rnnt::joint_z16_kernel<rnnt::F16, 1, false>', 'f16_t4096'),
    ('joint_f16', 'rnnt::joint_z16_kernel<rnnt::F16, 1, true>', 'f16_t4096'),
    ('joint_f16', 'rnnt::joint_z16_kernel<rnnt::F16, 4, false>', 'f16_c31'),
    ('joint_f16', 'rnnt::joint_z16_kernel<rnnt::F16, 4, true>', 'f16_c31'),
    ('joint_f16', 'rnnt::joint_z16_kernel<rnnt::F16, 8, false>', 'f16_block'),
    ('joint_f16', 'rnnt::joint_z16_kernel<rnnt::F16, 8, true>', 'f16_block'),
    ('joint_f16', 'rnnt::joint_z_kernel<rnnt::F16, 1, false, false>', 'f16_a57'),
    ('joint_f16', 'rnnt::joint_z_kernel<rnnt::F16, 1, false, true>', 'f16_a64_mis'),
    ('joint_f16', 'rnnt::joint_z_kernel<rnnt::F16, 1, true, false>', 'f16_a64'),
    ('joint_f16', 'rnnt::joint_z_kernel<rnnt::F16, 1, true, true>', 'f16_a64'),
    ('joint_f16', 'rnnt::joint_z_kernel<rnnt::F16, 4, false, false>', 'f16_c16_mis'),
    ('joint_f16', 'rnnt::joint_z_kernel<rnnt::F16, 4, false, true>', 'f16_c16_mis'),
    ('joint_f16', 'rnnt::joint_z_kernel<rnnt::F16, 4, true, false>', 'f16_c16'),
    ('joint_f16', 'rnnt::joint_z_kernel<rnnt::F16, 4, true, true>', 'f16_c16'),
    ('joint_f16', 'rnnt::joint_z_kernel<rnnt::F16, 8, false, false>', 'f16_block_mis'),
    ('joint_f16', 'rnnt::joint_z_kernel<rnnt::F16, 8, false, true>', 'f16_block_mis'),
    ('joint_f16', 'rnnt::joint_z_small_kernel<rnnt::F16>', 'f16_a56'),
    ('joint_f16', 'rnnt::lattice_kernel<float, 1, 1>', 'f16_t1023'),
    ('joint_f16', 'rnnt::lattice_kernel<float, 4, 2>', 'f16_lat_42'),
    ('joint_f16', 'rnnt::lattice_kernel<float, 8, 1>', 'f16_lat_81'),
    ('joint_f16', 'rnnt::lattice_kernel<float, 8, 2>', 'f16_lat_82'),
    ('joint_f16', 'rnnt::lattice_lin_kernel<0>', 'f16_a56'),
    ('joint_f32', 'rnnt::align_lattice_kernel<double>', 'f64_al_u64'),
    ('joint_f32', 'rnnt::align_lattice_kernel<float>', 'f32_al_add_u64'),
    ('joint_f32', 'rnnt::align_traceback_kernel<double>', 'f64_al_u64'),
    ('joint_f32', 'rnnt::align_traceback_kernel<float>', 'f32_al_add_u64'),
    ('joint_f32', 'rnnt::coef_cell_kernel<float>', 'f32_a56'),
    ('joint_f32', 'rnnt::coef_kernel<float, true>', 'f32_u49'),
    ('joint_f32', 'rnnt::joint_df_kernel<rnnt::F32, 1, true, false, false, false>', 'f32_nk_dg4'),
    ('joint_f32', 'rnnt::joint_df_kernel<rnnt::F32, 1, true, true, false, false>', 'f32_a56'),
    ('joint_f32', 'rnnt::joint_df_kernel<rnnt::F32, 1, true, true, false, true>', 'f32_u49'),
    ('joint_f32', 'rnnt::joint_df_kernel<rnnt::F32, 1, true, true, true, true>', 'f32_lat_81'),
    ('joint_f32', 'rnnt::joint_df_kernel<rnnt::F32, 2, true, false, false, false>', 'f32_block_mis'),
    ('joint_f32', 'rnnt::joint_df_kernel<rnnt::F32, 2, true, true, false, false>', 'f32_nk_a256'),
    ('joint_f32', 'rnnt::joint_df_kernel<rnnt::F32, 2, true, true, false, true>', 'f32_nk_a256_u70'),
    ('joint_f32', 'rnnt::joint_df_kernel<rnnt::F32, 2, true, true, true, true>', 'f32_u64'),
    ('joint_f32', 'rnnt::joint_df_kernel<rnnt::F32, 4, true, false, false, false>', 'f32_block'),
    ('joint_f32', 'rnnt::joint_dg_kernel<rnnt::F32, 1, true, false>', 'f32_a57'),
    ('joint_f32', 'rnnt::joint_dg_kernel<rnnt::F32, 1, true, true>', 'f32_nk_u64_dg4'),
    ('joint_f32', 'rnnt::joint_dg_kernel<rnnt::F32, 2, true, false>', 'f32_a56'),
    ('joint_f32', 'rnnt::joint_dg_kernel<rnnt::F32, 2, true, true>', 'f32_nk_t70_a50'),
    ('joint_f32', 'rnnt::joint_dg_kernel<rnnt::F32, 4, true, false>', 'f32_a100'),
    ('joint_f32', 'rnnt::joint_dg_kernel<rnnt::F32, 4, true, true>', 'f32_t64'),
    ('joint_f32', 'rnnt::joint_far_kernel<rnnt::F32>', 'f32_a56'),
    ('joint_f32', 'rnnt::joint_prep_kernel<0>', 'f32_a64'),
    ('joint_f32', 'rnnt::joint_rowmax_kernel<rnnt::F32, false, 0>', 'f32_a56'),
    ('joint_f32', 'rnnt::joint_rowmax_kernel<rnnt::F32, false, 1>', 'f32_a100_mis'),
    ('joint_f32', 'rnnt::joint_rowmax_kernel<rnnt::F32, false, 4>', 'f32_block_mis'),
    ('joint_f32', 'rnnt::joint_rowmax_kernel<rnnt::F32, true, 1>', 'f32_a100'),
    ('joint_f32', 'rnnt::joint_rowmax_kernel<rnnt::F32, true, 4>', 'f32_block'),
    ('joint_f32', 'rnnt::joint_sums_kernel<0>', 'f32_a56'),
    ('joint_f32', 'rnnt::joint_z_kernel<rnnt::F32, 1, false, false>', 'f32_a57'),
    ('joint_f32', 'rnnt::joint_z_kernel<rnnt::F32, 1, false, true>', 'f32_a64_mis'),
    ('joint_f32', 'rnnt::joint_z_kernel<rnnt::F32, 1, true, false>', 'f32_a64'),
    ('joint_f32', 'rnnt::joint_z_kernel<rnnt::F32, 1, true, true>', 'f32_a64'),
    ('joint_f32', 'rnnt::joint_z_kernel<rnnt::F32, 4, false, false>', 'f32_c16_mis'),
    ('joint_f32', 'rnnt::joint_z_kernel<rnnt::F32, 4, false, true>', 'f32_c16_mis'),
    ('joint_f32', 'rnnt::joint_z_kernel<rnnt::F32, 4, true, false>', 'f32_c16'),
    ('joint_f32', 'rnnt::joint_z_kernel<rnnt::F32, 4, true, true>', 'f32_c16'),
    ('joint_f32', 'rnnt::joint_z_kernel<rnnt::F32, 8, false, false>', 'f32_block_mis'),
    ('joint_f32', 'rnnt::joint_z_kernel<rnnt::F32, 8, false, true>', 'f32_block_mis'),
    ('joint_f32', 'rnnt::joint_z_kernel<rnnt::F32, 8, true, false>', 'f32_block'),
    ('joint_f32', 'rnnt::joint_z_kernel<rnnt::F32, 8, true, true>', 'f32_block'),
    ('joint_f32', 'rnnt::joint_z_small_kernel<rnnt::F32>', 'f32_a56'),
    ('joint_f32', 'rnnt::lattice_kernel<float, 1, 1>', 'f32_t1023'),
    ('joint_f32', 'rnnt::lattice_kernel<float, 4, 2>', 'f32_lat_42'),
    ('joint_f32', 'rnnt::lattice_kernel<float, 8, 1>', 'f32_lat_81'),
    ('joint_f32', 'rnnt::lattice_kernel<float, 8, 2>', 'f32_lat_82'),
    ('joint_f32', 'rnnt::lattice_lin_kernel<0>', 'f32_a56'),
]

# Instantiations the release build holds and no release rule of the joint launches, with the reason; "{tag}" is the object's
# store tag.  ALL: every joint object; F32 / H16: the fp32 object / both 16-bit ones.
_ALL, _F32, _H16 = ("joint_f32", "joint_bf16", "joint_f16"), ("joint_f32",), ("joint_bf16", "joint_f16")
_PF = "the operand ping-pong is on (Tune::jfpf / jgpf = 1) for fp32 storage and for fewer than four columns per lane"
_SPLIT_OH = "split_f needs maxU >= 64 and at most two column groups: A <= 64 (NKf = 1) or A <= 128 (NKf = 2, fp32 only)"
UNREACHABLE = [
    (_ALL, "rnnt::joint_df_kernel<{tag}, 1, false, false, false, false>", _PF),
    (_ALL, "rnnt::joint_df_kernel<{tag}, 2, false, false, false, false>", _PF),
    (_ALL, "rnnt::joint_df_kernel<{tag}, 1, true, false, true, false>",
     _SPLIT_OH + ", where the one-hot corrections are always on (A <= 256 fp32, onehot16 for 16-bit)"),
    (_ALL, "rnnt::joint_df_kernel<{tag}, 2, true, false, true, false>",
     _SPLIT_OH + ", where the one-hot corrections are always on (A <= 256 fp32, onehot16 for 16-bit)"),
    (_ALL, "rnnt::joint_df_kernel<{tag}, 1, true, true, true, false>",
     "split one-hot DF without the row-sum blank corrections: split_f implies maxU >= 64, hence the tiled coefficient "
     "kernel with its sums, so nocb holds (Tune::jnocb = 1)"),
    (_ALL, "rnnt::joint_df_kernel<{tag}, 2, true, true, true, false>",
     "split one-hot DF without the row-sum blank corrections: split_f implies maxU >= 64, hence nocb"),
    (_ALL, "rnnt::joint_df_kernel<{tag}, 4, true, true, false, false>",
     "four columns per lane need A >= 512 (fp32) / 1024 (16-bit), the one-hot corrections A <= 256"),
    (_ALL, "rnnt::joint_df_kernel<{tag}, 4, true, true, false, true>",
     "four columns per lane need A >= 512 (fp32) / 1024 (16-bit), the one-hot corrections A <= 256"),
    (_ALL, "rnnt::joint_dg_kernel<{tag}, 2, false, false>", _PF),
    (_F32, "rnnt::joint_df_kernel<{tag}, 4, false, false, false, false>", _PF),
    (_F32, "rnnt::joint_dg_kernel<{tag}, 1, false, false>", _PF),
    (_F32, "rnnt::joint_dg_kernel<{tag}, 4, false, false>", _PF),
    (_H16, "rnnt::joint_dg_kernel<{tag}, 1, false, false>", _PF),
    (_H16, "rnnt::joint_df_kernel<{tag}, 4, true, false, false, false>",
     "16-bit storage turns the operand ping-pong off at four columns per lane (AGPR budget)"),
    (_H16, "rnnt::joint_dg_kernel<{tag}, 4, true, false>",
     "16-bit storage turns the operand ping-pong off at four columns per lane (AGPR budget)"),
    (_H16, "rnnt::joint_df_kernel<{tag}, 1, true, true, false, false>",
     "16-bit one-hot DF is onehot16 only (A <= 64, maxU >= 64, tiled coefficients), which always has nocb"),
    (_H16, "rnnt::joint_df_kernel<{tag}, 2, true, true, false, false>",
     "16-bit one-hot DF is onehot16 only, which always has nocb"),
    (_H16, "rnnt::joint_df_kernel<{tag}, 1, true, true, false, true>",
     "onehot16 (A <= 64, maxU >= 64) always splits the contraction: at most two column groups"),
    (_H16, "rnnt::joint_df_kernel<{tag}, 2, true, true, false, true>",
     "onehot16 (A <= 64, maxU >= 64) always splits the contraction: at most two column groups"),
    (_H16, "rnnt::joint_z_kernel<{tag}, 8, true, false>",
     "S = 8 needs ceil(A / 32) >= 32 (A >= 993); vec then means A % 8 == 0 and aligned f, g: the matrix-core joint_z16_kernel"),
    (_H16, "rnnt::joint_z_kernel<{tag}, 8, true, true>",
     "S = 8 needs ceil(A / 32) >= 32 (A >= 993); vec then means A % 8 == 0 and aligned f, g: the matrix-core joint_z16_kernel"),
    (_H16, "rnnt::joint_df16_kernel<{tag}, 4, false>", "Tune::j16pf = 1: the matrix-core forms keep the operand ping-pong"),
    (_H16, "rnnt::joint_dg16_kernel<{tag}, 4, false>", "Tune::j16pf = 1: the matrix-core forms keep the operand ping-pong"),
    (_H16, "rnnt::joint_df16_kernel<{tag}, 8, true>", "Tune::j16nt = 4 columns per lane; 8 is the dev-build A/B form"),
    (_H16, "rnnt::joint_df16_kernel<{tag}, 8, false>", "Tune::j16nt = 4 and j16pf = 1"),
    (_H16, "rnnt::joint_dg16_kernel<{tag}, 8, true>", "Tune::j16nt = 4 columns per lane; 8 is the dev-build A/B form"),
    (_H16, "rnnt::joint_dg16_kernel<{tag}, 8, false>", "Tune::j16nt = 4 and j16pf = 1"),
]


def expected_inventory():
    """{object: {kernel: what covers it}} for the release build's three joint objects."""
    inv = {o: {} for o in JOBJECTS}
    for obj, k, case in FORMS:
        inv[obj][k] = "case " + case
    for objs, k, why in UNREACHABLE:
        for obj in objs:
            k2 = k.format(tag=JSTORES[{"joint_f32": "f32", "joint_bf16": "bf16", "joint_f16": "f16"}[obj]][1])
            assert k2 not in inv[obj], k2
            inv[obj][k2] = "unreachable: " + why
    return inv


# ----------------------------------------------------------------------------- the constants above, read from the source
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "warp-transducer_amd", "csrc")


def source_constants():
    """The values the rules above restate, parsed from the headers (tests/test_kernel_inventory.py compares them)."""
    def read(name):
        return open(os.path.join(CSRC, name)).read()
    kern, impl, host = read("rnnt_joint_kernels.h"), read("rnnt_joint_impl.h"), read("rnnt_host.h")
    align = read("rnnt_align_kernels.h")
    out = {"kJointZSmallA": int(re.search(r"constexpr int kJointZSmallA = (\d+);", kern).group(1)),
           "kAlignMaxWaves": int(re.search(r"constexpr int kAlignMaxWaves = (\d+);", align).group(1)),
           "kAlignLdsWords": int(re.search(r"constexpr int kAlignLdsWords = (\d+);", align).group(1))}
    # every 16-bit matrix-core gate (z16, df16, dg16) and its vocabulary bound
    out["mfma16_gates"] = re.findall(r"A % 8 == 0 (?:&& \(all4 & 15u\) == 0 )?&& A >= (\d+)", impl)
    out["sampled_min_a"] = int(re.search(r"const bool sampled = !small && A >= (\d+)", impl).group(1))
    out["rowmax_block_bytes"] = int(re.search(r"per_block = static_cast<size_t>\(A\) \* sizeof\(S\) >= (\d+)", impl).group(1))
    out["rowmax_lanes_a"] = int(re.search(r"per_lanes = A <= (\d+)", impl).group(1))
    m = re.search(r"int S = \(all_tiles >= (\d+) \|\| nchunk < (\d+)\) \? 1 : \(\(all_tiles < (\d+) && nchunk >= (\d+)\)", impl)
    out["z_split"] = tuple(int(x) for x in m.groups())
    out["coef_cell_max_u"] = int(re.search(r"coef_is_tiled\(const Plan<C>& p\) \{ return !\(p.maxU <= (\d+)", host).group(1))
    out["split_f_u"] = int(re.search(r"split_f = tn.jsplit && NKf <= 2 && maxU >= (\d+)", impl).group(1))
    m = re.search(r"split_g = tn.jsplit && maxT >= (\d+) && \(groups\(NKg\) <= 2 \|\| maxT >= (\d+)", impl)
    out["split_g_t"] = tuple(int(x) for x in m.groups())
    body = re.search(r"struct Tune \{(.*?)\};", host, re.S).group(1)
    out["tune"] = {k: int(v) for k, v in re.findall(r"(\w+) = (-?\d+)", body) if k in TUNE}
    return out


def restated_constants():
    return {"kJointZSmallA": JOINT_Z_SMALL_A, "kAlignMaxWaves": ALIGN_MAX_WAVES, "kAlignLdsWords": ALIGN_LDS_WORDS,
            "mfma16_gates": [str(MFMA16_MIN_A)] * 3, "sampled_min_a": SAMPLED_MIN_A, "rowmax_block_bytes": ROWMAX_BLOCK_BYTES,
            "rowmax_lanes_a": ROWMAX_LANES_A, "z_split": (Z_TILES_ONE, Z_CHUNKS_FOUR, Z_TILES_EIGHT, Z_CHUNKS_EIGHT),
            "coef_cell_max_u": COEF_CELL_MAX_U, "split_f_u": SPLIT_MIN_U, "split_g_t": (SPLIT_MIN_T, SPLIT_LONG_T), "tune": TUNE}
