"""The materialised path's kernel forms: which kernels the release build holds, the release rules that pick one per stage
(a restatement of launch_row_stats / launch_lattice / launch_coef / launch_grad, warp-transducer_amd/csrc), and one case per
form that reaches it.  tests/test_kernel_inventory.py checks the table against the code objects of libwarprnnt.so (no GPU);
tests/test_gpu_kernel_forms.py runs every case on the GPU, checks that the predicted kernel of each stage -- and no other --
ran, and compares the results with the fp64 oracle.  A threshold change that moves a form out of every case fails one of the
two, instead of leaving the form untested."""

# ----------------------------------------------------------------------------- release constants (csrc/rnnt_host.h, rnnt_kernels.h)
TILE_BUDGET = 52 * 1024            # Tune::tilekb
TILE_MAX_ROW_BYTES = 4096          # kTileMaxRowBytes
BLOCK_MIN_ROW_BYTES = 12288        # row_stats_block_kernel
TILE2D_MAX_ROW_BYTES = 208
PSKIPB, PSKIPMIN = 8192, 128       # Tune::pskipb, pskipmin
ONE_GROUP_BYTES = 32 << 20         # kOneGroupBytes
COEF_GROUPS = 8                    # kCoefGroups
OVERLAP_MIN_DIAGONALS = 768        # kOverlapMinDiagonals

# store type -> (object of the release build, store tag, lattice type, element bytes)
STORES = {"f32": ("f32", "rnnt::F32", "float", 4), "f64": ("f64", "rnnt::F64", "double", 8),
          "bf16": ("h16", "rnnt::BF16", "float", 2), "f16": ("h16", "rnnt::F16", "float", 2)}
OBJECTS = {"f32": "rnnt_gpu.hip", "f64": "rnnt_gpu_f64.hip", "h16": "rnnt_gpu_h16.hip"}

STAGES = ("stats", "lattice", "coef", "grad")


def stage_of(name):
    """Stage of a (demangled, argument-free) kernel name of the materialised path, or None."""
    base = name.split("<")[0].split("::")[-1]
    if base.startswith("row_stats"):
        return "stats"
    if base.startswith("lattice_kernel") or base.startswith("lattice_lin_kernel"):
        return "lattice"
    if base.startswith("coef_"):
        return "coef"
    if base.startswith("grad_") or base == "fill_row_scale_kernel":
        return "grad"
    return None


def tile_group(row_bytes):
    g = 1
    while g < 64 and (256 // g) * row_bytes + 32 > TILE_BUDGET:
        g *= 2
    return g


def tile_limit(g):
    """Largest row size (bytes) the tile kernel takes at lane group g."""
    return min((TILE_BUDGET - 32) // (256 // g), TILE_MAX_ROW_BYTES)


def lat_stride(u):
    return (u + 7) & ~7


def predict(case, cus):
    """{stage: set of kernel names} the release rules launch for `case` on a device with `cus` compute units."""
    N, T, U, A = case_shape(case, cus)
    obj, tag, lat, esz = STORES[case["dtype"]]
    rb = A * esz
    packed = case.get("layout") == "packed"
    training = case.get("train", True)
    misalign = case.get("misalign", False)
    out = {}
    # statistics (acts always 16-byte aligned here: torch allocations; grads at another 16-byte phase clear run_gpu's vec_ok,
    # which the tile and block forms need)
    vec_ok = not misalign
    if not packed and rb % 8 == 0 and rb <= TILE2D_MAX_ROW_BYTES and U >= 64 and (N * T * U * rb) % 16 == 0:
        out["stats"] = {"rnnt::row_stats_tile2d_kernel<%s, 16, 16>" % tag}
    elif vec_ok and rb <= TILE_MAX_ROW_BYTES and (256 // tile_group(rb)) * rb + 32 <= 64 * 1024:
        out["stats"] = {"rnnt::row_stats_tile_kernel<%s, %d>" % (tag, tile_group(rb))}
    elif vec_ok and rb >= BLOCK_MIN_ROW_BYTES:
        out["stats"] = {"rnnt::row_stats_block_kernel<%s, true, 4>" % tag}
    else:
        out["stats"] = {"rnnt::row_stats_kernel<%s, 4, true>" % tag}
    # lattice
    up = lat_stride(U)
    dirs = 2 if training else 1
    if up <= 64 and lat == "float" and N * dirs <= cus:
        out["lattice"] = {"rnnt::lattice_lin_kernel<0>"}
    elif up <= 64:
        out["lattice"] = {"rnnt::lattice_kernel<%s, 1, 1>" % lat}
    elif up <= 256:
        out["lattice"] = {"rnnt::lattice_kernel<%s, 8, 1>" % lat}
    elif up <= 512:
        out["lattice"] = {"rnnt::lattice_kernel<%s, 4, 2>" % lat}
    else:
        out["lattice"] = {"rnnt::lattice_kernel<%s, 8, 2>" % lat}
    # coefficients
    if training:
        out["coef"] = {"rnnt::coef_cell_kernel<%s>" % lat} if U <= 48 else {"rnnt::coef_kernel<%s, false>" % lat}
    # gradient
    if training and case.get("entry") != "fwd_only":
        scale = case.get("scale") is not None
        if misalign:
            out["grad"] = {"rnnt::grad_rows_kernel<%s, 4, %s>" % (tag, "true" if scale else "false")}
        elif packed and scale:
            out["grad"] = {"rnnt::fill_row_scale_kernel<%s>" % lat, "rnnt::grad_flat_kernel<%s, 2, 2, 0>" % tag}
        else:
            ps = 0 if packed else 1 if rb >= PSKIPB else 2 if rb >= PSKIPMIN else 0
            out["grad"] = {"rnnt::grad_flat_kernel<%s, %d, 2, %d>" % (tag, 1 if scale else 0, ps)}
    return out


def coef_launches(case, cus):
    """Launches of coef_cell_kernel (make_layout's group): more than one when the record table exceeds 32 MB."""
    N, T, U, A = case_shape(case, cus)
    lat = 8 if case["dtype"] == "f64" else 4
    rec1 = T * U * 4 * lat
    recs = rec1 * N
    if recs <= ONE_GROUP_BYTES:
        return 1
    head = max((recs + COEF_GROUPS - 1) // COEF_GROUPS, ONE_GROUP_BYTES, rec1)
    group = min(head // rec1, N)
    return (N + group - 1) // group


def case_shape(case, cus):
    n = case["N"]
    if isinstance(n, str):                          # relative to the compute-unit count: "cus//2" or "cus//2+1"
        assert n in ("cus//2", "cus//2+1"), n
        n = cus // 2 + (1 if n.endswith("+1") else 0)
    return int(n), case["T"], case["U"], case["A"]


# ----------------------------------------------------------------------------- the cases
def _row_bytes_cases():
    """Statistics forms by row size: each tile lane group just below and above its boundaries, kTileMaxRowBytes, the
    wavefront and block forms; tile2d at 200 / 208 / 216 bytes and maxU 63 / 64."""
    cases = []
    for d, (_, _, _, esz) in STORES.items():
        sizes = set()
        for g in (1, 2, 4, 8, 16, 32):
            hi = tile_limit(g) // esz * esz                       # largest row of this group
            sizes.add(hi)
            sizes.add(hi + esz)                                   # smallest of the next form
        sizes |= {esz, TILE_MAX_ROW_BYTES, TILE_MAX_ROW_BYTES + esz, PSKIPB - esz, PSKIPB, BLOCK_MIN_ROW_BYTES - esz, BLOCK_MIN_ROW_BYTES}
        for rb in sorted(s for s in sizes if s % esz == 0):
            cases.append({"name": "%s_rb%d" % (d, rb), "dtype": d, "N": 2, "T": 3, "U": 3, "A": rb // esz, "entry": "async"})
        for rb in (200, 208, 216):
            for u in (63, 64):
                if rb % esz == 0:
                    cases.append({"name": "%s_t2d_rb%d_u%d" % (d, rb, u), "dtype": d, "N": 2, "T": 2, "U": u, "A": rb // esz,
                                  "entry": "call"})
    return cases


def _other_cases():
    cases = []
    for d in STORES:
        big = 8192 // STORES[d][3]                 # A of an 8 KB row: skip-padded-rows form 1
        cases += [
            # lattice forms (the linear chain / one-wavefront form on either side of N * dirs vs the CU count)
            {"name": d + "_lat_lin", "dtype": d, "N": "cus//2", "T": 3, "U": 5, "A": 3, "entry": "async"},
            {"name": d + "_lat_11", "dtype": d, "N": "cus//2+1", "T": 3, "U": 5, "A": 3, "entry": "async"},
            {"name": d + "_lat_81", "dtype": d, "N": 2, "T": 3, "U": 100, "A": 2, "entry": "twophase"},
            {"name": d + "_lat_42", "dtype": d, "N": 2, "T": 3, "U": 300, "A": 2, "entry": "async", "scale": "ragged"},
            {"name": d + "_lat_82", "dtype": d, "N": 2, "T": 3, "U": 600, "A": 2, "entry": "call"},
            # gradient: SCALE x PADSKIP (padded: per-sample scale; packed: per-row scale)
            {"name": d + "_g_s1_p0", "dtype": d, "N": 3, "T": 4, "U": 3, "A": 5, "entry": "async", "scale": "ragged"},
            {"name": d + "_g_s1_p1", "dtype": d, "N": 2, "T": 2, "U": 2, "A": big, "entry": "twophase", "scale": "ragged"},
            {"name": d + "_g_s1_p2", "dtype": d, "N": 3, "T": 4, "U": 3, "A": 300 // STORES[d][3], "entry": "twophase", "scale": "ragged"},
            {"name": d + "_g_s0_p1", "dtype": d, "N": 2, "T": 2, "U": 2, "A": big, "entry": "call"},
            {"name": d + "_g_s2_p0", "dtype": d, "N": 3, "T": 4, "U": 3, "A": 7, "layout": "packed", "entry": "packed", "scale": "ragged"},
            {"name": d + "_g_s2_p0_2ph", "dtype": d, "N": 3, "T": 5, "U": 60, "A": 9, "layout": "packed", "entry": "packed_twophase",
             "scale": "ragged"},
            {"name": d + "_g_packed_s0", "dtype": d, "N": 3, "T": 4, "U": 3, "A": 7, "layout": "packed", "entry": "packed"},
            # acts and grads at different 16-byte phases: the row-form gradient kernel
            {"name": d + "_g_rows", "dtype": d, "N": 2, "T": 3, "U": 4, "A": 6, "entry": "async", "misalign": True},
            {"name": d + "_g_rows_s", "dtype": d, "N": 2, "T": 3, "U": 4, "A": 6, "entry": "async", "misalign": True, "scale": "ragged"},
        ]
    # the cell-per-thread coefficient kernel in several launches (record table > 32 MB, maxU <= 48)
    cases += [{"name": "f32_coef_groups", "dtype": "f32", "N": 1400, "T": 32, "U": 48, "A": 2, "entry": "async", "scale": "ragged"},
              {"name": "f64_coef_groups", "dtype": "f64", "N": 700, "T": 32, "U": 48, "A": 2, "entry": "async"},
              {"name": "bf16_coef_groups", "dtype": "bf16", "N": 1400, "T": 32, "U": 48, "A": 2, "entry": "twophase"}]
    # the two-half schedule with a per-sample scale, cut at n0 != N/2 (fp32: a sample's slab is 12 mod 16 bytes, N/2 = 3 cannot be the cut)
    cases += [{"name": "f32_two_half", "dtype": "f32", "N": 6, "T": 761, "U": 9, "A": 3, "entry": "async", "scale": "ragged", "aux": True,
               "n0": 4},
              {"name": "bf16_two_half", "dtype": "bf16", "N": 6, "T": 761, "U": 9, "A": 4, "entry": "async", "scale": "ragged", "aux": True,
               "n0": 2}]                     # (8 mod 16 bytes: the cut below N/2)
    return cases


CASES = {c["name"]: c for c in _row_bytes_cases() + _other_cases()}


def two_half_cut(case):
    """n0 of run_gpu for a two-half case: the sample count nearest N/2 whose slab is whole 16-byte packets."""
    N, T, U, A = case["N"], case["T"], case["U"], case["A"]
    per = T * U * A * STORES[case["dtype"]][3]
    for d in range(9):
        for c in (N // 2 - d, N // 2 + d):
            if 1 <= c < N and (per * c) % 16 == 0:
                return c
    return None


# ----------------------------------------------------------------------------- the inventory
def predicted_rows(cus=256):
    """{(object, kernel): [cases]} that the release rules reach with CASES on a device of `cus` compute units."""
    rows = {}
    for name, c in CASES.items():
        obj = STORES[c["dtype"]][0]
        for ks in predict(c, cus).values():
            for k in ks:
                rows.setdefault((obj, k), []).append(name)
    return rows


# One row per launched form: (object, kernel, the case that reaches it).  Written out, not derived: deleting a row, or a form
# the build gains or loses, fails tests/test_kernel_inventory.py.
FORMS = [
    ('f32', 'rnnt::coef_cell_kernel<float>', 'f32_rb4'),
    ('f32', 'rnnt::coef_kernel<float, false>', 'f32_t2d_rb200_u63'),
    ('f32', 'rnnt::fill_row_scale_kernel<float>', 'f32_g_s2_p0'),
    ('f32', 'rnnt::grad_flat_kernel<rnnt::F32, 0, 2, 0>', 'f32_rb4'),
    ('f32', 'rnnt::grad_flat_kernel<rnnt::F32, 0, 2, 1>', 'f32_rb8192'),
    ('f32', 'rnnt::grad_flat_kernel<rnnt::F32, 0, 2, 2>', 'f32_rb204'),
    ('f32', 'rnnt::grad_flat_kernel<rnnt::F32, 1, 2, 0>', 'f32_lat_42'),
    ('f32', 'rnnt::grad_flat_kernel<rnnt::F32, 1, 2, 1>', 'f32_g_s1_p1'),
    ('f32', 'rnnt::grad_flat_kernel<rnnt::F32, 1, 2, 2>', 'f32_g_s1_p2'),
    ('f32', 'rnnt::grad_flat_kernel<rnnt::F32, 2, 2, 0>', 'f32_g_s2_p0'),
    ('f32', 'rnnt::grad_rows_kernel<rnnt::F32, 4, false>', 'f32_g_rows'),
    ('f32', 'rnnt::grad_rows_kernel<rnnt::F32, 4, true>', 'f32_g_rows_s'),
    ('f32', 'rnnt::lattice_kernel<float, 1, 1>', 'f32_lat_11'),
    ('f32', 'rnnt::lattice_kernel<float, 4, 2>', 'f32_lat_42'),
    ('f32', 'rnnt::lattice_kernel<float, 8, 1>', 'f32_lat_81'),
    ('f32', 'rnnt::lattice_kernel<float, 8, 2>', 'f32_lat_82'),
    ('f32', 'rnnt::lattice_lin_kernel<0>', 'f32_rb4'),
    ('f32', 'rnnt::row_stats_block_kernel<rnnt::F32, true, 4>', 'f32_rb12288'),
    ('f32', 'rnnt::row_stats_kernel<rnnt::F32, 4, true>', 'f32_rb4100'),
    ('f32', 'rnnt::row_stats_tile2d_kernel<rnnt::F32, 16, 16>', 'f32_t2d_rb200_u64'),
    ('f32', 'rnnt::row_stats_tile_kernel<rnnt::F32, 16>', 'f32_rb1664'),
    ('f32', 'rnnt::row_stats_tile_kernel<rnnt::F32, 1>', 'f32_rb4'),
    ('f32', 'rnnt::row_stats_tile_kernel<rnnt::F32, 2>', 'f32_rb208'),
    ('f32', 'rnnt::row_stats_tile_kernel<rnnt::F32, 32>', 'f32_rb3328'),
    ('f32', 'rnnt::row_stats_tile_kernel<rnnt::F32, 4>', 'f32_rb416'),
    ('f32', 'rnnt::row_stats_tile_kernel<rnnt::F32, 8>', 'f32_rb832'),
    ('f64', 'rnnt::coef_cell_kernel<double>', 'f64_rb8'),
    ('f64', 'rnnt::coef_kernel<double, false>', 'f64_t2d_rb200_u63'),
    ('f64', 'rnnt::fill_row_scale_kernel<double>', 'f64_g_s2_p0'),
    ('f64', 'rnnt::grad_flat_kernel<rnnt::F64, 0, 2, 0>', 'f64_rb8'),
    ('f64', 'rnnt::grad_flat_kernel<rnnt::F64, 0, 2, 1>', 'f64_rb8192'),
    ('f64', 'rnnt::grad_flat_kernel<rnnt::F64, 0, 2, 2>', 'f64_rb200'),
    ('f64', 'rnnt::grad_flat_kernel<rnnt::F64, 1, 2, 0>', 'f64_lat_42'),
    ('f64', 'rnnt::grad_flat_kernel<rnnt::F64, 1, 2, 1>', 'f64_g_s1_p1'),
    ('f64', 'rnnt::grad_flat_kernel<rnnt::F64, 1, 2, 2>', 'f64_g_s1_p2'),
    ('f64', 'rnnt::grad_flat_kernel<rnnt::F64, 2, 2, 0>', 'f64_g_s2_p0'),
    ('f64', 'rnnt::grad_rows_kernel<rnnt::F64, 4, false>', 'f64_g_rows'),
    ('f64', 'rnnt::grad_rows_kernel<rnnt::F64, 4, true>', 'f64_g_rows_s'),
    ('f64', 'rnnt::lattice_kernel<double, 1, 1>', 'f64_rb8'),
    ('f64', 'rnnt::lattice_kernel<double, 4, 2>', 'f64_lat_42'),
    ('f64', 'rnnt::lattice_kernel<double, 8, 1>', 'f64_lat_81'),
    ('f64', 'rnnt::lattice_kernel<double, 8, 2>', 'f64_lat_82'),
    ('f64', 'rnnt::row_stats_block_kernel<rnnt::F64, true, 4>', 'f64_rb12288'),
    ('f64', 'rnnt::row_stats_kernel<rnnt::F64, 4, true>', 'f64_rb4104'),
    ('f64', 'rnnt::row_stats_tile2d_kernel<rnnt::F64, 16, 16>', 'f64_t2d_rb200_u64'),
    ('f64', 'rnnt::row_stats_tile_kernel<rnnt::F64, 16>', 'f64_rb1664'),
    ('f64', 'rnnt::row_stats_tile_kernel<rnnt::F64, 1>', 'f64_rb8'),
    ('f64', 'rnnt::row_stats_tile_kernel<rnnt::F64, 2>', 'f64_rb208'),
    ('f64', 'rnnt::row_stats_tile_kernel<rnnt::F64, 32>', 'f64_rb3328'),
    ('f64', 'rnnt::row_stats_tile_kernel<rnnt::F64, 4>', 'f64_rb416'),
    ('f64', 'rnnt::row_stats_tile_kernel<rnnt::F64, 8>', 'f64_rb832'),
    ('h16', 'rnnt::coef_cell_kernel<float>', 'bf16_rb2'),
    ('h16', 'rnnt::coef_kernel<float, false>', 'bf16_t2d_rb200_u63'),
    ('h16', 'rnnt::fill_row_scale_kernel<float>', 'bf16_g_s2_p0'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::BF16, 0, 2, 0>', 'bf16_rb2'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::BF16, 0, 2, 1>', 'bf16_rb8192'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::BF16, 0, 2, 2>', 'bf16_rb206'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::BF16, 1, 2, 0>', 'bf16_lat_42'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::BF16, 1, 2, 1>', 'bf16_g_s1_p1'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::BF16, 1, 2, 2>', 'bf16_g_s1_p2'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::BF16, 2, 2, 0>', 'bf16_g_s2_p0'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::F16, 0, 2, 0>', 'f16_rb2'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::F16, 0, 2, 1>', 'f16_rb8192'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::F16, 0, 2, 2>', 'f16_rb206'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::F16, 1, 2, 0>', 'f16_lat_42'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::F16, 1, 2, 1>', 'f16_g_s1_p1'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::F16, 1, 2, 2>', 'f16_g_s1_p2'),
    ('h16', 'rnnt::grad_flat_kernel<rnnt::F16, 2, 2, 0>', 'f16_g_s2_p0'),
    ('h16', 'rnnt::grad_rows_kernel<rnnt::BF16, 4, false>', 'bf16_g_rows'),
    ('h16', 'rnnt::grad_rows_kernel<rnnt::BF16, 4, true>', 'bf16_g_rows_s'),
    ('h16', 'rnnt::grad_rows_kernel<rnnt::F16, 4, false>', 'f16_g_rows'),
    ('h16', 'rnnt::grad_rows_kernel<rnnt::F16, 4, true>', 'f16_g_rows_s'),
    ('h16', 'rnnt::lattice_kernel<float, 1, 1>', 'bf16_lat_11'),
    ('h16', 'rnnt::lattice_kernel<float, 4, 2>', 'bf16_lat_42'),
    ('h16', 'rnnt::lattice_kernel<float, 8, 1>', 'bf16_lat_81'),
    ('h16', 'rnnt::lattice_kernel<float, 8, 2>', 'bf16_lat_82'),
    ('h16', 'rnnt::lattice_lin_kernel<0>', 'bf16_rb2'),
    ('h16', 'rnnt::row_stats_block_kernel<rnnt::BF16, true, 4>', 'bf16_rb12288'),
    ('h16', 'rnnt::row_stats_block_kernel<rnnt::F16, true, 4>', 'f16_rb12288'),
    ('h16', 'rnnt::row_stats_kernel<rnnt::BF16, 4, true>', 'bf16_rb4098'),
    ('h16', 'rnnt::row_stats_kernel<rnnt::F16, 4, true>', 'f16_rb4098'),
    ('h16', 'rnnt::row_stats_tile2d_kernel<rnnt::BF16, 16, 16>', 'bf16_t2d_rb200_u64'),
    ('h16', 'rnnt::row_stats_tile2d_kernel<rnnt::F16, 16, 16>', 'f16_t2d_rb200_u64'),
    ('h16', 'rnnt::row_stats_tile_kernel<rnnt::BF16, 16>', 'bf16_rb1664'),
    ('h16', 'rnnt::row_stats_tile_kernel<rnnt::BF16, 1>', 'bf16_rb2'),
    ('h16', 'rnnt::row_stats_tile_kernel<rnnt::BF16, 2>', 'bf16_rb208'),
    ('h16', 'rnnt::row_stats_tile_kernel<rnnt::BF16, 32>', 'bf16_rb3328'),
    ('h16', 'rnnt::row_stats_tile_kernel<rnnt::BF16, 4>', 'bf16_rb416'),
    ('h16', 'rnnt::row_stats_tile_kernel<rnnt::BF16, 8>', 'bf16_rb832'),
    ('h16', 'rnnt::row_stats_tile_kernel<rnnt::F16, 16>', 'f16_rb1664'),
    ('h16', 'rnnt::row_stats_tile_kernel<rnnt::F16, 1>', 'f16_rb2'),
    ('h16', 'rnnt::row_stats_tile_kernel<rnnt::F16, 2>', 'f16_rb208'),
    ('h16', 'rnnt::row_stats_tile_kernel<rnnt::F16, 32>', 'f16_rb3328'),
    ('h16', 'rnnt::row_stats_tile_kernel<rnnt::F16, 4>', 'f16_rb416'),
    ('h16', 'rnnt::row_stats_tile_kernel<rnnt::F16, 8>', 'f16_rb832'),
]

# Instantiations the release build holds and the release rules never launch on the materialised path -- listed so that the
# exclusion is visible (and fails the inventory once a rule starts reaching one, or the build drops it).
UNREACHABLE = {
    "rnnt::row_stats_tile_kernel<{tag}, 64>": "kTileMaxRowBytes = 4096 caps the lane group at 32 (64 needs rows > 6652 bytes)",
    "rnnt::row_stats_tile2d_kernel<{tag}, 8, 32>": "Tune::tile2d = 2 (16 x 16 tiles) in a release build; 8 x 32 is the dev-build A/B form",
}
# Kernels of the materialised objects outside the four stages, and where they are tested.
OTHER = {
    "f32": {"rnnt::lattice_dump_kernel<float>": "compute_rnnt_loss_lattice_dump: tests/test_gpu_lattice_dump.py",
            "rnnt::lattice_dump_kernel<double>": "compute_rnnt_loss_lattice_dump: tests/test_gpu_lattice_dump.py",
            "rnnt::loss_sum_kernel<float>": "compute_rnnt_loss_sharded: tests/test_gpu_sharded_rccl.py",
            "rnnt::loss_sum_kernel<double>": "compute_rnnt_loss_sharded: tests/test_gpu_sharded_rccl.py"},
}
# RNNT_DEV-only forms (row_stats_kernel<.., 2|8, ..>, row_stats_block_kernel<.., false, ..>, grad_flat_kernel<.., 0, 1|4, 0>) are
# not in a release build at all; the inventory fails if one appears there.  The additive joint's objects (rnnt_joint*.hip) have
# their table in tests/joint_forms.py.


def expected_inventory():
    """{object: {kernel: what covers it}} for the release build."""
    inv = {o: {} for o in OBJECTS}
    for obj, k, case in FORMS:
        inv[obj][k] = "case " + case
    for d, (obj, tag, lat, _) in STORES.items():
        for k, why in UNREACHABLE.items():
            inv[obj][k.format(tag=tag, lat=lat)] = "unreachable: " + why
    for obj, ks in OTHER.items():
        for k, why in ks.items():
            inv[obj][k] = "outside the four stages: " + why
    return inv
