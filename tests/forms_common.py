"""What the form tables of the side libraries (tests/pruned_forms.py, tdt_forms.py, hat_forms.py, ...) share: the stores, the
lanes per row of the statistics kernels and the corners of their shared row reduction, the lattice rule of launch_lattice (csrc/rnnt_host.h) and the scaffolding that turns CASES and predict into the rows a device
reaches and the inventory the code objects must hold."""
from tests import kernel_forms as K

# dtype -> (object, store tag, lattice type, element bytes)
STORES = {"f32": ("f32", "rnnt::F32", "float", 4), "f64": ("f64", "rnnt::F64", "double", 8),
          "bf16": ("h16", "rnnt::BF16", "float", 2), "f16": ("h16", "rnnt::F16", "float", 2)}


def object_of(case):
    return STORES[case["dtype"]][0]


def stats_group(row_bytes, wide_bytes=2048, narrow_bytes=256):
    """stats_grid (csrc/rnnt_side_host.h): the lanes per row of a statistics kernel -- 4 up to 256 bytes, 16 up to
    `wide_bytes` (HAT: 4096), else 64."""
    return 4 if row_bytes <= narrow_bytes else 16 if row_bytes <= wide_bytes else 64


def row_corners(esz, A, G, off=0, stride=None):
    """What the rows of a tensor reach in row_lse (csrc/rnnt_row_lse.h): A elements of `esz` bytes read by G lanes, row r
    at byte off + r * stride * esz (stride: elements from row to row, A unless the row holds more columns).
    -> (skip, rounds): some row starts off a 16-byte boundary; the rounds of four packets per lane EVERY row takes."""
    V = 16 // esz
    skips = {((off + r * (stride or A) * esz) % 16) // esz for r in range(16)}
    return any(skips), min(-(-((s + A + V - 1) // V) // (4 * G)) for s in skips)


def lattice_form(lat, U, N, dirs, cus):
    up = K.lat_stride(U)
    if lat == "float" and up <= 64 and N * dirs <= cus:
        return "rnnt::lattice_lin_kernel<0>"
    if up <= 64:
        return "rnnt::lattice_kernel<%s, 1, 1>" % lat
    if up <= 256:
        return "rnnt::lattice_kernel<%s, 8, 1>" % lat
    if up <= 512:
        return "rnnt::lattice_kernel<%s, 4, 2>" % lat
    return "rnnt::lattice_kernel<%s, 8, 2>" % lat


def predicted_rows(cases, predict, cus):
    """{(object, kernel): [cases]} the release rules reach with `cases` on a device of `cus` compute units."""
    rows = {}
    for name, c in cases.items():
        for ks in predict(c, cus).values():
            for k in ks:
                rows.setdefault((object_of(c), k), []).append(name)
    return rows


def expected_inventory(objects, rows, unreachable):
    """{object: set of kernels} the code objects must hold exactly: the reached rows and the listed unreachable ones."""
    inv = {o: set() for o in objects}
    for obj, k in list(rows) + list(unreachable):
        inv[obj].add(k)
    return inv
