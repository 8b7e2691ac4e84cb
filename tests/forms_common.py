"""What the form tables of the side libraries (tests/pruned_forms.py, tdt_forms.py, hat_forms.py) share: the stores, the
lattice rule of launch_lattice (csrc/rnnt_host.h) and the scaffolding that turns CASES and predict into the rows a device
reaches and the inventory the code objects must hold."""
from tests import kernel_forms as K

# dtype -> (object, store tag, lattice type, element bytes)
STORES = {"f32": ("f32", "rnnt::F32", "float", 4), "f64": ("f64", "rnnt::F64", "double", 8),
          "bf16": ("h16", "rnnt::BF16", "float", 2), "f16": ("h16", "rnnt::F16", "float", 2)}


def object_of(case):
    return STORES[case["dtype"]][0]


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
