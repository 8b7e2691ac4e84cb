"""No GPU: the kernel launches of the side libraries' host drivers (csrc/rnnt_*_impl.h), read from the sources, for
tests/test_side_limits_table.py (not collected, not a conftest).

Per hipLaunchKernelGGL statement: the kernel's base name (a macro parameter in the kernel's place is resolved through the
macro's uses), the grid expression (a dim3 variable is resolved to its initialiser) and its class --
  sliced   the statement sits in a `for (int b0 ...` loop or passes b0: the samples go over a grid dimension in slices
  elem     the grid is elem_grid(E): at most 65536 blocks, a grid-stride loop over the elements
  jn_row   the grid is jn_row_grid(rows, per_block): at most kJnMaxGrid blocks
  lp       the grid is lp_grid(work, per_block): at most kLpMaxGrid blocks
  whole_n  N itself is a component of the grid and there is no loop: legal on grid.x (2^31 - 1), a limit on grid.y / z
  other    none of these (grids of N / 256 blocks, the flat packet streams)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warp-transducer_amd", "csrc")
SIDE = ("tdt", "mblank", "mono", "ar", "delay", "pstream", "pruned", "hat", "kd", "mi", "bestpath", "tdt_align", "joiner",
        "logprobs")
CAPS = {"elem_grid": "elem", "jn_row_grid": "jn_row", "lp_grid": "lp"}


def _balanced(text, i):
    """text[i] == '(' -> the index just past its matching ')'."""
    depth = 0
    for j in range(i, len(text)):
        if text[j] == "(":
            depth += 1
        elif text[j] == ")":
            depth -= 1
            if depth == 0:
                return j + 1
    raise ValueError("unbalanced parentheses at %d" % i)


def _split_args(text):
    """The top-level comma-separated arguments of `text` (parentheses, braces and template brackets of casts nest)."""
    out, depth, cur = [], 0, ""
    for ch in text:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def _loops(text):
    """[(start, end)] of the bodies of the `for (int b0 ...` loops."""
    out = []
    for m in re.finditer(r"for\s*\(\s*int\s+b0\b", text):
        j = _balanced(text, text.index("(", m.start()))
        while text[j] in " \t\n\\":
            j += 1
        if text[j] == "{":
            depth, k = 0, j
            while True:
                depth += {"{": 1, "}": -1}.get(text[k], 0)
                k += 1
                if depth == 0:
                    break
            out.append((j, k))
        else:                                                      # a single statement: up to its ';' outside parentheses
            depth, k = 0, j
            while not (text[k] == ";" and depth == 0):
                depth += {"(": 1, ")": -1}.get(text[k], 0)
                k += 1
            out.append((j, k + 1))
    return out


def _macro_uses(text, pos, param):
    """The kernel names a macro is used with, where the launch at `pos` has the macro's parameter in the kernel's place."""
    defs = [m for m in re.finditer(r"#define\s+(\w+)\(([^)]*)\)", text) if m.start() < pos]
    assert defs, param
    d = defs[-1]
    assert param in [p.strip() for p in d.group(2).split(",")], (d.group(0), param)
    at = [p.strip() for p in d.group(2).split(",")].index(param)
    names = set()
    for u in re.finditer(r"\b%s\(" % d.group(1), text):
        if u.start() <= d.end():
            continue
        args = _split_args(text[u.end():_balanced(text, u.end() - 1) - 1])
        names.add(args[at])
    assert names, d.group(1)
    return names


def _grid_text(text, pos, arg):
    """The grid argument of a launch, a dim3 variable replaced by its nearest initialiser in front of the launch."""
    if not re.fullmatch(r"[A-Za-z_]\w*", arg):
        return arg
    best = None
    for m in re.finditer(r"\b%s\(" % re.escape(arg), text[:pos]):
        stmt = text[text.rfind(";", 0, m.start()) + 1:m.start()]
        if "dim3" in stmt:
            best = m
    assert best is not None, arg
    return text[best.end():_balanced(text, best.end() - 1) - 1]


def launches(lib):
    """[{kernel, klass, grid, line, stmt}] of the launches in csrc/rnnt_<lib>_impl.h; stmt: the statement's position in the
    source (a statement inside a macro that is used with several kernels gives one entry per kernel, all of the same stmt)."""
    text = open(os.path.join(CSRC, "rnnt_%s_impl.h" % lib)).read()
    text = re.sub(r"//[^\n]*", lambda m: " " * len(m.group(0)), text)          # (comments out, positions kept)
    loops = _loops(text)
    out = []
    for m in re.finditer(r"hipLaunchKernelGGL\(", text):
        end = _balanced(text, m.end() - 1)
        args = _split_args(text[m.end():end - 1].replace("\\\n", " "))
        kern = args[0].strip("() ")
        base = kern.split("<")[0]
        names = _macro_uses(text, m.start(), base) if base.isupper() else {base}
        grid = _grid_text(text, m.start(), args[1])
        body = " ".join(args[1:])
        cap = next((c for fn, c in CAPS.items() if fn + "(" in grid), None)
        if any(a <= m.start() < b for a, b in loops) or re.search(r"\bb0\b", body):
            klass = "sliced"
        elif cap:
            klass = cap
        elif any(re.fullmatch(r"(\w+\.)?N", c) for c in _split_args(re.sub(r"^dim3\((.*)\)$", r"\1", grid.strip()))):
            klass = "whole_n"
        else:
            klass = "other"
        for n in sorted(names):
            out.append(dict(kernel=n, klass=klass, grid=" ".join(grid.split()), line=text.count("\n", 0, m.start()) + 1,
                            stmt=m.start()))
    return out


def by_class(lib):
    """{class: set of kernel base names} of one library."""
    out = {}
    for l in launches(lib):
        out.setdefault(l["klass"], set()).add(l["kernel"])
    return out
