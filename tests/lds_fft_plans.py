"""The runtime LDS FFT planner (csrc/hip/lds_fft_plan.h) as the tests see it:
tests/lds_fft_plan_query.cc compiled and asked, the invariants every plan must
keep, the plan-space classes and a covering set of lengths, and the thin
planes of tests/test_lds_fft_sweep_gpu.py.

The invariants take plain values (radices, counts), so that
tests/test_lds_fft_plan.py can feed them doctored plans as well as the
planner's own. Nothing here restates the planner: every number comes from the
query program.
"""
import collections
import functools
import math
import os
import subprocess

import numpy as np

import fft_plans as fp

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT = 10240          # the issue's length limit; asserted against the header's
SWEEP_LAST = 2 * LIMIT

Length = collections.namedtuple(
    "Length", "n f64 factorized max_len count radices can_split n1 n2 cols")
Pass = collections.namedtuple("Pass", "sub_len groups n_groups n_cols col_tiles grid lds")
PlanePlan = collections.namedtuple("PlanePlan", "w h f64 ok row_count col_count split a b")
Constants = collections.namedtuple("Constants", "threads max_passes lds_bytes max_wg_elems bpt")

ALLOWED = {False: {2, 3, 4, 5, 7, 8, 9, 16}, True: {2, 3, 4, 5, 7, 8}}
BIG2 = {False: 16, True: 8}        # the repeated power-of-two radix
COLS_CAP = {False: 32, True: 16}   # split passes: adjacent columns per tile
ALWAYS = (2, 3, 5, 7, 9, 15, 105, 10125, 10240)


def elem_bytes(f64):
    return 16 if f64 else 8


def is_smooth(n):
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def _host_build():
    from test_subminor_plan import _host_build as hb
    return hb()


def compile_query(directory):
    b = _host_build()
    exe = os.path.join(str(directory), "lds_fft_plan_query")
    subprocess.run([b.CXX, *b.CXX_FLAGS, os.path.join(HERE, "lds_fft_plan_query.cc"), "-o", exe],
                   check=True)
    return exe


def _length(fields):
    n, f64, ok, max_len, count = (int(v) for v in fields[1:6])
    radices = () if fields[6] == "-" else tuple(int(r) for r in fields[6].split(","))
    can_split, n1, n2, cols = (int(v) for v in fields[7:11])
    return Length(n, bool(f64), bool(ok), max_len, count, radices, bool(can_split), n1, n2, cols)


class Planner:
    """The compiled query program."""

    def __init__(self, exe):
        self.exe = exe

    def _run(self, *args):
        out = subprocess.run([self.exe, *map(str, args)], check=True, capture_output=True,
                             text=True).stdout
        return [line.split() for line in out.splitlines()]

    @functools.lru_cache(maxsize=None)
    def constants(self):
        lines = self._run("constants")
        c = [int(v) for v in lines[0][1:]]
        return Constants(*c, {int(l[1]): int(l[2]) for l in lines[1:]})

    @functools.lru_cache(maxsize=None)
    def sweep(self, f64, first=2, last=SWEEP_LAST):
        """{n: Length} for first <= n <= last."""
        return {p.n: p for p in map(_length, self._run("sweep", first, last, int(f64)))}

    def length(self, n, f64):
        return _length(self._run(n, int(f64))[0])

    @functools.lru_cache(maxsize=None)
    def plane(self, w, h, f64, columns=0):
        lines = self._run(w, h, int(f64), columns)
        head = [int(v) for v in lines[0][1:]]
        passes = {l[0]: Pass(*(int(v) for v in l[1:])) for l in lines[1:]}
        return PlanePlan(head[0], head[1], bool(head[2]), bool(head[3]), head[4], head[5],
                         bool(head[6]), passes.get("A"), passes.get("B"))

    def accepted(self, f64):
        """{n: Length} of the lengths rdl_conv_create_ex takes."""
        return {n: p for n, p in self.sweep(f64).items() if p.factorized and n <= p.max_len}


# ---------------------------------------------------------- comparison helper
EPS = {True: 2.3e-16, False: 1.2e-7}


def check_forward(got, ref, n_points, f64, what):
    """A forward spectrum of unit noise over n_points points, as
    test_lds_fft_forward: eps x 8 sqrt(log2 N) sqrt(N). Returns (error,
    bound) like the helpers of tests/fft_plans.py."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    bound = EPS[f64] * 8 * np.sqrt(np.log2(n_points)) * np.sqrt(n_points)
    assert err <= bound, f"{what}: |spectrum - numpy| {err:.3g} > {bound:.3g}"
    return err, bound


# ------------------------------------------------------------------ invariants
# Each raises AssertionError naming what broke.
def check_radices(n, f64, radices, k):
    assert math.prod(radices) == n, f"{n}: radices {radices} multiply to {math.prod(radices)}"
    assert set(radices) <= ALLOWED[f64], f"{n}: radix outside {sorted(ALLOWED[f64])}: {radices}"
    assert len(radices) <= k.max_passes, f"{n}: {len(radices)} passes"
    odd_seen_after_even = False
    even = False
    for r in radices:
        if r % 2 == 0:
            even = True
        elif even:
            odd_seen_after_even = True
    assert not odd_seen_after_even, f"{n}: an odd radix follows an even one: {radices}"
    evens = [r for r in radices if r % 2 == 0]
    while evens and evens[0] == BIG2[f64]:
        evens.pop(0)
    # what follows the 16s (float) / 8s (double): at most one each of 8, 4, 2
    assert all(r < BIG2[f64] for r in evens) and len(set(evens)) == len(evens) and \
        evens == sorted(evens, reverse=True), f"{n}: trailing even radices {evens} in {radices}"


def slots(n, radix, count, k):
    """BPT slots one thread of StockhamPass uses: ceil((n / R) count / threads)."""
    return -(-(n // radix) * count // k.threads)


def check_count(n, f64, radices, count, k, stride=None):
    """`count` transforms of length n per workgroup (LDS stride n, or the
    split passes' n + 1)."""
    stride = n if stride is None else stride
    assert 1 <= count, f"{n}: count {count}"
    assert count * stride <= k.max_wg_elems, f"{n}: count {count} x {stride} > {k.max_wg_elems}"
    assert count * stride * elem_bytes(f64) <= k.lds_bytes, f"{n}: count {count} overflows LDS"
    for r in radices:
        used = slots(n, r, count, k)
        assert used <= k.bpt[r], (f"{n}: radix {r} with count {count} needs {used} register "
                                  f"slots, StockhamPass has {k.bpt[r]}")


def check_plane_count(n, f64, radices, count, k):
    assert count <= 64, f"{n}: count {count} > 64"
    check_count(n, f64, radices, count, k)


def largest_divisor_below_sqrt(n):
    return max(d for d in range(1, math.isqrt(n) + 1) if n % d == 0)


def check_split_factors(p):
    n1 = largest_divisor_below_sqrt(p.n)
    assert p.can_split == (n1 >= 4 and p.n // n1 >= 4), f"{p.n}: can_split {p.can_split}"
    if p.can_split:
        assert (p.n1, p.n2) == (n1, p.n // n1), f"{p.n}: split {p.n1} x {p.n2}"


def check_split_pass(n, f64, sub_radices, sub_len, cols, groups, k):
    """One split pass: groups x cols transforms of length sub_len, LDS stride
    sub_len + 1."""
    assert groups >= 1, f"{n}: groups {groups}"
    assert cols >= 1 and cols * (sub_len + 1) <= k.max_wg_elems, f"{n}: cols {cols} x {sub_len}+1"
    assert groups * cols * (sub_len + 1) * elem_bytes(f64) <= k.lds_bytes, \
        f"{n}: {groups} x {cols} x ({sub_len} + 1) overflows LDS"
    for r in sub_radices:
        used = slots(sub_len, r, groups * cols, k)
        assert used <= k.bpt[r], (f"{n}: split radix {r} with {groups} x {cols} transforms of "
                                  f"{sub_len} needs {used} slots, StockhamPass has {k.bpt[r]}")


# --------------------------------------------------------------------- classes
def pass_classes(p, k):
    """(radix, first pass or later, BPT slots a thread uses) of every pass."""
    return {(r, q == 0, slots(p.n, r, p.count, k)) for q, r in enumerate(p.radices)}


def greedy_cover(classes_of):
    """{key: set of classes} -> keys covering the union: each time the key
    with the most uncovered classes, the smallest such key."""
    todo = set().union(*classes_of.values())
    chosen = []
    while todo:
        best = max(sorted(classes_of), key=lambda key: len(classes_of[key] & todo))
        chosen.append(best)
        todo -= classes_of[best]
    return chosen


def sweep_lengths(planner, f64, tables=None):
    """(the pass classes, the greedy cover, every length of the sweep). With
    the plan tables, the cover is taken from the lengths without a
    compile-time plan in this precision: only there do the runtime kernels run
    on either axis."""
    k = planner.constants()
    acc = planner.accepted(f64)
    classes_of = {n: pass_classes(p, k) for n, p in acc.items()}
    classes = set().union(*classes_of.values())
    if tables is not None:
        families = ("rows_f64", "cols_f64", "convd") if f64 else ("rows_f32", "cols_f32", "steps")
        planned = set().union(*(fp.lengths(tables, f) for f in families))
        classes_of = {n: c for n, c in classes_of.items() if n not in planned}
    cover = greedy_cover(classes_of)
    chosen = list(cover) + [n for n in ALWAYS if n not in cover]
    return classes, cover, chosen


def compile_time_lengths(tables):
    """(row lengths, column lengths) with a compile-time plan, either precision."""
    rows = set(fp.lengths(tables, "rows_f64")) | set(fp.lengths(tables, "rows_f32"))
    cols = set()
    for family in ("cols_f64", "cols_f32", "convd", "steps"):
        cols |= set(fp.lengths(tables, family))
    return rows, cols


def height_for_rows(planner, tables, n, f64):
    """n on the rows: the smallest odd smooth h >= 2 row_count + 1 without a
    compile-time column plan: at least two workgroups, the last one partial,
    and a final unpaired row."""
    count = planner.accepted(f64)[n].count
    _, cols = compile_time_lengths(tables)
    h = 2 * count + 1
    while not (h % 2 == 1 and is_smooth(h) and h not in cols):
        h += 1
    return h


def width_for_columns(planner, tables, n, f64):
    """n on the columns: the smallest even smooth w without a compile-time
    row plan with w/2 + 1 > 8 col_count and, for col_count > 1, w/2 + 1 no
    multiple of it: more than one tile per XCD slot, a partial last tile, and
    blocks that return at k0 >= n_cols."""
    count = planner.accepted(f64)[n].count
    rows, _ = compile_time_lengths(tables)
    w = 2
    while not (is_smooth(w) and w not in rows and w // 2 + 1 > 8 * count and
               (count == 1 or (w // 2 + 1) % count != 0)):
        w += 2
    return w


# ---------------------------------------------------------------- split classes
def split_width(p, tables):
    """The split plane's width: the smallest even smooth w without a row plan
    whose w/2 + 1 columns make more than one column tile, the last partial."""
    rows, _ = compile_time_lengths(tables)
    w = 2
    while not (is_smooth(w) and w not in rows and w // 2 + 1 > p.cols and
               (p.cols == 1 or (w // 2 + 1) % p.cols != 0)):
        w += 2
    return w


def split_classes(planner, p, tables):
    """The split-pass classes of column length p.n on its thin plane."""
    w = split_width(p, tables)
    plane = planner.plane(w, p.n, p.f64, 2)
    assert plane.ok and plane.split, (w, p.n)
    sub = planner.accepted(p.f64)
    out = set()
    if p.cols < COLS_CAP[p.f64]:
        out.add(("cols-below-cap",))
    for name, ps, length in (("A", plane.a, p.n1), ("B", plane.b, p.n2)):
        if ps.groups == 1:
            out.add(("groups-1", name))
        if ps.n_groups % ps.groups:
            out.add(("partial-group-tile", name))
        if ps.n_cols % p.cols:
            out.add(("partial-column-tile", name))
        out |= {("radix", name, r) for r in sub[length].radices}
    return out


def split_lengths(planner, tables, f64):
    """(the split classes, a greedy cover of them)."""
    acc = planner.accepted(f64)
    classes_of = {n: split_classes(planner, p, tables) for n, p in acc.items() if p.can_split}
    return set().union(*classes_of.values()), greedy_cover(classes_of)
