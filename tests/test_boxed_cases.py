"""The cases of tests/boxed_cases.py must be able to fail: every one of them is
run through a plain NumPy model of the operation (which must pass: its answers
are the ones fixed by construction and the oracle's) and through models that
are wrong on purpose, each of which must fail at least one case of the set
tests/test_boxed_primitives_gpu.py runs on the device. No GPU here: these are
models in Python, not kernels.
"""
import numpy as np
import pytest

import boxed_cases as B
from oracle_lib import get_oracle
from rdl_lib import integration

F = np.float32

PEAK_FAMILIES = {"planted vector": B.planted_vector, "planted scalar": B.planted_scalar,
                 "planted masked": B.planted_masked, "rows": B.rows_cases,
                 "special": B.special_cases}


@pytest.fixture(scope="module")
def orc():
    return get_oracle()


def oracle_peak(orc, g, q):
    found, x, y, value = orc.find_peak(g.img, q.allow_negative, q.start_y, q.end_y, q.hb, q.vb,
                                       mask=g.mask_of(q), simple=not q.avx)
    return (int(found), x, y, B.bits(value))


@pytest.fixture(scope="module")
def peak_groups():
    return {name: list(gen()) for name, gen in PEAK_FAMILIES.items()}


def test_peak_model_passes_every_case(orc, peak_groups):
    """The correct model gives the constructed answer and the oracle's."""
    n = 0
    for family in list(peak_groups.values()) + [list(B.small_cases()), list(B.beyond_cases())]:
        for g in family:
            for q in g.queries:
                got = B.find_peak(g.img, q, g.mask_of(q))
                if q.expect is not None:
                    assert B.same_peak(got, q.expect), (g.name, q)
                if q.oracle:
                    assert B.same_peak(got, oracle_peak(orc, g, q)), (g.name, q)
                n += 1
    assert n > 30000


@pytest.fixture(scope="module")
def peak_kills(peak_groups):
    """mutant -> the families with a case it fails."""
    kills = {m: set() for m in B.PEAK_MUTANTS}
    for family, groups in peak_groups.items():
        for m in B.PEAK_MUTANTS:
            kills[m] |= {family for g in groups for q in g.queries
                         if not B.same_peak(B.find_peak(g.img, q, g.mask_of(q), m), q.expect)}
    return kills


def test_every_peak_mutant_fails_a_case(peak_kills):
    for mutant, families in peak_kills.items():
        assert families, mutant


def test_each_peak_family_is_needed(peak_kills):
    """Without a family some mutant survives the others: the block-boundary
    cases alone catch a dropped last row, the special values alone the three
    qualification slips, the planted edges alone a box a column too wide (and
    every other box mutant as well), the masked ones the shifted mask read."""
    for mutant in ("last row of a block dropped (2)", "last row of a block dropped (3)"):
        assert peak_kills[mutant] == {"rows"}
    for mutant in (">= FLT_MIN", "NaN qualifies", "-Inf does not qualify"):
        assert peak_kills[mutant] == {"special"}
    planted = {"planted vector", "planted scalar", "planted masked"}
    for mutant in ("left wider", "right wider"):
        assert peak_kills[mutant] and peak_kills[mutant] <= planted, mutant
    for mutant in B.BOX_MUTANTS:
        assert {"planted vector", "planted scalar"} <= peak_kills[mutant], mutant
    assert peak_kills["mask read one byte on"] <= {"planted masked", "planted scalar"}
    assert "planted masked" in peak_kills["mask read one byte on"]
    assert "rows" in peak_kills["last index on ties"]


def test_small_cases_catch_the_box_mutants(orc):
    """The exhaustive small shapes, judged by the correct model (which the test
    above ties to the oracle), fail every box, start_y and end_y mutant too."""
    groups = list(B.small_cases())
    assert sum(len(g.queries) for g in groups) == 29344
    for mutant in list(B.BOX_MUTANTS) + ["end_y ignored", "start_y ignored"]:
        assert any(B.find_peak(g.img, q, g.mask_of(q), mutant)
                   != B.find_peak(g.img, q, g.mask_of(q))
                   for g in groups[::7] for q in g.queries), mutant


def _old_search_box(w, h, sy, ey, hb, vb):
    """LaunchFindPeak's box as it stood, in 32-bit unsigned arithmetic: an end
    below its start raised first, the clamp to the image afterwards."""
    u = 0xffffffff
    xs, xe = hb, (w - hb) & u
    ys, ye = max(sy, vb), min(ey, (h - vb) & u)
    xe, ye = max(xe, xs), max(ye, ys)
    return xs, min(xe, w), ys, min(ye, h)


def test_search_box_is_the_plain_integer_box(tmp_path):
    """rdl::MakeSearchBox (csrc/hip/conv_peak_box.h), the box LaunchFindPeak
    searches, in 32-bit unsigned arithmetic, against boxed_cases.box in plain
    integers, over every query of the small shapes and of the borders beyond
    the image: xs <= xe <= w and ys <= ye <= h always, so `rows` and
    `xs + threadIdx.x` cannot wrap."""
    import os
    import subprocess
    from test_subminor_plan import _host_build
    b = _host_build()
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "search_box_dump")
    subprocess.run([b.CXX, *b.CXX_FLAGS, os.path.join(here, "search_box_dump.cc"), "-o", exe],
                   check=True)
    asked = [(g.img.shape[1], g.img.shape[0], q.start_y, q.end_y, q.hb, q.vb)
             for g in list(B.small_cases()) + list(B.beyond_cases()) for q in g.queries]
    text = subprocess.run([exe], input="".join("%d %d %d %d %d %d\n" % a for a in asked),
                          check=True, capture_output=True, text=True).stdout
    boxes = [tuple(int(v) for v in line.split()) for line in text.splitlines()]
    assert len(boxes) == len(asked)
    for (w, h, sy, ey, hb, vb), (xs, xe, ys, ye) in zip(asked, boxes):
        assert (xs, xe, ys, ye) == B.box(w, h, sy, ey, hb, vb), (w, h, sy, ey, hb, vb)
        assert xs <= xe <= w and ys <= ye <= h
        old = _old_search_box(w, h, sy, ey, hb, vb)
        if hb <= w and vb <= h and sy <= h:         # nothing beyond the image: unchanged
            assert old == (xs, xe, ys, ye)
    # what the old order left beyond the image: ye < ys, so that `rows` wrapped (to
    # height + 1 for start_y = 2^32 - 1, whose workgroups then searched image rows),
    # and xe < xs with xs + threadIdx.x wrapping into the row
    assert _old_search_box(8, 6, 2 ** 32 - 1, 6, 0, 0) == (0, 8, 2 ** 32 - 1, 6)
    assert _old_search_box(5, 4, 0, 4, 2 ** 32 - 1, 0) == (2 ** 32 - 1, 5, 0, 4)
    assert (8, 6, 2 ** 32 - 1, 6, 0, 0) in asked and (5, 4, 0, 4, 2 ** 32 - 1, 0) in asked


def test_deferred_rounds_and_subset():
    for which in (0, 1):
        pairs = B.deferred_round(which)
        assert len(pairs) == B.PEAK_SLOTS
        assert len({g.img.shape for g, _ in pairs}) >= 8
        assert {g.mask is not None and q.masked for g, q in pairs} == {True, False}
        assert {g.img_off for g, _ in pairs} == {0, 1}
    a, b = B.deferred_round(0), B.deferred_round(1)
    assert sum(ga is gb for (ga, _), (gb, _) in zip(a, b)) == 0
    names = " ".join(g.name for g in B.representative_subset())
    for part in ("vector", "scalar width", "image + 4", "mask off", "rows 2049", "all NaN"):
        assert part in names


# --------------------------------------------------------------- subtraction
def run_subtract_cases(orc, mutant):
    """The failures of `mutant` (None: the model) over every case."""
    out = []
    for w, h, comps in B.subtract_cases():
        img, psf = B.subtract_images(w, h)
        for x, y, factor in comps:
            got, want = img.copy(), img.copy()
            B.subtract(got, psf, x, y, factor, mutant)
            orc.subtract(want, psf, x, y, factor)
            out += [(w, h, x, y, f) for f in B.subtract_failures(got, img, want, x, y, factor)]
    return out


def test_subtract_model_passes_every_case(orc):
    assert run_subtract_cases(orc, None) == []
    assert {1, 256, 257, 2048, 2049, 2050, 4100} <= B.window_sizes()
    for w, h, x, y, factor, (px, py), inside in B.subtract_nan_cases():
        img, psf = B.subtract_images(w, h)
        clean = img.copy()
        orc.subtract(clean, psf, x, y, factor)
        psf[py, px] = np.nan
        got, want = img.copy(), img.copy()
        B.subtract(got, psf, x, y, factor)
        orc.subtract(want, psf, x, y, factor)
        assert B.subtract_failures(got, img, want, x, y, factor) == []
        assert np.isnan(want).sum() == int(inside)
        if not inside:
            assert np.array_equal(want, clean)


@pytest.mark.parametrize("mutant", B.SUBTRACT_MUTANTS)
def test_every_subtract_mutant_fails_a_case(orc, mutant):
    failures = run_subtract_cases(orc, mutant)
    assert failures
    if mutant == "x loop stops after 2048":
        assert {f[0] for f in failures} <= {4096, 4097, 4100, 4101}     # only the wide windows


# --------------------------------------------------------------- integration
def integrate_expectation(orc, case):
    if case.expect is not None:
        return case.expect
    n_images = case.images.shape[0]
    return orc.integrate(case.images.reshape(n_images, 1, case.n), case.weights, case.n_pol,
                         case.pol_factor, square=case.mode == B.SQUARE,
                         squared_joins=case.mode == B.SQUARED_JOINS).ravel()


def integrate_fails(orc, case, mutant):
    dest = np.full(case.n, -6e18, F)
    B.integrate(case, dest, mutant)
    want = integrate_expectation(orc, case)
    return not np.array_equal(dest.view(np.uint32), want.view(np.uint32))


@pytest.fixture(scope="module")
def integrate_case_list():
    return sorted(B.integrate_cases(), key=lambda c: c.n)     # the 2 097 409-pixel ones last


def test_integrate_model_passes_every_case(orc, integrate_case_list):
    names = [c.name for c in integrate_case_list]
    assert len(set(names)) == len(names)
    for case in integrate_case_list:
        assert not integrate_fails(orc, case, None), case.name
        if case.factor is None:     # the factor the C-ABI's callers compute
            g = integration(case.n_ch, case.n_pol, case.weights, case.pol_factor, case.mode)
            assert F(g.factor) == B.integration_factor(case.n_ch, case.weights, case.pol_factor,
                                                       case.mode)
            assert g.copy_fast_path == case.copy_fast_path


@pytest.mark.parametrize("mutant", B.INTEGRATE_MUTANTS)
def test_every_integrate_mutant_fails_a_case(orc, integrate_case_list, mutant):
    killers = []
    for case in integrate_case_list:
        if integrate_fails(orc, case, mutant):
            killers.append(case.name)
            break
    assert killers, mutant
    if mutant == "grid stride stops at 2 097 152":
        assert "n=2097409" in killers[0]
    if mutant == "fma first term":
        assert "minus zero" in killers[0]
    if mutant == "pol_mask ignored":
        assert "pol_mask" in killers[0]
