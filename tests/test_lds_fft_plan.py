"""The runtime LDS FFT planner (csrc/hip/lds_fft_plan.h) over its whole
domain, on the CPU: tests/lds_fft_plan_query.cc prints the plan of every
length from 2 to 20480 in both precisions, and every accepted plan must fit
what the kernels of lds_fft.hip declare: the radices StockhamPass is
instantiated for, its register array v[BPT][R] (ceil((n / R) count / threads)
slots used per thread), kMaxWgElems and the 160 KiB of LDS, for the row and
column passes and for both split passes. A doctored plan (a radix swapped,
count + 1, cols doubled) must fail the same checks.

profiles/lds_fft_plan_census.txt is census_text() of this module (python
tests/test_lds_fft_plan.py writes it); test_census_file_is_current compares.
"""
import collections
import math
import os
import sys

import pytest

import fft_plans as fp
import lds_fft_plans as lp

HERE = os.path.dirname(os.path.abspath(__file__))
CENSUS = os.path.join(os.path.dirname(HERE), "profiles", "lds_fft_plan_census.txt")
PRECISIONS = [pytest.param(False, id="f32"), pytest.param(True, id="f64")]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return lp.Planner(lp.compile_query(tmp_path_factory.mktemp("ldsplan")))


@pytest.fixture(scope="module")
def tables():
    return fp.plan_tables()


def test_constants(planner):
    k = planner.constants()
    assert k.max_wg_elems == lp.LIMIT
    assert k.lds_bytes == 160 * 1024 and k.threads in (256, 512, 1024)
    for r in range(2, 17):  # StockhamPass: BPT = ceil((kMaxWgElems / R) / threads)
        assert k.bpt[r] == -(-(k.max_wg_elems // r) // k.threads)


@pytest.mark.parametrize("f64", PRECISIONS)
def test_acceptance(planner, f64):
    sweep = planner.sweep(f64)
    assert sorted(sweep) == list(range(2, lp.SWEEP_LAST + 1))
    for n, p in sweep.items():
        accepted = p.factorized and n <= p.max_len
        assert accepted == (lp.is_smooth(n) and n <= lp.LIMIT), n
        assert p.factorized == lp.is_smooth(n), n
        assert p.max_len == lp.LIMIT
    acc = planner.accepted(f64)
    assert len(acc) == 341
    assert sum(n % 2 for n in acc) == 73
    assert max(acc) == lp.LIMIT and max(n for n in acc if n % 2) == 10125
    for n in lp.ALWAYS:
        assert n in acc
    # the plane query refuses what the length query does
    assert planner.plane(64, 22, f64).ok is False
    assert planner.plane(11, 64, f64).ok is False
    assert planner.plane(2 * lp.LIMIT, 8, f64).ok is False
    assert planner.plane(64, 64, f64).ok is True


@pytest.mark.parametrize("f64", PRECISIONS)
def test_radices(planner, f64):
    k = planner.constants()
    acc = planner.accepted(f64)
    for n, p in acc.items():
        lp.check_radices(n, f64, p.radices, k)
    assert max(len(p.radices) for p in acc.values()) == (8 if f64 else 6)
    assert set().union(*(set(p.radices) for p in acc.values())) == lp.ALLOWED[f64]


@pytest.mark.parametrize("f64", PRECISIONS)
def test_counts(planner, f64):
    k = planner.constants()
    acc = planner.accepted(f64)
    for n, p in acc.items():
        lp.check_plane_count(n, f64, p.radices, p.count, k)
    counts = {p.count for p in acc.values()}
    assert min(counts) == 1 and max(counts) == 64
    # a plane's two counts are its two lengths' counts
    for w, h in ((30, 1350), (1350, 30), (10240, 3), (2, 10240), (10125, 135)):
        plane = planner.plane(w, h, f64)
        assert (plane.row_count, plane.col_count) == (acc[w].count, acc[h].count)
    # the limit: one double transform owns the whole LDS, and the last
    # register slot of every pass is in use
    top = acc[lp.LIMIT]
    assert top.count == 1
    if f64:
        assert lp.LIMIT * lp.elem_bytes(True) == k.lds_bytes
    assert all(lp.slots(lp.LIMIT, r, 1, k) == k.bpt[r] for r in top.radices)


@pytest.mark.parametrize("f64", PRECISIONS)
def test_split(planner, tables, f64):
    k = planner.constants()
    acc = planner.accepted(f64)
    n_split = 0
    for n, p in acc.items():
        lp.check_split_factors(p)
        if not p.can_split:
            assert planner.plane(64, n, f64, 2).ok is False
            continue
        n_split += 1
        assert p.n1 * p.n2 == n and p.n1 in acc and p.n2 in acc
        assert p.cols * (max(p.n1, p.n2) + 1) <= k.max_wg_elems
        plane = planner.plane(lp.split_width(p, tables), n, f64, 2)
        assert plane.ok and plane.split
        for ps, length in ((plane.a, p.n1), (plane.b, p.n2)):
            assert ps.sub_len == length
            lp.check_split_pass(n, f64, acc[length].radices, length, p.cols, ps.groups, k)
            assert ps.lds == ps.groups * p.cols * (length + 1) * lp.elem_bytes(f64)
            assert ps.n_groups == n // length and ps.groups <= ps.n_groups
            assert ps.col_tiles == -(-ps.n_cols // p.cols)
            assert ps.grid == ps.col_tiles * -(-ps.n_groups // ps.groups)
    assert n_split == len([n for n in acc if lp.largest_divisor_below_sqrt(n) >= 4])
    # Two of the split classes never occur below the limit: a smooth length
    # always has a divisor close enough to its root for `cols` to reach its cap
    # and for pass A to take more than one sub-column. Reported here if a
    # planner change makes them occur (the GPU sweep would then need them).
    classes, _ = lp.split_lengths(planner, tables, f64)
    assert ("cols-below-cap",) not in classes and ("groups-1", "A") not in classes
    assert ("groups-1", "B") in classes


@pytest.mark.parametrize("f64", PRECISIONS)
def test_classes_and_cover(planner, tables, f64):
    k = planner.constants()
    acc = planner.accepted(f64)
    classes, cover, chosen = lp.sweep_lengths(planner, f64)
    assert len(classes) == (30 if f64 else 33)
    assert len(cover) == (13 if f64 else 16)
    head = [1200, 7056, 18, 50, 196, 32, 54, 108] if f64 else \
        [1350, 4704, 9261, 30, 12, 50, 72, 192]
    assert cover[:8] == head
    # the sweep's cover: from the lengths without a compile-time plan (1200
    # has float64 plans), still every class
    same, cover, chosen = lp.sweep_lengths(planner, f64, tables)
    assert same == classes
    if f64:
        assert fp.expected_fast(tables, 1200, 135, True) and 1200 not in cover
    assert set().union(*(lp.pass_classes(acc[n], k) for n in cover)) == classes
    assert set(lp.ALWAYS) <= set(chosen)
    for n in chosen:
        assert fp.expected_fast(tables, n, 135, f64) == fp.expected_fast(tables, 1024, n, f64) == 0
    _, col_plans = lp.compile_time_lengths(tables)
    row_plans, _ = lp.compile_time_lengths(tables)
    for n in chosen:
        h = lp.height_for_rows(planner, tables, n, f64)
        assert h % 2 == 1 and h in acc and h not in col_plans and h >= 2 * acc[n].count + 1
        w = lp.width_for_columns(planner, tables, n, f64)
        cc = acc[n].count
        assert w % 2 == 0 and w in acc and w not in row_plans and w // 2 + 1 > 8 * cc
        assert cc == 1 or (w // 2 + 1) % cc
    sclasses, scover = lp.split_lengths(planner, tables, f64)
    assert set().union(*(lp.split_classes(planner, acc[n], tables) for n in scover)) == sclasses
    for name in "AB":
        assert {r for c, *rest in sclasses if c == "radix" and rest[0] == name
                for r in rest[1:]} == lp.ALLOWED[f64]


# ------------------------------------------------------------- doctored plans
@pytest.mark.parametrize("f64", PRECISIONS)
def test_doctored_plans_are_rejected(planner, tables, f64):
    k = planner.constants()
    acc = planner.accepted(f64)
    p = acc[1200 if f64 else 1350]
    lp.check_radices(p.n, f64, p.radices, k)
    # a radix swapped for another: the product
    swapped = (2 if p.radices[0] != 2 else 3,) + p.radices[1:]
    with pytest.raises(AssertionError, match="multiply"):
        lp.check_radices(p.n, f64, swapped, k)
    # the same product through a radix the kernels have no pass for
    with pytest.raises(AssertionError, match="outside"):
        lp.check_radices(36, f64, (6, 6), k)
    if f64:  # double has no radix-16 / radix-9 pass
        with pytest.raises(AssertionError, match="outside"):
            lp.check_radices(144, True, (9, 16), k)
    with pytest.raises(AssertionError, match="odd radix follows"):
        lp.check_radices(p.n, f64, p.radices[::-1], k)
    with pytest.raises(AssertionError, match="trailing"):
        lp.check_radices(16, f64, (4, 4), k)
    with pytest.raises(AssertionError, match="trailing"):
        lp.check_radices(128, f64, (4, 2, 16) if not f64 else (2, 8, 8), k)
    with pytest.raises(AssertionError, match="passes"):
        lp.check_radices(2 ** 25, f64, (2,) * 25, k)
    # count + 1, where the planner's count is bounded by each of the limits
    limit = acc[lp.LIMIT]
    with pytest.raises(AssertionError, match="> 10240"):
        lp.check_plane_count(lp.LIMIT, f64, limit.radices, limit.count + 1, k)
    small = acc[2]
    assert small.count == 64
    with pytest.raises(AssertionError, match="> 64"):
        lp.check_plane_count(2, f64, small.radices, small.count + 1, k)
    # the register slots alone (the other limits lifted): four transforms of
    # 4096 fill both radix-8 slots of every thread, a fifth needs another
    roomy = lp.Constants(k.threads, k.max_passes, 10 * k.lds_bytes, 10 * k.max_wg_elems, k.bpt)
    lp.check_count(4096, f64, (8, 8, 8, 8), 4, roomy)
    with pytest.raises(AssertionError, match="register slots"):
        lp.check_count(4096, f64, (8, 8, 8, 8), 5, roomy)
    with pytest.raises(AssertionError, match="overflows LDS"):
        lp.check_count(4096, f64, (), 2, lp.Constants(
            k.threads, k.max_passes, k.lds_bytes // 8, k.max_wg_elems, k.bpt))
    # cols doubled, at the length whose sub-transforms are longest
    # (pass B takes one sub-column per tile there: nothing else can give way)
    worst = max((q for q in acc.values() if q.can_split), key=lambda q: q.n2)
    plane = planner.plane(lp.split_width(worst, tables), worst.n, f64, 2)
    assert plane.b.groups == 1
    lp.check_split_pass(worst.n, f64, acc[worst.n2].radices, worst.n2, worst.cols, 1, k)
    # double plans aim at half the LDS (two workgroups per CU), so one doubling
    # still fits and is a valid plan; the second does not
    doubled = 4 * worst.cols if f64 else 2 * worst.cols
    if f64:
        lp.check_split_pass(worst.n, f64, acc[worst.n2].radices, worst.n2, 2 * worst.cols, 1, k)
    with pytest.raises(AssertionError, match=r"cols \d+ x"):
        lp.check_split_pass(worst.n, f64, acc[worst.n2].radices, worst.n2, doubled, 1, k)
    # with the element limit lifted the same doctored plan runs out of LDS
    # and of register slots
    lifted = lp.Constants(k.threads, k.max_passes, k.lds_bytes, 10 * k.max_wg_elems, k.bpt)
    with pytest.raises(AssertionError, match="overflows LDS" if f64 else "slots"):
        lp.check_split_pass(worst.n, f64, acc[worst.n2].radices, worst.n2, doubled, 1, lifted)
    with pytest.raises(AssertionError, match="groups 0"):
        lp.check_split_pass(64, f64, (8,), 8, 16, 0, k)
    # a doctored split: factors that are not the planner's
    with pytest.raises(AssertionError, match="split"):
        lp.check_split_factors(acc[64]._replace(n1=4, n2=16))
    with pytest.raises(AssertionError, match="can_split"):
        lp.check_split_factors(acc[15]._replace(can_split=True))


# ------------------------------------------------------ the comparison helpers
@pytest.mark.parametrize("f64", PRECISIONS)
def test_comparison_helpers_reject_one_element_off(f64):
    """What tests/test_lds_fft_sweep_gpu.py compares with: each helper takes
    the reference itself and rejects it with one element moved by twice the
    bound."""
    import numpy as np
    rng = np.random.default_rng(3)
    h, w = 9, 30
    img = rng.standard_normal((h, w)).astype(np.float32).astype(np.float64)
    ker = rng.standard_normal((h, w))
    spec = np.fft.rfft2(img)
    for ref, n_points in ((spec, w * h), (np.fft.rfft(img, axis=1), w)):
        err, bound = lp.check_forward(ref.copy(), ref, n_points, f64, "control")
        assert err == 0.0 and bound > 0
        off = ref.copy()
        off[h // 2, 3] += 2 * bound
        with pytest.raises(AssertionError, match="control"):
            lp.check_forward(off, ref, n_points, f64, "control")
        with pytest.raises(AssertionError, match="control"):  # a NaN never passes
            lp.check_forward(np.full_like(ref, np.nan), ref, n_points, f64, "control")
    conv = np.fft.irfft2(spec * np.fft.rfft2(ker), s=(h, w))
    got = conv.astype(np.float32).astype(np.float64)  # what a float image can hold
    err, bound = fp.check_image(got, conv, w * h, f64, "control")
    assert err <= bound
    scale = np.abs(conv).max() * np.sqrt(np.log2(w * h))
    y, x = np.unravel_index(np.argmax(np.abs(conv)), conv.shape)  # the widest per-pixel bound
    step = 0.5 * np.spacing(np.float32(np.abs(conv).max())) + 1e-12 * scale if f64 else bound
    off = conv.copy()
    off[y, x] += 2 * step
    with pytest.raises(AssertionError, match="control"):
        fp.check_image(off, conv, w * h, f64, "control")
    if f64:
        residual = rng.standard_normal((h, w)).astype(np.float32)
        good = residual - conv.astype(np.float32)
        err, bound = fp.check_correction(good, residual, conv, float(np.abs(conv).max()), "control")
        assert err == 0.0
        off = good.copy()
        off[2, 5] += np.float32(2 * bound)
        with pytest.raises(AssertionError, match="control"):
            fp.check_correction(off, residual, conv, float(np.abs(conv).max()), "control")


# --------------------------------------------------------------------- census
def census_text(planner, tables):
    k = planner.constants()
    out = ["# The runtime LDS FFT planner (csrc/hip/lds_fft_plan.h) over every length it",
           "# accepts, from tests/lds_fft_plan_query.cc; written by",
           "# python tests/test_lds_fft_plan.py, compared by test_census_file_is_current.",
           f"# threads {k.threads}, kMaxWgElems {k.max_wg_elems}, kFftLdsBytes {k.lds_bytes}, "
           f"kFftMaxPasses {k.max_passes}",
           "# BPT(R): " + " ".join(f"{r}:{k.bpt[r]}" for r in sorted(lp.ALLOWED[False]))]
    for f64 in (False, True):
        name = "float64" if f64 else "float32"
        acc = planner.accepted(f64)
        out += ["", f"[{name}] lengths {len(acc)} (odd {sum(n % 2 for n in acc)}), "
                    f"largest {max(acc)}, largest odd {max(n for n in acc if n % 2)}"]
        seqs = collections.Counter(p.radices for p in acc.values())
        by_len = collections.Counter(len(p.radices) for p in acc.values())
        out.append(f"[{name}] distinct radix sequences {len(seqs)}; lengths by number of passes: "
                   + " ".join(f"{n}:{c}" for n, c in sorted(by_len.items())))
        counts = collections.Counter(p.count for p in acc.values())
        out.append(f"[{name}] transforms per workgroup (count:lengths): "
                   + " ".join(f"{c}:{m}" for c, m in sorted(counts.items())))
        classes, cover, chosen = lp.sweep_lengths(planner, f64, tables)
        out.append(f"[{name}] pass classes {len(classes)}, greedy cover among the lengths without a "
                   f"compile-time plan {len(cover)} lengths: "
                   + " ".join(map(str, cover)))
        out.append(f"[{name}] always added: " + " ".join(str(n) for n in chosen[len(cover):]))
        out.append(f"[{name}] class (radix, first|later, slots used of BPT) -> chosen lengths")
        for r, first, used in sorted(classes):
            hit = [n for n in chosen if (r, first, used) in lp.pass_classes(acc[n], k)]
            out.append(f"  radix {r:2d} {'first' if first else 'later'} {used}/{k.bpt[r]}: "
                       + " ".join(map(str, hit)))
        can = [p for p in acc.values() if p.can_split]
        sclasses, scover = lp.split_lengths(planner, tables, f64)
        out.append(f"[{name}] split: {len(can)} lengths can split, {len(acc) - len(can)} cannot; "
                   f"cols " + " ".join(f"{c}:{m}" for c, m in sorted(
                       collections.Counter(p.cols for p in can).items())))
        out.append(f"[{name}] split classes {len(sclasses)}, greedy cover: "
                   + " ".join(f"{n}={acc[n].n1}x{acc[n].n2}" for n in scover))
        for c in sorted(sclasses, key=str):
            hit = [n for n in scover if c in lp.split_classes(planner, acc[n], tables)]
            out.append("  " + " ".join(map(str, c)) + ": " + " ".join(map(str, hit)))
        out.append("  never occur: cols-below-cap, groups-1 A")
    return "\n".join(out) + "\n"


def test_census_file_is_current(planner, tables):
    text = census_text(planner, tables)
    assert text.count("lengths 341 (odd 73)") == 2
    with open(CENSUS) as f:
        assert f.read() == text, "run python tests/test_lds_fft_plan.py to rewrite the census"
    # every class has at least one chosen length
    for line in text.splitlines():
        if line.startswith("  ") and not line.startswith("  never"):
            assert line.split(": ", 1)[1].strip(), line


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, HERE)
    with tempfile.TemporaryDirectory() as tmp:
        text = census_text(lp.Planner(lp.compile_query(tmp)), fp.plan_tables())
    with open(CENSUS, "w") as f:
        f.write(text)
    print(text)
