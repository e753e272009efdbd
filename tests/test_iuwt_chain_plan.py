"""PlanChain (csrc/hip/iuwt_chain_plan.h), the launch geometry of the IUWT
row-chain kernels, against what those kernels (csrc/hip/iuwt.hip) need from a
plan; no GPU.

tests/iuwt_chain_plan_dump.cc prints the plan, or its refusal, over a sweep
of widths 4 .. 16388, heights 1 .. 1100, spacings 2^k - 1 (k = 1 .. 12), both
directions and the four strip-width overrides. Every row must equal the numpy
restatement of tests/iuwt_cases.py (which the GPU tests use to know the path a
shape takes), and every planned row must satisfy the needs listed in
test_plans_meet_the_kernels_needs, each with the place in the kernel it comes
from.

test_census then states, for each of the 18 decomposition and 6
recomposition instantiations, the smallest case of the sweep that launches
it, or that none does, and where the refusals begin; the text is
profiles/iuwt_chain_plan_census.txt, which tests/test_iuwt.py reads to check
that its shapes reach every reachable instantiation. The instantiation is a
function of (strip width, spacing, direction) alone, and the sweep holds
every strip width (every multiple of 4 up to 1024) with every spacing, so
"unreachable" holds for every call, not only for the sweep.
"""
import importlib.util
import io
import os
import subprocess

import numpy as np
import pytest

from iuwt_cases import REFUSALS, plan_chain

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CENSUS = os.path.join(ROOT, "profiles", "iuwt_chain_plan_census.txt")
COLUMNS = ["w", "h", "d", "decompose", "ws_override", "ok", "ws", "n_strips", "n_seg", "n_res",
           "blocks", "lds", "na", "no", "ni"]
PLAN_FIELDS = COLUMNS[6:]


def _host_build():
    spec = importlib.util.spec_from_file_location(
        "rdl_build", os.path.join(ROOT, "ska-sdp-func-radler_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    b = _host_build()
    exe = str(tmp_path_factory.mktemp("iuwt_plan") / "iuwt_chain_plan_dump")
    subprocess.run([b.CXX, *b.CXX_FLAGS, os.path.join(HERE, "iuwt_chain_plan_dump.cc"),
                    "-o", exe], check=True)
    text = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    table = np.loadtxt(io.StringIO(text), dtype=np.int64)
    assert table.shape[1] == len(COLUMNS)
    return {name: table[:, i] for i, name in enumerate(COLUMNS)}


def floor4(v):
    """Floor4 of iuwt.hip: towards minus infinity, for negative values too."""
    return np.where(v >= 0, v & ~3, -((-v + 3) & ~3))


def test_sweep_covers_the_issue_domain(rows):
    assert rows["w"].min() == 4 and rows["w"].max() == 16388
    assert rows["h"].min() == 1 and rows["h"].max() == 1100
    assert set(np.unique(rows["d"])) == {(1 << k) - 1 for k in range(1, 13)}
    assert set(np.unique(rows["decompose"])) == {0, 1}
    assert set(np.unique(rows["ws_override"])) == {0, 256, 768, 1024}
    # every strip width with every spacing (the docstring's argument)
    full = rows["w"] <= 1028
    assert set(np.unique(rows["w"][full])) == set(range(4, 1029, 4))


def test_restatement_equals_plan_chain(rows):
    p = plan_chain(rows["w"], rows["h"], rows["d"], rows["decompose"], rows["ws_override"])
    assert np.array_equal(p["refusal"] == 0, rows["ok"] == 1)
    ok = rows["ok"] == 1
    for name in PLAN_FIELDS:
        bad = np.flatnonzero(ok & (p[name] != rows[name]))
        assert bad.size == 0, (name, {c: rows[c][bad[:3]] for c in COLUMNS}, p[name][bad[:3]])
        assert not rows[name][~ok].any()


def test_plans_meet_the_kernels_needs(rows):
    ok = rows["ok"] == 1
    r = {k: v[ok] for k, v in rows.items()}
    w, h, d, dec = r["w"], r["h"], r["d"], r["decompose"] == 1
    ws, na, no, ni = r["ws"], r["na"], r["no"], r["ni"]

    # ChainRow::Load reads float4s at columns ab + 4 g of rows of width w, and
    # a strip starts at x0 = strip * ws (ChainBlock): both multiples of 4. The
    # output loops cover 256 NO columns per strip and NO <= 4 is instantiated
    # (LaunchChainO).
    assert np.all(ws % 4 == 0) and np.all(ws >= 4) and np.all(ws <= 1024)
    assert np.all(np.isin(na, (1, 2))) and np.all(np.isin(no, (1, 2, 4)))

    # ChainBlock: strip = L % n_strips, x0 = strip * ws; the stores stop at
    # x < w. The strips cover [0, w), and the last one is not empty.
    assert np.all(r["n_strips"] * ws >= w)
    assert np.all((r["n_strips"] - 1) * ws < w)

    # The a-row slot (arow, kSlot = 1024 NA floats): the kernel's own wa4 =
    # (x0 + ws + halo - Floor4(x0 - halo) + 3) / 4 float4s must fit 256 NA,
    # else ChainRow::Load (g < 256 NA) leaves the row's last columns unloaded.
    halo = np.where(dec, 4 * d, 2 * d)
    key = np.stack([ws, halo, na], axis=1)
    uniq, inverse = np.unique(key, axis=0, return_inverse=True)
    strips = np.zeros(len(uniq), np.int64)
    np.maximum.at(strips, inverse.ravel(), r["n_strips"])
    for (ws_u, halo_u, na_u), n_strips in zip(uniq, strips):
        x0 = np.arange(n_strips, dtype=np.int64) * ws_u
        ab = floor4(x0 - halo_u)
        assert np.all(ab <= x0 - halo_u)
        wa4 = (x0 + ws_u + halo_u - ab + 3) // 4
        assert np.all(wa4 <= 256 * na_u), (ws_u, halo_u, na_u, wa4.max())

    # The column loops: `for i < NO: x = x0 + tid + 256 i; if (x < x0 + ws)`
    # (ring2, aring, the coefficient row, the recomposition) and `for i < NI:
    # x = xi0 + tid + 256 i; if (x < xi0 + wi)` with wi = ws + 4 d (ring1, the
    # i1 row of the decomposition); LaunchChainT instantiates NI - NO = 0, 1, 2
    # and sends anything else to + 2.
    assert np.all(256 * no >= ws)
    assert np.all(256 * ni[dec] >= ws[dec] + 4 * d[dec])
    assert np.all(np.isin((ni - no)[dec], (0, 1, 2)))

    # ChainBlock: r = rest / n_seg must run over every residue that has rows
    # (r < d and r < h); a chain has at most k_max = ceil(h / d) positions,
    # cut into n_seg segments of kseg = ceil(k_max / n_seg).
    k_max = (h + d - 1) // d
    n_seg = r["n_seg"]
    assert np.array_equal(r["n_res"], np.minimum(d, h))
    assert np.all(n_seg >= 1)
    assert np.all(n_seg * ((k_max + n_seg - 1) // n_seg) >= k_max)

    # ChainBlock: L = (b % 8) * per + b / 8 with per = ceil(n_blocks / 8) must
    # hit each of the n_blocks (residue, segment, strip) triples exactly once
    # over the launched blocks; L is a uint32.
    n_blocks = r["n_res"] * n_seg * r["n_strips"]
    assert np.all(r["blocks"] % 8 == 0) and np.all(r["blocks"] >= n_blocks)
    assert np.all(r["blocks"] < 1 << 31)
    pairs = np.unique(np.stack([n_blocks, r["blocks"]], axis=1), axis=0)
    for nb, blocks in pairs:
        b = np.arange(blocks, dtype=np.int64)
        per = (nb + 7) // 8
        L = (b % 8) * per + b // 8
        hit = np.sort(L[L < nb])
        assert hit.size == nb and np.array_equal(hit, np.arange(nb)), (nb, blocks)

    # The kernels' carve-up of the dynamic LDS, in floats. IuwtDecomposeChain:
    # arow [2][1024 NA], ring1 [5][wi], i1row [2][wi], ring2 [5][ws], aring
    # [6][ws]. IuwtRecomposeChain: arow [2][1024 NA], ring1 [5][ws]. A
    # workgroup of gfx950 has 160 KiB.
    wi = ws + 4 * d
    arow = 2 * 1024 * na
    carve = np.where(dec, arow + 5 * wi + 2 * wi + 5 * ws + 6 * ws, arow + 5 * ws) * 4
    assert np.array_equal(r["lds"], carve)
    assert np.all(r["lds"] <= 160 * 1024)


def instantiations():
    dec = [("dec", na, no, dn) for na in (1, 2) for no in (1, 2, 4) for dn in (0, 1, 2)]
    rec = [("rec", na, no, 0) for na in (1, 2) for no in (1, 2, 4)]
    return dec + rec


def _case(rows, i):
    ov = int(rows["ws_override"][i])
    return (f"w={rows['w'][i]} h={rows['h'][i]} d={rows['d'][i]} "
            f"ws_override={ov if ov else 'none'}")


def _smallest(rows, mask):
    """The first row of `mask` by (pixels, spacing, width, override)."""
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return None
    order = np.lexsort((rows["ws_override"][idx], rows["w"][idx], rows["d"][idx],
                        rows["w"][idx] * rows["h"][idx]))
    return int(idx[order[0]])


def census_text(rows):
    ok = rows["ok"] == 1
    out = ["# Row-chain kernel instantiations and refusals of PlanChain over the sweep of",
           "# tests/iuwt_chain_plan_dump.cc (written by tests/test_iuwt_chain_plan.py).",
           "# instantiation: smallest reaching case (by pixels, spacing, width, override)"]
    for (direction, na, no, dn) in instantiations():
        dec = direction == "dec"
        mask = ok & (rows["decompose"] == int(dec)) & (rows["na"] == na) & (rows["no"] == no)
        if dec:
            mask &= rows["ni"] - rows["no"] == dn
        name = (f"IuwtDecomposeChain<{na},{no},{no + dn}>" if dec
                else f"IuwtRecomposeChain<{na},{no}>")
        i = _smallest(rows, mask)
        where = "unreachable" if i is None else (
            f"{_case(rows, i)} (strip {rows['ws'][i]}, LDS {rows['lds'][i]} B)")
        out.append(f"inst {direction} na={na} no={no} dn={dn} {name}: {where}")
    p = plan_chain(rows["w"], rows["h"], rows["d"], rows["decompose"], rows["ws_override"])
    out.append("# refusals: the first spacing refused per direction with the default strip")
    out.append("# width at full-width strips (w >= 512), then each reason's smallest call")
    for dec, direction in ((1, "dec"), (0, "rec")):
        full = (rows["decompose"] == dec) & (rows["ws_override"] == 0) & (rows["w"] >= 512)
        d_first = rows["d"][full & ~ok].min()
        at = full & (rows["d"] == d_first)
        reasons = sorted({REFUSALS[int(c)] for c in np.unique(p["refusal"][at])})
        assert not ok[at].any() and ok[full & (rows["d"] < d_first)].all()
        out.append(f"first {direction}: d={d_first} refused at every such width and height "
                   f"({'; '.join(reasons)}), every smaller d planned")
    # a call plans its spacings in ascending order and stops at the first
    # refusal, so it meets a refusal only where every smaller spacing of the
    # same (w, h, direction, override) is planned
    key = np.stack([rows[c] for c in ("w", "h", "decompose", "ws_override")], axis=1)
    _, group = np.unique(key, axis=0, return_inverse=True)
    group = group.ravel()
    first_refused = np.full(group.max() + 1, np.iinfo(np.int64).max)
    np.minimum.at(first_refused, group[~ok], rows["d"][~ok])
    met = ~ok & (rows["d"] == first_refused[group])
    for dec, direction in ((1, "dec"), (0, "rec")):
        for code in sorted(k for k in REFUSALS if k):
            i = _smallest(rows, met & (p["refusal"] == code) & (rows["decompose"] == dec))
            where = "no call meets it" if i is None else _case(rows, i)
            out.append(f"refusal {direction} {code} ({REFUSALS[code]}): {where}")
    over = ok & (rows["lds"] > 64 * 1024)
    for dec, direction in ((1, "dec"), (0, "rec")):
        i = _smallest(rows, over & (rows["decompose"] == dec))
        where = "never" if i is None else f"{_case(rows, i)} (LDS {rows['lds'][i]} B)"
        out.append(f"lds-opt-in {direction} (more than 64 KiB): {where}")
    return "\n".join(out) + "\n"


def test_census(rows):
    text = census_text(rows)
    print(text)
    lines = [ln for ln in text.splitlines() if ln.startswith("inst ")]
    assert len(lines) == 18 + 6
    old = open(CENSUS).read() if os.path.exists(CENSUS) else None
    if old != text:
        try:
            with open(CENSUS, "w") as f:
                f.write(text)
        except OSError:
            pass
    assert old == text, "profiles/iuwt_chain_plan_census.txt was stale; rewritten, commit it"
