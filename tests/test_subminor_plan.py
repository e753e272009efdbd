"""PlanSubminorLoop (csrc/hip/subminor_plan.h), the sub-minor loop's kernel
choice, against the choices recorded from the code it replaced.

tests/subminor_plan_dump.cc prints the plan over a fixed sweep of the
function's domain; every field of every row must equal
tests/golden/subminor_plan_parent.npz, which was produced for the same inputs
by the decision block of SubminorLaunch as it stood before the function
existed (the block copied unedited into a stand-alone program).

Four of the function's five errors occur in the sweep. The fifth ("too many
pixels per participant") cannot occur for any input: the table kernel needs a
pairwise table, whose size bound (n_sel^2 <= 2^28) keeps a selection at or
below 16384 pixels, and one participant of 1024 threads x 16 items holds
those. The check is kept in the function as the guard it was.
"""
import importlib.util
import io
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "subminor_plan_parent.npz")
COLUMNS = ["mode", "target", "n_sel", "n_images", "n_pol", "integ_mode", "copy_fast_path",
           "has_rms", "has_spectral", "has_logpoly", "n_cus", "coop_limit", "tab", "tab_threads",
           "big_target",
           "error_id", "error", "kind", "threads", "items", "n_blocks", "per_block", "use_lds",
           "lds_bytes", "build_table", "part_stride", "rec_bytes", "ni_template", "trace_kind"]
KINDS = {"Lds": 0, "Reg": 1, "Wave": 2, "Big": 3, "Tab": 4, "TabN": 5}
RDL_ERR_ARG = 1


def _host_build():
    spec = importlib.util.spec_from_file_location(
        "rdl_build", os.path.join(ROOT, "ska-sdp-func-radler_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plan_matches_parent_choices(tmp_path):
    b = _host_build()
    exe = str(tmp_path / "subminor_plan_dump")
    subprocess.run([b.CXX, *b.CXX_FLAGS, os.path.join(HERE, "subminor_plan_dump.cc"), "-o", exe],
                   check=True)
    text = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = np.loadtxt(io.StringIO(text), dtype=np.int64, comments="E")
    texts = [line.split(" ", 2)[2] for line in text.splitlines() if line.startswith("E ")]

    gold = np.load(GOLDEN)
    assert texts == list(gold["error_texts"])
    assert rows.shape == (len(gold["n_sel"]), len(COLUMNS))
    for i, name in enumerate(COLUMNS):
        bad = np.flatnonzero(rows[:, i] != gold[name].astype(np.int64))
        assert bad.size == 0, (name, bad[:5], rows[bad[:5]])

    # the sweep reaches every kernel and every error that can occur
    ok = rows[:, COLUMNS.index("error")] == 0
    kinds = rows[:, COLUMNS.index("kind")]
    for name, k in KINDS.items():
        assert np.any(ok & (kinds == k)), name
    assert set(np.unique(rows[~ok, COLUMNS.index("error")])) == {RDL_ERR_ARG}
    assert sorted(texts) == sorted([
        "register sub-minor kernel cannot hold this selection",
        "single-wave sub-minor kernel cannot hold this selection",
        "1024-thread sub-minor kernel cannot hold this selection",
        "table sub-minor kernel does not apply to this selection"])
    ids = rows[:, COLUMNS.index("error_id")]
    assert np.array_equal(ids != 0, ~ok)
    assert set(np.unique(ids[~ok])) == set(range(1, len(texts) + 1))
