"""AlgorithmType.python on the device (csrc/python/python_deconvolution.cc;
reference: cpp/algorithms/python_deconvolution.cc and its KAT
cpp/test/test_python_deconvolution.cc).

The user's file runs in the interpreter that runs Radler, so it reports what
it saw by appending to a list on a probe module put into sys.modules
(python_deconvolution_lib.py). Every numeric expectation is exact: one
original channel per deconvolution channel with image_weight 1 makes
load-and-average the identity, float32 -> float64 -> float32 is the identity,
and the functions scale by powers of two. Images are 40 wide x 24 high
wherever a transposed height / width could hide.

The cases that give device memory to torch run in one child process that
imports torch before radler, so that both use one HIP runtime
(python_deconvolution_torch_child.py); test_with_torch reports each of them.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from python_deconvolution_lib import (BANDS, GRID_HOST, HEIGHT, N_FREQ, N_POL, TORCH_CASES,
                                      WIDTH, Joined, base_settings, check_grid,
                                      expect_bad_return, make_inputs, probe_module, write)
from radler_import import radler as rd

pytestmark = pytest.mark.gpu

CALL_ERROR = "Error occurred while executing python deconvolution function"


@pytest.fixture
def probe():
    with probe_module() as module:
        yield module


@pytest.fixture(scope="module")
def inputs():
    return make_inputs()


# ------------------------------------------------------------ error reporting
@pytest.mark.parametrize("function", ["deconvolve", "deconvolve_device"])
def test_error_reporting(tmp_path, function):
    path = write(tmp_path, f"""#! /usr/bin/python

def {function}(residual, model, psf, meta):
  raise RuntimeError("This is a test to see if WSClean handles a raise correctly")
""")
    s = base_settings(path, 64, 64)
    s.minor_iteration_count = 1000
    s.absolute_threshold = 1.0e-8
    psf, residual, model = (np.zeros((64, 64), np.float32) for _ in range(3))
    radler = rd.Radler(s, psf, residual, model, 0.0)
    with pytest.raises(RuntimeError) as e:
        radler.perform(1)
    assert "This is a test" in str(e.value)
    assert CALL_ERROR in str(e.value)


# --------------------------------------------------------------- host contract
HOST_FILE = """
import numpy as np
import radler_python_probe as probe


def deconvolve(residual, model, psf, meta):
    arrays = dict(residual=residual, model=model, psf=psf)
    probe.calls.append(dict(
        shapes={k: a.shape for k, a in arrays.items()},
        dtypes={k: a.dtype for k, a in arrays.items()},
        contiguous={k: bool(a.flags.c_contiguous) for k, a in arrays.items()},
        copies={k: a.copy() for k, a in arrays.items()},
        distinct=len({a.__array_interface__["data"][0] for a in arrays.values()}),
        channels=[(c.frequency, c.weight) for c in meta.channels],
        iteration_number=meta.iteration_number,
        final_threshold=meta.final_threshold,
        gain=meta.gain,
        max_iterations=meta.max_iterations,
        major_iter_threshold=meta.major_iter_threshold,
        mgain=meta.mgain,
        square_joined_channels=meta.square_joined_channels,
    ))
    n_freq, n_pol = residual.shape[:2]
    k = np.arange(n_freq * n_pol, dtype=np.float64).reshape(n_freq, n_pol, 1, 1)
    meta.iteration_number += 7
    return {"residual": residual * 2.0 ** -(k + 1.0), "model": model + 0.5 * residual,
            "level": 0.25, "continue": CONTINUE}
"""


def test_host_contract(tmp_path, probe, inputs):
    run = Joined(inputs, write(tmp_path, HOST_FILE.replace("CONTINUE", "False")))
    assert run.radler.perform(1) is False
    assert run.radler.iteration_number == 7
    assert len(probe.calls) == 1
    call = probe.calls[0]
    image_shape = (N_FREQ, N_POL, HEIGHT, WIDTH)
    assert call["shapes"] == dict(residual=image_shape, model=image_shape,
                                  psf=(N_FREQ, HEIGHT, WIDTH))
    assert all(d == np.float64 for d in call["dtypes"].values())
    assert all(call["contiguous"].values()) and call["distinct"] == 3
    residual, model, psf = inputs
    # plane for plane: element [f, p] is image f * n_pol + p
    for f in range(N_FREQ):
        assert np.array_equal(call["copies"]["psf"][f], psf[f].astype(np.float64))
        for p in range(N_POL):
            assert np.array_equal(call["copies"]["residual"][f, p],
                                  residual[f, p].astype(np.float64)), (f, p)
            assert np.array_equal(call["copies"]["model"][f, p],
                                  model[f, p].astype(np.float64)), (f, p)
    s = run.settings
    assert call["channels"] == [((lo + hi) / 2.0, 1.0) for lo, hi in BANDS]
    assert call["iteration_number"] == 0
    assert call["gain"] == s.minor_loop_gain
    assert call["mgain"] == s.major_loop_gain
    assert call["max_iterations"] == s.minor_iteration_count
    assert call["final_threshold"] == s.absolute_threshold
    assert call["major_iter_threshold"] == 0.0
    assert call["square_joined_channels"] is False
    # what the caller's arrays received: the float32 cast of the same expression
    k = np.arange(N_FREQ * N_POL, dtype=np.float64).reshape(N_FREQ, N_POL, 1, 1)
    r64, m64 = residual.astype(np.float64), model.astype(np.float64)
    expect_residual = (r64 * 2.0 ** -(k + 1.0)).astype(np.float32)
    expect_model = (m64 + 0.5 * r64).astype(np.float32)
    assert np.array_equal(run.residual.view(np.uint32), expect_residual.view(np.uint32))
    assert np.array_equal(run.model.view(np.uint32), expect_model.view(np.uint32))
    assert np.array_equal(run.psf, psf)


def test_host_continue(tmp_path, probe, inputs):
    run = Joined(inputs, write(tmp_path, HOST_FILE.replace("CONTINUE", "True")))
    assert run.radler.perform(1) is True
    assert run.radler.iteration_number == 7
    assert run.radler.perform(run.settings.major_iteration_count) is False
    assert run.radler.iteration_number == 14
    assert [c["iteration_number"] for c in probe.calls] == [0, 7]


# ----------------------------------------------------------------- bad returns
HOST_GOOD = 'dict(residual=residual, model=model, level=0.0, **{"continue": False})'
BAD_RETURNS = {
    "host-not_a_dict": ("deconvolve", "    return [residual, model, 0.0, False]", "dictionary"),
    "host-missing_key": ("deconvolve",
                         '    return {"residual": residual, "level": 0.0, "continue": False}',
                         "'model'"),
    "host-wrong_shape": ("deconvolve",
                         f"    out = {HOST_GOOD}\n"
                         '    out["residual"] = residual.swapaxes(2, 3).copy()\n    return out',
                         r"'residual'.*shape \(1, 1, 40, 24\).*\(1, 1, 24, 40\)"),
    "device-not_a_dict": ("deconvolve_device", "    return None", "dictionary"),
    "device-missing_key": ("deconvolve_device", '    return {"level": 0.0}', "'continue'"),
    "device-no_dlpack": ("deconvolve_device",
                         '    return {"level": 0.0, "continue": False, "residual": 3.0}',
                         "'residual'.*__dlpack__"),
}


@pytest.mark.parametrize("case", sorted(BAD_RETURNS))
def test_bad_return(tmp_path, case):
    expect_bad_return(tmp_path, *BAD_RETURNS[case])


# ------------------------------------------------------------- spectral fitter
FITTER_FILE = """
import numpy as np
import radler_python_probe as probe


def deconvolve(residual, model, psf, meta):
    fitter = meta.spectral_fitter
    seen = dict(channels=[(c.frequency, c.weight) for c in meta.channels])
    values = np.array(VALUES)
    for name, call in (("fit", lambda: fitter.fit(values, 3, 4)),
                       ("fit_and_evaluate", lambda: fitter.fit_and_evaluate(values, 3, 4)),
                       ("short", lambda: fitter.fit_and_evaluate(values[:2], 0, 0)),
                       ("short_fit", lambda: fitter.fit(values[:2]))):
        try:
            seen[name] = call()
        except RuntimeError as e:
            seen[name] = str(e)
    seen["same_object"] = seen["fit_and_evaluate"] is values
    probe.calls.append(seen)
    return {"residual": residual, "model": model, "level": 0.0, "continue": False}
"""
CUBE_BANDS = np.array([(100.0e6, 110.0e6), (120.0e6, 130.0e6), (140.0e6, 150.0e6)])
# exactly linear in frequency (and in x = frequency / reference - 1)
LINEAR = [1.0, 1.5, 2.0]


def run_cube(tmp_path, mode, terms):
    path = write(tmp_path, FITTER_FILE.replace("VALUES", repr(LINEAR)))
    s = base_settings(path)
    s.spectral_fitting.mode = mode
    s.spectral_fitting.terms = terms
    rng = np.random.default_rng(9)
    psf, residual = (rng.standard_normal((3, HEIGHT, WIDTH)).astype(np.float32)
                     for _ in range(2))
    model = np.zeros_like(residual)
    radler = rd.Radler(s, psf, residual, model, 0.0, frequencies=CUBE_BANDS)
    radler.perform(1)


def test_meta_spectral_fitter_polynomial(tmp_path, probe):
    run_cube(tmp_path, rd.SpectralFittingMode.polynomial, 2)
    seen = probe.calls[0]
    centres = [float(b.mean()) for b in CUBE_BANDS]
    assert seen["channels"] == [(c, 1.0) for c in centres]
    own = rd.SpectralFitter(rd.SpectralFittingMode.polynomial, 2, centres, [1.0, 1.0, 1.0])
    for name, expect in (("fit", own.fit(LINEAR, 3, 4)),
                         ("fit_and_evaluate", own.fit_and_evaluate(LINEAR, 3, 4))):
        got = seen[name]
        assert got.dtype == np.float64 and got.shape == (len(expect),), name
        assert np.array_equal(got.astype(np.float32).view(np.uint32),
                              np.asarray(expect, np.float32).view(np.uint32)), name
    # the fit of a linear spectrum returns it, to the rounding of the float32
    # evaluation: a few units in the last place of the largest value
    assert np.abs(seen["fit_and_evaluate"] - LINEAR).max() <= 4 * 2.0 ** -24 * max(LINEAR)
    assert not seen["same_object"]
    for name in ("short", "short_fit"):
        assert "got 2" in seen[name] and "need 3" in seen[name], seen[name]


def test_meta_spectral_fitter_without_fitting(tmp_path, probe):
    run_cube(tmp_path, rd.SpectralFittingMode.no_fitting, 0)
    seen = probe.calls[0]
    assert isinstance(seen["fit"], str) and "no spectral fitting" in seen["fit"]
    assert seen["same_object"]
    assert seen["short"].shape == (2,)  # returned as it came: nothing is checked
    assert seen["channels"] == []  # the fitter holds no frequencies without a mode


# ----------------------------------------------------------- rdl_device_sync
def test_rdl_device_sync():
    from rdl_lib import Session
    session = Session(0)
    lib = session.rdl.lib
    lib.rdl_device_sync.argtypes = [C.c_void_p]
    assert lib.rdl_device_sync(session.h) == 0  # RDL_OK
    assert lib.rdl_device_sync(None) != 0
    assert len(lib.rdl_last_error()) > 0
    assert lib.rdl_device_sync(session.h) == 0
    session.close()


# ------------------------------------------------------------------------ grid
@pytest.mark.parametrize("max_threads", [1, 2], ids=["in_turn", "pooled"])
def test_grid_calls_twice_per_subimage(tmp_path, probe, max_threads):
    check_grid(tmp_path, probe, max_threads, GRID_HOST)


# ------------------------------------------------------ device memory in torch
@pytest.fixture(scope="module")
def torch_results(tmp_path_factory):
    """Every torch case, run once in one child process."""
    here = os.path.dirname(os.path.abspath(__file__))
    results = tmp_path_factory.mktemp("torch_child") / "results.json"
    child = subprocess.run(
        [sys.executable, os.path.join(here, "python_deconvolution_torch_child.py"),
         str(results)], capture_output=True, text=True)
    report = f"exit status {child.returncode}\n{child.stdout[-2000:]}\n{child.stderr[-4000:]}"
    assert results.exists(), report
    return json.loads(results.read_text()), report


@pytest.mark.parametrize("case", TORCH_CASES)
def test_with_torch(torch_results, case):
    """The device contract with torch as the DLPack consumer: the views'
    device, dtype, shape and strides, the in-place edit, the returned copy,
    the four kinds of bad 'residual' / 'model', tensors kept past the call, and
    the grid on both paths."""
    results, report = torch_results
    assert "child" not in results, results["child"]
    assert case in results, report
    assert results[case] is None, results[case]
