"""Shared by tests/test_python_deconvolution_gpu.py and its child process
tests/python_deconvolution_torch_child.py: the inputs, the Radler objects and
the user files of the AlgorithmType.python tests.

The user's file runs in the interpreter that runs Radler, so it reports what
it saw by appending to a list on a probe module put into sys.modules.
"""
import contextlib
import sys
import types

import numpy as np

from radler_import import radler as rd

WIDTH, HEIGHT = 40, 24
N_FREQ, N_POL = 2, 2
BANDS = [(100.0e6, 110.0e6), (120.0e6, 130.0e6)]
PROBE = "radler_python_probe"

# The cases that hand device memory to torch. They run in a child process that
# imports torch before radler (python_deconvolution_torch_child.py says why).
TORCH_CASES = (
    "bad_return_wrong_shape", "bad_return_float64", "bad_return_non_contiguous",
    "bad_return_cpu", "in_place_level_and_continue", "in_place_none", "in_place_the_views",
    "returned_copy", "tensors_outlive_the_call", "grid_in_turn", "grid_pooled",
)


@contextlib.contextmanager
def probe_module():
    module = types.ModuleType(PROBE)
    module.calls = []
    module.kept = []
    sys.modules[PROBE] = module
    try:
        yield module
    finally:
        module.calls.clear()
        module.kept.clear()
        del sys.modules[PROBE]


def make_inputs():
    """Eight distinct image planes and two PSFs; read-only, copied by each use."""
    rng = np.random.default_rng(20241021)
    residual = rng.standard_normal((N_FREQ, N_POL, HEIGHT, WIDTH)).astype(np.float32)
    model = rng.standard_normal((N_FREQ, N_POL, HEIGHT, WIDTH)).astype(np.float32)
    psf = rng.standard_normal((N_FREQ, HEIGHT, WIDTH)).astype(np.float32)
    for a in (residual, model, psf):
        a.setflags(write=False)
    return residual, model, psf


def write(directory, text, name="user_deconvolution.py"):
    path = directory / name
    path.write_text(text)
    return str(path)


def base_settings(filename, width=WIDTH, height=HEIGHT):
    s = rd.Settings()
    s.algorithm_type = rd.AlgorithmType.python
    s.python.filename = filename
    s.trimmed_image_width, s.trimmed_image_height = width, height
    s.pixel_scale.x = s.pixel_scale.y = 1.0 / 60.0 * np.pi / 180.0
    # values a float holds exactly: meta reports them through the algorithm's floats
    s.minor_iteration_count = 123
    s.absolute_threshold = 2.0 ** -6
    s.minor_loop_gain = 0.125
    s.major_loop_gain = 0.75
    return s


class Joined:
    """A Radler over two channels x two polarizations of the shared inputs."""

    def __init__(self, inputs, filename):
        self.residual, self.model, self.psf = (a.copy() for a in inputs)
        self.settings = base_settings(filename)
        self.settings.spectral_fitting.mode = rd.SpectralFittingMode.polynomial
        self.settings.spectral_fitting.terms = 2
        table = rd.WorkTable([], N_FREQ, N_FREQ)
        polarizations = [rd.Polarization.stokes_i, rd.Polarization.stokes_q]
        for f in range(N_FREQ):
            for p in range(N_POL):
                e = rd.WorkTableEntry()
                e.original_channel_index = f
                e.polarization = polarizations[p]
                e.band_start_frequency, e.band_end_frequency = BANDS[f]
                e.image_weight = 1.0
                if p == 0:
                    e.psfs.append(self.psf[f])
                e.residual = self.residual[f, p]
                e.model = self.model[f, p]
                table.add_entry(e)
        self.radler = rd.Radler(self.settings, table, 0.0)


def single(filename, width=WIDTH, height=HEIGHT, seed=5):
    """A one-image Radler; returns it with the arrays it views."""
    rng = np.random.default_rng(seed)
    psf, residual = (rng.standard_normal((height, width)).astype(np.float32) for _ in range(2))
    model = np.zeros_like(residual)
    return rd.Radler(base_settings(filename, width, height), psf, residual, model, 0.0), \
        (psf, residual, model)


def result_file(function, body):
    return f"""
import numpy as np

def {function}(residual, model, psf, meta):
{body}
"""


def expect_bad_return(directory, function, body, message):
    """perform() raises a RuntimeError that says (regular expression) what is wrong."""
    import re
    radler, keep = single(write(directory, result_file(function, body)))
    try:
        radler.perform(1)
    except RuntimeError as e:
        assert re.search(message, str(e)), str(e)
    else:
        raise AssertionError("perform() accepted the return value")


# ------------------------------------------------------------------------ grid
GRID_HOST = """
import numpy as np
import radler_python_probe as probe


def deconvolve(residual, model, psf, meta):
    probe.calls.append((residual.shape, psf.shape, meta.max_iterations,
                        meta.major_iter_threshold))
    return {"residual": residual, "model": model, "level": np.abs(residual).max(),
            "continue": False}
"""
GRID_DEVICE = """
import torch
import radler_python_probe as probe


def deconvolve_device(residual, model, psf, meta):
    r = torch.from_dlpack(residual)
    probe.calls.append((tuple(r.shape), tuple(torch.from_dlpack(psf).shape),
                        meta.max_iterations, meta.major_iter_threshold))
    return {"level": float(r.abs().max()), "continue": False}
"""


def check_grid(directory, probe, max_threads, source):
    """64 x 64 split 2 x 1: the function is called twice per subimage, first
    to find its peak (max_iterations == 0), then to clean; a function that
    returns its inputs leaves the images as they were."""
    size = 64
    s = base_settings(write(directory, source), size, size)
    s.parallel.grid_width, s.parallel.grid_height = 2, 1
    s.parallel.max_threads = max_threads
    rng = np.random.default_rng(11)
    psf, residual = (rng.standard_normal((size, size)).astype(np.float32) for _ in range(2))
    model = np.zeros_like(residual)
    before = residual.copy()
    radler = rd.Radler(s, psf, residual, model, 0.0)
    assert radler.perform(1) is False
    # a pass over both subimages to find the peaks, then a pass to clean
    assert len(probe.calls) == 4, probe.calls
    find_peak, clean = probe.calls[:2], probe.calls[2:]
    assert [c[2] for c in find_peak] == [0, 0]
    assert [c[2] for c in clean] == [s.minor_iteration_count] * 2
    assert all(c[3] > 0.0 for c in clean)
    assert sorted(c[0] for c in find_peak) == sorted(c[0] for c in clean)
    for shape, psf_shape, _, _ in probe.calls:
        assert shape[:2] == (1, 1) and psf_shape == (1,) + shape[2:]
        assert 0 < shape[2] <= size and 0 < shape[3] <= size
    assert sum(c[0][3] for c in clean) >= size  # the two subimages span the width
    assert np.array_equal(residual, before)
    assert not model.any()
