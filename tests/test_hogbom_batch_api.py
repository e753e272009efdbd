"""rdl_hogbom_batch_run's argument errors and radler.PlaneBatch's refused
settings, on a machine without a device.

Every argument error of the C-ABI is returned before the first device call:
the session handle these calls pass is a block of zero bytes that no device
call could use. Every setting PlaneBatch does not honour raises a
RuntimeError that names it before a session is asked for.
"""
import ctypes as C
import os

import numpy as np
import pytest

from hogbom_batch_lib import MAX_PIXELS, BatchOut, BatchParams
from rdl_lib import HIP_SO

RDL_ERR_ARG = 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HIP_SO):
        pytest.skip("librdl_hip.so not built")
    lib = C.CDLL(HIP_SO)
    lib.rdl_last_error.restype = C.c_char_p
    return lib


class Call:
    """A well-formed call on two 6 x 4 planes, apart from its session."""

    def __init__(self):
        self.session = C.create_string_buffer(4096)
        self.block = C.create_string_buffer(4096)  # stands for device memory: never touched
        p = self.p = BatchParams()
        p.width, p.height, p.n_planes = 6, 4, 2
        addr = C.addressof(self.block)
        p.d_residuals = p.d_models = p.d_psfs = p.d_mask = addr
        p.residual_stride = p.model_stride = p.psf_stride = p.mask_stride = 24
        p.gain, p.major_loop_gain = 0.1, 1.0
        self.threshold = np.zeros(2, np.float32)
        self.iteration_start = np.zeros(2, np.uint64)
        self.max_iterations = np.full(2, 10, np.uint64)
        self.active = np.ones(2, np.uint8)
        self.out = (BatchOut * 2)()
        self.trace = np.zeros((2, 4, 2), np.uint32)
        self.args = dict(s=C.addressof(self.session), p=C.addressof(p),
                         threshold=self.threshold.ctypes.data,
                         iteration_start=self.iteration_start.ctypes.data,
                         max_iterations=self.max_iterations.ctypes.data,
                         active=self.active.ctypes.data, out=C.addressof(self.out),
                         trace=self.trace.ctypes.data)

    def run(self, lib):
        a = self.args
        rc = lib.rdl_hogbom_batch_run(
            C.c_void_p(a["s"]), C.c_void_p(a["p"]), C.c_void_p(a["threshold"]),
            C.c_void_p(a["iteration_start"]), C.c_void_p(a["max_iterations"]),
            C.c_void_p(a["active"]), C.c_void_p(a["out"]), C.c_void_p(a["trace"]), C.c_uint64(4))
        return rc, lib.rdl_last_error().decode()


@pytest.mark.parametrize("name", ["s", "p", "threshold", "iteration_start", "max_iterations",
                                  "active", "out"])
def test_null_argument(lib, name):
    call = Call()
    call.args[name] = None
    rc, message = call.run(lib)
    assert rc == RDL_ERR_ARG and "NULL" in message


@pytest.mark.parametrize("name", ["d_residuals", "d_models", "d_psfs"])
def test_null_stack(lib, name):
    call = Call()
    setattr(call.p, name, None)
    rc, message = call.run(lib)
    assert rc == RDL_ERR_ARG and "NULL" in message


def test_no_planes(lib):
    call = Call()
    call.p.n_planes = 0
    rc, message = call.run(lib)
    assert rc == RDL_ERR_ARG and "no planes" in message


def test_unknown_flag(lib):
    call = Call()
    call.p.flags = 2
    rc, message = call.run(lib)
    assert rc == RDL_ERR_ARG and "flag" in message


@pytest.mark.parametrize("w,h", [(0, 4), (6, 0)])
def test_empty_plane(lib, w, h):
    call = Call()
    call.p.width, call.p.height = w, h
    rc, message = call.run(lib)
    assert rc == RDL_ERR_ARG and "empty" in message


@pytest.mark.parametrize("w,h", [(1025, 1024), (1, MAX_PIXELS + 1), (65536, 65536),
                                 (0xffffffff, 0xffffffff)])
def test_plane_above_the_pixel_cap(lib, w, h):
    call = Call()
    call.p.width, call.p.height = w, h
    big = 1 << 62
    call.p.residual_stride = call.p.model_stride = call.p.psf_stride = call.p.mask_stride = big
    rc, message = call.run(lib)
    assert rc == RDL_ERR_ARG and "2^20" in message


@pytest.mark.parametrize("name,stride", [
    ("residual_stride", 23), ("residual_stride", 0), ("model_stride", 23), ("model_stride", 0),
    ("psf_stride", 23), ("psf_stride", 1), ("mask_stride", 23), ("mask_stride", 1)])
def test_stride_below_a_plane(lib, name, stride):
    call = Call()
    setattr(call.p, name, stride)
    rc, message = call.run(lib)
    assert rc == RDL_ERR_ARG and name.split("_")[0] in message and "stride" in message


# ------------------------------------------------------- radler.PlaneBatch
def batch_settings(rd, w=6, h=4):
    s = rd.Settings()
    s.trimmed_image_width, s.trimmed_image_height = w, h
    s.algorithm_type = rd.AlgorithmType.generic_clean
    s.generic.use_sub_minor_optimization = False
    s.minor_iteration_count = 10
    return s


def _set(path, value):
    def change(rd, s):
        target = s
        *parents, leaf = path.split(".")
        for name in parents:
            target = getattr(target, name)
        setattr(target, leaf, value(rd) if callable(value) else value)
    return change


REFUSED = {
    "algorithm_type": _set("algorithm_type", lambda rd: rd.AlgorithmType.multiscale),
    "generic.use_sub_minor_optimization": _set("generic.use_sub_minor_optimization", True),
    "auto_mask_sigma": _set("auto_mask_sigma", 3.0),
    "absolute_auto_mask_threshold": _set("absolute_auto_mask_threshold", 0.1),
    "local_rms.method": _set("local_rms.method", lambda rd: rd.LocalRmsMethod.rms_window),
    "local_rms.image": _set("local_rms.image", "rms.fits"),
    "spectral_fitting.mode": _set("spectral_fitting.mode",
                                  lambda rd: rd.SpectralFittingMode.polynomial),
    "parallel.grid_width": _set("parallel.grid_width", 2),
    "parallel.grid_height": _set("parallel.grid_height", 2),
    # (C++-only in the Settings binding: radler.gpu.set_component_optimization)
    "component_optimization_algorithm": lambda rd, s: rd.gpu.set_component_optimization(
        s, rd.OptimizationAlgorithm.gradient_descent),
    "linked_polarizations": _set("linked_polarizations",
                                 lambda rd: {rd.Polarization.stokes_i, rd.Polarization.stokes_q}),
    "squared_joins": _set("squared_joins", True),
    "spectral_correction": _set("spectral_correction", [1.0, -0.7]),
    "fits_mask": _set("fits_mask", "mask.fits"),
    "casa_mask": _set("casa_mask", "mask.image"),
    "horizon_mask_distance": _set("horizon_mask_distance", 0.1),
    "save_source_list": _set("save_source_list", True),
}


@pytest.fixture(scope="module")
def rd():
    from radler_import import radler
    return radler


def stacks(n_planes=2, w=6, h=4):
    psf = np.zeros((h, w), np.float32)
    psf[h // 2, w // 2] = 1.0
    return psf, np.ones((n_planes, h, w), np.float32), np.zeros((n_planes, h, w), np.float32)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_plane_batch_refuses_setting(rd, name):
    s = batch_settings(rd)
    REFUSED[name](rd, s)
    with pytest.raises(RuntimeError) as error:
        rd.PlaneBatch(s, *stacks())
    assert "settings." + name + " " in str(error.value)


def test_plane_batch_refuses_planes_above_the_pixel_cap(rd):
    """The shapes agree with the settings; no array of that size is needed to
    be refused: the settings are checked against the stacks first, so the
    stacks here are of the refused size but never read."""
    w, h = 1025, 1024
    psf = np.zeros((h, w), np.float32)
    planes = np.zeros((1, h, w), np.float32)
    with pytest.raises(RuntimeError) as error:
        rd.PlaneBatch(batch_settings(rd, w, h), psf, planes, planes.copy())
    assert "trimmed_image_width" in str(error.value) and "2^20" in str(error.value)


def test_plane_batch_accepts_the_honoured_settings(rd):
    """Constructing needs no device; every honoured setting may be set."""
    s = batch_settings(rd)
    s.absolute_threshold, s.auto_threshold_sigma = 0.01, 3.0
    s.minor_loop_gain, s.major_loop_gain = 0.2, 0.8
    s.major_iteration_count = 3
    s.allow_negative_components, s.stop_on_negative_components = False, True
    s.border_ratio, s.divergence_limit = 0.1, 2.0
    psf, residuals, models = stacks(3)
    mask = np.ones((4, 6), bool)
    batch = rd.PlaneBatch(s, psf, residuals, models, mask)
    assert batch.n_planes == 3 and list(batch.iteration_numbers) == [0, 0, 0]
    assert batch.iteration_numbers.dtype == np.uint64
    per_plane = rd.PlaneBatch(s, np.stack([psf] * 3), residuals, models,
                              np.ones((3, 4, 6), np.uint8))
    assert per_plane.n_planes == 3


@pytest.mark.parametrize("case", ["psf-count", "model-shape", "mask-shape", "mask-dtype",
                                  "plane-size", "residual-2d"])
def test_plane_batch_argument_errors(rd, case):
    s = batch_settings(rd)
    psf, residuals, models = stacks(3)
    args = dict(psfs=psf, residuals=residuals, models=models, masks=None)
    if case == "psf-count":
        args["psfs"] = np.stack([psf] * 2)
    elif case == "model-shape":
        args["models"] = models[:2].copy()
    elif case == "mask-shape":
        args["masks"] = np.ones((2, 4, 6), np.uint8)
    elif case == "mask-dtype":
        args["masks"] = np.ones((4, 6), np.float32)
    elif case == "plane-size":
        s.trimmed_image_width = 7
    else:
        args["residuals"], args["models"] = residuals[0].copy(), models[0].copy()
    with pytest.raises((RuntimeError, TypeError)):
        rd.PlaneBatch(s, args["psfs"], args["residuals"], args["models"], args["masks"])
