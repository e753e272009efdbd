"""The scale > 0 model update of the fast multiscale loop stamps the shape
kernel once per component, or convolves the loop's model by FFT when that is
cheaper. The stamping kernel skips selected pixels whose model value stayed
zero, so its cost follows the loop's components, not its selected pixels:
the gate is min(selected, components) x n^2 <= 1e9 (RDL_MODEL_GATE=0: the
selected pixels alone, as before).

The case: a 512^2 image of one broad blob (sigma 60 px), scales 0 and 200
(a 201 x 201 shape kernel, so the old gate turns at 1e9 / 201^2 = 24 752
selected pixels), sub_minor_loop_gain 0.9 and 20 minor iterations. The
scale-200 loop selects every pixel above a tenth of the convolved peak inside
the 100-pixel scale border: for a Gaussian of sigma >= 60 that is more than
2 pi 60^2 ln 10 = 52 000 pixels (checked below on the CPU), while the loop
cleans at most 20 components. Both methods add the same convolution to the
model (equal to rounding), and the loop never reads the
model, so traces and residuals are bit-identical."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PIXEL = 1.0 / 3600.0 * np.pi / 180.0
IMG_TOL = 1e-6  # of max|dirty|: the bound tests/test_configs_gpu.py applies to models
W = 512
SCALE = 200.0
N_KERNEL = 201
SIGMA = 60.0


def blob_problem():
    from synthetic import make_dirty, make_psf
    psf = make_psf(W, W, fwhm=4.0)
    yy, xx = np.mgrid[0:W, 0:W].astype(np.float64)
    sky = np.exp(-0.5 * ((xx - 250.0) ** 2 + (yy - 262.0) ** 2) / SIGMA ** 2)
    sky /= 2.0 * np.pi * 1.7 ** 2  # the beam's area: a dirty peak near 1
    return psf, make_dirty(psf, sky, 1e-4, seed=5)


def test_case_selects_more_pixels_than_the_old_gate_allows():
    """On the CPU: the dirty image itself is narrower than its scale-200
    convolution, and already has more than 1e9 / 201^2 pixels above a tenth
    of its peak inside the scale border."""
    _, dirty = blob_problem()
    border = int(np.ceil(SCALE * 0.5))
    box = dirty[border:W - border, border:W - border]
    n_above = np.count_nonzero(box > 0.1 * dirty.max())
    assert n_above > 50000 and n_above * N_KERNEL ** 2 > 2 * 1e9


def settings(rd):
    s = rd.Settings()
    s.algorithm_type = rd.AlgorithmType.multiscale
    s.trimmed_image_width = s.trimmed_image_height = W
    s.pixel_scale.x = s.pixel_scale.y = PIXEL
    s.minor_iteration_count = 20
    s.absolute_threshold = 1e-3
    s.major_loop_gain = 1.0
    s.border_ratio = 0.0
    s.multiscale.scale_list = [0.0, SCALE]
    s.multiscale.sub_minor_loop_gain = 0.9
    return s


class Families:
    def __init__(self):
        from rdl_lib import HIP_SO
        self.lib = C.CDLL(HIP_SO)
        self.lib.rdl_timing_get_all.argtypes = [C.c_char_p, C.POINTER(C.c_double),
                                                C.POINTER(C.c_uint64), C.POINTER(C.c_double)]

    def start(self):
        self.lib.rdl_timing_reset_all()
        self.lib.rdl_timing_enable_all(1)

    def stop(self):
        self.lib.rdl_timing_enable_all(0)
        out = {}
        for fam in ("add", "stamp_model"):
            ms, n, b = C.c_double(), C.c_uint64(), C.c_double()
            self.lib.rdl_timing_get_all(fam.encode(), C.byref(ms), C.byref(n), C.byref(b))
            out[fam] = n.value
        self.lib.rdl_timing_reset_all()
        return out


def run(rd, psf, dirty, gate, trace):
    fams = Families()
    if gate is None:
        os.environ.pop("RDL_MODEL_GATE", None)
    else:
        os.environ["RDL_MODEL_GATE"] = gate
    try:
        r = rd.gpu.DeviceRun(settings(rd), psf, dirty, [], 2.0 * PIXEL, trace=trace)
        r.restore()
        r.sync()
        fams.start()
        result = r.execute()
        r.sync()
        launches = fams.stop()
        out = dict(iterations=result["iterations"], residual=r.residual(), model=r.model(),
                   trace=np.array(r.trace()) if trace else None, launches=launches)
        del r
        return out
    finally:
        os.environ.pop("RDL_MODEL_GATE", None)


@pytest.mark.gpu
@pytest.mark.parametrize("trace", [True, False], ids=["synchronous", "deferred"])
def test_gate_on_components_stamps_where_the_old_gate_transformed(trace):
    from radler_import import radler as rd
    psf, dirty = blob_problem()
    old = run(rd, psf, dirty, "0", trace)
    new = run(rd, psf, dirty, None, trace)
    # not vacuous: the old gate sends this case through the FFT
    assert old["launches"]["add"] > 0, old["launches"]
    assert new["launches"]["add"] == 0, new["launches"]
    assert new["launches"]["stamp_model"] > old["launches"]["stamp_model"], (new["launches"],
                                                                             old["launches"])
    assert old["iterations"] == new["iterations"] > 0
    if trace:
        assert len(new["trace"]) > 0 and np.array_equal(old["trace"], new["trace"])
        assert (new["trace"].reshape(-1, 3)[:, 2] == 1).any(), "no scale-200 component"
    assert np.array_equal(old["residual"].view(np.uint32), new["residual"].view(np.uint32))
    diff = float(np.abs(old["model"] - new["model"]).max())
    tol = IMG_TOL * float(np.abs(dirty).max())
    print(f"model: max |FFT - stamped| = {diff:.3e}, bound {tol:.3e}, "
          f"max |model| = {float(np.abs(new['model']).max()):.3e}")
    assert np.abs(new["model"]).max() > 0
    assert diff <= tol
