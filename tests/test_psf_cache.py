"""The PSF-derived products of a multiscale major iteration (scale-convolved
PSFs, twice-convolved PSFs, padded PSF spectra, the per-scale PSF peaks) are
kept for the next major iteration while the PSFs, the scales and the sizes
stay the same (MultiScalePsfProducts). A kept product is the product
that would be made again from the same inputs by the same kernels, so runs
with the cache (default) and without it (RDL_PSF_CACHE=0) are bit-identical;
the PSFs are compared by content, so a PSF changed by one ulp between two
major iterations is seen. The switches are read once per major iteration, so
both sides run in this process."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PIXEL = 1.0 / 3600.0 * np.pi / 180.0


def make_settings(rd, w, scale_list=None):
    s = rd.Settings()
    s.algorithm_type = rd.AlgorithmType.multiscale
    s.trimmed_image_width = s.trimmed_image_height = w
    s.pixel_scale.x = s.pixel_scale.y = PIXEL
    s.minor_iteration_count = 4000
    s.absolute_threshold = 2e-3
    s.major_loop_gain = 0.7
    s.border_ratio = 0.0
    if scale_list is None:
        s.multiscale.max_scales = 3
    else:
        s.multiscale.scale_list = scale_list
    return s


def two_major_iterations(rd, env, w=256, scale_list=None, channels=1, change=None,
                         trace_profile=False):
    """Two Radler.perform calls on one Radler under the environment `env`;
    change(psf) edits the PSF array (which the accessors borrow) between
    them. Returns residual, model, flags, iterations and the host profile of
    the second call."""
    from config_problems import joined_channels
    from synthetic import problem
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = make_settings(rd, w, scale_list)
        extra = {}
        if channels == 1:
            psf, dirty = problem(w, w, 40, 5, seed=77)
        else:
            freqs = [100e6 + 10e6 * i for i in range(channels)]
            psf, dirty = joined_channels(w, 40, 5, seed=78, frequencies=freqs)
            extra = dict(n_deconvolution_groups=channels,
                         frequencies=np.array([[f, f] for f in freqs], np.float64),
                         weights=np.ones(channels, np.float64))
        psf = np.ascontiguousarray(psf, np.float32).copy()
        res, mod = dirty.copy(), np.zeros_like(dirty)
        r = rd.Radler(s, psf, res, mod, 2.0 * PIXEL, **extra)
        flags = [r.perform(0)]
        first_iterations = r.iteration_number
        if change is not None:
            change(psf)
        rd.gpu.host_profile_reset()
        rd.gpu.host_profile_enable(True)
        try:
            flags.append(r.perform(1))
        finally:
            rd.gpu.host_profile_enable(False)
        prof = rd.gpu.host_profile()
        assert 0 < first_iterations < r.iteration_number, "both major iterations must clean"
        return dict(residual=res, model=mod, flags=flags, iterations=r.iteration_number,
                    first_iterations=first_iterations, profile=prof)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same(a, b):
    for k in ("residual", "model"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert a["flags"] == b["flags"]
    assert a["iterations"] == b["iterations"]
    assert a["first_iterations"] == b["first_iterations"]


def made_again(prof):
    return prof.get("ms.convolve_psfs", (0, 0.0))[0]


OFF = {"RDL_PSF_CACHE": "0"}
ON = {"RDL_PSF_CACHE": "1"}


def one_ulp(psf):
    flat = psf.reshape(-1)
    i = flat.size // 3
    flat[i] = np.nextafter(flat[i], np.float32(np.inf))


@pytest.fixture(scope="module")
def rd():
    from radler_import import radler
    return radler


@pytest.fixture(scope="module")
def reference(rd):
    """The run without the cache, computed once."""
    return two_major_iterations(rd, OFF)


@pytest.mark.gpu
def test_cache_hit_is_bit_identical_and_skips_the_setup(rd, reference):
    assert made_again(reference["profile"]) == 1
    assert "ms.psf_cache_check" not in reference["profile"]
    hit = two_major_iterations(rd, ON)
    same(hit, reference)
    # the second major iteration made none of the products again
    prof = hit["profile"]
    assert prof.get("ms.psf_cache_check", (0, 0.0))[0] == 1
    assert "ms.convolve_psfs" not in prof
    assert "ms.twice_convolved" not in prof
    assert prof.get("ms.execute", (0, 0.0))[0] == 1


@pytest.mark.gpu
def test_traces_with_and_without_the_cache(rd):
    """DeviceRun keeps its algorithm (and its PSFs) over execute() calls: the
    component traces of two major iterations, cache against no cache."""
    from synthetic import problem
    psf, dirty = problem(256, 256, 40, 5, seed=77)
    out = {}
    for name, env in (("off", "0"), ("on", "1")):
        os.environ["RDL_PSF_CACHE"] = env
        try:
            run = rd.gpu.DeviceRun(make_settings(rd, 256), psf, dirty, [], 2.0 * PIXEL,
                                   trace=True)
            traces = []
            for _ in range(2):
                run.execute()
                traces.append(np.array(run.trace()))
            out[name] = (traces, run.residual(), run.model())
            del run
        finally:
            del os.environ["RDL_PSF_CACHE"]
    assert len(out["on"][0][0]) > 0 and len(out["on"][0][1]) > 0
    for a, b in zip(out["on"][0], out["off"][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(out["on"][1], out["off"][1])
    assert np.array_equal(out["on"][2], out["off"][2])


@pytest.mark.gpu
def test_one_ulp_of_one_psf_pixel_misses(rd, reference):
    off = two_major_iterations(rd, OFF, change=one_ulp)
    on = two_major_iterations(rd, ON, change=one_ulp)
    same(on, off)
    assert on["profile"].get("ms.psf_cache_check", (0, 0.0))[0] == 1
    assert made_again(on["profile"]) == 1
    # and the changed PSF matters: the unchanged run ends elsewhere
    assert not np.array_equal(off["residual"], reference["residual"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["scale_list", "size", "joined"])
def test_other_problems_after_a_cached_one(rd, reference, case):
    """A changed scale list, a changed image size, and a two-channel joined
    set with one changed PSF, each run after the cached 256^2 problem in the
    same process: each matches its own run without the cache."""
    two_major_iterations(rd, ON)  # leaves the base problem's products behind
    kw = {"scale_list": dict(scale_list=[0.0, 6.0, 20.0]),
          "size": dict(w=320),
          "joined": dict(channels=2, change=lambda psf: one_ulp(psf[1]))}[case]
    on = two_major_iterations(rd, ON, **kw)
    off = two_major_iterations(rd, OFF, **kw)
    same(on, off)
    if case == "joined":
        assert made_again(on["profile"]) == 1  # the changed channel PSF was seen
    else:
        assert made_again(on["profile"]) == 0  # a hit on this problem's own products


@pytest.mark.gpu
def test_a_budget_too_small_for_anything(rd, reference):
    small = two_major_iterations(rd, {"RDL_PSF_CACHE": "1", "RDL_PSF_CACHE_MB": "0"})
    same(small, reference)
    assert made_again(small["profile"]) == 1
    assert "ms.psf_cache_check" not in small["profile"]


@pytest.mark.gpu
def test_a_budget_that_fits_the_convolved_set_only(rd):
    """512^2 float planes are 1 MiB each. One PSF and three scales: the
    convolved set with its reference copies is 3 + 1 + 1 = 5 planes, which a
    5 MiB budget holds to the byte, and no later product (a twice-convolved
    plane is 1 MiB more). The second major iteration then hits, and makes the
    products that did not fit again."""
    kw = dict(w=512, scale_list=[0.0, 6.0, 20.0])
    off = two_major_iterations(rd, OFF, **kw)
    part = two_major_iterations(rd, {"RDL_PSF_CACHE": "1", "RDL_PSF_CACHE_MB": "5"}, **kw)
    same(part, off)
    prof = part["profile"]
    assert prof.get("ms.psf_cache_check", (0, 0.0))[0] == 1
    assert "ms.convolve_psfs" not in prof
    assert prof.get("ms.twice_convolved", (0, 0.0))[0] >= 1
