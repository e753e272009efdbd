"""radler.restore (radler::math::RestoreImage) on the MI355X: residual + model
convolved with the clean beam, against the exact linear convolution in numpy
float64 with the box cut from primitive_refs.place_gaussian.

Per pixel, with c the reference convolution and r the residual:
  |got - (r + c)| <= 2^-24 (|r + c| + |c|) + 1e-12 sum|model|
the two float roundings the contract allows (the convolution, then the sum)
and a loose cover for the float64 transform, whose error is of order
log2(N) 2^-53 sum|model|. Where the beam's box does not reach, c = 0: the
assertion a circular convolution fails.
"""
import math

import numpy as np
import pytest

import render_refs as R
from radler_import import radler as rd

pytestmark = pytest.mark.gpu

F = np.float32
PIX = 1.0 / 3600.0 * np.pi / 180.0
SIZES = [(64, 48), (74, 58)]
PA = math.radians(30.0)
# (major, minor) FWHM in pixels of pixel_scale_l, pixel_scale_m / pixel_scale_l
BEAMS = {"3x2": (3.0, 2.0, 1.0), "3x2_tall_pixels": (3.0, 2.0, 1.5), "12x8_clipped": (12.0, 8.0, 1.0)}


def sources(w, h, seed):
    """a dozen point sources of both signs, two of them in opposite corners"""
    rng = np.random.default_rng(seed)
    model = np.zeros((h, w), F)
    model[0, 0], model[h - 1, w - 1] = 1.0, -0.7
    while np.count_nonzero(model) < 12:
        model[rng.integers(0, h), rng.integers(0, w)] = rng.uniform(0.05, 0.9) * rng.choice([-1, 1])
    residual = (1e-4 * float(np.max(np.abs(model))) * rng.standard_normal((h, w))).astype(F)
    return residual, model


def beam_of(name):
    major, minor, ratio = BEAMS[name]
    return major * PIX, minor * PIX, PA, PIX, ratio * PIX


def check(got, residual, model, kernel, what):
    conv = R.linear_convolve(model, kernel)
    ref = residual.astype(np.float64) + conv
    bound = R.restore_bound(residual, conv, model)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(np.max(err / bound))
    print(f"restore {what}: max |got - ref| = {np.max(err):.3g}, max error / bound = {worst:.3g}, "
          f"max |ref| = {np.max(np.abs(ref)):.3g}")
    assert got.dtype == F and got.shape == residual.shape
    assert np.all(err <= bound)
    return conv


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("beam", list(BEAMS))
def test_restore_against_the_linear_convolution(w, h, beam):
    residual, model = sources(w, h, seed=w)
    args = beam_of(beam)
    kernel, box = R.beam_kernel(w, h, *args)
    assert box % 2 == 0 and (box == min(w, h)) == (beam == "12x8_clipped")
    kept = residual.copy(), model.copy()
    got = rd.restore(residual, model, *args)
    assert np.array_equal(residual, kept[0]) and np.array_equal(model, kept[1])
    check(got, residual, model, kernel, f"{w}x{h} {beam}")
    assert float(np.max(np.abs(got - residual))) > 0.5  # the beam has peak 1 (Jy/beam)


@pytest.mark.parametrize("w,h", SIZES)
def test_restore_with_a_zero_beam_adds_the_model(w, h):
    residual, model = sources(w, h, seed=3)
    got = rd.restore(residual, model, 0.0, 0.0, 0.0, PIX, PIX)
    assert np.array_equal(got, residual + model)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("beam", list(BEAMS))
def test_restore_does_not_wrap(w, h, beam):
    """One source at (0, 0): every pixel farther than box / 2 from it in x or y
    keeps its residual, the opposite edges included."""
    rng = np.random.default_rng(11)
    model = np.zeros((h, w), F)
    model[0, 0] = 1.0
    residual = (1e-4 * rng.standard_normal((h, w))).astype(F)
    args = beam_of(beam)
    kernel, box = R.beam_kernel(w, h, *args)
    got = rd.restore(residual, model, *args)
    check(got, residual, model, kernel, f"{w}x{h} {beam}, corner source")
    yy, xx = np.mgrid[0:h, 0:w]
    far = (xx > box // 2) | (yy > box // 2)
    assert np.count_nonzero(far[:, w - 1]) and np.count_nonzero(far[h - 1, :])
    untouched = np.abs(got[far].astype(np.float64) - residual[far].astype(np.float64))
    assert np.all(untouched <= 2.0 ** -24 * np.abs(residual[far]) + 1e-12)


def test_restore_of_a_stack_is_the_planes_one_by_one():
    w, h = 74, 58
    pairs = [sources(w, h, seed=s) for s in (1, 2, 3)]
    residuals = np.stack([p[0] for p in pairs])
    models = np.stack([p[1] for p in pairs])
    args = beam_of("3x2")
    kept = residuals.copy(), models.copy()
    got = rd.restore(residuals, models, *args)
    assert got.shape == (3, h, w)
    assert np.array_equal(residuals, kept[0]) and np.array_equal(models, kept[1])
    for k in range(3):
        one = rd.restore(residuals[k], models[k], *args)
        assert np.array_equal(got[k].view(np.uint32), one.view(np.uint32))


def test_restore_refuses_half_a_beam():
    image = np.zeros((48, 64), F)
    with pytest.raises(ValueError):
        rd.restore(image, image, 3.0 * PIX, 0.0, 0.0, PIX, PIX)
    with pytest.raises(ValueError):
        rd.restore(image, image, 3.0 * PIX, 2.0 * PIX, 0.0, PIX, 0.0)
