"""The three device primitives of the adaptive-scale-pixel algorithm
(include/rdl_hip.h, "adaptive scale pixel"; csrc/hip/asp.hip) and the
Gaussian fitter built on them (csrc/host/gaussian_fit.h), against the numpy
float64 references of tests/asp_lib.py. Images are 64 wide and 48 high, so a
width/height swap shows."""
import numpy as np
import pytest

import asp_lib as A
from radler_import import radler as rd

pytestmark = pytest.mark.gpu

W, H = 64, 48
F = np.float32


@pytest.fixture(scope="module")
def sess():
    s = A.Session(0)
    yield s
    s.close()


def noisy_gaussian(width, height, params, seed):
    a, x0, y0, fmaj, fmin, pa = params
    yy, xx = np.mgrid[0:height, 0:width]
    rng = np.random.RandomState(seed)
    image = a * A.gaussian(xx, yy, x0, y0, fmaj, fmin, pa) + 0.05 * rng.standard_normal(
        (height, width))
    return image.astype(F)


# ------------------------------------------------------------------ fit sums
# (image width, image height, box): under one block; clipped into a corner;
# the whole image (3 blocks); many blocks
BOXES = [(W, H, (27, 18, 10, 10)), (W, H, (27, 25, 37, 23)), (W, H, (0, 0, W, H)),
         (160, 128, (20, 0, 128, 128))]
# (pa, centre offset from the box's middle): pa 0, pa 0.7, a half-pixel centre
SHAPES = [(0.0, 0.0), (0.7, 0.0), (0.3, 0.5)]


@pytest.mark.parametrize("pa,half_pixel", SHAPES)
@pytest.mark.parametrize("width,height,box", BOXES)
def test_fit_sums_match_numpy_and_repeat_bit_for_bit(sess, width, height, box, pa, half_pixel):
    bx, by, bw, bh = box
    cx, cy = bx + bw // 2 + half_pixel, by + bh // 2 + half_pixel
    truth = (1.3, cx + 0.4, cy - 0.3, 6.5, 3.5, pa + 0.1)
    image = noisy_gaussian(width, height, truth, seed=bw * 131 + bh)
    params = (1.1, cx, cy, 5.0, 4.0, pa)
    d = sess.array(image)
    got = A.fit_sums(sess, d, width, height, box, params)
    again = A.fit_sums(sess, d, width, height, box, params)
    d.free()
    want = A.fit_sums_ref(image, box, params)
    print("fit sums: max relative error per kind",
          [float(np.abs(got[k] - want[k]).max() / np.abs(want[k]).max())
           for k in (slice(0, 21), slice(21, 27), slice(27, 28))])
    assert got.tobytes() == again.tobytes()
    # double accumulation of at most ~1.6e4 terms from identical float inputs:
    # only exp's last ulps and the summation order differ
    for kind in (slice(0, 21), slice(21, 27), slice(27, 28)):
        assert np.abs(got[kind] - want[kind]).max() <= 1e-9 * np.abs(want[kind]).max()


def test_fit_sums_reject_a_box_outside_the_image(sess):
    d = sess.array(np.zeros((H, W), F))
    for box in [(60, 0, 5, 5), (0, 44, 5, 5), (0, 0, 0, 5), (W, 0, 1, 1)]:
        with pytest.raises(A.RdlError, match="box"):
            A.fit_sums(sess, d, W, H, box, (1.0, 3.0, 3.0, 4.0, 3.0, 0.0))
    d.free()


# -------------------------------------------------------------------- render
# (x0, y0, fmaj, fmin, pa, flux): sub-pixel centre; elongated and rotated; a
# centre 3 pixels from a corner (clips); FWHM 1.2 px
RENDERS = [(30.3, 22.6, 6.0, 6.0, 0.0, 10.0), (31.5, 24.25, 14.0, 2.5, 0.9, -4.0),
           (W - 4.0, H - 4.0, 7.0, 4.0, -0.4, 3.0), (20.7, 11.2, 1.2, 1.2, 0.0, 2.0)]


@pytest.mark.parametrize("case", RENDERS)
def test_draw_gaussian_matches_numpy(sess, case):
    x0, y0, fmaj, fmin, pa, flux = case
    rng = np.random.RandomState(7)
    previous = (1e-3 * rng.standard_normal((H, W))).astype(F)
    # a guard row of sentinels above and below the plane
    guarded = np.full((H + 2, W), 12345.0, F)
    guarded[1:-1] = previous
    d = sess.array(guarded)
    A.draw_gaussian(sess, d.offset(W * 4), W, H, x0, y0, fmaj, fmin, pa, flux)
    out = d.get()
    d.free()
    assert np.all(out[0] == 12345.0) and np.all(out[-1] == 12345.0)
    got = out[1:-1]
    want = A.draw_ref(previous, x0, y0, fmaj, fmin, pa, flux)
    tolerance = 2 * np.spacing(np.abs(want)) + np.spacing(np.abs(previous))
    excess = np.abs(got.astype(np.float64) - want) - tolerance
    print("render: pixels changed", int(np.sum(got != previous)), "worst error / tolerance",
          float(np.max(np.abs(got.astype(np.float64) - want) / tolerance)))
    assert np.all(excess <= 0)
    assert np.any(got != previous)


def test_draw_gaussian_of_a_contained_ellipse_sums_to_the_flux(sess):
    d = sess.array(np.zeros((H, W), F))
    A.draw_gaussian(sess, d, W, H, 30.3, 22.6, 6.0, 4.0, 0.5, 10.0)
    total = float(np.sum(d.get().astype(np.float64)))
    d.free()
    np.testing.assert_allclose(total, 10.0, rtol=1e-5)


# ----------------------------------------------------------- weighted values
def test_weighted_values_match_numpy(sess):
    rng = np.random.RandomState(3)
    planes = rng.uniform(0.1, 1.0, (5, H, W)).astype(F)
    centres = [(0, 0), (W - 1, H - 1), (31, 24), (5, 40), (60, 3)]
    fmaj, fmin, pa = 7.0, 4.0, 0.7
    d = sess.array(planes)
    got = A.weighted_values(sess, d, 5, W, H, centres, fmaj, fmin, pa)
    again = A.weighted_values(sess, d, 5, W, H, centres, fmaj, fmin, pa)
    d.free()
    want = np.array([A.weighted_value_ref(planes[i], centres[i][0], centres[i][1], fmaj, fmin, pa)
                     for i in range(5)])
    print("weighted values: relative errors", np.abs(got - want) / np.abs(want))
    assert got.tobytes() == again.tobytes()
    np.testing.assert_allclose(got, want, rtol=1e-9)


def test_weighted_values_of_a_wide_ellipse_span_many_chunks(sess):
    # a 6 sigma box larger than the plane: every pixel, clipped on all sides
    rng = np.random.RandomState(4)
    planes = rng.uniform(0.1, 1.0, (2, H, W)).astype(F)
    centres = [(10, 12), (50, 30)]
    d = sess.array(planes)
    got = A.weighted_values(sess, d, 2, W, H, centres, 40.0, 25.0, -0.3)
    d.free()
    want = np.array([A.weighted_value_ref(planes[i], centres[i][0], centres[i][1], 40.0, 25.0,
                                          -0.3) for i in range(2)])
    np.testing.assert_allclose(got, want, rtol=1e-9)


# ------------------------------------------------------------ fit round trip
ELLIPSE = (30.3, 22.6, 9.0, 5.0, 0.5)  # x0, y0, FWHM_maj, FWHM_min, pa
FLUX = 100.0


@pytest.fixture(scope="module")
def round_trip_tolerance():
    """How far the numpy reference's own answer moves between the float64
    image and its float32 rounding, times 100 (the device and numpy share the
    rules but not exp)."""
    yy, xx = np.mgrid[0:H, 0:W]
    image64 = FLUX * A.unit_norm(ELLIPSE[2], ELLIPSE[3]) * A.gaussian(xx, yy, *ELLIPSE)
    image32 = image64.astype(F)
    start = (float(image32[23, 30]), 30.0, 23.0, 6.0, 6.0, 0.0)
    move = np.abs(np.array(A.fit_full_ref(image64, *start)) -
                  np.array(A.fit_full_ref(image32, *start))).max()
    print("round trip: the reference moves", move, "between float64 and float32; tolerance",
          100 * move)
    assert 0.0 < move < 1e-6
    return 100.0 * move


def test_fit_round_trip(sess, round_trip_tolerance):
    d = sess.array(np.zeros((H, W), F))
    A.draw_gaussian(sess, d, W, H, *ELLIPSE, FLUX)
    image = d.get()
    d.free()
    start = (float(image[23, 30]), 30.0, 23.0, 6.0, 6.0, 0.0)
    got = np.array(rd.fitters.fit_2d_gaussian_full(image, *start))
    want = np.array(A.fit_full_ref(image, *start))
    print("round trip: device", got, "numpy", want, "difference", np.abs(got - want))
    truth = np.array((FLUX * A.unit_norm(ELLIPSE[2], ELLIPSE[3]),) + ELLIPSE)
    np.testing.assert_allclose(want, truth, rtol=1e-3)
    np.testing.assert_allclose(got, truth, rtol=1e-3)
    assert np.abs(got - want).max() <= round_trip_tolerance


def test_fit_then_deconvolve_recovers_the_source_in_quadrature(round_trip_tolerance):
    n = 128
    yy, xx = np.mgrid[0:n, 0:n]
    source = 10.0 * A.unit_norm(12.0, 12.0) * A.gaussian(xx, yy, 70.0, 60.0, 12.0, 12.0, 0.0)
    psf = A.gaussian(xx, yy, n // 2, n // 2, 4.0, 4.0, 0.0)
    convolved = np.fft.irfft2(np.fft.rfft2(source) * np.fft.rfft2(np.fft.ifftshift(psf)),
                              s=(n, n)).astype(F)
    y, x = np.unravel_index(np.argmax(convolved), convolved.shape)
    fit = rd.fitters.fit_2d_gaussian_full(convolved, float(convolved[y, x]), float(x), float(y),
                                          8.0, 8.0, 0.0)
    beam = rd.fitters.fit_2d_gaussian_centred(psf.astype(F), 3.0)
    major, minor, _ = rd.fitters.deconvolve_gaussian(fit[3], fit[4], fit[5], *beam)
    print("quadrature: fit", fit, "beam", beam, "deconvolved", major, minor)
    assert abs(major - 12.0) <= round_trip_tolerance
    assert abs(minor - 12.0) <= round_trip_tolerance
