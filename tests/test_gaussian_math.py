"""rd.fitters.deconvolve_gaussian (csrc/host/gaussian_fit.h: the closed-form
deconvolution of one elliptical Gaussian from another, a pure host function)
and the Python surface of the adaptive-scale-pixel algorithm. No GPU."""
import numpy as np
import pytest

from asp_lib import deconvolve_ref
from radler_import import radler as rd


@pytest.mark.parametrize("fit,psf", [((12.0, 7.0), (4.0, 3.0)), ((6.0, 5.0), (3.0, 2.9)),
                                     ((30.0, 2.5), (2.0, 2.0))])
@pytest.mark.parametrize("pa", [0.0, 0.7, -1.2])
def test_aligned_ellipses_subtract_in_quadrature(fit, psf, pa):
    major, minor, angle = rd.fitters.deconvolve_gaussian(fit[0], fit[1], pa, psf[0], psf[1], pa)
    np.testing.assert_allclose(major ** 2, fit[0] ** 2 - psf[0] ** 2, rtol=1e-12)
    np.testing.assert_allclose(minor ** 2, fit[1] ** 2 - psf[1] ** 2, rtol=1e-12)
    if pa == 0.0:
        assert angle == 0.0
    else:
        # the same axis (angles are equal modulo pi)
        assert abs(np.sin(angle - pa)) < 1e-9


@pytest.mark.parametrize("case", [(12.0, 7.0, 0.3, 4.0, 3.0, -0.9), (9.0, 5.0, 0.5, 4.0, 4.0, 0.0),
                                  (6.0, 5.5, -1.1, 5.0, 2.0, 1.3)])
def test_rotated_case_matches_second_moment_subtraction(case):
    got = rd.fitters.deconvolve_gaussian(*case)
    want = deconvolve_ref(*case)
    np.testing.assert_allclose(got[0], want[0], rtol=1e-12)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-12)
    assert abs(np.sin(got[2] - want[2])) < 1e-9
    assert got[0] >= got[1] > 0.0
    assert -np.pi / 2 <= got[2] <= np.pi / 2


def test_equal_ellipses_give_a_non_finite_major_axis():
    major, _, _ = rd.fitters.deconvolve_gaussian(6.0, 4.0, 0.4, 6.0, 4.0, 0.4)
    assert not np.isfinite(major)


@pytest.mark.parametrize("case", [(3.0, 2.0, 0.0, 4.0, 3.0, 0.0),   # smaller everywhere
                                  (8.0, 2.0, 0.0, 4.0, 3.0, 0.0),   # narrower along the minor axis
                                  (6.0, 4.0, 0.0, 6.0, 4.0, 1.0)])  # the same ellipse, turned
def test_a_smaller_ellipse_gives_a_non_finite_major_axis(case):
    major, _, _ = rd.fitters.deconvolve_gaussian(*case)
    assert not np.isfinite(major)


def test_algorithm_type_has_adaptive_scale_pixel():
    assert hasattr(rd.AlgorithmType, "adaptive_scale_pixel")
    s = rd.Settings()
    s.algorithm_type = rd.AlgorithmType.adaptive_scale_pixel
    assert s.algorithm_type == rd.AlgorithmType.adaptive_scale_pixel


def test_numpy_fit_reference_recovers_a_noiseless_ellipse():
    """The reference driver of tests/asp_lib.py (the product's rules in numpy
    float64) on its own: it recovers the ellipse the GPU round-trip test uses
    to far better than that test's 1e-3."""
    from asp_lib import draw_ref, fit_full_ref
    image = draw_ref(np.zeros((48, 64), np.float32), 30.3, 22.6, 9.0, 5.0, 0.5, 100.0)
    fit = fit_full_ref(image, float(image[23, 30]), 30.0, 23.0, 6.0, 6.0, 0.0)
    np.testing.assert_allclose(fit[1:], (30.3, 22.6, 9.0, 5.0, 0.5), rtol=1e-5)
