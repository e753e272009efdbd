"""The adaptive-scale-pixel algorithm (csrc/host/asp_algorithm.{h,cc};
reference cpp/algorithms/asp_algorithm.cc) through Radler.perform on the
MI355X: the reference's point-source known-answer test (cpp/test/
test_radler.cc:106-172 lists kAdaptiveScalePixel among its algorithms), an
extended source, two joined channels and a gridded run."""
import numpy as np
import pytest

import asp_lib as A
from radler_fixtures import (BEAM_SIZE, HEIGHT, MINOR_ITERATION_COUNT, PIXEL_SCALE, WIDTH,
                             get_psf, get_residual, make_settings)
from radler_import import radler as rd

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.mark.parametrize("shift", [(0, 0), (7, -11), (-9, 15)])
def test_point_source(shift):
    settings = make_settings()
    settings.algorithm_type = rd.AlgorithmType.adaptive_scale_pixel
    psf, residual = get_psf(), get_residual(2.5, *shift)
    model = np.zeros_like(residual)
    r = rd.Radler(settings, psf, residual, model, BEAM_SIZE, rd.Polarization.stokes_i)
    assert r.perform(0) is False
    assert r.iteration_number <= MINOR_ITERATION_COUNT
    source = (HEIGHT // 2 + shift[1], WIDTH // 2 + shift[0])
    print("point source: iterations", r.iteration_number, "max |residual|",
          float(np.abs(residual).max()), "model at the source", float(model[source]))
    assert np.abs(residual).max() < 2e-6
    np.testing.assert_allclose(model[source], 2.5, rtol=1e-6)  # BOOST_CHECK_CLOSE 1e-4 %
    elsewhere = model.copy()
    elsewhere[source] = 0.0
    assert np.abs(elsewhere).max() < 2e-6


# ------------------------------------------------------------ extended source
N = 128
PSF_FWHM = 4.0
GAIN = 0.1
ITERATION_CAP = 300


@pytest.fixture(scope="module")
def extended():
    """PSF (peak 1) and dirty image in numpy float64: a Gaussian of FWHM 12 px
    and flux 10 at (70, 60) plus a point of flux 1 at (30, 90), convolved with
    the PSF. Shared; the tests copy what they change."""
    yy, xx = np.mgrid[0:N, 0:N]
    psf = A.gaussian(xx, yy, N // 2, N // 2, PSF_FWHM, PSF_FWHM, 0.0)
    sky = 10.0 * A.unit_norm(12.0, 12.0) * A.gaussian(xx, yy, 70.0, 60.0, 12.0, 12.0, 0.0)
    sky[90, 30] += 1.0
    dirty = np.fft.irfft2(np.fft.rfft2(sky) * np.fft.rfft2(np.fft.ifftshift(psf)), s=(N, N))
    return psf.astype(F), dirty.astype(F)


def asp_settings(threshold, grid=1):
    s = rd.Settings()
    s.algorithm_type = rd.AlgorithmType.adaptive_scale_pixel
    s.trimmed_image_width = s.trimmed_image_height = N
    s.pixel_scale.x = s.pixel_scale.y = PIXEL_SCALE
    s.minor_iteration_count = ITERATION_CAP
    s.minor_loop_gain = GAIN
    s.absolute_threshold = threshold
    s.parallel.grid_width = s.parallel.grid_height = grid
    return s


def flux_identity_error(dirty, residual, model, psf):
    """|sum residual - (sum dirty - sum model * sum psf)|: zero for any
    implementation that subtracts what it adds."""
    d, r, m, p = (float(np.sum(a.astype(np.float64))) for a in (dirty, residual, model, psf))
    return abs(r - (d - m * p)), d


def test_extended_source(extended):
    psf, dirty = extended
    residual, model = dirty.copy(), np.zeros_like(dirty)
    threshold = 0.05 * float(dirty.max())
    r = rd.Radler(asp_settings(threshold), psf, residual, model, PSF_FWHM * PIXEL_SCALE,
                  rd.Polarization.stokes_i)
    r.perform(0)
    error, total = flux_identity_error(dirty, residual, model, psf)
    print("extended: iterations", r.iteration_number, "residual peak",
          float(np.abs(residual).max()), "threshold", threshold, "model flux",
          float(model.sum()), "identity error / sum dirty", error / total)
    assert 0 < r.iteration_number < ITERATION_CAP
    assert np.abs(residual).max() <= threshold
    # float rounding over ~30 components of 16 k pixels is bounded near 2e-6
    # relative; the margin is 50x that bound
    assert error <= 1e-4 * total


def test_two_joined_channels(extended):
    psf, dirty = extended
    amplitudes = (1.0, 0.6)
    dirties = [(a * dirty).astype(F) for a in amplitudes]
    residuals = [d.copy() for d in dirties]
    models = [np.zeros_like(dirty) for _ in amplitudes]
    s = asp_settings(0.05 * float(np.mean(amplitudes)) * float(dirty.max()))
    s.spectral_fitting.mode = rd.SpectralFittingMode.polynomial
    s.spectral_fitting.terms = 2
    t = rd.WorkTable([], 2, 2)
    for i in range(2):
        e = rd.WorkTableEntry()
        e.psfs.append(psf)
        e.residual = residuals[i]
        e.model = models[i]
        e.original_channel_index = i
        e.index = i
        e.band_start_frequency = 100e6 + 10e6 * i
        e.band_end_frequency = 110e6 + 10e6 * i
        e.image_weight = 1.0
        e.polarization = rd.Polarization.stokes_i
        t.add_entry(e)
    r = rd.Radler(s, t, PSF_FWHM * PIXEL_SCALE)
    r.perform(0)
    assert 0 < r.iteration_number < ITERATION_CAP
    for i in range(2):
        error, total = flux_identity_error(dirties[i], residuals[i], models[i], psf)
        print("joined: channel", i, "iterations", r.iteration_number, "residual peak",
              float(np.abs(residuals[i]).max()), "model flux", float(models[i].sum()),
              "identity error / sum dirty", error / total)
        assert error <= 1e-4 * total
        assert np.abs(residuals[i]).max() < np.abs(dirties[i]).max()


def test_gridded_run(extended):
    psf, dirty = extended
    residual, model = dirty.copy(), np.zeros_like(dirty)
    r = rd.Radler(asp_settings(0.05 * float(dirty.max()), grid=2), psf, residual, model,
                  PSF_FWHM * PIXEL_SCALE, rd.Polarization.stokes_i)
    r.perform(0)
    print("gridded: iterations", r.iteration_number, "residual peak",
          float(np.abs(residual).max()), "start peak", float(np.abs(dirty).max()))
    assert np.all(np.isfinite(residual)) and np.all(np.isfinite(model))
    assert np.abs(residual).max() < np.abs(dirty).max()
