"""ComponentList.write_sources on the MI355X: the source catalogue of a
Radler run (the reference's ComponentList::WriteSources), and the batched
device fit of ComponentList.write against its host path: the two files may
differ in the fitted terms only, within the tolerance of the fit
(tests/test_component_terms_gpu.py) after the 7-digit print."""
import math

import numpy as np
import pytest

from fits_helper import write_fits
from radler_fixtures import BEAM_SIZE, HEIGHT, WIDTH, get_psf, make_settings
from radler_import import radler as rd
from synthetic import make_dirty, make_psf, make_sky
from test_write_sources import read_rows

pytestmark = pytest.mark.gpu

MODE = rd.SpectralFittingMode
PIXEL_SCALE = 1.0 / 3600.0 * np.pi / 180.0


@pytest.mark.parametrize("lm_shift_given", [True, False])
def test_write_component_list(tmp_path, lm_shift_given):
    """python/test/test_radler.py:285-346: a flat residual takes every one of
    42 iterations on a pixel of its own; the file has a header and 42 rows."""
    settings = make_settings()
    settings.save_source_list = True
    settings.minor_iteration_count = 42
    settings.algorithm_type = rd.AlgorithmType.generic_clean
    residual = np.ones((HEIGHT, WIDTH), np.float32)
    model = np.zeros_like(residual)
    psf = get_psf()  # the Radler works on these arrays: they stay alive
    r = rd.Radler(settings, psf, residual, model, BEAM_SIZE, rd.Polarization.stokes_i)
    assert r.perform(0) is False
    assert r.iteration_number <= 42
    cl = r.component_list
    assert cl.n_scales == 1
    assert cl.component_count(0) == 42
    path = str(tmp_path / "test_write_sources.txt")
    if lm_shift_given:
        cl.write_sources(r, path, settings.pixel_scale.x, settings.pixel_scale.y, 0.3, 0.4,
                         0.0, 0.0)
    else:
        cl.write_sources(r, path, settings.pixel_scale.x, settings.pixel_scale.y, 0.3, 0.4)
    with open(path) as f:
        assert len(f.readlines()) == 43
    _, rows = read_rows(path)
    assert [row["name"] for row in rows] == [f"s0c{i}" for i in range(42)]
    assert all(row["type"] == "POINT" and row["si_text"] == "" for row in rows)


def joined_multiscale(mode, terms, grid=(1, 1), w=64, forced_filename=None):
    """A small joined cube (3 channels, two blobs) cleaned with multiscale."""
    n_ch = 3
    # three points and two blobs a few pixels wide: components of several scales
    psf = make_psf(w, w)
    sky = make_sky(w, w, 3, 0, seed=21) + \
        make_sky(w, w, 0, 2, seed=22, flux_range=(0.5, 1.0), blob_sigma=(3.0, 5.0))
    dirty = make_dirty(psf, sky, 1e-3, seed=21)
    rng = np.random.default_rng(21)
    dirties = np.stack([dirty * np.float32(1.0 + 0.15 * k) + np.float32(1e-3) *
                        rng.standard_normal((w, w)).astype(np.float32)
                        for k in range(n_ch)]).astype(np.float32)
    psfs, models = np.stack([psf] * n_ch), np.zeros_like(dirties)
    s = rd.Settings()
    s.algorithm_type = rd.AlgorithmType.multiscale
    s.trimmed_image_width = s.trimmed_image_height = w
    s.pixel_scale.x = s.pixel_scale.y = PIXEL_SCALE
    s.minor_iteration_count = 300
    s.absolute_threshold = 8e-3
    s.border_ratio = 0.0
    s.save_source_list = True
    s.multiscale.max_scales = 3
    s.parallel.grid_width, s.parallel.grid_height = grid
    s.parallel.max_threads = 1
    s.spectral_fitting.mode = mode
    s.spectral_fitting.terms = terms
    if forced_filename is not None:
        s.spectral_fitting.forced_filename = forced_filename
    freqs = np.array([[1.0e8 + 2e7 * k, 1.2e8 + 2e7 * k] for k in range(n_ch)])
    r = rd.Radler(s, psfs, dirties, models, 2.0 * PIXEL_SCALE, n_ch, freqs,
                  np.array([1.0, 2.0, 1.5]))
    r.perform(0)
    return s, r, (psfs, dirties, models)  # the arrays the Radler works on stay alive


def lines_without_terms(path):
    """Every row with its terms cut out, and the terms."""
    header, rows = read_rows(path)
    rest = [[row[k] for k in ("name", "type", "ra", "dec", "log_si", "ref", "major", "minor",
                              "orientation")] for row in rows]
    return header, rest, np.asarray([row["terms"] for row in rows], np.float64)


@pytest.mark.parametrize("mode,terms", [(MODE.polynomial, 2), (MODE.log_polynomial, 2)])
def test_multiscale_catalogue_device_fit_matches_host_fit(tmp_path, mode, terms):
    s, r, _keep = joined_multiscale(mode, terms)
    cl = r.component_list
    n = sum(cl.component_count(i) for i in range(cl.n_scales))
    assert n > 10
    fitter, scale_sizes = r.spectral_fitter, r.scale_sizes
    assert fitter.mode == mode and len(fitter.frequencies) == 3
    paths = [str(tmp_path / name) for name in ("sources.txt", "host.txt", "device.txt")]
    cl.write_sources(r, paths[0], PIXEL_SCALE, PIXEL_SCALE, 0.3, 0.4)
    cl.write(paths[1], fitter, scale_sizes, PIXEL_SCALE, PIXEL_SCALE, 0.3, 0.4)
    cl.write(paths[2], fitter, scale_sizes, PIXEL_SCALE, PIXEL_SCALE, 0.3, 0.4, device=True)
    header, rest, host_terms = lines_without_terms(paths[1])
    assert len(rest) == n

    # at least one GAUSSIAN row, with the axes of its scale
    to_arcsec = 180.0 * 3600.0 / math.pi
    gaussians = [row for row in rest if row[1] == "GAUSSIAN"]
    assert gaussians
    for row in rest:
        scale = scale_sizes[int(row[0][1:row[0].index("c")])]
        assert (row[1] == "GAUSSIAN") == (scale != 0.0)
        if scale != 0.0:
            fwhm = 2.0 * math.sqrt(2.0 * math.log(2.0)) * scale * 3.0 / 16.0
            np.testing.assert_allclose([float(row[6]), float(row[7])],
                                       fwhm * PIXEL_SCALE * to_arcsec, rtol=1e-6)
            assert row[8] == "0"
        else:
            assert row[6:] == ["", "", ""]

    log_si = "true" if mode == MODE.log_polynomial else "false"
    assert all(row[4] == log_si for row in rest)
    for path in (paths[0], paths[2]):
        other_header, other_rest, other_terms = lines_without_terms(path)
        assert other_header == header
        assert other_rest == rest  # byte-identical apart from the terms
        assert other_terms.shape == host_terms.shape == (n, terms)
        if mode == MODE.polynomial:
            # one float rounding of a double sum (2^-23), then the 7-digit print
            np.testing.assert_allclose(other_terms, host_terms, rtol=1e-6)
        else:
            atol = 2e-5 * max(1.0, float(np.max(np.abs(host_terms))))
            np.testing.assert_allclose(other_terms, host_terms, rtol=2e-5, atol=atol)


def test_tiled_run_writes_one_catalogue(tmp_path):
    s, r, _keep = joined_multiscale(MODE.polynomial, 2, grid=(2, 2), w=96)
    cl = r.component_list
    n = sum(cl.component_count(i) for i in range(cl.n_scales))
    assert n > 10
    path = str(tmp_path / "sources.txt")
    cl.write_sources(r, path, PIXEL_SCALE, PIXEL_SCALE, 0.3, 0.4)
    with open(path) as f:
        assert len(f.readlines()) == n + 1
    _, rows = read_rows(path)
    for i in range(cl.n_scales):
        assert [row["name"] for row in rows if row["name"].startswith(f"s{i}c")] == \
            [f"s{i}c{k}" for k in range(cl.component_count(i))]


def test_forced_terms_catalogue(tmp_path):
    """A Radler in forced-terms mode keeps the term planes in its algorithm,
    not in its fitter: write_sources takes them from there. Against write
    with a fitter that holds the same plane, host and device path: t_1 is the
    plane's value at the component, t_0 within 2 float ulps and the print."""
    w = 64
    yy, xx = np.mgrid[0:w, 0:w].astype(np.float64)
    t1 = (-1.0 + 0.01 * xx + 0.02 * yy).astype(np.float32)
    cube = str(tmp_path / "terms.fits")
    write_fits(cube, t1[None])
    s, r, _keep = joined_multiscale(MODE.forced_terms, 2, forced_filename=cube)
    cl = r.component_list
    n = sum(cl.component_count(i) for i in range(cl.n_scales))
    assert n > 10
    fitter, scale_sizes = r.spectral_fitter, r.scale_sizes
    assert fitter.mode == MODE.forced_terms
    fitter.set_forced_terms([t1])
    paths = [str(tmp_path / name) for name in ("sources.txt", "host.txt", "device.txt")]
    cl.write_sources(r, paths[0], PIXEL_SCALE, PIXEL_SCALE, 0.3, 0.4)
    cl.write(paths[1], fitter, scale_sizes, PIXEL_SCALE, PIXEL_SCALE, 0.3, 0.4)
    cl.write(paths[2], fitter, scale_sizes, PIXEL_SCALE, PIXEL_SCALE, 0.3, 0.4, device=True)
    header, rest, host_terms = lines_without_terms(paths[1])
    assert len(rest) == n and all(row[4] == "true" for row in rest)
    positions = [p for i in range(cl.n_scales) for p in cl.get_positions(i)]
    plane = np.asarray([t1[y, x] for x, y in positions], np.float64)
    for path in paths:
        other_header, other_rest, other_terms = lines_without_terms(path)
        assert other_header == header and other_rest == rest
        assert other_terms.shape == (n, 2)
        np.testing.assert_allclose(other_terms[:, 1], plane, rtol=1e-6)
        np.testing.assert_allclose(other_terms[:, 0], host_terms[:, 0], rtol=1e-6)
