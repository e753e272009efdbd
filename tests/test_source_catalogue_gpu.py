"""radler.SourceCatalogue.draw_model and .restore on the MI355X.

The clean-beam convention is pinned to radler.restore's (csrc/host/restore.h):
a catalogue of on-pixel points restored must equal radler.restore of the
residual and the delta model, and a GAUSSIAN row with the beam's axes and
orientation must be the beam's own kernel (primitive_refs.place_gaussian).

Bounds. A restored pixel is residual + float(sum): two float roundings, as
radler.restore's contract has them (render_refs.restore_bound). The catalogue
draws every source over a 6 sigma box, outside which the beam is below
exp(-18) = 1.6e-8 of its peak: 1.6e-8 sum|S_i| covers what is cut."""
import math

import numpy as np
import pytest

import primitive_refs as P
import render_refs as R
import sources_lib as L
from radler_fixtures import BEAM_SIZE, HEIGHT, WIDTH, get_psf, get_residual, make_settings
from radler_import import radler as rd
from test_restore_gpu import BEAMS, PA

pytestmark = pytest.mark.gpu

F = np.float32
PIX = 1.0 / 3600.0 * np.pi / 180.0
W, H = 74, 58
RA0, DEC0 = 0.3, 0.4
NU = [1.5e8]
CUT = 1.6e-8  # exp(-18)


def write_catalogue(path, rows, header="Format = Name, Type, Ra, Dec, I, MajorAxis, MinorAxis, "
                                       "Orientation"):
    """rows: (type, ra, dec, flux, major, minor, orientation); the angles in
    radians are printed to 1 ms / 1 mas, so on-pixel sources are on-pixel to
    1e-2 of a 1 arcsec pixel only: tests that need more place their sources
    with geometry_of_exact_offsets."""
    with open(path, "w") as f:
        f.write(header + "\n")
        for i, (kind, ra, dec, flux, major, minor, orientation) in enumerate(rows):
            f.write(f"s{i}, {kind}, {L.format_ra(ra)}, {L.format_dec(dec)}, {flux!r}, "
                    f"{major!r}, {minor!r}, {orientation!r}\n")
    return rd.SourceCatalogue.read(path)


def geometry_of_exact_offsets(scale_x, scale_y):
    """A phase centre at (0, 0) and pixel scales that are whole milliseconds of
    RA and milliarcseconds of Dec near the requested ones: at dec 0 a source on
    the equator k pixels from the centre has ra = asin(k scale_x), and one on
    the meridian dec = asin(k scale_y). For offsets of up to 12 pixels of
    1.5 arcsec asin(v) - v = v^3 / 6 < 1.2e-13 rad, under 2e-8 pixels."""
    ms, mas = math.pi / 12.0 / 3600e3, math.pi / 180.0 / 3600e3
    return round(scale_x / ms) * ms, round(scale_y / mas) * mas


def beam_of(name):
    major, minor, ratio = BEAMS[name]
    return major * PIX, minor * PIX, PA, PIX, ratio * PIX


# ------------------------------------------------------------------- 3a
@pytest.mark.parametrize("beam", ["3x2", "3x2_tall_pixels"])
def test_on_pixel_points_are_the_delta_model_and_restore_as_radler_restore(tmp_path, beam):
    major, minor, pa, scale_x, scale_y = beam_of(beam)
    # sources on the row and the column through the phase centre, where the
    # printed coordinates are exact: see geometry_of_exact_offsets
    scale_x, scale_y = geometry_of_exact_offsets(scale_x, scale_y)
    rng = np.random.default_rng(4)
    model = np.zeros((H, W), F)
    cx, cy = W // 2, H // 2
    spots = [(cx, cy), (cx - 12, cy), (cx + 11, cy), (cx + 3, cy), (cx, cy - 12), (cx, cy + 10),
             (cx, cy + 2), (cx - 1, cy)]
    rows = []
    for k, (x, y) in enumerate(spots):
        flux = float(F(rng.uniform(0.05, 0.9) * (-1.0 if k % 3 == 2 else 1.0)))
        model[y, x] = flux
        ra = math.asin((cx - x) * scale_x)
        dec = math.asin((y - cy) * scale_y)
        rows.append(("POINT", ra, dec, flux, 0.0, 0.0, 0.0))
    cat = write_catalogue(str(tmp_path / "points.txt"), rows)
    xy = cat.pixel_positions(W, H, scale_x, scale_y, 0.0, 0.0)
    offset = float(np.max(np.abs(xy - np.asarray(spots))))
    print(f"largest distance of a source from its pixel centre: {offset:.3g} pixels")
    assert offset < 2e-8

    drawn = cat.draw_model(W, H, scale_x, scale_y, 0.0, 0.0, NU)
    assert drawn.shape == (1, H, W) and drawn.dtype == F
    assert np.array_equal(drawn[0], model)

    residual = (1e-4 * rng.standard_normal((H, W))).astype(F)
    kept = residual.copy()
    want = rd.restore(residual, model, major, minor, pa, scale_x, scale_y)
    got = cat.restore(residual, scale_x, scale_y, 0.0, 0.0, NU, major, minor, pa)
    assert np.array_equal(residual, kept) and got.shape == (H, W) and got.dtype == F
    kernel, _ = R.beam_kernel(W, H, major, minor, pa, scale_x, scale_y)
    conv = R.linear_convolve(model, kernel)
    bound = R.restore_bound(residual, conv, model) + CUT * float(np.sum(np.abs(model)))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"restore {beam}: max |catalogue - radler.restore| = {np.max(err):.3g}, max error / "
          f"bound = {np.max(err / bound):.3g}, peak {np.max(np.abs(want)):.3g}")
    assert np.all(err <= bound)
    assert float(np.max(np.abs(got - residual))) > 0.5


# ------------------------------------------------------------------- 3b
@pytest.mark.parametrize("beam", ["3x2", "3x2_tall_pixels"])
def test_a_sub_pixel_point_restores_to_the_beam_at_its_centre(tmp_path, beam):
    major, minor, pa, scale_x, scale_y = beam_of(beam)
    x0, y0, flux = 40 + 0.3, 21 - 0.4, 1.75
    ra, dec = L.xy_to_radec(x0, y0, W, H, scale_x, scale_y, RA0, DEC0)
    cat = write_catalogue(str(tmp_path / "point.txt"), [("POINT", ra, dec, flux, 0.0, 0.0, 0.0)])
    # the centre the catalogue holds, after the 1 ms / 1 mas print
    (x0, y0), = cat.pixel_positions(W, H, scale_x, scale_y, RA0, DEC0)
    assert abs(x0 - 40.3) < 0.02 and abs(y0 - 20.6) < 0.02
    rng = np.random.default_rng(6)
    residual = (1e-4 * rng.standard_normal((H, W))).astype(F)
    got = cat.restore(residual, scale_x, scale_y, RA0, DEC0, NU, major, minor, pa)
    cov = L.pixel_covariance(major, minor, pa, scale_x, scale_y)
    beam_image = flux * L.gaussian_of(cov, x0, y0, W, H)
    half = L.shape_of(cov, x0, y0, W, H)[5]
    yy, xx = np.mgrid[0:H, 0:W]
    inside = (np.abs(xx - math.floor(x0 + 0.5)) <= half) & (np.abs(yy - math.floor(y0 + 0.5)) <= half)
    assert np.all(beam_image[~inside] <= CUT * flux)
    want = residual.astype(np.float64) + np.where(inside, beam_image, 0.0)
    # the quadratic form in double: a few 1e-16 of an exponent of at most 18 or so
    bound = 2.0 ** -24 * (np.abs(want) + np.abs(beam_image)) + 1e-12 * beam_image
    err = np.abs(got.astype(np.float64) - want)
    print(f"sub-pixel point, {beam}: max error / bound = {np.max(err / bound):.3g}")
    assert np.all(err <= bound)
    assert np.array_equal(got[~inside], residual[~inside])
    # the brightest pixel is one of the four around the centre, and below the
    # flux: the centre is off the grid
    py, px = np.unravel_index(np.argmax(got), got.shape)
    assert (py, px) == np.unravel_index(np.argmax(want), want.shape)
    assert py in (20, 21) and px in (40, 41)
    assert 0.7 * flux < got[py, px] < 0.995 * flux


# ------------------------------------------------------------------- 3c
@pytest.mark.parametrize("beam", ["3x2", "3x2_tall_pixels"])
def test_a_gaussian_row_with_the_beams_shape_is_the_beam_kernel(tmp_path, beam):
    major, minor, pa, scale_x, scale_y = beam_of(beam)
    scale_x, scale_y = geometry_of_exact_offsets(scale_x, scale_y)
    cx, cy, flux = W // 2, H // 2, 2.5
    rows = [("GAUSSIAN", 0.0, 0.0, flux, major / L.ARCSEC, minor / L.ARCSEC, math.degrees(pa))]
    cat = write_catalogue(str(tmp_path / "gaussian.txt"), rows)
    drawn = cat.draw_model(W, H, scale_x, scale_y, 0.0, 0.0, NU)[0]
    cov = L.pixel_covariance(major, minor, pa, scale_x, scale_y)
    half = L.shape_of(cov, cx, cy, W, H)[5]
    box = 2 * half + 2
    assert box <= min(W, H)
    to_sigma = L.FWHM_TO_SIGMA
    placed, _ = P.place_gaussian(W, H, box, scale_x, scale_y, major * to_sigma, minor * to_sigma,
                                 pa + 0.5 * math.pi)
    kernel = np.roll(placed, (cy, cx), axis=(0, 1))  # its centre on the source's pixel
    yy, xx = np.mgrid[0:H, 0:W]
    inside = (np.abs(xx - cx) <= half) & (np.abs(yy - cy) <= half)
    norm = flux / (2.0 * math.pi * math.sqrt(np.linalg.det(cov)))
    want = np.where(inside, norm * kernel, 0.0)
    # the amplitude is rounded to float, then the pixel
    bound = 2.0 ** -23 * np.abs(want) + 1e-12 * norm
    err = np.abs(drawn.astype(np.float64) - want)
    print(f"gaussian row against the beam kernel, {beam}: max error / bound = "
          f"{np.max(err[inside] / bound[inside]):.3g}, integral {float(np.sum(drawn)):.6g}")
    assert np.all(err <= bound)
    # unit integral x S: sampling a Gaussian of sigma >= 0.55 pixels aliases by
    # 2 exp(-2 pi^2 sigma^2) = 5e-3 at most
    assert abs(float(np.sum(drawn, dtype=np.float64)) - flux) < 1e-2 * flux
    assert np.max(kernel) == 1.0 and kernel[cy, cx] == 1.0


@pytest.mark.parametrize("beam", ["3x2", "3x2_tall_pixels"])
def test_a_gaussian_source_restores_to_the_sum_of_the_covariances(tmp_path, beam):
    major, minor, pa, scale_x, scale_y = beam_of(beam)
    x0, y0, flux = 30 + 0.25, 33 - 0.35, 1.5
    source = (4.0 * PIX, 2.5 * PIX, math.radians(-50.0))
    ra, dec = L.xy_to_radec(x0, y0, W, H, scale_x, scale_y, RA0, DEC0)
    rows = [("GAUSSIAN", ra, dec, flux, source[0] / L.ARCSEC, source[1] / L.ARCSEC,
             math.degrees(source[2]))]
    cat = write_catalogue(str(tmp_path / "gaussian.txt"), rows)
    (x0, y0), = cat.pixel_positions(W, H, scale_x, scale_y, RA0, DEC0)
    rng = np.random.default_rng(9)
    residual = (1e-4 * rng.standard_normal((H, W))).astype(F)
    got = cat.restore(residual, scale_x, scale_y, RA0, DEC0, NU, major, minor, pa)
    cov_beam = L.pixel_covariance(major, minor, pa, scale_x, scale_y)
    cov = L.pixel_covariance(*source, scale_x, scale_y) + cov_beam
    peak = flux * math.sqrt(np.linalg.det(cov_beam) / np.linalg.det(cov))
    image = peak * L.gaussian_of(cov, x0, y0, W, H)
    half = L.shape_of(cov, x0, y0, W, H)[5]
    yy, xx = np.mgrid[0:H, 0:W]
    inside = (np.abs(xx - math.floor(x0 + 0.5)) <= half) & (np.abs(yy - math.floor(y0 + 0.5)) <= half)
    assert np.all(image[~inside] <= CUT * peak)
    want = residual.astype(np.float64) + np.where(inside, image, 0.0)
    # the amplitude is rounded to float, then the sum, then the addition
    bound = 2.0 ** -24 * (np.abs(want) + 2.0 * np.abs(image)) + 1e-12 * image
    err = np.abs(got.astype(np.float64) - want)
    print(f"gaussian source restored, {beam}: max error / bound = {np.max(err / bound):.3g}, "
          f"peak {peak:.4g} of flux {flux}")
    assert np.all(err <= bound)
    assert 0.15 * flux < peak < 0.7 * flux


# ------------------------------------------------------------------- 3d
def test_a_radler_run_written_read_drawn_and_restored(tmp_path):
    """The smallest two-channel clean: the point source of radler_fixtures at
    the phase centre, whose printed coordinates (all zeros) are exact; a source
    elsewhere is printed to 1 ms of RA (15 mas), up to 1e-4 of these 1 arcmin
    pixels, which changes a restored beam by about 1e-4 of its peak, far above
    the float roundings that the restore bound allows.

    The catalogue holds the fitted terms to 7 digits, so a restored image
    agrees with radler.restore of ComponentList.render_model's planes to float
    rounding only where the terms print exactly. Three components at gain 1/2
    of channel fluxes 2 and 1 sum to 1.75 and 0.875; with the reference
    frequency midway between the channels the two polynomial terms are 1.3125
    and -5.25, which 7 digits hold. (Six such components, 1.96875 and
    0.984375, give the term 1.4765625: the file then differs by 2.4e-7 of the
    peak, inside the 1e-6 of draw_model but 2.5 to 3.8 x the restore bound.)
    restore is also compared with radler.restore of the model the catalogue
    itself draws: the two differ in how the beam is applied and nothing else."""
    s = make_settings()
    s.save_source_list = True
    s.minor_iteration_count = 3
    s.minor_loop_gain = 0.5
    s.spectral_fitting.mode = rd.SpectralFittingMode.polynomial
    s.spectral_fitting.terms = 2
    residuals = np.stack([get_residual(2.0, 0, 0), get_residual(1.0, 0, 0)])
    psfs, models = np.stack([get_psf()] * 2), np.zeros_like(residuals)
    freqs = np.array([[1.0e8, 1.2e8], [1.2e8, 1.4e8]])
    r = rd.Radler(s, psfs, residuals, models, BEAM_SIZE, 2, freqs, np.array([1.0, 1.0]))
    r.perform(0)
    cl = r.component_list
    assert cl.n_scales == 1 and cl.component_count(0) >= 1
    path = str(tmp_path / "sources.txt")
    scale = s.pixel_scale.x
    cl.write_sources(r, path, scale, scale, 0.0, 0.0)
    cat = rd.SourceCatalogue.read(path)
    assert len(cat) == cl.component_count(0) and set(cat.types) == {"POINT"}
    nus = list(r.spectral_fitter.frequencies)
    assert len(nus) == 2
    print(f"terms read: {[float(v) for v in cat.flux]} {[t.tolist() for t in cat.terms]}, the "
          f"list's values {cl.get_component(0, 0)[2]}, reference {cat.reference_frequency:g} Hz")

    want = cl.render_model(r, nus)
    got = cat.draw_model(WIDTH, HEIGHT, scale, scale, 0.0, 0.0, nus)
    assert got.shape == want.shape == (2, HEIGHT, WIDTH)
    peak = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))))
    print(f"draw_model against render_model: max |difference| = {err:.3g}, bound "
          f"{1e-6 * peak:.3g}, {len(cat)} sources, peak {peak:.4g}")
    assert peak > 0.5 and err <= 1e-6 * peak
    assert np.array_equal(np.nonzero(got), np.nonzero(want))

    beam = (3.0 * scale, 2.0 * scale, PA)
    restored = cat.restore(residuals, scale, scale, 0.0, 0.0, nus, *beam)
    assert restored.shape == (2, HEIGHT, WIDTH)
    kernel, _ = R.beam_kernel(WIDTH, HEIGHT, *beam, scale, scale)
    for name, model in (("render_model's planes", want), ("the drawn model", got)):
        restored_want = rd.restore(residuals, model, *beam, scale, scale)
        for g in range(2):
            conv = R.linear_convolve(model[g], kernel)
            bound = R.restore_bound(residuals[g], conv, model[g]) + \
                CUT * float(np.sum(np.abs(model[g])))
            e = np.abs(restored[g].astype(np.float64) - restored_want[g].astype(np.float64))
            print(f"restore against radler.restore of {name}, channel {g}: max error / bound = "
                  f"{np.max(e / bound):.3g}, peak {np.max(np.abs(restored_want[g])):.4g}")
            assert np.all(e <= bound)
    assert float(np.max(np.abs(restored - residuals))) > 0.5
