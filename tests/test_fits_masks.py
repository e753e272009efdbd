"""FITS input and output of Radler (csrc/host/fits_image.cc, radler.cc
ReadMask / ReadForcedSpectrumImages / the local-RMS image; reference:
cpp/radler.cc:189-195, 410-527).

CPU: the reader against files written with numpy (2 to 4 axes, BITPIX -32,
-64 and 16 with BSCALE / BZERO, malformed files); Radler's construction-time
checks (mask size, term-cube plane count) with the reference's messages; the
horizon mask file against its definition, exactly.
GPU: a FITS clean mask keeps the model inside the mask; a local-RMS image
file steers the first component.
"""
import numpy as np
import pytest

from fits_helper import BLOCK, card, fits_bytes, header_bytes, write_fits
from radler_import import radler as rd


# ------------------------------------------------------------------ reader
@pytest.mark.parametrize("shape,bitpix,ctypes,n_freq,scaling", [
    ((5, 7), -32, None, 1, {}),
    ((2, 5, 7), -32, None, 1, {}),
    ((1, 3, 6, 9), -32, ["RA---SIN", "DEC--SIN", "FREQ", "STOKES"], 3, {}),
    ((3, 1, 6, 9), -64, ["RA---SIN", "DEC--SIN", "STOKES", "FREQ-LSR"], 3, {}),
    ((2, 5, 7), -64, None, 1, {}),
    ((2, 5, 7), 16, None, 1, dict(bscale=0.25, bzero=100.0)),
    ((4, 3), 16, None, 1, dict(bscale=2.0)),
])
def test_reader_round_trip(tmp_path, shape, bitpix, ctypes, n_freq, scaling):
    rng = np.random.default_rng(len(shape) * 10 + abs(bitpix))
    data = rng.standard_normal(shape) * 50.0
    if bitpix == -32:
        data = data.astype(np.float32)
    path = str(tmp_path / "image.fits")
    expect = write_fits(path, data, bitpix=bitpix, ctypes=ctypes, **scaling)
    planes, n_images, n_frequencies = rd.io.read_fits(path)
    assert n_images == int(np.prod(shape[:-2])) == planes.shape[0]
    assert n_frequencies == n_freq
    assert planes.dtype == np.float32
    # pixel (x, y) of plane k is element [k, y, x]: file order, no flip
    assert np.array_equal(planes, expect)
    for k in range(n_images):
        assert np.array_equal(rd.io.read_fits_index(path, k), expect[k])
    with pytest.raises(RuntimeError, match="image.fits"):
        rd.io.read_fits_index(path, n_images)


def test_reader_rejects_malformed_files(tmp_path):
    data = np.arange(35, dtype=np.float32).reshape(5, 7)
    good, _ = fits_bytes(data)

    def check(name, raw, why):
        path = tmp_path / name
        path.write_bytes(raw)
        with pytest.raises(RuntimeError, match=name) as e:
            rd.io.read_fits(str(path))
        assert why in str(e.value), str(e.value)

    check("truncated.fits", good[:BLOCK + 35 * 4 - 8], "truncated")
    check("header_only.fits", good[:BLOCK], "truncated")
    check("short.fits", good[:100], "END")
    cards = [card("SIMPLE", True), card("BITPIX", -32), card("NAXIS", 2),
             card("NAXIS1", 7), card("NAXIS2", 5)]
    check("no_end.fits", header_bytes(cards, end=False) + good[BLOCK:], "END")
    one = [card("SIMPLE", True), card("BITPIX", -32), card("NAXIS", 1), card("NAXIS1", 35)]
    check("naxis1.fits", header_bytes(one) + good[BLOCK:], "NAXIS")
    b64 = [card("SIMPLE", True), card("BITPIX", 64), card("NAXIS", 2), card("NAXIS1", 7),
           card("NAXIS2", 5)]
    check("bitpix64.fits", header_bytes(b64) + b"\0" * BLOCK, "BITPIX")
    neg = [card("SIMPLE", True), card("BITPIX", -32), card("NAXIS", 2), card("NAXIS1", -7),
           card("NAXIS2", 5)]
    check("negative.fits", header_bytes(neg) + good[BLOCK:], "NAXIS1")
    huge = [card("SIMPLE", True), card("BITPIX", -32), card("NAXIS", 3),
            card("NAXIS1", 2 ** 31), card("NAXIS2", 2 ** 31), card("NAXIS3", 2 ** 31)]
    check("overflow.fits", header_bytes(huge) + good[BLOCK:], "overflow")
    check("not_fits.fits", b"x" * (2 * BLOCK), "SIMPLE")
    with pytest.raises(RuntimeError, match="missing.fits.*is not available"):
        rd.io.read_fits(str(tmp_path / "missing.fits"))


def test_writer_round_trip(tmp_path):
    data = np.random.default_rng(3).standard_normal((11, 6)).astype(np.float32)
    path = str(tmp_path / "out.fits")
    rd.io.write_fits(path, data, 0.01, 0.02)
    raw = open(path, "rb").read()
    assert len(raw) % BLOCK == 0
    head = raw[:BLOCK].decode("ascii")
    cards = {head[i:i + 8].strip(): head[i + 10:i + 80].strip() for i in range(0, BLOCK, 80)}
    assert cards["SIMPLE"] == "T" and int(cards["BITPIX"]) == -32 and int(cards["NAXIS"]) == 2
    assert (int(cards["NAXIS1"]), int(cards["NAXIS2"])) == (6, 11)
    assert float(cards["CDELT1"]) == pytest.approx(-np.degrees(0.01), rel=1e-12)
    assert float(cards["CDELT2"]) == pytest.approx(np.degrees(0.02), rel=1e-12)
    assert "END" in cards
    assert np.array_equal(np.frombuffer(raw[BLOCK:BLOCK + data.size * 4], ">f4").reshape(11, 6),
                          data)
    planes, n_images, n_frequencies = rd.io.read_fits(path)
    assert (n_images, n_frequencies) == (1, 1) and np.array_equal(planes[0], data)


# ------------------------------------------------ Radler construction (CPU)
def _settings(w, h, scale=1.0 / 3600.0 * np.pi / 180.0):
    s = rd.Settings()
    s.trimmed_image_width, s.trimmed_image_height = w, h
    s.pixel_scale.x = s.pixel_scale.y = scale
    s.minor_iteration_count = 100
    s.absolute_threshold = 1e-3
    return s


def _cube(n, w, h):
    z = np.zeros((n, h, w), np.float32)
    return z, z.copy(), z.copy()


def _frequencies(n):
    f = 1.0e8 + 1.0e7 * np.arange(n)
    return np.stack([f, f], axis=1)


def test_fits_mask_of_the_wrong_size_is_rejected(tmp_path):
    s = _settings(16, 12)
    s.fits_mask = str(tmp_path / "mask.fits")
    write_fits(s.fits_mask, np.ones((12, 15), np.float32))
    psf, res, mod = _cube(1, 16, 12)
    with pytest.raises(RuntimeError, match="Specified Fits file mask did not have same "
                                           "dimensions as output image!"):
        rd.Radler(s, psf[0], res[0], mod[0], 0.0)
    # a per-channel mask cube needs channels_out planes
    write_fits(s.fits_mask, np.ones((1, 3, 12, 16), np.float32),
               ctypes=["RA---SIN", "DEC--SIN", "FREQ", "STOKES"])
    s.channels_out = 2
    with pytest.raises(RuntimeError, match=r"The number of frequencies in the specified fits "
                                           r"mask \(3\) does not match the number of requested "
                                           r"output channels \(2\)"):
        rd.Radler(s, psf[0], res[0], mod[0], 0.0)
    s.channels_out = 3
    rd.Radler(s, psf[0], res[0], mod[0], 0.0)  # accepted: no GPU is needed to construct
    s.fits_mask = str(tmp_path / "absent.fits")
    with pytest.raises(RuntimeError, match="absent.fits' is not available"):
        rd.Radler(s, psf[0], res[0], mod[0], 0.0)
    s.fits_mask = ""
    s.casa_mask = "mask.casa"
    with pytest.raises(RuntimeError, match="not available in the MI355X build"):
        rd.Radler(s, psf[0], res[0], mod[0], 0.0)


def test_forced_term_cube_checks(tmp_path):
    s = _settings(16, 12)
    s.spectral_fitting.mode = rd.SpectralFittingMode.forced_terms
    s.spectral_fitting.terms = 3
    s.spectral_fitting.forced_filename = str(tmp_path / "terms.fits")
    psf, res, mod = _cube(2, 16, 12)
    args = (0.0, 2, _frequencies(2), np.ones(2))
    write_fits(s.spectral_fitting.forced_filename, np.zeros((1, 12, 16), np.float32))
    with pytest.raises(RuntimeError, match="The number of images in the forced spectrum fits "
                                           "file does not match"):
        rd.Radler(s, psf, res, mod, *args)
    write_fits(s.spectral_fitting.forced_filename, np.zeros((2, 16, 12), np.float32))
    with pytest.raises(RuntimeError, match="The image dimensions of the forced spectrum fits "
                                           "file do not match"):
        rd.Radler(s, psf, res, mod, *args)
    write_fits(s.spectral_fitting.forced_filename, np.zeros((2, 12, 16), np.float32))
    rd.Radler(s, psf, res, mod, *args)
    # component optimisation has no defined meaning with forced terms
    rd.gpu.set_component_optimization(s, rd.OptimizationAlgorithm.gradient_descent)
    with pytest.raises(RuntimeError, match="cannot be combined with forced-term"):
        rd.Radler(s, psf, res, mod, *args)


@pytest.mark.parametrize("named", [True, False])
def test_horizon_mask_file(tmp_path, named):
    """cpp/radler.cc:484-524: pixels with l^2 + m^2 >= sin^2(pi/2 - distance)
    are masked, l = (w/2 - x) dx, m = (y - h/2) dy; the mask is written as a
    FITS image of ones and zeros."""
    w, h = 64, 48
    # a scale of 0.02 would put pixels such as (dx, dy) = (12, 16) exactly on
    # the boundary (0.0004 x 400 = 0.16); with 0.021 the nearest are
    # 0.000441 x 362 = 0.159642 and 0.000441 x 363 = 0.160083
    scale = 0.021
    s = _settings(w, h, scale)
    s.horizon_mask_distance = np.pi / 2 - np.arcsin(0.4)
    if named:
        s.horizon_mask_filename = path = str(tmp_path / "horizon.fits")
    else:
        s.prefix_name = str(tmp_path / "run7")
        path = s.prefix_name + "-horizon-mask.fits"
    psf, res, mod = _cube(1, w, h)
    rd.Radler(s, psf[0], res[0], mod[0], 0.0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = ((w / 2 - xx) * scale) ** 2 + ((yy - h / 2) * scale) ** 2
    assert np.abs(r2 - 0.16).min() > 1e-9  # no pixel on the boundary
    planes, n_images, _ = rd.io.read_fits(path)
    assert n_images == 1
    expect = (r2 < 0.16).astype(np.float32)
    assert 0 < expect.sum() < expect.size
    assert np.array_equal(planes[0], expect)


# ---------------------------------------------------------------------- GPU
def _compact_psf(w, h, fwhm=4.0, radius=10):
    """A Gaussian core cut off at `radius` pixels: CLEAN of sources further
    than that from each other and from the edges does not couple them."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = (xx - w // 2) ** 2 + (yy - h // 2) ** 2
    psf = np.exp(-0.5 * r2 / (fwhm / 2.3548) ** 2) * (r2 <= radius * radius)
    return psf.astype(np.float32)


def _shift(psf, x0, y0):
    """psf with its centre at (x0, y0), zero filled."""
    h, w = psf.shape
    out = np.zeros_like(psf)
    dx, dy = x0 - w // 2, y0 - h // 2
    ys, xs = slice(max(dy, 0), h + min(dy, 0)), slice(max(dx, 0), w + min(dx, 0))
    yd, xd = slice(max(-dy, 0), h + min(-dy, 0)), slice(max(-dx, 0), w + min(-dx, 0))
    out[ys, xs] = psf[yd, xd]
    return out


@pytest.mark.gpu
def test_fits_mask_confines_the_model(tmp_path):
    w, h = 64, 48
    psf = _compact_psf(w, h)
    inside, outside = (20, 24), (44, 20)
    residual = (_shift(psf, *inside) + _shift(psf, *outside)).astype(np.float32)
    model = np.zeros_like(residual)
    mask = np.zeros((h, w), np.float32)
    mask[:, :32] = 7.0  # non-zero means clean
    s = _settings(w, h)
    s.algorithm_type = rd.AlgorithmType.generic_clean
    s.generic.use_sub_minor_optimization = False
    s.border_ratio = 0.0
    s.absolute_threshold = 0.01
    s.minor_iteration_count = 500
    s.fits_mask = str(tmp_path / "mask.fits")
    write_fits(s.fits_mask, mask)
    r = rd.Radler(s, psf, residual, model, 0.0)
    r.perform(0)
    assert r.iteration_number > 10
    assert np.count_nonzero(model[:, 32:]) == 0
    assert model[:, :32].sum() > 0.9
    assert residual[outside[1], outside[0]] > 0.9
    assert abs(residual[inside[1], inside[0]]) <= 0.011


@pytest.mark.gpu
def test_local_rms_image_file_steers_the_first_component(tmp_path):
    w, h = 64, 48
    psf = _compact_psf(w, h)
    left, right = (20, 24), (44, 20)
    residual = (_shift(psf, *left) + 2.0 * _shift(psf, *right)).astype(np.float32)
    model = np.zeros_like(residual)
    rms = np.ones((h, w), np.float32)
    rms[:, 32:] = 10.0
    s = _settings(w, h)
    s.algorithm_type = rd.AlgorithmType.generic_clean
    s.generic.use_sub_minor_optimization = False
    s.border_ratio = 0.0
    s.minor_iteration_count = 1
    s.local_rms.image = str(tmp_path / "rms.fits")
    write_fits(s.local_rms.image, rms)
    r = rd.Radler(s, psf, residual, model, 0.0)
    r.perform(0)
    assert r.iteration_number == 1
    ys, xs = np.nonzero(model)
    assert list(zip(xs, ys)) == [left]
    assert model[left[1], left[0]] == pytest.approx(0.1, rel=1e-5)
    s.local_rms.image = str(tmp_path / "absent.fits")
    r = rd.Radler(s, psf, residual.copy(), np.zeros_like(model), 0.0)
    with pytest.raises(RuntimeError, match="absent.fits' is not available"):
        r.perform(0)
