"""radler.SourceCatalogue on the host: the reader of the text format
ComponentList.write emits, its spectra and its coordinates. No GPU is needed;
tests/test_draw_sources_gpu.py and tests/test_source_catalogue_gpu.py cover
the device side."""
import math

import numpy as np
import pytest

import sources_lib as L
from radler_import import radler as rd

MODE = rd.SpectralFittingMode
W, H = 40, 24
PIX = 1.0 / 3600.0 * math.pi / 180.0  # 1 arcsec: 1 ms of RA and 1 mas of Dec are sub-pixel
RA0, DEC0 = 0.3, 0.4
SCALES = [0.0, 4.0, 9.0]
FREQUENCIES = [1.0e8, 1.4e8]


def make_list():
    """~20 components over 3 scales at 2 frequencies, both corners included."""
    rng = np.random.default_rng(5)
    cl = rd.ComponentList(W, H, len(SCALES), len(FREQUENCIES))
    seen = set()
    for s in range(len(SCALES)):
        spots = [(0, 0), (W - 1, H - 1)] if s == 0 else []
        while len(spots) < 7:
            spots.append((int(rng.integers(0, W)), int(rng.integers(0, H))))
        for x, y in spots:
            if (s, x, y) in seen:
                continue
            seen.add((s, x, y))
            amp = float(rng.uniform(0.05, 2.0))
            cl.add(x, y, s, [amp, amp * float(rng.uniform(0.6, 1.3))])
    cl.merge_duplicates()
    return cl


@pytest.mark.parametrize("mode", [MODE.polynomial, MODE.log_polynomial])
@pytest.mark.parametrize("shift", [(0.0, 0.0), (0.002, -0.0035)])
def test_round_trip(tmp_path, mode, shift):
    cl = make_list()
    fitter = rd.SpectralFitter(mode, 2, FREQUENCIES, [1.0, 1.0])
    path = str(tmp_path / "sources.txt")
    cl.write(path, fitter, SCALES, PIX, PIX, RA0, DEC0, shift[0], shift[1], device=False)
    cat = rd.SourceCatalogue.read(path)
    counts = [cl.component_count(s) for s in range(len(SCALES))]
    assert len(cat) == sum(counts) and sum(counts) >= 19
    assert cat.names == [f"s{s}c{i}" for s in range(len(SCALES)) for i in range(counts[s])]
    assert cat.types == [("POINT" if SCALES[s] == 0.0 else "GAUSSIAN")
                         for s in range(len(SCALES)) for _ in range(counts[s])]
    assert cat.reference_frequency == fitter.reference_frequency
    assert np.all(cat.logarithmic == (mode == MODE.log_polynomial))
    # the terms, to the 7 significant digits the writer prints
    terms = np.concatenate([cl.fit_terms(s, fitter) for s in range(len(SCALES))])
    got = np.column_stack([cat.flux, np.asarray([t[0] for t in cat.terms])])
    assert all(t.shape == (1,) and t.dtype == np.float32 for t in cat.terms)
    np.testing.assert_allclose(got, terms, rtol=5e-7)
    # the positions: back on the integer pixels
    xy = cat.pixel_positions(W, H, PIX, PIX, RA0, DEC0, shift[0], shift[1])
    assert cat.dropped == 0 and xy.shape == (len(cat), 2)
    want = [p for s in range(len(SCALES)) for p in cl.get_positions(s)]
    assert [(math.floor(x + 0.5), math.floor(y + 0.5)) for x, y in xy] == want
    assert (0, 0) in want and (W - 1, H - 1) in want
    assert np.max(np.abs(xy - np.asarray(want))) < 0.02  # 1 ms of RA is 0.015 arcsec
    # the Gaussian axes, as printed: the FWHM of the scale in arcsec
    row = 0
    for s in range(len(SCALES)):
        fwhm = 2.0 * math.sqrt(2.0 * math.log(2.0)) * SCALES[s] * 3.0 / 16.0
        for _ in range(counts[s]):
            np.testing.assert_allclose([cat.major[row], cat.minor[row]], fwhm, rtol=1e-12,
                                       atol=0.0)
            assert cat.orientation[row] == 0.0
            row += 1


HAND = """# a hand-written catalogue: columns reordered, optional ones missing

format = Type, Name, Dec, Ra, SpectralIndex, I, Flag, ReferenceFrequency='1.5e8', LogarithmicSI

  # an indented comment
POINT, north, +40.30.15.250, 01:10:20.500, [], 2.5, x, ,
GAUSSIAN, south, -05.00.00.100, -00:00:30.000, [-0.7], 1.25, y, 1.2e8, true
point, curved, 00.00.01, 23:59:59.999, [-0.7, 0.1, -0.02], 0.5, z, , true

Point, linear, -00.30.00.000, 12:00:00, [0.3, -0.1, 0.05], -1.5, , 2e8, false
POINT, short, 10.00.00.000, 02:00:00.000, , 3.0
"""


def test_hand_written_file(tmp_path):
    path = str(tmp_path / "hand.txt")
    with open(path, "w") as f:
        f.write(HAND)
    cat = rd.SourceCatalogue.read(path)
    assert len(cat) == 5
    assert cat.names == ["north", "south", "curved", "linear", "short"]
    assert cat.types == ["POINT", "GAUSSIAN", "POINT", "POINT", "POINT"]
    assert cat.reference_frequency == 1.5e8
    hours, degrees = math.pi / 12.0, math.pi / 180.0
    ra = [(1 + 10 / 60 + 20.5 / 3600) * hours, -(30.0 / 3600) * hours,
          (23 + 59 / 60 + 59.999 / 3600) * hours, 12 * hours, 2 * hours]
    dec = [(40 + 30 / 60 + 15.25 / 3600) * degrees, -(5 + 0.1 / 3600) * degrees,
           (1.0 / 3600) * degrees, -0.5 * degrees, 10 * degrees]
    np.testing.assert_allclose(cat.ra, ra, rtol=0, atol=1e-14)
    np.testing.assert_allclose(cat.dec, dec, rtol=0, atol=1e-14)
    assert cat.flux.dtype == np.float32
    assert list(cat.flux) == [2.5, 1.25, 0.5, -1.5, 3.0]
    assert [len(t) for t in cat.terms] == [0, 1, 3, 3, 0]
    assert list(cat.terms[2]) == [np.float32(-0.7), np.float32(0.1), np.float32(-0.02)]
    assert list(cat.logarithmic) == [True, True, True, False, True]
    assert list(cat.reference_frequencies) == [1.5e8, 1.2e8, 1.5e8, 2e8, 1.5e8]
    # no shape columns: every axis is 0
    assert not np.any(cat.major) and not np.any(cat.minor) and not np.any(cat.orientation)

    nus = [0.9e8, 1.5e8, 2.3e8]
    table = cat.flux_at(nus)
    assert table.shape == (3, 5) and table.dtype == np.float32
    for g, nu in enumerate(nus):
        assert table[g, 0] == np.float32(2.5) and table[g, 4] == np.float32(3.0)  # no terms
        for i in (1, 2):
            want = L.log_flux([cat.flux[i], *cat.terms[i]], nu, cat.reference_frequencies[i])
            assert abs(table[g, i] - want) <= 1e-6 * abs(want)
        want = L.polynomial_flux([cat.flux[3], *cat.terms[3]], nu, 2e8)
        assert table[g, 3] == want  # the same float loop
    assert table[1, 2] == np.float32(0.5)  # at its reference frequency


def test_shape_columns_and_defaults(tmp_path):
    path = str(tmp_path / "shapes.txt")
    with open(path, "w") as f:
        f.write("Format = Name, Type, Ra, Dec, I, MajorAxis, MinorAxis, Orientation\n"
                "a, GAUSSIAN, 00:00:00.000, 00.00.00.000, 1, 30.5, 12.25, 35\n"
                "b, POINT, 00:00:00.000, 00.00.00.000, 1, , ,\n")
    cat = rd.SourceCatalogue.read(path)
    assert list(cat.major) == [30.5, 0.0] and list(cat.minor) == [12.25, 0.0]
    assert list(cat.orientation) == [35.0, 0.0]
    assert cat.reference_frequency == 0.0 and list(cat.logarithmic) == [True, True]
    assert np.array_equal(cat.flux_at([1e8]), np.ones((1, 2), np.float32))


HEAD = "Format = Name, Type, Ra, Dec, I, SpectralIndex, LogarithmicSI, ReferenceFrequency='1e8'\n"
GOOD = "a, POINT, 01:00:00.000, 10.00.00.000, 1.0, [], true,\n"
BAD_FILES = {
    "no_format": ("# nothing but a comment\n" + GOOD, 2, "Format"),
    "no_format_at_all": ("# nothing\n\n", 3, "Format"),
    "unknown_type": (HEAD + GOOD + "b, DISK, 01:00:00.000, 10.00.00.000, 1.0, [], true,\n", 3,
                     "DISK"),
    "bad_ra": (HEAD + "b, POINT, 01:61:00.000, 10.00.00.000, 1.0, [], true,\n", 2, "Ra"),
    "bad_ra_text": (HEAD + "b, POINT, 1h00m, 10.00.00.000, 1.0, [], true,\n", 2, "Ra"),
    "bad_dec": (HEAD + "\n" + GOOD + "b, POINT, 01:00:00.000, 10:00:00.000, 1.0, [], true,\n", 4,
                "Dec"),
    "unterminated_bracket": (HEAD + "b, POINT, 01:00:00.000, 10.00.00.000, 1.0, [-0.7, true,\n",
                             2, "["),
    "too_few_fields": (HEAD + GOOD + GOOD + "b, POINT, 01:00:00.000\n", 4, "few"),
    "terms_without_reference": (
        "Format = Name, Type, Ra, Dec, I, SpectralIndex\n"
        "a, POINT, 01:00:00.000, 10.00.00.000, 1.0, []\n"
        "b, POINT, 01:00:00.000, 10.00.00.000, 1.0, [-0.7]\n", 3, "ReferenceFrequency"),
    "bad_flux": (HEAD + "b, POINT, 01:00:00.000, 10.00.00.000, bright, [], true,\n", 2, "bright"),
}


@pytest.mark.parametrize("case", list(BAD_FILES))
def test_malformed_lines_name_the_file_and_the_line(tmp_path, case):
    text, line, word = BAD_FILES[case]
    path = str(tmp_path / f"{case}.txt")
    with open(path, "w") as f:
        f.write(text)
    with pytest.raises(RuntimeError) as e:
        rd.SourceCatalogue.read(path)
    message = str(e.value)
    assert path in message and f"line {line}:" in message and word in message, message


def test_missing_file(tmp_path):
    path = str(tmp_path / "absent.txt")
    with pytest.raises(RuntimeError) as e:
        rd.SourceCatalogue.read(path)
    assert path in str(e.value)


def test_sources_behind_the_phase_centre_are_dropped(tmp_path):
    path = str(tmp_path / "sky.txt")
    ra1, dec1 = L.xy_to_radec(10.3, 7.6, W, H, PIX, 1.5 * PIX, RA0, DEC0)
    rows = [("near", ra1, dec1), ("behind", RA0 + math.pi, -DEC0),
            ("far", RA0 + 0.75 * math.pi, 0.1)]
    with open(path, "w") as f:
        f.write("Format = Name, Type, Ra, Dec, I\n")
        for name, ra, dec in rows:
            f.write(f"{name}, POINT, {L.format_ra(ra)}, {L.format_dec(dec)}, 1.0\n")
    cat = rd.SourceCatalogue.read(path)
    assert cat.dropped == 0
    xy = cat.pixel_positions(W, H, PIX, 1.5 * PIX, RA0, DEC0)
    assert cat.dropped == 2
    assert np.all(np.isnan(xy[1:])) and np.all(np.isfinite(xy[0]))
    # non-square pixels, a fractional position: to the precision of the text
    np.testing.assert_allclose(xy[0], [10.3, 7.6], atol=0.02)
    want = L.radec_to_xy(cat.ra[0], cat.dec[0], W, H, PIX, 1.5 * PIX, RA0, DEC0)
    np.testing.assert_allclose(xy[0], want, atol=1e-6)


def test_argument_errors_need_no_gpu(tmp_path):
    path = str(tmp_path / "one.txt")
    with open(path, "w") as f:
        f.write("Format = Name, Type, Ra, Dec, I\na, POINT, 00:00:00.000, 00.00.00.000, 1.0\n")
    cat = rd.SourceCatalogue.read(path)
    nus = [1e8]
    for args in [(0, H, PIX, PIX, 0.0, 0.0, nus), (W, 0, PIX, PIX, 0.0, 0.0, nus),
                 (W, H, 0.0, PIX, 0.0, 0.0, nus), (W, H, PIX, -PIX, 0.0, 0.0, nus),
                 (W, H, PIX, PIX, 0.0, 0.0, []), (W, H, PIX, PIX, 0.0, 0.0, [1e8, 0.0]),
                 (W, H, PIX, PIX, 0.0, 0.0, [1e8] * 65), (W, H, PIX, PIX, math.nan, 0.0, nus)]:
        with pytest.raises(ValueError):
            cat.draw_model(*args)
    image = np.zeros((H, W), np.float32)
    beam = (3.0 * PIX, 2.0 * PIX, 0.5)
    for images, rest in [(image, (PIX, PIX, 0.0, 0.0, nus, 0.0, 0.0, 0.0)),       # no beam
                         (image, (PIX, PIX, 0.0, 0.0, nus, 3.0 * PIX, 0.0, 0.0)),  # half a beam
                         (image, (PIX, 0.0, 0.0, 0.0, nus, *beam)),
                         (image, (PIX, PIX, 0.0, 0.0, [1e8, 2e8], *beam)),         # 1 plane, 2 nu
                         (np.zeros((2, H, W), np.float32), (PIX, PIX, 0.0, 0.0, nus, *beam)),
                         (np.zeros(W, np.float32), (PIX, PIX, 0.0, 0.0, nus, *beam)),
                         (image, (PIX, PIX, 0.0, 0.0, [-1e8], *beam))]:
        with pytest.raises(ValueError):
            cat.restore(images, *rest)
    with pytest.raises(ValueError):
        cat.flux_at([0.0])
