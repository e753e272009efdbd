"""ComponentList.write: the source catalogue of a component list (the
reference's ComponentList::Write, cpp/component_list.cc:59-140, in the text
format of cpp/utils/write_model.h), through the host path: one fitter.fit per
component. No GPU is needed; tests/test_write_sources_gpu.py covers the
batched device fit and Radler's write_sources."""
import math
import re

import numpy as np
import pytest

from radler_import import radler as rd

W, H = 40, 24  # non-square: a swapped axis shows
PIXEL_SCALE = 1.0 / 60.0 * math.pi / 180.0
HEADER = ("Format = Name, Type, Ra, Dec, I, SpectralIndex, LogarithmicSI, "
          "ReferenceFrequency='{ref}', MajorAxis, MinorAxis, Orientation")
MODE = rd.SpectralFittingMode


def no_fitting():
    return rd.SpectralFitter(MODE.no_fitting, 0, [], [])


def split_row(line):
    """name, type, ra, dec, t0, [t1..], log_si, ref, major, minor, orientation"""
    m = re.match(r"^([^,]*),([^,]*),([^,]*),([^,]*),([^,]*),\[([^\]]*)\],(.*)$", line)
    assert m, line
    rest = m.group(7).split(",")
    assert len(rest) == 5, line
    si = [float(t) for t in m.group(6).split(",")] if m.group(6) else []
    return {"name": m.group(1), "type": m.group(2), "ra": m.group(3), "dec": m.group(4),
            "terms": [float(m.group(5))] + si, "si_text": m.group(6), "log_si": rest[0],
            "ref": rest[1], "major": rest[2], "minor": rest[3], "orientation": rest[4]}


def read_rows(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""  # every row ends in a newline
    return lines[0], [split_row(line) for line in lines[1:-1]]


def lm_to_radec(l, m, ra0, dec0):
    n = math.sqrt(1.0 - l * l - m * m)
    return (ra0 + math.atan2(l, n * math.cos(dec0) - m * math.sin(dec0)),
            math.asin(m * math.cos(dec0) + n * math.sin(dec0)))


def parse_sexagesimal(text, pattern):
    assert re.match(pattern, text), text
    sign = -1.0 if text.startswith("-") else 1.0
    a, b, c = re.match(r"^-?(\d\d).(\d\d).(\d\d\.\d{3})$", text).groups()
    return sign * (int(a) + int(b) / 60.0 + float(c) / 3600.0)


def parse_ra(text):
    """radians"""
    return parse_sexagesimal(text, r"^-?\d\d:\d\d:\d\d\.\d{3}$") * math.pi / 12.0


def parse_dec(text):
    return parse_sexagesimal(text, r"^-?\d\d\.\d\d\.\d\d\.\d{3}$") * math.pi / 180.0


def test_format(tmp_path):
    cl = rd.ComponentList(W, H, 2, 1)
    cl.add(3, 5, 0, [1.5])
    cl.add(39, 23, 0, [-0.25])
    cl.add(20, 12, 1, [1e-7])
    cl.merge_duplicates()
    path = str(tmp_path / "sources.txt")
    scale_x, scale_y = PIXEL_SCALE, 0.5 * PIXEL_SCALE
    cl.write(path, no_fitting(), [0.0, 16.0], scale_x, scale_y, 0.3, 0.4)
    header, rows = read_rows(path)
    assert header == HEADER.format(ref="0")  # a fitter without frequencies
    assert [r["name"] for r in rows] == ["s0c0", "s0c1", "s1c0"]
    assert [r["type"] for r in rows] == ["POINT", "POINT", "GAUSSIAN"]
    lines = open(path).read().split("\n")
    for line, row, value in zip(lines[1:], rows, [1.5, -0.25, 1e-7]):
        assert row["si_text"] == "" and ",[]," in line
        assert row["log_si"] == "false"
        assert row["terms"] == [value]
    assert lines[1].endswith(",1.5,[],false,0,,,")
    assert lines[2].endswith(",-0.25,[],false,0,,,")
    assert "1e-07,[]" in lines[3]  # default stream notation
    fwhm = 2.0 * math.sqrt(2.0 * math.log(2.0)) * 16.0 * 3.0 / 16.0
    to_arcsec = 180.0 * 3600.0 / math.pi
    np.testing.assert_allclose(float(rows[2]["major"]), fwhm * scale_x * to_arcsec, rtol=1e-12)
    np.testing.assert_allclose(float(rows[2]["minor"]), fwhm * scale_y * to_arcsec, rtol=1e-12)
    assert rows[2]["orientation"] == "0"


def test_reference_frequency_has_16_digits(tmp_path):
    freqs = [100e6 + 1.0 / 3.0, 150e6, 200e6 + 1.0 / 7.0]
    fitter = rd.SpectralFitter(MODE.polynomial, 2, freqs, [1.0, 2.0, 1.0])
    cl = rd.ComponentList(W, H, 1, 3)
    cl.add(1, 2, 0, [1.0, 2.0, 3.0])
    cl.merge_duplicates()
    path = str(tmp_path / "sources.txt")
    cl.write(path, fitter, [0.0], PIXEL_SCALE, PIXEL_SCALE, 0.0, 0.0)
    header, rows = read_rows(path)
    ref = "%.16g" % fitter.reference_frequency
    assert header == HEADER.format(ref=ref)
    assert rows[0]["ref"] == ref
    assert float(ref) == fitter.reference_frequency


@pytest.mark.parametrize("centre", [(0.3, 0.4), (-0.2, -0.5), (6.2, 1.5)])
@pytest.mark.parametrize("shift", [(0.0, 0.0), (0.002, -0.0035)])
def test_coordinates(tmp_path, centre, shift):
    ra0, dec0 = centre
    positions = [(W // 2, H // 2), (0, 0), (W - 1, H - 1), (7, 19)]
    cl = rd.ComponentList(W, H, 1, 1)
    for x, y in positions:
        cl.add(x, y, 0, [1.0])
    cl.merge_duplicates()
    path = str(tmp_path / "sources.txt")
    scale_x, scale_y = PIXEL_SCALE, 0.75 * PIXEL_SCALE
    cl.write(path, no_fitting(), [0.0], scale_x, scale_y, ra0, dec0, shift[0], shift[1])
    _, rows = read_rows(path)
    listed = cl.get_positions(0)
    assert sorted(listed) == sorted(positions)
    half_ms = 0.5e-3 / 3600.0 * math.pi / 12.0   # half a printed unit of time
    half_mas = 0.5e-3 / 3600.0 * math.pi / 180.0
    for (x, y), row in zip(listed, rows):
        l = (W / 2 - x) * scale_x + shift[0]
        m = (y - H / 2) * scale_y + shift[1]
        ra, dec = lm_to_radec(l, m, ra0, dec0)
        ra = math.fmod(ra, 2.0 * math.pi)  # printed as fmod(hours, 24), sign kept
        assert abs(parse_ra(row["ra"]) - ra) <= half_ms + 1e-12, (row, ra)
        assert abs(parse_dec(row["dec"]) - dec) <= half_mas + 1e-12, (row, dec)
        assert row["ra"].startswith("-") == (ra0 < 0)
        assert row["dec"].startswith("-") == (dec0 < 0)
        if (x, y) == (W // 2, H // 2) and shift == (0.0, 0.0):
            # the centre pixel is the phase centre itself
            assert abs(parse_ra(row["ra"]) - ra0) <= half_ms + 1e-12
            assert abs(parse_dec(row["dec"]) - dec0) <= half_mas + 1e-12


def fitters():
    poly = rd.SpectralFitter(MODE.polynomial, 3, [100e6, 120e6, 140e6, 160e6, 180e6],
                             [1.0, 2.0, 0.0, 1.0, 0.5])
    logp = rd.SpectralFitter(MODE.log_polynomial, 3,
                             [100e6, 115e6, 130e6, 150e6, 170e6, 200e6], [1.0] * 6)
    forced = rd.SpectralFitter(MODE.forced_terms, 3, [100e6, 130e6, 160e6, 200e6],
                               [1.0, 0.5, 2.0, 1.0])
    rng = np.random.default_rng(11)
    forced.set_forced_terms([rng.uniform(-1.0, 0.2, (H, W)).astype(np.float32),
                             rng.uniform(-0.3, 0.3, (H, W)).astype(np.float32)])
    return {"polynomial": (poly, "false"), "log_polynomial": (logp, "true"),
            "forced_terms": (forced, "true")}


@pytest.mark.parametrize("mode", ["polynomial", "log_polynomial", "forced_terms"])
def test_terms(tmp_path, mode):
    fitter, log_si = fitters()[mode]
    n_freq = len(fitter.frequencies)
    rng = np.random.default_rng(5)
    x = (fitter.reference_frequency / np.asarray(fitter.frequencies))
    cl = rd.ComponentList(W, H, 2, n_freq)
    for scale, (px, py) in [(0, (0, 0)), (0, (W - 1, H - 1)), (0, (17, 3)), (1, (W - 1, H - 1)),
                            (1, (0, 0)), (1, (5, 20))]:
        values = rng.uniform(0.5, 2.0) * x ** rng.uniform(0.0, 1.5) \
            * (1.0 + 0.02 * rng.standard_normal(n_freq))
        if (scale, px) == (1, 5):
            values = -values  # a negative component
        cl.add(px, py, scale, [float(v) for v in values.astype(np.float32)])
    cl.merge_duplicates()
    path = str(tmp_path / "sources.txt")
    cl.write(path, fitter, [0.0, 16.0], PIXEL_SCALE, PIXEL_SCALE, 0.3, 0.4)
    _, rows = read_rows(path)
    expected_names, expected_terms = [], []
    for s in range(2):
        for i in range(cl.component_count(s)):
            px, py, values = cl.get_component(s, i)
            expected_names.append(f"s{s}c{i}")
            expected_terms.append(np.asarray(fitter.fit(values, px, py), np.float32))
    assert [r["name"] for r in rows] == expected_names
    assert len(rows) == 6
    for row, want in zip(rows, expected_terms):
        assert row["log_si"] == log_si
        assert len(row["terms"]) == 3
        np.testing.assert_allclose(np.asarray(row["terms"], np.float64),
                                   want.astype(np.float64), rtol=1e-6)
    # fit_terms exposes the same terms unprinted
    got = np.concatenate([cl.fit_terms(s, fitter) for s in range(2)])
    np.testing.assert_array_equal(got, np.asarray(expected_terms, np.float32))


def test_unmerged_components_are_refused(tmp_path):
    cl = rd.ComponentList(W, H, 1, 1)
    cl.add(1, 1, 0, [1.0])
    with pytest.raises(RuntimeError, match="yet unmerged components"):
        cl.write(str(tmp_path / "s.txt"), no_fitting(), [0.0], PIXEL_SCALE, PIXEL_SCALE, 0.0, 0.0)


def test_several_frequencies_need_a_fitting_mode(tmp_path):
    cl = rd.ComponentList(W, H, 1, 2)
    cl.add(1, 1, 0, [1.0, 2.0])
    cl.merge_duplicates()
    with pytest.raises(RuntimeError, match="not specified a spectral fitting method"):
        cl.write(str(tmp_path / "s.txt"), no_fitting(), [0.0], PIXEL_SCALE, PIXEL_SCALE, 0.0, 0.0)


def test_channel_count_mismatch_is_refused(tmp_path):
    cl = rd.ComponentList(W, H, 1, 3)
    cl.add(1, 1, 0, [1.0, 2.0, 3.0])
    cl.merge_duplicates()
    fitter = rd.SpectralFitter(MODE.polynomial, 2, [100e6, 120e6, 140e6, 160e6], [1.0] * 4)
    with pytest.raises(RuntimeError, match=r"3 frequencies.*4 channels"):
        cl.write(str(tmp_path / "s.txt"), fitter, [0.0], PIXEL_SCALE, PIXEL_SCALE, 0.0, 0.0)
