"""The plan tables of the compile-time-planned FFT engine as tests/fft_plans.py
reads them from csrc/hip/fft_fast_*.hip, and negative controls of the
comparison helpers that tests/test_fft_plans.py applies to every plan on the
GPU. No GPU here.

* the tables: every entry's length equals its trailing comment, no length
  twice in a family, the float64 row and column ladders agree, the three
  float ladders agree, every convolution-column plan has a column plan, and
  the four-step launch grids divide exactly (N1 % GB, N2 % GA);
* the helpers: each rejects numpy's own result with one spectrum bin off by
  10 x its bound, and the result of a length-1792 column transform (radices
  8, 8, 4, 7, the float one-pass plan's) with one pass's twiddles left out;
  each accepts the undoctored result;
* the tiled spectrum order round-trips, w / 2 + 1 a multiple of 16 or not.
"""
import re

import numpy as np
import pytest

import fft_plans as fp

TABLES = fp.plan_tables()
ENTRIES = fp.parse_entries()


def test_every_family_is_parsed():
    for family in fp.FAMILIES:
        assert TABLES[family], family
    assert sum(len(v) for v in TABLES.values()) == len(ENTRIES)
    # nothing that looks like a table entry was passed over
    for name in fp.SOURCES:
        text = open(fp.HIP_DIR + "/" + name).read()
        calls = [ln for ln in text.splitlines()
                 if re.search(r"\bRDL_(FAST_ROWS|FAST_COLS|CONV_D|FAST_STEPS)\(", ln)
                 and not ln.lstrip().startswith("#")]
        assert len(calls) == sum(e.file == name for e in ENTRIES), name


@pytest.mark.parametrize("entry", ENTRIES,
                         ids=[f"{e.family}-{e.file}:{e.line}" for e in ENTRIES])
def test_length_equals_its_comment(entry):
    assert entry.comment is not None, "a plan entry without its // length comment"
    assert entry.plan.length == entry.comment, entry
    assert all(r >= 2 for rs in ([entry.plan.radices] if entry.family != "steps"
                                 else entry.plan.radices) for r in rs)


@pytest.mark.parametrize("family", fp.FAMILIES)
def test_no_length_twice(family):
    ns = [p.length for p in TABLES[family]]
    assert len(ns) == len(set(ns)), sorted(n for n in set(ns) if ns.count(n) > 1)


def test_ladders_agree():
    assert fp.lengths(TABLES, "rows_f64") == fp.lengths(TABLES, "cols_f64")
    assert fp.lengths(TABLES, "rows_f32") == fp.lengths(TABLES, "steps")
    assert fp.lengths(TABLES, "rows_f32") == fp.lengths(TABLES, "cols_f32")
    assert set(fp.lengths(TABLES, "convd")) <= set(fp.lengths(TABLES, "cols_f64"))
    assert all(p.precision == "f64" for f in ("rows_f64", "cols_f64", "convd") for p in TABLES[f])
    assert all(p.precision == "f32" for f in ("rows_f32", "cols_f32", "steps") for p in TABLES[f])


@pytest.mark.parametrize("plan", TABLES["steps"], ids=lambda p: str(p.length))
def test_four_step_grids_divide(plan):
    """FastStepLaunch's grids are n_tiles * (N1 / GB) and n_tiles * (N2 / GA),
    unchecked."""
    assert plan.n1 % plan.gb == 0 and plan.n2 % plan.ga == 0, plan
    ra, rb = plan.radices
    assert np.prod(ra) == plan.n1 and np.prod(rb) == plan.n2, plan


def test_header_comment_counts_the_row_plans():
    text = open(fp.HIP_DIR + "/fft_fast_rows_f64.hip").read()
    m = re.search(r"(\d+) plans", text.split("#include")[0])
    assert m and int(m.group(1)) == len(TABLES["rows_f64"])


def test_planes_cover_every_plan_in_both_roles():
    f64, f32, one = fp.planes(TABLES)
    n64, n32 = len(TABLES["rows_f64"]), len(TABLES["rows_f32"])
    assert len(f64) == len(set(f64)) == 2 * n64 - 1
    assert len(f32) == len(set(f32)) == 2 * n32 - 1
    assert len(one) == len(TABLES["cols_f32"])
    assert sorted({w for w, _ in f64}) == sorted({h for _, h in f64}) == fp.lengths(TABLES,
                                                                                   "rows_f64")
    assert sorted({w for w, _ in f32}) == sorted({h for _, h in f32}) == fp.lengths(TABLES,
                                                                                   "rows_f32")
    assert max(w * h for w, h in f64) <= 9450 * 1050
    # the flags the GPU test expects of the binary
    convd = set(fp.lengths(TABLES, "convd"))
    for w, h in f64:
        assert fp.expected_fast(TABLES, w, h, True) == (3 | (8 if h in convd else 0))
    for w, h in f32:
        assert fp.expected_fast(TABLES, w, h, False) == 7
    for w, h in one:
        assert fp.expected_fast(TABLES, w, h, False) == 1


@pytest.mark.parametrize("w,h", [(1280, 5), (96, 7), (30, 4), (62, 3), (2, 2)])
def test_tile_round_trip(w, h):
    nu = w // 2 + 1
    rng = np.random.default_rng(w)
    nat = (rng.standard_normal((h, nu)) + 1j * rng.standard_normal((h, nu))).astype(np.complex64)
    flat = fp.tile(nat)
    nt = (nu + 15) // 16
    assert flat.shape == (nt * 16 * h,)
    assert np.array_equal(fp.untile(flat, w, h), nat)
    # element (y, k) at ((k / 16) * h + y) * 16 + k % 16 (rdl_hip.h)
    y, k = h - 1, nu - 1
    assert flat[((k // 16) * h + y) * 16 + k % 16] == nat[y, k]
    # the padding of the last tile is zero, and tiling what untile returns restores the buffer
    assert np.count_nonzero(flat) <= np.count_nonzero(nat)
    assert np.array_equal(fp.tile(fp.untile(flat, w, h)), flat)


# ------------------------------------------------------- negative controls
W, H, RADICES = 32, 1792, (8, 8, 4, 7)
N = W * H


class Case:
    """One thin plane's float64 references, the same quantities with the
    column transform's pass 2 run without its twiddles, and a way to put one
    spectrum bin off."""

    def __init__(self):
        self.img = fp.noise_image(W, H, 11)
        rows = np.fft.rfft(self.img.astype(np.float64), axis=1)
        self.spec = np.fft.rfft2(self.img.astype(np.float64))
        self.good = fp.mixed_radix_dft(rows, RADICES)
        self.broken = fp.mixed_radix_dft(rows, RADICES, skip_twiddles=2)
        y, x = np.mgrid[-4:5, -4:5]
        self.shape = np.exp(-(x * x + y * y) / 8.0).astype(np.float32)  # even in x and y
        placed = fp.placed_kernel(self.shape.astype(np.float64), W, H)
        self.kspec = np.fft.rfft2(placed)
        self.kspec_broken = fp.mixed_radix_dft(np.fft.rfft(placed, axis=1), RADICES,
                                               skip_twiddles=2)
        self.conv = self.image_of(self.spec)
        self.residual = np.random.default_rng(12).standard_normal((H, W)).astype(np.float32)

    def image_of(self, spec, bin_offset=0.0):
        """The convolved image of a forward spectrum; bin_offset: added to
        one bin of the product, scaled so the image moves by that much (a
        cosine of that amplitude)."""
        prod = spec * self.kspec
        if bin_offset:
            prod = prod.copy()
            prod[H // 7, W // 4] += bin_offset * N / 2
        return np.fft.irfft2(prod, s=(H, W))


@pytest.fixture(scope="module")
def case():
    return Case()


def _spectrum64(c, got):
    return fp.check_spectrum(got, c.spec, N, True, "control")


def _spectrum32(c, got):
    return fp.check_spectrum(got.astype(np.complex64), c.spec, N, False, "control")


def _rows(c, got):
    # the rows pass alone: the column transform applied to one column
    return fp.check_spectrum(got[:, 3], c.spec[:, 3], H, True, "control")


SPECTRUM_HELPERS = {"spectrum-f64": _spectrum64, "spectrum-f32": _spectrum32, "rows-f64": _rows}


def _image64(c, conv):
    return fp.check_image(conv.astype(np.float32), c.conv, N, True, "control")


def _image32(c, conv):
    return fp.check_image(conv.astype(np.float32), c.conv, N, False, "control")


def _correction(c, conv):
    win = (slice(3, H - 5), slice(1, W - 2))
    got = c.residual[win] - conv[win].astype(np.float32)
    return fp.check_correction(got, c.residual[win], c.conv[win], float(np.abs(c.conv).max()),
                               "control")


def _scale(c, conv):
    return fp.check_scale(conv.astype(np.float32), c.conv, "control")


IMAGE_HELPERS = {"image-f64": _image64, "image-f32": _image32, "correction": _correction,
                 "scale": _scale}


@pytest.mark.parametrize("name", sorted(SPECTRUM_HELPERS))
def test_spectrum_helper_controls(case, name):
    helper = SPECTRUM_HELPERS[name]
    err, bound = helper(case, case.spec)  # numpy itself
    assert err == 0.0 or name == "spectrum-f32"
    err, bound = helper(case, case.good)  # the passes with their twiddles
    assert err <= bound
    off = case.spec.copy()
    off[H // 7, 3] += 10 * bound
    with pytest.raises(AssertionError, match="control"):
        helper(case, off)
    with pytest.raises(AssertionError, match="control"):
        helper(case, case.broken)


@pytest.mark.parametrize("name", sorted(IMAGE_HELPERS))
def test_image_helper_controls(case, name):
    helper = IMAGE_HELPERS[name]
    err, bound = helper(case, case.conv)
    assert err <= bound
    err, bound = helper(case, case.image_of(case.good))
    assert err <= bound
    # the float64 image bound is per pixel (a ratio against 1): its widest term
    if name == "image-f64":
        scale = np.abs(case.conv).max() * np.sqrt(np.log2(N))
        bound = 0.5 * np.spacing(np.float32(np.abs(case.conv).max())) + 1e-12 * scale
    with pytest.raises(AssertionError, match="control"):
        helper(case, case.image_of(case.spec, bin_offset=10 * bound))
    with pytest.raises(AssertionError, match="control"):
        helper(case, case.image_of(case.broken))


def test_real_kernel_helper_controls(case):
    ref = case.kspec
    err, bound = fp.check_real_kernel(ref.real.astype(np.float32), ref, "control")
    assert err <= bound
    off = ref.real.astype(np.float32)
    off[H // 7, 3] += np.float32(10 * bound)
    with pytest.raises(AssertionError, match="control"):
        fp.check_real_kernel(off, ref, "control")
    with pytest.raises(AssertionError, match="control"):
        fp.check_real_kernel(case.kspec_broken.real.astype(np.float32), ref, "control")
    # a reference that is not real (a kernel off its centre) is refused too
    shifted = np.fft.rfft2(np.roll(fp.placed_kernel(case.shape.astype(np.float64), W, H), 1, 1))
    with pytest.raises(AssertionError, match="not real"):
        fp.check_real_kernel(shifted.real.astype(np.float32), shifted, "control")


def test_mixed_radix_dft_is_a_dft():
    rng = np.random.default_rng(5)
    for radices in ((8, 8, 4, 7), (7, 5, 5, 3), (16, 3), (2,)):
        n = int(np.prod(radices))
        x = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
        assert np.abs(fp.mixed_radix_dft(x, radices) - np.fft.fft(x, axis=0)).max() <= 1e-11
    # the first pass has no twiddles (span 1): leaving them out changes nothing
    x = rng.standard_normal((1792, 2)) + 0j
    assert np.array_equal(fp.mixed_radix_dft(x, RADICES, skip_twiddles=0),
                          fp.mixed_radix_dft(x, RADICES))


def test_peak_in_box_takes_the_first_of_equal_values():
    img = np.zeros((6, 8), np.float32)
    img[2, 3] = img[4, 2] = 5.0
    img[0, 0] = 9.0   # outside the box
    img[3, 4] = -7.0
    assert fp.peak_in_box(img, 1, 1, False) == (3, 2, 5.0)
    assert fp.peak_in_box(img, 1, 1, True) == (4, 3, -7.0)
    assert fp.peak_in_box(img, 0, 0, False) == (0, 0, 9.0)
