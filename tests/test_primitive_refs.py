"""The references of tests/primitive_refs.py, checked before they judge a kernel:
against the oracle where it has the operation, against hand-worked 3 x 3 cases
elsewhere, and the three discrimination conditions the GPU tests rest on (a
reference that could not tell the wrong kernel from the right one is no test).
CPU only."""
import math

import numpy as np
import pytest

import primitive_refs as R
from oracle_lib import get_oracle


@pytest.fixture(scope="module")
def orc():
    return get_oracle()


F = np.float32


# ------------------------------------------------------- against the oracle
@pytest.mark.parametrize("w,h,window", [(24, 30, 48), (37, 29, 5), (64, 40, 25), (9, 7, 2)])
def test_sliding_min_matches_oracle(orc, w, h, window):
    rng = np.random.default_rng(w * h + window)
    img = rng.standard_normal((h, w)).astype(F)
    assert np.array_equal(R.bits(R.sliding_min(img, window)),
                          R.bits(orc.sliding_minimum(img, window)))
    tied = np.round(img * 2) / 2 + F(0)   # no -0.0: which of two equal zeros wins is not specified
    assert np.array_equal(R.bits(R.sliding_min(tied, window)),
                          R.bits(orc.sliding_minimum(tied, window)))


@pytest.mark.parametrize("strength", [0.0, 1.0, 0.5])
def test_rms_factor_matches_oracle(orc, strength):
    rng = np.random.default_rng(11)
    rms = rng.uniform(0.1, 3.0, (17, 23)).astype(F)
    rms[3, 4] = rms[9, 0] = 0.0   # the minimum: stddev = 0 ...
    out_o, lowest_o = orc.make_rms_factor_image(rms, strength)
    out_r, lowest_r = R.rms_factor(rms, strength)
    assert lowest_r == lowest_o == 0.0
    assert R.ulp_distance(out_r.astype(F), out_o).max() <= (0 if strength != 0.5 else 1)
    rms = rng.uniform(0.1, 3.0, (17, 23)).astype(F)   # ... and a positive minimum
    out_o, lowest_o = orc.make_rms_factor_image(rms, strength)
    out_r, lowest_r = R.rms_factor(rms, strength)
    assert lowest_r == lowest_o == float(rms.min())
    assert R.ulp_distance(out_r.astype(F), out_o).max() <= (0 if strength != 0.5 else 1)
    if strength == 0.0:
        assert np.all(out_r == 1.0)
    with pytest.raises(ValueError):
        R.rms_factor(-rms, strength)


def test_integrate_matches_oracle(orc):
    rng = np.random.default_rng(12)
    images = rng.standard_normal((3, 9, 11)).astype(F)
    weights = [1.0, 2.0, 0.5]
    got = orc.integrate(images, weights)
    ref = R.integrate_linear(images, weights)
    # three float multiply-adds and the factor: a few float roundings of the terms
    tol = 8 * 2.0 ** -24 * np.tensordot(np.asarray(weights), np.abs(images), 1) / 3.5
    assert np.all(np.abs(got - ref) <= tol)


@pytest.mark.parametrize("w,h,pw,ph", [(5, 3, 8, 8), (63, 65, 64, 70), (12, 10, 12, 10)])
def test_trim_untrim_geometry_matches_oracle(orc, w, h, pw, ph):
    """Untrim, PrepareConvolutionKernel (centre (pw/2, ph/2) to the origin),
    circular convolution, Trim: with a wrong offset in either helper the PSF's
    centre, or the window, would move by a pixel."""
    rng = np.random.default_rng(w + pw)
    img = rng.standard_normal((h, w)).astype(F)
    psf = rng.standard_normal((h, w)).astype(F)
    got = orc.padded_convolution(img, psf, pw, ph)
    kernel = np.roll(R.untrim(psf, pw, ph).astype(np.float64), (-(ph // 2), -(pw // 2)), (0, 1))
    plane = R.untrim(img, pw, ph).astype(np.float64)
    conv = np.real(np.fft.ifft2(np.fft.fft2(plane) * np.fft.fft2(kernel)))
    ref = R.trim(conv, w, h)
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    shifted = np.roll(ref, 1, axis=1)
    assert np.abs(got - shifted).max() > 1e-2 * np.abs(ref).max()
    # and the two are inverse to each other, offsets rounded down
    assert np.array_equal(R.trim(R.untrim(img, pw, ph), w, h), img)
    assert R.untrim(img, pw, ph)[(ph - h) // 2, (pw - w) // 2] == img[0, 0]


# ------------------------------------------------------- hand-worked cases
A3 = np.array([[1, -2, 3], [0, 5, -6], [7, 8, -9]], F)
B3 = np.array([[2, 2, 2], [1, 0, -1], [0.5, 0.25, -1]], F)


def test_elementwise_by_hand():
    assert np.array_equal(R.axpy_assign(A3, 0.5), A3 / 2)
    assert np.array_equal(R.scale(A3, -2), [[-2, 4, -6], [0, -10, 12], [-14, -16, 18]])
    assert np.array_equal(R.add(A3, B3), [[3, 0, 5], [1, 5, -7], [7.5, 8.25, -10]])
    assert np.array_equal(R.square(A3), [[1, 4, 9], [0, 25, 36], [49, 64, 81]])
    assert np.array_equal(R.multiply(A3, B3), [[2, -4, 6], [0, 0, 6], [3.5, 2, 9]])
    assert np.array_equal(R.axpy_f64_scale(A3, 0.5), A3 / 2)
    assert np.array_equal(R.axpy_f64_unfused(B3, A3, 2.0), 2 * A3 + B3)
    assert np.array_equal(R.axpy_fused_exact(B3, A3, 0.5), A3 / 2 + B3)
    assert R.fma_f32([3.0], 0.5, [0.25])[0] == F(1.75)
    # one rounding: 1 + 2^-24 (1 + 2^-24 exactly representable product) rounds up
    # only because the low part of the product survives to the final rounding
    a, alpha, d = F(1 + 2.0 ** -12), F(1 + 2.0 ** -12), F(2.0 ** -25)
    assert R.fma_f32([a], alpha, [d])[0] == F(1 + 2.0 ** -11 + 2.0 ** -23)
    assert a * alpha + d == F(1 + 2.0 ** -11)
    assert R.convert(np.array([1e39, -1e39, 1e-46, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24]), 0).tolist() \
        == [np.inf, -np.inf, 0.0, 1.0, float(F(1 + 2.0 ** -22))]
    assert R.convert(np.array([0.1], F), 1)[0] == float(F(0.1))
    assert np.array_equal(R.integrate_linear(np.stack([A3, B3]), [1, 3]), (A3 + 3.0 * B3) / 4)


def test_masked_and_rms_steps_by_hand():
    model = np.array([[0, -0.0, 1], [np.nan, 2, 0], [0, 0, -3]], F)
    got = R.masked_copy(model, A3, -1)
    assert np.array_equal(got, [[0, 0, -3], [0, -5, 0], [0, 0, 9]])
    assert not np.signbit(got[0, 0]) and np.signbit(got[1, 0])   # 0, and -1 * 0 copied under NaN
    got = R.masked_add(model, A3)
    assert np.array_equal(got[~np.isnan(got)], [0, 0, 4, 7, 0, 0, 0, -12])
    assert np.isnan(got[1, 0]) and np.signbit(got[0, 1])
    assert np.array_equal(R.rms_finish(np.array([4, 9, 0], F), 0.25), [1, 1.5, 0])
    lim = R.rms_negativity_limit(np.array([1, 1, 3, 0.5, 2], F), np.array([-10, 10, 0, -0.0, 1], F))
    assert np.array_equal(lim, [3, 3, 3, 0.5, 2])
    eq = F(np.float64(F(7.0)) * (1.5 / 5.0))
    assert R.rms_negativity_limit([eq], [F(-7)])[0] == eq
    out, low = R.rms_factor(np.array([[2, 0, 4], [8, 2, 16], [2, 2, 2]], F) + 0, 1.0)
    assert low == 0.0 and np.all(out == 0)
    out, low = R.rms_factor(np.array([2, 4, 8], F), 1.0)
    assert low == 2.0 and out.tolist() == [1, 0.5, 0.25]
    out, low = R.rms_factor(np.array([2, 8, 32], F), 0.5)
    assert np.allclose(out, [1, 0.5, 0.25], rtol=1e-15)
    assert R.rms_factor(np.array([0, 4, 8], F), 0.0)[0].tolist() == [1, 1, 1]
    assert R.rms_factor(np.array([-0.0, 4], F), 1.0)[1] == 0.0   # -0.0 is not negative


def test_box_by_hand():
    src = np.arange(20, dtype=F).reshape(4, 5)
    dst = np.full((3, 4), -1, F)
    mask = np.array([[1, 0], [0, 1]], np.uint8)
    assert np.array_equal(R.box(dst, 1, 1, src, 2, 1, 2, 2, None, R.BOX_COPY),
                          [[-1, -1, -1, -1], [-1, 7, 8, -1], [-1, 12, 13, -1]])
    assert np.array_equal(R.box(dst, 1, 1, src, 2, 1, 2, 2, mask, R.BOX_COPY_MASKED),
                          [[-1, -1, -1, -1], [-1, 7, -1, -1], [-1, -1, 13, -1]])
    assert np.array_equal(R.box(dst, 1, 1, src, 2, 1, 2, 2, mask, R.BOX_COPY_ZERO),
                          [[-1, -1, -1, -1], [-1, 7, 0, -1], [-1, 0, 13, -1]])
    assert np.array_equal(R.box(dst, 2, 0, src, 0, 2, 2, 2, mask, R.BOX_ADD),
                          [[-1, -1, 9, 10], [-1, -1, 14, 15], [-1, -1, -1, -1]])


def test_bits_differ_by_hand():
    a = np.array([0.0, np.nan, 1.0], F)
    assert not R.bits_differ(a, a.copy())
    assert R.bits_differ(a, np.array([-0.0, np.nan, 1.0], F))
    assert not R.bits_differ(np.array([], F), np.array([], F))


def test_trim_untrim_extend_by_hand():
    s = np.array([[1, 2], [3, 4]], F)
    assert np.array_equal(R.untrim(s, 5, 3), [[0, 1, 2, 0, 0], [0, 3, 4, 0, 0], [0, 0, 0, 0, 0]])
    assert np.array_equal(R.trim(np.arange(15, dtype=F).reshape(3, 5), 2, 2), [[1, 2], [6, 7]])
    assert np.array_equal(R.periodic_extend(s, 5, 3, 1, 0),
                          [[2, 1, 2, 1, 2], [4, 3, 4, 3, 4], [2, 1, 2, 1, 2]])


def test_order_statistics_by_hand():
    v = np.array([5, -1, 3, 3, -np.inf, 0.0, -0.0, np.inf, 2], F)
    assert R.select_kth(v, 0, 0, 0) == -np.inf and R.select_kth(v, 0, 0, 8) == np.inf
    assert R.median(v, 0, 0) == 2
    assert R.median(v, 1, 3) == 3            # |v - 3| = 2 4 0 0 inf 3 3 inf 1
    assert R.median(v[:4], 0, 0) == 3 and R.median(v[:2], 1, 1) == 3   # even n: 0.5 (lo + hi)
    assert R.select_kth(v[:4], 1, 1, 3) == 4


def test_max_abs_by_hand_and_vectorised_equals_loops():
    d = np.array([[9, -9, 1], [2, -7, 7], [np.nan, 3, -np.inf]], F)
    assert R.max_abs_loops(d, 0, 0, True) == (1, 2, 2, np.inf)    # |-inf|
    assert R.max_abs_loops(d, 0, 0, False) == (1, 0, 0, 9)        # -inf and NaN never
    assert R.max_abs_loops(-d, 0, 0, False) == (1, 2, 2, np.inf)
    assert R.max_abs_loops(d[:2], 0, 0, True) == (1, 0, 0, 9)     # first of the ties 9, |-9|
    assert R.max_abs_loops(d, 1, 1, True) == (1, 1, 1, 7)
    assert R.max_abs_loops(d, 1, 1, False) == (1, 1, 1, -7)
    m = np.array([[0, 0, 0], [1, 0, 1], [1, 1, 0]], np.uint8)
    assert R.max_abs_loops(d, 0, 0, True, m) == (1, 2, 1, 7)
    assert R.max_abs_loops(d, 0, 0, True, 0 * m) == (0, 3, 3, F(R.FLT_LOWEST))
    low = np.full((3, 3), R.FLT_LOWEST, F)
    assert R.max_abs_loops(low, 0, 0, False) == (0, 3, 3, F(R.FLT_LOWEST))
    assert R.max_abs_loops(low, 0, 0, True) == (1, 0, 0, -F(R.FLT_LOWEST))
    rng = np.random.default_rng(5)
    for trial in range(40):
        h, w = rng.integers(1, 9, 2)
        a = (rng.integers(-3, 4, (h, w)) / 2).astype(F)
        for special in (np.nan, np.inf, -np.inf, R.FLT_LOWEST):
            if rng.random() < 0.3:
                a[rng.integers(h), rng.integers(w)] = special
        mask = rng.integers(0, 2, (h, w)).astype(np.uint8) if trial % 2 else None
        xb, yb = rng.integers(0, w // 2 + 1), rng.integers(0, h // 2 + 1)
        for neg in (True, False):
            assert R.max_abs(a, xb, yb, neg, mask) == R.max_abs_loops(a, xb, yb, neg, mask)


def test_iuwt_pieces_by_hand():
    c = np.stack([A3, B3])
    mask, area = R.iuwt_select(c, 0, 2, [4.0, -1.0], 0, 0)
    assert np.array_equal(mask[0], [[0, 0, 0], [0, 1, 0], [1, 1, 0]])
    assert np.array_equal(mask[1], [[1, 1, 1], [0, 0, 0], [0, 0, 0]])   # 1, -1: strict both ways
    assert area == 6
    mask, area = R.iuwt_select(c, 1, 2, [4.0, -0.5], 1, 0, prior=np.ones((3, 3)))
    assert not mask[0].any() and np.array_equal(mask[1], [[0, 1, 0], [0, 0, 0], [0, 0, 0]])
    assert area == 1
    nan = c.copy()
    nan[:, 1, 1] = np.nan
    assert R.iuwt_select(nan, 0, 2, [4.0, -1.0], 0, 0)[0][:, 1, 1].tolist() == [0, 0]
    assert np.array_equal(R.iuwt_apply_mask(A3[None], [[1, 0, 0], [0, 1, 0], [0, 0, 2]])[0],
                          [[1, 0, 0], [0, 5, 0], [0, 0, -9]])
    img = np.array([[0, 0.5, 0], [0, 0, 0], [-100, 0.5, 2]], F)   # m = 100: |v| > 1
    first, last = R.bbox_rows(img)
    assert first.tolist() == [-1, -1, 0] and last.tolist() == [-1, -1, 2]
    assert [x.tolist() for x in R.bbox_rows(np.zeros((2, 3), F))] == [[-1, -1], [-1, -1]]
    assert [x.tolist() for x in R.bbox_rows(np.zeros((2, 0), F))] == [[-1, -1], [-1, -1]]


def test_sums_by_hand():
    assert R.exact_sum(R.dot_terms(A3, B3)) == 24.5
    m, n = R.snr_terms(A3, B3)
    assert R.exact_sum(m) == 15.3125
    assert R.exact_sum(n) == float(((B3 - A3).astype(np.float64) ** 2).sum())
    # the difference is rounded to float first: 1 - 2^-30 is 1 in float
    m, n = R.snr_terms(np.array([2.0 ** -30], F), np.array([1.0], F))
    assert n[0] == 1.0
    assert R.rms(np.array([3, 4, 0, 0], F)) == F(2.5)
    assert R.reduction_tolerance([1.0, -2.0, 3.0]) == 3 * 2.0 ** -52 * 6


def test_place_gaussian_by_hand():
    g, written = R.place_gaussian(4, 5, 3, 1.0, 2.0, 1.0, 1.0, 0.0)
    e = math.exp
    # box 3, centre (1, 1) at the origin; m steps are 2 apart
    assert g[0, 0] == 1.0
    assert g[0, 1] == g[0, 3] == e(-0.5) and g[1, 0] == g[4, 0] == e(-2.0)
    assert g[1, 1] == g[4, 3] == e(-2.5)
    assert written.sum() == 9 and g[~written].sum() == 0 and g[2].sum() == 0
    # rotated by 90 degrees the axes swap: sigma_major now runs along m
    g, _ = R.place_gaussian(4, 5, 3, 1.0, 1.0, 2.0, 1.0, math.pi / 2)
    assert np.isclose(g[1, 0], e(-0.5 * 0.25), rtol=1e-15) and np.isclose(g[0, 1], e(-0.5), rtol=1e-15)


def test_spectrum_and_fft_by_hand():
    ref, tr, ti = R.spectrum_multiply(np.array([1 + 2j]), np.array([3 - 1j]), 0.5)
    assert ref[0] == 2.5 + 2.5j
    assert tr[0] == 4 * 2.0 ** -24 * 5 * 0.5 and ti[0] == 4 * 2.0 ** -24 * 7 * 0.5
    x = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert np.allclose(R.fft_inverse(np.fft.rfft2(x), 4, 3), 12 * x, atol=1e-12)


def test_model_scatter_by_hand():
    pos = np.array([(0 << 16) | 1, (2 << 16) | 0, (2 << 16) | 2], np.uint32)   # (x, y) = (1,0) (0,2) (2,2)
    vals = np.array([0.5, 0.0, 0.0], F)
    assert np.array_equal(R.model_plane(pos, vals, 4, 4, 1, 1, np.float64),
                          [[0, 0, 0, 0], [0, 0, 0.5, 0], [0, 0, 0, 0], [0, 0, 0, 0]])
    assert R.model_rows(pos, vals, 5, 1).tolist() == [0, 1, 0, 0, 0]   # row 2 holds zeros only
    dest = np.full((3, 3), 9, F)
    assert np.array_equal(R.model_masked(dest, pos, vals, [0, 1, 0, 0, 0], 1),
                          [[0, 0.5, 0], [9, 9, 9], [0, 9, 0]])
    assert np.array_equal(R.update_mask(np.eye(3), pos, np.stack([vals, [0, 0, 2]])),
                          [[1, 1, 0], [0, 1, 0], [0, 0, 1]])


# --------------------------------------------- discrimination conditions
def test_fma_inputs_tell_fused_from_unfused():
    a, alpha, dest = R.exact_fma_inputs(1 << 16)
    exact64 = a.astype(np.float64) * np.float64(alpha) + dest.astype(np.float64)
    wide = a.astype(np.longdouble) * np.longdouble(alpha) + dest.astype(np.longdouble)
    assert np.array_equal(exact64.astype(np.longdouble), wide)   # the float64 value is exact
    fused = exact64.astype(F)
    idx = np.arange(0, a.size, 257)
    assert np.array_equal(R.bits(R.fma_f32(a[idx], alpha, dest[idx])), R.bits(fused[idx]))
    assert np.array_equal(R.bits(R.axpy_fused_exact(dest, a, alpha)), R.bits(fused))
    unfused = a * alpha + dest          # two float roundings
    assert np.mean(R.bits(unfused) != R.bits(fused)) >= 0.10


def test_reduction_inputs_tell_float_from_double_accumulation():
    n = 3 * 262144 + 77
    v = np.random.default_rng(1).uniform(1.0, 2.0, n).astype(F)
    terms = R.dot_terms(v, v)
    exact, tol = R.exact_sum(terms), R.reduction_tolerance(terms)
    assert tol < 1e-3
    sequential_f32 = np.cumsum(v * v, dtype=F)[-1]
    assert abs(float(sequential_f32) - exact) > tol
    assert abs(np.sum(terms) - exact) <= tol
    assert abs(np.cumsum(terms)[-1] - exact) <= tol   # the worst order, sequential


def test_bbox_threshold_pixel_needs_the_double_compare():
    v, m = F(0.07), F(7)
    assert float(v) > float(m) * 0.01
    assert not (v > F(0.07))
    assert not (v > m * F(0.01))
    img = np.array([[7, 0, 0.07]], F)
    assert R.bbox_rows(img)[1].tolist() == [2]
