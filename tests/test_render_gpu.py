"""A component list back into model images on the MI355X.

* rdl_render_components (direct, ctypes): every written pixel against the host
  SpectralFitter.evaluate — bit-equal for polynomial terms and for values,
  within 1 float ulp for log-polynomial and forced terms (both sides run
  rdl::lp::Evaluate; only the device exp may differ from libm's in the last
  double bits) — and every other pixel +0.0 whatever the planes held.
* rdl_spectrum_multiply_add against primitive_refs.spectrum_multiply.
* ComponentList.render against the float64 reference of tests/render_refs.py:
  |got - ref| <= n_nonzero_scales x RTOL x max_s max |K_s (*) |D_s||, RTOL = 1e-6
  the project's measured float32-transform bound per scale convolution.
* The list reproduces the model Perform() built:
  |render_model - model| <= (iteration_number + n_scales) x RTOL x that peak
  (every scale-transformed plane of either computation is bounded by the peak
  and carries at most RTOL of it; the float adds are two orders below).
"""
import ctypes as C
import math

import numpy as np
import pytest

import primitive_refs as P
import render_refs as R
from oracle_lib import get_oracle
from radler_import import radler as rd
from rdl_lib import Session
from synthetic import make_dirty, make_psf, make_sky, problem

pytestmark = pytest.mark.gpu

MODE = rd.SpectralFittingMode
POLYNOMIAL, LOGPOLY, FORCED, VALUES = 0, 1, 2, 3
F = np.float32
W, H = 40, 24
COUNTS = [0, 1, 63, 64, 65, 257]
# one launch of rdl_render_components covers RDL_RENDER_LANES = 256 x 1024
# components: one more goes round the grid-stride loop
LANES = 256 * 1024
BIG = LANES + 1
BIG_W, BIG_H = 520, 505  # just holds BIG distinct positions
PIXEL_SCALE = 1.0 / 3600.0 * np.pi / 180.0
SHAPES = [(0, rd.MultiscaleShape.tapered_quadratic), (1, rd.MultiscaleShape.gaussian)]


@pytest.fixture(scope="module")
def sess():
    s = Session(0)
    yield s
    s.close()


# ------------------------------------------------- rdl_render_components
def evaluation_fitter(mode):
    """evaluate() takes as many terms as it is given, whatever the fitter fits"""
    kind = MODE.polynomial if mode == POLYNOMIAL else MODE.log_polynomial
    return rd.SpectralFitter(kind, 2, list(np.linspace(100e6, 200e6, 9)), [1.0] * 9)


OUT_FREQUENCIES = [110e6, 151e6, 230e6]


def positions(rng, n, w, h):
    """n distinct pixels, the four corners first"""
    corners = [0, w - 1, (h - 1) * w, h * w - 1][:n]
    rest = np.setdiff1d(rng.permutation(w * h), corners, assume_unique=True)[:n - len(corners)]
    p = np.concatenate([np.asarray(corners, np.int64), rest]).astype(np.int64)
    return np.ascontiguousarray(np.stack([p % w, p // w]).astype(np.uint32))


def term_rows(rng, n_in, n):
    rows = np.empty((n_in, n), np.float64)
    rows[0] = rng.uniform(0.05, 3.0, n) * rng.choice([-1.0, 1.0], n)
    for k in range(1, n_in):
        rows[k] = rng.uniform(-1.5, 0.5, n) * 0.4 ** (k - 1)
    return np.ascontiguousarray(rows.astype(F))


def device_render(sess, mode, rows, xy, w, h, at, n_out, pad=0):
    """-> planes (n_out, h, w) of rdl_render_components over poisoned planes
    plane_stride = w * h + pad apart; the padding must come back untouched."""
    n = xy.shape[1]
    stride = w * h + pad
    poison = np.full((n_out, stride), np.nan, F)
    poison[:, ::3] = -77.0
    d_planes = sess.array(poison)
    d_rows = sess.array(rows if n else np.zeros(4, F))
    h_at = None if at is None else (C.c_double * len(at))(*at)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    try:
        sess.rdl.rdl_render_components(
            sess.h, C.c_uint32(mode), C.c_uint32(rows.shape[0]), d_rows.vp,
            C.c_size_t(max(n, 1)), C.c_size_t(n), ptr(xy[0]) if n else None,
            ptr(xy[1]) if n else None, C.c_uint32(w), C.c_uint32(h), h_at, C.c_uint32(n_out),
            d_planes.vp, C.c_size_t(stride))
        sess.sync()
        got = d_planes.get()
    finally:
        d_planes.free()
        d_rows.free()
    assert np.array_equal(got[:, w * h:].view(np.uint32), poison[:, w * h:].view(np.uint32))
    return got[:, :w * h].reshape(n_out, h, w)


def outputs(mode, fitter, frequencies):
    ref = fitter.reference_frequency
    if mode == POLYNOMIAL:
        return [f / ref - 1.0 for f in frequencies]
    return [math.log10(f / ref) for f in frequencies]


def numpy_fluxes(mode, rows, at):
    """The evaluation restated in numpy for whole lists: the float loop of
    SpectralFitter::Evaluate (bit for bit), or rdl::lp::Evaluate in float64
    (numpy's exp: within 1 float ulp after the rounding)."""
    out = np.empty((len(at), rows.shape[1]), F)
    for g, a in enumerate(at):
        if mode == POLYNOMIAL:
            x, value, power = F(a), rows[0].copy(), np.ones(rows.shape[1], F)
            for k in range(1, rows.shape[0]):
                power = power * x
                value = value + power * rows[k]
            out[g] = value
        else:
            e = np.zeros(rows.shape[1])
            for k in range(rows.shape[0] - 1, 0, -1):
                e = (e + rows[k].astype(np.float64)) * a
            out[g] = (rows[0].astype(np.float64) * np.exp(2.302585092994045684 * e)).astype(F)
    return out


def check_render(sess, mode, n_in, n, n_out, w=W, h=H, pad=0, sample=None):
    rng = np.random.default_rng(1000 * mode + 100 * n_in + 10 * n_out + n % 997)
    xy = positions(rng, n, w, h)
    if mode == VALUES:
        rows = np.ascontiguousarray(rng.standard_normal((n_in, n)).astype(F))
        at, frequencies, fitter = None, None, None
    else:
        rows = term_rows(rng, n_in, n)
        fitter = evaluation_fitter(mode)
        frequencies = OUT_FREQUENCIES[:n_out]
        at = outputs(mode, fitter, frequencies)
    got = device_render(sess, mode, rows, xy, w, h, at, n_out, pad)
    # every pixel not in the list is +0.0
    listed = np.zeros((h, w), bool)
    listed[xy[1], xy[0]] = True
    assert np.count_nonzero(listed) == n
    assert not np.any(got[:, ~listed].view(np.uint32))
    if n == 0:
        return
    written = got[:, xy[1], xy[0]]  # (n_out, n)
    if mode == VALUES:
        assert np.array_equal(written.view(np.uint32), rows.view(np.uint32))
        return
    whole = numpy_fluxes(mode, rows, at)
    some = np.arange(n) if sample is None or n <= sample else \
        np.sort(np.random.default_rng(7).choice(n, sample, replace=False))
    host = np.asarray([[fitter.evaluate([float(t) for t in rows[:, i]], f) for i in some]
                       for f in frequencies], F)
    assert np.all(np.isfinite(written))
    if mode == POLYNOMIAL:
        assert np.array_equal(written[:, some].view(np.uint32), host.view(np.uint32))
        assert np.array_equal(written.view(np.uint32), whole.view(np.uint32))
    else:
        ulps = np.abs(written[:, some].astype(np.float64) - host.astype(np.float64)) / \
            np.spacing(np.abs(host)).astype(np.float64)
        print(f"mode {mode}, {n_in} terms, {n} components: max {np.max(ulps):.3g} ulp from "
              f"the host, bit-equal {np.mean(ulps == 0):.4f}")
        assert np.all(ulps <= 1.0)
        assert np.all(np.abs(written.astype(np.float64) - whole.astype(np.float64)) <=
                      np.spacing(np.abs(whole)).astype(np.float64))


@pytest.mark.parametrize("mode", [POLYNOMIAL, LOGPOLY, FORCED, VALUES])
@pytest.mark.parametrize("n_out", [1, 3])
@pytest.mark.parametrize("n", COUNTS)
def test_render_components_counts(sess, mode, n_out, n):
    check_render(sess, mode, n_out if mode == VALUES else 3, n, n_out, pad=0 if n_out == 1 else 7)


@pytest.mark.parametrize("mode", [POLYNOMIAL, LOGPOLY, FORCED])
@pytest.mark.parametrize("n_in", [1, 2, 4, 8])
def test_render_components_term_counts(sess, mode, n_in):
    check_render(sess, mode, n_in, 65, 3)


def test_render_components_polynomial_with_more_terms_than_a_fit_holds(sess):
    check_render(sess, POLYNOMIAL, 12, 65, 1)


@pytest.mark.parametrize("mode", [POLYNOMIAL, LOGPOLY, FORCED, VALUES])
def test_render_components_more_than_one_grid_round(sess, mode):
    assert BIG_W * BIG_H >= BIG > LANES
    check_render(sess, mode, 3, BIG, 3, BIG_W, BIG_H, sample=1000)


# --------------------------------------------- rdl_spectrum_multiply_add
@pytest.mark.parametrize("n", [0, 1, 63, 65, 4099])
def test_spectrum_multiply_add(sess, n):
    """acc + a * b * scale: primitive_refs.spectrum_multiply's bound on the
    product, plus one float rounding of the sum."""
    rng = np.random.default_rng(n)
    cplx = lambda m: (rng.standard_normal(m) + 1j * rng.standard_normal(m)).astype(  # noqa: E731
        np.complex64)
    a, b, acc = cplx(n), cplx(n), cplx(n + 4)  # 4 guard elements behind the n
    scale = F(1.0 / 3.25)
    d_a = sess.array(a.view(F) if n else np.zeros(4, F))
    d_b = sess.array(b.view(F) if n else np.zeros(4, F))
    d_acc = sess.array(acc.view(F))
    sess.rdl.rdl_spectrum_multiply_add(sess.h, d_acc.vp, d_a.vp, d_b.vp, C.c_size_t(n),
                                       C.c_float(scale))
    sess.sync()
    got = d_acc.get().view(np.complex64)
    for d in (d_a, d_b, d_acc):
        d.free()
    assert np.array_equal(got[n:].view(np.uint32), acc[n:].view(np.uint32))
    product, tol_re, tol_im = P.spectrum_multiply(a, b, scale)
    want = acc[:n].astype(np.complex128) + product
    got = got[:n].astype(np.complex128)
    assert np.all(np.abs(got.real - want.real) <= tol_re + 2.0 ** -24 * (np.abs(want.real) + tol_re))
    assert np.all(np.abs(got.imag - want.imag) <= tol_im + 2.0 ** -24 * (np.abs(want.imag) + tol_im))


# ------------------------------------------------- ComponentList.render
SCALES = [0.0, 4.0, 9.0]
LIST_FREQUENCIES = [1.0e8, 1.2e8, 1.4e8]
NO_FIT = rd.SpectralFitter(MODE.no_fitting, 0, [], [])


def make_list(w, h, seed, amplitudes_of_both_signs=True):
    """~40 components over three scales with power-law spectra at the three
    list frequencies: a corner, both sides of every edge within a kernel's
    radius, the rest anywhere."""
    rng = np.random.default_rng(seed)
    cl = rd.ComponentList(w, h, len(SCALES), len(LIST_FREQUENCIES))
    f = np.asarray(LIST_FREQUENCIES) / 1.2e8
    edge = [(0, 0), (w - 1, h - 1), (1, h // 2), (w - 2, h // 3), (w // 2, 1), (w // 3, h - 2),
            (w - 1, 0), (3, h - 1)]
    for s in range(len(SCALES)):
        p = positions(rng, 10, w, h)[:, 4:].T.tolist() + [list(e) for e in edge]
        seen = set()
        for x, y in p:
            if (x, y) in seen:
                continue
            seen.add((x, y))
            amp = rng.uniform(0.05, 2.0) * (rng.choice([-1.0, 1.0])
                                            if amplitudes_of_both_signs else 1.0)
            values = amp * f ** rng.uniform(-1.5, 0.5) * (1.0 + 0.01 * rng.standard_normal(3))
            cl.add(int(x), int(y), s, [float(v) for v in values.astype(F)])
    cl.merge_duplicates()
    return cl


def render_reference(cl, w, h, shape_index):
    kernels = R.shape_kernels(get_oracle(), SCALES, w, h, shape_index)
    return R.render(w, h, kernels, R.lists_of(cl))


@pytest.mark.parametrize("w,h", [(64, 48), (74, 58)])
@pytest.mark.parametrize("shape_index,shape", SHAPES)
def test_render_values_against_the_float64_reference(w, h, shape_index, shape):
    cl = make_list(w, h, seed=w + shape_index)
    assert sum(cl.component_count(s) for s in range(3)) >= 28
    assert all(cl.component_count(s) for s in range(3))
    ref, peak = render_reference(cl, w, h, shape_index)
    bound = 2 * R.RTOL * peak  # two non-zero scales
    fitter = rd.SpectralFitter(MODE.polynomial, 2, LIST_FREQUENCIES, [1.0, 2.0, 1.5])
    got = cl.render(fitter, SCALES, [], shape)
    assert got.shape == (3, h, w) and got.dtype == F
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print(f"render {w}x{h} shape {shape_index}: max |got - ref| = {err:.3g} = "
          f"{err / peak:.3g} x peak, bound {bound:.3g} = {2 * R.RTOL:.3g} x peak")
    assert err <= bound
    # the list's own values need no fitter that fits
    assert np.array_equal(cl.render(NO_FIT, SCALES, [], shape), got)


def forced_plane(w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return (-1.0 + 0.01 * xx + 0.02 * yy).astype(F)


@pytest.mark.parametrize("w,h", [(64, 48), (74, 58)])
@pytest.mark.parametrize("mode,n_terms", [(MODE.polynomial, 2), (MODE.log_polynomial, 3),
                                          (MODE.forced_terms, 2)])
def test_render_at_requested_frequencies(w, h, mode, n_terms):
    """Planes at frequencies outside the list's own equal the values render of
    a list whose values are fitter.evaluate(fit_terms, nu): the spectral step
    apart from the convolution. The bound: the two renders' transforms (RTOL
    per non-zero scale of the peak), and 1 float ulp of every component's flux
    carried through the kernels (2^-23 of the same peak at most)."""
    nus = [0.8e8, 1.7e8]
    cl = make_list(w, h, seed=7, amplitudes_of_both_signs=mode == MODE.polynomial)
    fitter = rd.SpectralFitter(mode, n_terms, LIST_FREQUENCIES, [1.0, 2.0, 1.5])
    if mode == MODE.forced_terms:
        fitter.set_forced_terms([forced_plane(w, h)])
    evaluated = rd.ComponentList(w, h, len(SCALES), len(nus))
    for s in range(len(SCALES)):
        terms = cl.fit_terms(s, fitter, device=True)
        assert terms.shape == (cl.component_count(s), n_terms)
        for (x, y), t in zip(cl.get_positions(s), terms):
            evaluated.add(x, y, s, [fitter.evaluate([float(v) for v in t], nu) for nu in nus])
    evaluated.merge_duplicates()
    shape_index, shape = SHAPES[0]
    want = evaluated.render(NO_FIT, SCALES, [], shape)
    got = cl.render(fitter, SCALES, nus, shape)
    assert got.shape == want.shape == (2, h, w)
    _, peak = render_reference(evaluated, w, h, shape_index)
    bound = (2 * R.RTOL + 2.0 ** -23) * peak
    err = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))))
    print(f"render at 2 frequencies, {mode}, {w}x{h}: max |got - want| = {err:.3g} = "
          f"{err / peak:.3g} x peak, bound {bound:.3g}")
    assert err <= bound
    assert np.max(np.abs(want)) > 0.1  # something was rendered


def test_render_single_frequency_list_is_the_same_at_every_frequency():
    w, h = 64, 48
    cl = rd.ComponentList(w, h, 2, 1)
    for x, y, s, v in [(0, 0, 0, 1.5), (w - 1, h - 1, 1, 2.0), (5, 7, 1, 0.25)]:
        cl.add(x, y, s, [v])
    cl.merge_duplicates()
    shape = rd.MultiscaleShape.tapered_quadratic
    own = cl.render(NO_FIT, [0.0, 4.0], [], shape)
    at = cl.render(NO_FIT, [0.0, 4.0], [0.9e8, 3.0e8], shape)
    assert own.shape == (1, h, w) and at.shape == (2, h, w)
    assert np.array_equal(at[0], own[0]) and np.array_equal(at[1], own[0])
    assert own[0, 0, 0] > 1.5  # the point, plus the wrapped corner of the scale-4 source


# ------------------------------------------- the list reproduces the model
def cleaned(w, psf, residual, model, n_channels=1, minor_iteration_count=60):
    s = rd.Settings()
    s.algorithm_type = rd.AlgorithmType.multiscale
    s.trimmed_image_width = s.trimmed_image_height = w
    s.pixel_scale.x = s.pixel_scale.y = PIXEL_SCALE
    s.minor_iteration_count = minor_iteration_count
    s.absolute_threshold = 5e-3
    s.border_ratio = 0.0
    s.save_source_list = True
    s.parallel.max_threads = 1
    s.multiscale.max_scales = 4
    s.multiscale.fast_sub_minor_loop = True
    if n_channels == 1:
        r = rd.Radler(s, psf, residual, model, 2.0 * PIXEL_SCALE)
    else:
        s.spectral_fitting.mode = MODE.polynomial
        s.spectral_fitting.terms = 2
        freqs = np.array([[1.0e8 + 2e7 * k, 1.2e8 + 2e7 * k] for k in range(n_channels)])
        r = rd.Radler(s, psf, residual, model, 2.0 * PIXEL_SCALE, n_channels, freqs,
                      np.array([1.0, 2.0, 1.5]))
    r.perform(0)
    return r


def check_list_reproduces_model(r, model, w, minor_iteration_count=60):
    cl = r.component_list
    model = model.reshape(-1, w, w)
    n_scales = cl.n_scales
    assert 1 <= r.iteration_number <= minor_iteration_count
    assert sum(cl.component_count(s) for s in range(n_scales)) >= 3
    print("components per scale:", [cl.component_count(s) for s in range(n_scales)],
          "scale sizes:", r.scale_sizes)
    got = cl.render_model(r)
    assert got.shape == model.shape
    kernels = R.shape_kernels(get_oracle(), r.scale_sizes, w, w, 0)
    _, peak = R.render(w, w, kernels, R.lists_of(cl))
    bound = (r.iteration_number + n_scales) * R.RTOL * peak
    for g in range(len(model)):
        err = float(np.max(np.abs(got[g].astype(np.float64) - model[g].astype(np.float64))))
        print(f"list -> model, plane {g} of {len(model)}: max |render - model| = {err:.3g} = "
              f"{err / peak:.3g} x peak, bound {bound:.3g} ({r.iteration_number} iterations, "
              f"{n_scales} scales, max |model| {np.max(np.abs(model[g])):.3g})")
        assert err <= bound
    assert np.max(np.abs(model)) > 100 * bound  # the statement is not empty


@pytest.mark.parametrize("minor_iteration_count", [60, 800])
def test_list_reproduces_the_model_of_perform(minor_iteration_count):
    """60 iterations: few `model +=` steps, a tight bound. 800 (the run of
    tests/test_multiscale_component_list.py): components of several scales."""
    w = 128
    psf, dirty = problem(w, w, 25, 3, seed=8, noise=1e-3)
    residual, model = dirty.copy(), np.zeros_like(dirty)
    r = cleaned(w, psf, residual, model, minor_iteration_count=minor_iteration_count)
    check_list_reproduces_model(r, model, w, minor_iteration_count)
    if minor_iteration_count == 800:
        cl = r.component_list
        assert sum(1 for s in range(1, cl.n_scales) if cl.component_count(s)) >= 2


def test_list_reproduces_every_channel_of_a_joined_run():
    w, n_ch = 64, 3
    psf = make_psf(w, w)
    sky = make_sky(w, w, 3, 0, seed=21) + \
        make_sky(w, w, 0, 2, seed=22, flux_range=(0.5, 1.0), blob_sigma=(3.0, 5.0))
    dirty = make_dirty(psf, sky, 1e-3, seed=21)
    rng = np.random.default_rng(21)
    dirties = np.stack([dirty * F(1.0 + 0.15 * k) + F(1e-3) *
                        rng.standard_normal((w, w)).astype(F) for k in range(n_ch)]).astype(F)
    psfs, models = np.stack([psf] * n_ch), np.zeros_like(dirties)
    r = cleaned(w, psfs, dirties, models, n_ch)
    assert r.component_list.n_frequencies == n_ch
    check_list_reproduces_model(r, models, w)
