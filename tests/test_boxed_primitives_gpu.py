"""The peak search, the PSF subtraction, the image-set integration, the kernel
placement passes and the shape stamp, called directly through the C-ABI at
their edges. Cases and plain references: tests/boxed_cases.py, shown to be able
to fail by tests/test_boxed_cases.py. Every comparison is bit for bit against
the oracle, bit for bit against exact integer arithmetic, or a set of pixels;
there is no tolerance. Every device input and output lies between sentinel
guards (a finite -6e18: read as a candidate it wins any allow_negative search,
written it fails get()).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import boxed_cases as B
from boxed_peak_child import DeviceGroup, U32, peak_tuple, run_groups
from oracle_lib import get_oracle
from rdl_lib import MAX_IMAGES, RdlError, Session, integration
from test_primitives_gpu import GUARD, SZ, Guarded, HostGuarded, err_arg, free, same_bits, sentinel

pytestmark = pytest.mark.gpu

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def sess():
    s = Session(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def orc():
    return get_oracle()


# ----------------------------------------------------------------- peak search
def oracle_peak(orc, g, q):
    found, x, y, value = orc.find_peak(g.img, q.allow_negative, q.start_y, q.end_y, q.hb, q.vb,
                                       mask=g.mask_of(q), simple=not q.avx)
    return (int(found), x, y, B.bits(value))


def check_peak(orc, g, q, got):
    """`got` against the answer fixed by construction and the oracle's."""
    if q.expect is not None:
        assert B.same_peak(got, q.expect), (g.name, q, got, q.expect)
    if q.oracle:
        want = oracle_peak(orc, g, q)
        assert B.same_peak(got, want), (g.name, q, got, want)
    assert q.expect is not None or q.oracle
    if not got[0]:
        assert got[3] == 0, (g.name, q)         # nothing found: the value is +0


def run_peak_groups(sess, orc, groups):
    calls = 0
    for g in groups:
        dev = DeviceGroup(sess, g)
        for q in g.queries:
            check_peak(orc, g, q, dev.find(sess, q))
        calls += len(g.queries)
        dev.close()
    return calls


@pytest.mark.parametrize("family,calls", [("planted_vector", 488), ("planted_scalar", 340),
                                          ("planted_masked", 432)])
def test_peak_planted_box_edges(sess, orc, family, calls):
    """BIG on every corner and edge midpoint of the box, 2 * BIG just outside
    it on the same row and column, either sign, allow_negative on and off
    (boxed_cases.planted). A box 1, 3 or 5 pixels wide is impossible where
    width % 4 == 0 (width - 2 * h_border is even): the vector path has the 2-
    and 4-wide boxes, the scalar path the odd ones."""
    assert run_peak_groups(sess, orc, getattr(B, family)()) == calls


def test_peak_rows_to_workgroups(sess, orc):
    assert run_peak_groups(sess, orc, B.rows_cases()) == 12 * 8


def test_peak_special_values(sess, orc):
    assert run_peak_groups(sess, orc, B.special_cases()) == 648


def test_peak_small_shapes_exhaustively(sess, orc):
    """Every box of every image of width 1..9, 12, 16 and height 1..5, the
    whole grid: 29 344 searches, each against the oracle."""
    assert run_peak_groups(sess, orc, B.small_cases()) == 29344


def test_peak_borders_beyond_the_image(sess):
    """h_border >= width, v_border > height, start_y > height: status RDL_OK,
    the empty box's answer under each semantics, guards intact. The reference
    reads past the image there, so there is no oracle value. Before
    LaunchFindPeak clamped ye to the height ahead of the ye < ys repair,
    start_y = 2^32 - 1 with end_y = height left ye < ys, `rows` wrapped to
    height + 1 and the workgroups after the first searched the image's rows."""
    assert run_peak_groups(sess, None, B.beyond_cases()) == 3 * 17 * 6


def test_peak_deferred_slots(sess, orc):
    """All RDL_PEAK_SLOTS searches enqueued back to back (one partials buffer,
    a ticket each), one collect, slot by slot against synchronous calls; a
    collect of 3 writes 3; a second round over the same slots with other
    images (the tickets returned to 0). tests/test_deferred_result.py covers
    the loops that use the slots, not the slots themselves."""
    lib = sess.rdl
    for which in (0, 1):
        pairs = B.deferred_round(which)
        devs = {}
        for g, _ in pairs:
            if id(g) not in devs:
                devs[id(g)] = DeviceGroup(sess, g)
        sync = [devs[id(g)].find(sess, q) for g, q in pairs]
        for slot, (g, q) in enumerate(pairs):
            lib.rdl_find_peak_enqueue(sess.h, *devs[id(g)].args(q), U32(slot))
        out = HostGuarded(4 * B.PEAK_SLOTS, np.uint32)
        lib.rdl_find_peak_collect(sess.h, U32(B.PEAK_SLOTS), out.vp)
        words = out.get().reshape(B.PEAK_SLOTS, 4)
        for slot, (g, q) in enumerate(pairs):
            got = peak_tuple(words[slot])
            assert got == sync[slot], (slot, g.name, q)
            check_peak(orc, g, q, got)
        three = HostGuarded(12, np.uint32)
        lib.rdl_find_peak_collect(sess.h, U32(3), three.vp)
        np.testing.assert_array_equal(three.get().reshape(3, 4), words[:3])
        for dev in devs.values():
            dev.close()
    g, q = pairs[0]
    dev = DeviceGroup(sess, g)
    err_arg(lib.rdl_find_peak_enqueue, sess.h, *dev.args(q), U32(B.PEAK_SLOTS))
    err_arg(lib.rdl_find_peak_collect, sess.h, U32(B.PEAK_SLOTS + 1), out.vp)
    lib.rdl_find_peak_collect(sess.h, U32(0), None)
    out.get()
    dev.close()


def test_peak_two_launch_form(sess, orc, tmp_path):
    """RDL_PEAK_FINISH=0 (read once per process: one child process) gives the
    same answers as the fused finish, value for value."""
    groups = B.representative_subset()
    here = run_groups(sess, groups)
    rows = iter(here)
    for g in groups:
        for q in g.queries:
            check_peak(orc, g, q, tuple(int(v) for v in next(rows)))
    out = tmp_path / "two_launch.npy"
    child = subprocess.run([sys.executable, os.path.join(HERE, "boxed_peak_child.py"), str(out)],
                           env=dict(os.environ, RDL_PEAK_FINISH="0"), capture_output=True,
                           text=True, timeout=300)
    assert child.returncode == 0 and out.exists(), child.stderr[-4000:]
    np.testing.assert_array_equal(np.load(out), here)


# ------------------------------------------------------------- PSF subtraction
def upload_between_guards(buf, data):
    buf.dev.upload(np.concatenate([sentinel(GUARD, F), data.ravel(), sentinel(GUARD, F)]))


@pytest.mark.parametrize("w,h,comps", list(B.subtract_cases()),
                         ids=[f"{w}x{h}" for w, h, _ in B.subtract_cases()])
def test_subtract_psf(sess, orc, w, h, comps):
    """Bits against the oracle's subtract; the changed pixels are exactly the
    window of simple_clean.cc:96-131 (boxed_cases.subtract_failures)."""
    img, psf = B.subtract_images(w, h)
    dimg, dpsf = Guarded(sess, img), Guarded(sess, psf)
    for x, y, factor in comps:
        upload_between_guards(dimg, img)
        sess.rdl.rdl_subtract_psf(sess.h, dimg.vp, dpsf.vp, U32(w), U32(h), U32(x), U32(y),
                                  C.c_float(factor))
        want = img.copy()
        orc.subtract(want, psf, x, y, factor)
        assert B.subtract_failures(dimg.get((h, w)), img, want, x, y, factor) == [], (x, y, factor)
    same_bits(dpsf.get((h, w)), psf)
    free(dimg, dpsf)


def test_subtract_psf_nan_and_refusals(sess, orc):
    for w, h, x, y, factor, (px, py), inside in B.subtract_nan_cases():
        img, psf = B.subtract_images(w, h)
        psf[py, px] = np.nan
        dimg, dpsf = Guarded(sess, img), Guarded(sess, psf)
        sess.rdl.rdl_subtract_psf(sess.h, dimg.vp, dpsf.vp, U32(w), U32(h), U32(x), U32(y),
                                  C.c_float(factor))
        want = img.copy()
        orc.subtract(want, psf, x, y, factor)
        got = dimg.get((h, w))
        assert B.subtract_failures(got, img, want, x, y, factor) == []
        assert int(np.isnan(got).sum()) == int(inside)
        free(dimg, dpsf)
    img, psf = B.subtract_images(9, 7)
    dimg, dpsf = Guarded(sess, img), Guarded(sess, psf)
    for x, y in ((9, 3), (4, 7), (9, 7), (2 ** 32 - 1, 0)):
        err_arg(sess.rdl.rdl_subtract_psf, sess.h, dimg.vp, dpsf.vp, U32(9), U32(7), U32(x), U32(y),
                C.c_float(1.0))
    same_bits(dimg.get((7, 9)), img)
    free(dimg, dpsf)


# ----------------------------------------------------------------- integration
def integration_of(case):
    g = integration(case.n_ch, case.n_pol, case.weights, case.pol_factor, case.mode)
    assert g.copy_fast_path == case.copy_fast_path
    g.pol_mask = case.pol_mask
    if case.factor is not None:
        g.factor = case.factor
    return g


def oracle_integrate(orc, case):
    return orc.integrate(case.images.reshape(case.images.shape[0], 1, case.n), case.weights,
                         case.n_pol, case.pol_factor, square=case.mode == B.SQUARE,
                         squared_joins=case.mode == B.SQUARED_JOINS).ravel()


@pytest.mark.parametrize("only", [1, 255, 256, 257, B.GRID_CAP + 257, "RDL_MAX_IMAGES"])
def test_integrate(sess, orc, only):
    """Bits against orc.integrate; a partial pol_mask, which the oracle lacks,
    and the sign of a zero result against exact arithmetic
    (boxed_cases.integrate_cases)."""
    n_cases = 0
    for case in B.integrate_cases(only):
        g = integration_of(case)
        dimg, dout = Guarded(sess, case.images), Guarded(sess, n=case.n)
        sess.rdl.rdl_integrate(sess.h, C.byref(g), dimg.vp, SZ(case.n), dout.vp)
        got = dout.get()
        if case.expect is not None:
            same_bits(got, case.expect)
        if case.factor is None and case.pol_mask == (1 << case.n_pol) - 1:
            same_bits(got, oracle_integrate(orc, case))
        free(dimg, dout)
        n_cases += 1
    assert n_cases >= 4


def test_integrate_refusals(sess):
    images = np.ones((2, 10), F)
    dimg, dout = Guarded(sess, images), Guarded(sess, n=10)
    for n_images in (0, MAX_IMAGES + 1):
        g = integration(2, 1, [1.0, 1.0])
        g.n_images = n_images
        err_arg(sess.rdl.rdl_integrate, sess.h, C.byref(g), dimg.vp, SZ(10), dout.vp)
    g = integration(2, 1, [1.0, 1.0])
    sess.rdl.rdl_integrate(sess.h, C.byref(g), dimg.vp, SZ(0), dout.vp)      # RDL_OK, no write
    dout.get()
    sess.rdl.rdl_integrate(sess.h, C.byref(g), dimg.vp, SZ(10), dout.vp)
    same_bits(dout.get(), np.ones(10, F))
    free(dimg, dout)


# ------------------------------------------------- kernel placement and stamp
def psf_kernel_ref(psf, pw, ph):
    """The restatement tests/test_gpu_kernels.py::test_prepare_kernels uses."""
    h, w = psf.shape
    unt = np.zeros((ph, pw), F)
    unt[(ph - h) // 2:(ph - h) // 2 + h, (pw - w) // 2:(pw - w) // 2 + w] = psf
    return np.roll(unt, (-(ph // 2), -(pw // 2)), axis=(0, 1))


@pytest.mark.parametrize("w,h,pw,ph", [(1, 1, 1, 1), (5, 3, 8, 8), (63, 65, 64, 70), (5, 3, 5, 8),
                                       (64, 70, 64, 70),
                                       (2040, 2050, 2049, 2052)])    # past 16384 * 256
def test_prepare_psf_kernel(sess, w, h, pw, ph):
    psf = np.random.default_rng(w + ph).standard_normal((h, w)).astype(F)
    dpsf = Guarded(sess, psf)
    d32, d64 = Guarded(sess, n=pw * ph), Guarded(sess, n=pw * ph, dtype=np.float64)
    sess.rdl.rdl_prepare_psf_kernel(sess.h, d32.vp, U32(pw), U32(ph), dpsf.vp, U32(w), U32(h))
    sess.rdl.rdl_prepare_psf_kernel_f64(sess.h, d64.vp, U32(pw), U32(ph), dpsf.vp, U32(w), U32(h))
    want = psf_kernel_ref(psf, pw, ph)
    got32 = d32.get((ph, pw))
    same_bits(got32, want)
    same_bits(d64.get((ph, pw)), got32.astype(np.float64))
    dpsf.get()
    free(dpsf, d32, d64)


def test_prepare_psf_kernel_refusals(sess):
    dpsf, d32 = Guarded(sess, np.ones((4, 6), F)), Guarded(sess, n=64, dtype=np.float64)
    for pw, ph in ((5, 4), (6, 3)):
        err_arg(sess.rdl.rdl_prepare_psf_kernel, sess.h, d32.vp, U32(pw), U32(ph), dpsf.vp,
                U32(6), U32(4))
        err_arg(sess.rdl.rdl_prepare_psf_kernel_f64, sess.h, d32.vp, U32(pw), U32(ph), dpsf.vp,
                U32(6), U32(4))
    d32.get()
    free(dpsf, d32)


@pytest.mark.parametrize("n,w,h", [(1, 258, 260), (2, 258, 260), (64, 258, 260), (257, 258, 260),
                                   (1, 259, 261), (2, 259, 261), (64, 259, 261), (257, 259, 261),
                                   (1, 1, 1), (2, 2, 2), (64, 64, 64), (257, 257, 257),
                                   (2049, 2049, 2049)])     # n^2 past 16384 * 256
def test_prepare_small_kernel(sess, n, w, h):
    k = np.random.default_rng(n + w).standard_normal((n, n)).astype(F)
    d = Guarded(sess, n=w * h)
    sess.rdl.rdl_prepare_small_kernel(sess.h, d.vp, U32(w), U32(h), k.ctypes.data_as(C.c_void_p),
                                      U32(n))
    full = np.zeros((h, w), F)
    full[:n, :n] = k
    same_bits(d.get((h, w)), np.roll(full, (-(n // 2), -(n // 2)), axis=(0, 1)))
    free(d)


def test_prepare_small_kernel_refusals(sess):
    k = np.ones((9, 9), F)
    d = Guarded(sess, n=8 * 12)
    for w, h in ((8, 12), (12, 8)):
        with pytest.raises(RdlError, match="Kernel size is larger than the image size"):
            sess.rdl.rdl_prepare_small_kernel(sess.h, d.vp, U32(w), U32(h),
                                              k.ctypes.data_as(C.c_void_p), U32(9))
    d.get()
    free(d)


def add_shape_ref(img, k, x, y, gain):
    """multiscale_transforms.h:62-89 on exact inputs (an integer kernel and
    image, a power-of-two gain: the product and the sum are exact)."""
    h, w = img.shape
    n = k.shape[0]
    left = x - n // 2 if x > n // 2 else 0
    top = y - n // 2 if y > n // 2 else 0
    right, bottom = min(x + (n + 1) // 2, w), min(y + (n + 1) // 2, h)
    img[top:bottom, left:right] += k[top + n // 2 - y:bottom + n // 2 - y,
                                     left + n // 2 - x:right + n // 2 - x] * F(gain)


@pytest.mark.parametrize("w,h", [(300, 200), (40, 30)])     # the second: kernels larger than it
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 129])
def test_add_shape_component(sess, n, w, h):
    """Every corner, (1, h - 2) and the centre; at the centre of 300 x 200 the
    n = 129 window is 129 pixels wide (three 64-thread workgroups, the last
    holding one pixel)."""
    rng = np.random.default_rng(n + w)
    k = rng.integers(-8, 9, (n, n)).astype(F)
    img = rng.integers(-100, 101, (h, w)).astype(F)
    d = Guarded(sess, img)
    want = img.copy()
    places = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (1, h - 2), (w // 2, h // 2)]
    for i, (x, y) in enumerate(places):
        gain = [0.5, -2.0][i % 2]
        sess.rdl.rdl_add_shape_component(sess.h, d.vp, U32(w), U32(h), k.ctypes.data_as(C.c_void_p),
                                         U32(n), U32(x), U32(y), C.c_float(gain))
        add_shape_ref(want, k, x, y, gain)
        same_bits(d.get((h, w)), want)
    for x, y in ((w, 0), (0, h)):
        err_arg(sess.rdl.rdl_add_shape_component, sess.h, d.vp, U32(w), U32(h),
                k.ctypes.data_as(C.c_void_p), U32(n), U32(x), U32(y), C.c_float(1.0))
    same_bits(d.get((h, w)), want)
    free(d)
