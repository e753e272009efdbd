"""The scale-0 peak search fused into the residual correction's inverse row
pass (rdl_conv_convolve_subtract_peak) against what it replaces:
rdl_conv_convolve_subtract followed by rdl_find_peak on the corrected
residual. Same inputs, so the residual is bit-identical and found / value /
x / y are identical.

Plans: 1050 (the smallest float64 compile-time row plan, 128 threads, the
gridded runs' subimage class; row-major spectrum), 4536 (a 4096^2 image,
256-thread rows, tiled spectrum) and 9072 (the 8192^2 image of the benchmark,
512-thread rows: the only class whose row kernel loads the residual row
before the transform). 1024 has no compile-time float64 rows: the call
corrects the residual, reports RDL_NOT_FUSED and leaves the peak slot alone.

The planted values dwarf the correction (a 300-component model through a
spectrum of unit-variance noise, scaled by 1 / n^2), so each case's maximum
sits where the case puts it; the two-equal-maxima and nothing-found cases use
an all-zero model, whose correction is exactly zero."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RDL_NOT_FUSED = 6
BIG = 1000.0


class Plan:
    """One conv plan with its kernel spectrum, model and base residual on the
    device, shared by the plan's cases."""

    def __init__(self, n, img):
        from rdl_lib import Session
        self.n, self.img = n, img
        self.s = s = Session(0)
        lib = s.rdl.lib
        lib.rdl_conv_convolve_subtract_bytes.restype = C.c_size_t
        lib.rdl_conv_convolve_subtract_bytes.argtypes = [C.c_void_p]
        self.c = C.c_void_p()
        s.rdl.rdl_conv_create_ex(s.h, n, n, 1, 0, C.byref(self.c))
        self.fast_rows = bool(lib.rdl_conv_fast(self.c) & 2)
        nc = n // 2 + 1
        self.work = s.array(shape=(max(lib.rdl_conv_convolve_subtract_bytes(self.c), 16),),
                            dtype=np.uint8)
        rng = np.random.default_rng(n)
        kern = np.empty((nc, n), np.complex128)  # column-major: column k at k * n
        kern.real = rng.standard_normal((nc, n), dtype=np.float32)
        kern.imag = rng.standard_normal((nc, n), dtype=np.float32)
        self.dk = s.array(kern)
        del kern
        self.ox = self.oy = (n - img) // 2
        model = np.zeros((img, img), np.float32)
        rows = rng.choice(img, 300, replace=False)
        model[rows, rng.integers(0, img, 300)] = rng.standard_normal(300).astype(np.float32)
        self.dmodel = s.array(model)
        self.dzero = s.array(np.zeros((img, img), np.float32))
        rowmask = np.zeros(n, np.uint8)
        rowmask[rows + self.oy] = 1
        self.drows = s.array(rowmask)
        self.base = rng.standard_normal((img, img), dtype=np.float32)
        self.rng = rng

    def correct(self, dr, dmodel, rowmask, peak=None):
        """The correction of device residual dr; peak = (hb, vb, allow_negative,
        dmask, avx, slot) asks for the fused search. Returns the status."""
        s, img = self.s, self.img
        args = [self.c, dmodel.vp, img, img, self.ox, self.oy, self.dk.vp, 1, 0,
                C.c_double(1.0 / (self.n * self.n)), self.drows.vp if rowmask else None,
                self.work.vp, dr.vp]
        if peak is None:
            return s.rdl.rdl_conv_convolve_subtract(*args)
        hb, vb, neg, dmask, avx, slot = peak
        rc = s.rdl.lib.rdl_conv_convolve_subtract_peak(
            *args, hb, vb, int(neg), None if dmask is None else dmask.vp, int(avx), slot)
        assert rc in (0, RDL_NOT_FUSED), s.rdl.lib.rdl_last_error().decode()
        return rc

    def collect(self, slot):
        from rdl_lib import Peak
        out = (Peak * (slot + 1))()
        self.s.rdl.rdl_find_peak_collect(self.s.h, slot + 1, out)
        p = out[slot]
        return bool(p.found), p.x, p.y, p.value

    def check(self, residual, zero_model=False, rowmask=True, hb=0, vb=0, neg=True, mask=None,
              avx=True, slot=0):
        """Fused against separate on one residual; returns the peak."""
        s, img = self.s, self.img
        dmodel = self.dzero if zero_model else self.dmodel
        dmask = None if mask is None else s.array(mask)
        d_ref, d_fused = s.array(residual), s.array(residual)
        self.correct(d_ref, dmodel, rowmask)
        want = s.find_peak(d_ref, img, img, allow_negative=neg, hb=hb, vb=vb, dmask=dmask,
                           avx=avx)
        rc = self.correct(d_fused, dmodel, rowmask, (hb, vb, neg, dmask, avx, slot))
        assert rc == 0, "this plan has compile-time rows: the search must be fused"
        got = self.collect(slot)
        ref, fused = d_ref.get(), d_fused.get()
        for d in (d_ref, d_fused, dmask):
            if d is not None:
                d.free()
        assert np.array_equal(ref.view(np.uint32), fused.view(np.uint32)), "residual differs"
        assert got[:3] == want[:3], (got, want)
        assert np.float32(got[3]).view(np.uint32) == np.float32(want[3]).view(np.uint32) or (
            np.isnan(got[3]) and np.isnan(want[3])), (got, want)
        return got, fused


_plans = {}


def plan(n, img):
    if (n, img) not in _plans:
        _plans[(n, img)] = Plan(n, img)
    return _plans[(n, img)]


# 1050: img 1000 -> ox 25 (the odd-window branch), img 1002 -> ox 24 (even);
# 4536 / 4096 -> ox 220 (even, the tiled spectrum)
SMALL = [(1050, 1000), (1050, 1002), (4536, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,img", SMALL)
def test_fused_peak_matches_separate_search(n, img):
    p = plan(n, img)
    assert p.fast_rows
    hb, vb = 7, 5
    corners = [(hb, vb), (img - hb - 1, vb), (hb, img - vb - 1), (img - hb - 1, img - vb - 1)]
    # the maximum on the first and last column and row of the box, each with a
    # larger value just outside the box; allow_negative on (a negative peak)
    # and off (the negative one must be ignored)
    for k, (x, y) in enumerate(corners):
        r = p.base.copy()
        r[y, x] = BIG
        r[y, x - 1 if x == hb else x + 1] = 2 * BIG
        r[y - 1 if y == vb else y + 1, x] = 2 * BIG
        r[img // 2, img // 2] = -1.5 * BIG
        for neg in (True, False):
            got, _ = p.check(r, hb=hb, vb=vb, neg=neg, rowmask=bool(k & 1), slot=k)
            want_xy = (img // 2, img // 2) if neg else (x, y)
            assert got[0] and (got[1], got[2]) == want_xy, (got, want_xy, neg)
    # no borders: the image's own first and last pixel
    for x, y in ((0, 0), (img - 1, img - 1)):
        r = p.base.copy()
        r[y, x] = BIG
        got, _ = p.check(r)
        assert got[0] and (got[1], got[2]) == (x, y)
    # a mask that excludes the largest value
    r = p.base.copy()
    r[10, 11] = 2 * BIG
    r[img - 9, img - 12] = BIG
    mask = np.ones((img, img), np.uint8)
    mask[10, 11] = 0
    got, _ = p.check(r, mask=mask, hb=2, vb=3)
    assert got[0] and (got[1], got[2]) == (img - 12, img - 9)
    # a NaN in the window is never selected
    r = p.base.copy()
    r[20, 21] = np.nan
    r[30, 33] = BIG
    got, fused = p.check(r)
    assert np.isnan(fused[20, 21]) and (got[1], got[2]) == (33, 30)


@pytest.mark.gpu
@pytest.mark.parametrize("n,img", SMALL)
def test_fused_peak_ties_and_nothing_found(n, img):
    p = plan(n, img)
    # two equal maxima (zero model: the correction is exactly zero, so the
    # values are written as they are): the lowest index wins, across rows
    # and inside a row
    r = p.base.copy()
    r[img - 3, 2] = BIG
    r[5, img - 4] = BIG
    got, fused = p.check(r, zero_model=True, rowmask=False)
    assert np.array_equal(fused, r)
    assert got[0] and (got[1], got[2]) == (img - 4, 5)
    r = p.base.copy()
    r[40, 100] = r[40, 7] = r[40, img - 1] = -BIG
    got, _ = p.check(r, zero_model=True, rowmask=False, neg=True)
    assert got[0] and (got[1], got[2]) == (7, 40)
    # nothing above FLT_MIN: nothing found (with the AVX semantics and no
    # mask, pixel 0 is reported, as rdl_find_peak does)
    z = np.zeros((img, img), np.float32)
    z[3, 3] = np.float32(1e-38)  # below FLT_MIN
    for avx in (True, False):
        got, _ = p.check(z, zero_model=True, rowmask=False, avx=avx)
        assert got[0] == bool(avx) and (not avx or (got[1], got[2]) == (0, 0))
    got, _ = p.check(z, zero_model=True, rowmask=False, mask=np.ones((img, img), np.uint8))
    assert not got[0]
    # only negative values with allow_negative off: nothing found either
    got, _ = p.check(-np.abs(p.base) - 1.0, zero_model=True, rowmask=False, neg=False,
                     avx=False)
    assert not got[0]
    # a border wider than half the image: an empty box
    got, _ = p.check(p.base, hb=img // 2 + 1, vb=0, avx=False)
    assert not got[0]


@pytest.mark.gpu
def test_fused_peak_on_the_benchmark_plan():
    """9072 / 8192: the 512-thread float64 rows, whose kernel loads the
    residual row before the transform."""
    n, img = 9072, 8192
    p = plan(n, img)
    assert p.fast_rows
    r = p.base
    r[img - 1, img - 1] = -BIG
    r[17, 4095] = 0.5 * BIG
    got, _ = p.check(r, hb=0, vb=0, neg=True)
    assert got[0] and (got[1], got[2]) == (img - 1, img - 1)
    got, _ = p.check(r, hb=16, vb=16, neg=False, rowmask=False, slot=2)
    assert got[0] and (got[1], got[2]) == (4095, 17)
    del _plans[(n, img)]


@pytest.mark.gpu
def test_plan_without_fast_rows_reports_not_fused():
    from rdl_lib import Session
    n, img = 1024, 1000
    p = plan(n, img)
    assert not p.fast_rows, "1024 float64 has no compile-time row plan"
    s = p.s
    # slot 1 holds a known search's result
    marker = np.zeros((8, 8), np.float32)
    marker[5, 6] = 42.0
    dmark = s.array(marker)
    s.rdl.rdl_find_peak_enqueue(s.h, dmark.vp, 8, 8, 0, 8, 0, 0, 1, None, 1, 1)
    r = p.base.copy()
    r[9, 9] = BIG
    d_ref, d_new = s.array(r), s.array(r)
    p.correct(d_ref, p.dmodel, True)
    rc = p.correct(d_new, p.dmodel, True, (0, 0, True, None, True, 1))
    assert rc == RDL_NOT_FUSED
    assert np.array_equal(d_ref.get().view(np.uint32), d_new.get().view(np.uint32))
    assert p.collect(1) == (True, 6, 5, 42.0)
