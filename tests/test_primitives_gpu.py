"""Every streaming primitive of include/rdl_hip.h, called directly through the
C-ABI at the sizes where a grid-stride kernel takes another path: one element,
one workgroup +-1, and cap * 256 + 257 elements for a kernel launched with at
most `cap` workgroups of 256 (second trip of the loop, partial last trip).

References are tests/primitive_refs.py (checked by tests/test_primitive_refs.py).
Bit-exact unless a test states a derived tolerance. Every output buffer has 64
elements of sentinel on each side, which must be unchanged afterwards.
"""
import ctypes as C

import numpy as np
import pytest

import primitive_refs as R
from oracle_lib import get_oracle
from rdl_lib import Peak, RdlError, Session, SubminorParams, SubminorResult, integration

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64
SENTINEL = {1: 0xA5, 4: 0xDEADBEEF, 8: 0xDEADBEEFDEADBEEF}   # a finite negative float / double
UINT = {1: np.uint8, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def sess():
    s = Session(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def orc():
    return get_oracle()


def sentinel(n, dtype):
    size = np.dtype(dtype).itemsize
    return np.full(n, SENTINEL[size], UINT[size]).view(dtype)


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def same_bits(got, want):
    np.testing.assert_array_equal(raw(got), raw(np.asarray(want, got.dtype)))


class Guarded:
    """A device buffer of n elements between two guards of GUARD sentinel
    elements; `data` (any shape, n elements) or sentinels fill the body."""

    def __init__(self, sess, data=None, n=None, dtype=F):
        if data is not None:
            data = np.ascontiguousarray(data)
            dtype, n = data.dtype, data.size
        self.n, self.dtype = n, np.dtype(dtype)
        host = sentinel(n + 2 * GUARD, dtype)
        if data is not None:
            host[GUARD:GUARD + n] = data.ravel()
        self.dev = sess.array(host)

    def at(self, elements=0):
        return C.c_void_p(self.dev.ptr + (GUARD + elements) * self.dtype.itemsize)

    @property
    def vp(self):
        return self.at(0)

    def get(self, shape=None):
        host = self.dev.get()
        want = sentinel(GUARD, self.dtype)
        same_bits(host[:GUARD], want)
        same_bits(host[GUARD + self.n:], want)
        body = host[GUARD:GUARD + self.n]
        return body if shape is None else body.reshape(shape)

    def free(self):
        self.dev.free()


class HostGuarded:
    """The same for an output the entry point writes to host memory."""

    def __init__(self, n, dtype):
        self.n = n
        self.host = sentinel(n + 2 * GUARD, dtype)

    @property
    def vp(self):
        return C.c_void_p(self.host.ctypes.data + GUARD * self.host.dtype.itemsize)

    def get(self):
        want = sentinel(GUARD, self.host.dtype)
        same_bits(self.host[:GUARD], want)
        same_bits(self.host[GUARD + self.n:], want)
        return self.host[GUARD:GUARD + self.n]


def free(*buffers):
    for b in buffers:
        b.free()


def sizes(cap):
    return [1, 255, 256, 257, cap * 256 + 257]


def err_arg(fn, *args):
    with pytest.raises(RdlError, match="rc=1:"):
        fn(*args)


SZ = C.c_size_t

# ---------------------------------------------------------------- elementwise
@pytest.mark.parametrize("n", sizes(8192))
def test_axpy_assign(sess, n):
    a = np.random.default_rng(n).standard_normal(n).astype(F)
    alpha = F(0.3)
    da, dd = Guarded(sess, a), Guarded(sess, n=n)
    sess.rdl.rdl_axpy(sess.h, dd.vp, da.vp, SZ(n), C.c_float(alpha), 1)
    same_bits(dd.get(), R.axpy_assign(a, alpha))
    free(da, dd)


@pytest.mark.parametrize("n", sizes(8192))
def test_axpy_fused(sess, n):
    """One rounding per element: inputs whose fused result is known exactly and
    differs from multiply-then-add in more than a quarter of the elements."""
    a, alpha, dest = R.exact_fma_inputs(n, seed=n)
    da, dd = Guarded(sess, a), Guarded(sess, dest)
    sess.rdl.rdl_axpy(sess.h, dd.vp, da.vp, SZ(n), C.c_float(alpha), 0)
    same_bits(dd.get(), R.axpy_fused_exact(dest, a, alpha))
    free(da, dd)


@pytest.mark.parametrize("n", sizes(8192))
def test_scale(sess, n):
    d = np.random.default_rng(n).standard_normal(n).astype(F)
    dd = Guarded(sess, d)
    sess.rdl.rdl_scale(sess.h, dd.vp, SZ(n), C.c_float(F(-1.7)))
    same_bits(dd.get(), R.scale(d, F(-1.7)))
    free(dd)


VEC_SIZES = [1, 3, 4, 5, 1027, 8389635]   # n / 4 + 1 vectors: 8192 * 256 + 257 for the last


@pytest.mark.parametrize("misaligned", [None, "dest", "a"])
@pytest.mark.parametrize("n", VEC_SIZES)
def test_add(sess, n, misaligned):
    """The float4 body + scalar tail (both pointers 16-byte aligned) and the
    scalar kernel (one pointer 4 bytes off)."""
    rng = np.random.default_rng(n)
    d, a = rng.standard_normal(n + 1).astype(F), rng.standard_normal(n + 1).astype(F)
    dd, da = Guarded(sess, d), Guarded(sess, a)
    od, oa = int(misaligned == "dest"), int(misaligned == "a")
    assert dd.vp.value % 16 == 0 and da.vp.value % 16 == 0
    sess.rdl.rdl_add(sess.h, dd.at(od), da.at(oa), SZ(n))
    want = d.copy()
    want[od:od + n] = R.add(d[od:od + n], a[oa:oa + n])
    same_bits(dd.get(), want)
    free(dd, da)


@pytest.mark.parametrize("n", sizes(8192))
def test_axpy_f64_scale(sess, n):
    d = np.random.default_rng(n).standard_normal(n).astype(F)
    dd = Guarded(sess, d)
    sess.rdl.rdl_axpy_f64(sess.h, dd.vp, None, SZ(n), C.c_double(0.1), 1)
    same_bits(dd.get(), R.axpy_f64_scale(d, 0.1))
    free(dd)


@pytest.mark.parametrize("n", sizes(8192))
def test_axpy_f64_fused(sess, n):
    """float(fma(double(a), 0.1, double(dest))): exact on 4096 sampled elements
    (first, last, both sides of the cap boundary, the tail); the whole array
    within 1 float32 ulp of the form with the product rounded to double first,
    which is one float64 rounding away."""
    rng = np.random.default_rng(n)
    a, d = rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)
    da, dd = Guarded(sess, a), Guarded(sess, d)
    sess.rdl.rdl_axpy_f64(sess.h, dd.vp, da.vp, SZ(n), C.c_double(0.1), 0)
    got = dd.get()
    cap = 8192 * 256
    fixed = [0, n - 1, cap - 1, cap, cap + 1] + list(range(n - 257, n))
    idx = np.unique(np.concatenate([np.array([i for i in fixed if 0 <= i < n]),
                                    rng.integers(0, n, 4096 - 262)]))
    same_bits(got[idx], R.fma_f32(a[idx], 0.1, d[idx]))
    assert R.ulp_distance(got, R.axpy_f64_unfused(d, a, 0.1)).max() <= 1
    free(da, dd)


CONVERT_SPECIALS = np.array([
    3.5e38, -3.5e38, 1e39, -1e39,                       # round to +-inf
    np.finfo(F).max, float(np.finfo(F).max) * (1 + 2.0 ** -26),   # just inside / rounds to max
    float(np.finfo(F).max) * (1 + 2.0 ** -25) * (1 + 2.0 ** -30),   # beyond the last tie: inf
    1e-40, -1e-40, 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * 1.0000001, 2.0 ** -151,   # subnormals
    1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, -(1 + 2.0 ** -24),   # ties
    0.0, -0.0, np.inf, -np.inf])


@pytest.mark.parametrize("n", sizes(4096))
def test_convert(sess, n):
    rng = np.random.default_rng(n)
    f = rng.standard_normal(n).astype(F)
    df, dout = Guarded(sess, f), Guarded(sess, n=n, dtype=np.float64)
    sess.rdl.rdl_convert(sess.h, df.vp, dout.vp, SZ(n), 1)
    same_bits(dout.get(), R.convert(f, 1))
    d = rng.standard_normal(n) * 1e3
    k = min(n, CONVERT_SPECIALS.size)
    d[:k] = CONVERT_SPECIALS[:k]
    d[n - k:] = CONVERT_SPECIALS[:k][::-1]
    dsrc, dback = Guarded(sess, d), Guarded(sess, n=n, dtype=F)
    sess.rdl.rdl_convert(sess.h, dsrc.vp, dback.vp, SZ(n), 0)
    with np.errstate(over="ignore", under="ignore"):
        same_bits(dback.get(), R.convert(d, 0))
    free(df, dout, dsrc, dback)


BOX_SHAPES = [(1, 1), (257, 3), (2049, 2049)]   # 2049^2 > 16384 * 256


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("op", [R.BOX_COPY, R.BOX_COPY_MASKED, R.BOX_COPY_ZERO, R.BOX_ADD])
@pytest.mark.parametrize("w,h", BOX_SHAPES)
def test_box(sess, w, h, op, masked):
    rng = np.random.default_rng(w * 7 + op)
    src_w, src_x, src_y = w + 5, 3, 2
    dst_w, dst_x, dst_y = w + 3, 2, 1
    src = rng.standard_normal((h + 3, src_w)).astype(F)
    dst = sentinel((h + 3) * dst_w, F).reshape(h + 3, dst_w)
    if op == R.BOX_ADD:
        dst[dst_y:dst_y + h, dst_x:dst_x + w] = rng.standard_normal((h, w)).astype(F)
    mask = (rng.random((h, w)) < 0.5).astype(np.uint8) if masked else None
    if masked and w * h > 1:
        mask.ravel()[[0, -1]] = [1, 0]
    ds, dd = Guarded(sess, src), Guarded(sess, dst)
    dm = Guarded(sess, mask) if masked else None
    sess.rdl.rdl_box(sess.h, dd.vp, dst_w, dst_x, dst_y, ds.vp, src_w, src_x, src_y, w, h,
                     dm.vp if masked else None, op)
    same_bits(dd.get(dst.shape), R.box(dst, dst_x, dst_y, src, src_x, src_y, w, h, mask, op))
    free(ds, dd)
    if masked:
        dm.free()


# odd differences; (2049 x 2052) and (2050 x 2049) exceed 16384 * 256
TRIM_SHAPES = [(1, 1, 1, 1), (5, 3, 8, 8), (63, 65, 64, 70), (2040, 2050, 2049, 2052),
               (2050, 2049, 2053, 2050)]


@pytest.mark.parametrize("w,h,pw,ph", TRIM_SHAPES)
def test_untrim_trim(sess, w, h, pw, ph):
    rng = np.random.default_rng(w + ph)
    img = rng.standard_normal((h, w)).astype(F)
    dimg, dpad = Guarded(sess, img), Guarded(sess, n=pw * ph)
    sess.rdl.rdl_untrim(sess.h, dpad.vp, pw, ph, dimg.vp, w, h)
    same_bits(dpad.get((ph, pw)), R.untrim(img, pw, ph))
    free(dimg, dpad)
    pad = rng.standard_normal((ph, pw)).astype(F)
    dpad, dout = Guarded(sess, pad), Guarded(sess, n=w * h)
    sess.rdl.rdl_trim(sess.h, dout.vp, w, h, dpad.vp, pw, ph)
    same_bits(dout.get((h, w)), R.trim(pad, w, h))
    free(dpad, dout)


@pytest.mark.parametrize("w,h,pw,ph,sx,sy", [(1, 1, 1, 1, 0, 0), (5, 3, 12, 9, 2, 1),
                                              (250, 90, 300, 120, 25, 15), (40, 30, 257, 64, 47, 33)])
def test_periodic_extend(sess, w, h, pw, ph, sx, sy):
    img = np.random.default_rng(pw).standard_normal((h, w)).astype(F)
    dimg, dout = Guarded(sess, img), Guarded(sess, n=pw * ph)
    sess.rdl.rdl_periodic_extend(sess.h, dout.vp, pw, ph, dimg.vp, w, h, sx, sy)
    same_bits(dout.get((ph, pw)), R.periodic_extend(img, pw, ph, sx, sy))
    # an empty destination launches nothing
    sess.rdl.rdl_periodic_extend(sess.h, dout.vp, 0, ph, dimg.vp, w, h, sx, sy)
    sess.rdl.rdl_periodic_extend(sess.h, dout.vp, pw, 0, dimg.vp, w, h, sx, sy)
    dout.get()
    free(dimg, dout)


# ---------------------------------------------------------------- bit compare
def differ(sess, a, b, nbytes, first):
    sess.rdl.rdl_bits_differ_enqueue(sess.h, a, b, SZ(nbytes), first)


def collect(sess):
    out = C.c_int(-1)
    sess.rdl.rdl_bits_differ_collect(sess.h, C.byref(out))
    return out.value


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("n", VEC_SIZES)
def test_bits_differ(sess, n, misaligned):
    """The uint4 body + word tail (both pointers 16-byte aligned) and the
    word-only path (a 4 bytes off); one differing word first, last, as the last
    word of the vector part and as the first word of the tail."""
    rng = np.random.default_rng(n)
    off = int(misaligned)
    a_words = rng.integers(0, 2 ** 32, n + 1, dtype=np.uint32)
    a_words[[off, off + n - 1]] = 0x7fc00123      # equal NaN patterns do not differ
    b_words = np.roll(a_words, -off)              # b[i] = a[i + off]
    da, db = Guarded(sess, a_words), Guarded(sess, b_words)
    assert da.vp.value % 16 == 0 and db.vp.value % 16 == 0
    pa, pb = da.at(off), db.at(0)
    differ(sess, pa, pb, 4 * n, 1)
    assert collect(sess) == 0
    positions = {0, n - 1, max(0, (n // 4) * 4 - 1), min(n - 1, (n // 4) * 4)}
    for p in sorted(positions):
        keep = b_words[p:p + 1].copy()
        other = keep ^ np.uint32(1 << (p % 32))
        hp = db.at(p)
        sess.rdl.rdl_memcpy_h2d(sess.h, hp, other.ctypes.data_as(C.c_void_p), SZ(4))
        differ(sess, pa, pb, 4 * n, 1)
        assert collect(sess) == 1, p
        sess.rdl.rdl_memcpy_h2d(sess.h, hp, keep.ctypes.data_as(C.c_void_p), SZ(4))
    differ(sess, pa, pb, 4 * n, 1)
    assert collect(sess) == 0
    same_bits(db.get(), b_words)
    free(da, db)


def test_bits_differ_zero_signs_chain_and_empty(sess):
    n = 1027
    a = np.random.default_rng(3).standard_normal(n).astype(F)
    a[5] = 0.0
    b = a.copy()
    b[5] = -0.0
    da, da2, db = Guarded(sess, a), Guarded(sess, a), Guarded(sess, b)
    differ(sess, da.vp, db.vp, 4 * n, 1)
    assert collect(sess) == 1               # +0.0 against -0.0
    differ(sess, da.vp, da2.vp, 4 * n, 1)
    differ(sess, da.vp, db.vp, 4 * n, 0)
    differ(sess, da.vp, da2.vp, 4 * n, 0)
    assert collect(sess) == 1               # the chain accumulates
    differ(sess, da.vp, da2.vp, 4 * n, 1)
    assert collect(sess) == 0               # a new first = 1 clears it
    differ(sess, da.vp, db.vp, 0, 1)
    assert collect(sess) == 0               # no bytes: nothing differs
    differ(sess, da.vp, db.vp, 4 * n, 1)
    differ(sess, da.vp, db.vp, 0, 0)
    assert collect(sess) == 1               # ... and nothing is cleared
    free(da, da2, db)


# ------------------------------------------------------------------ local RMS
@pytest.mark.parametrize("n", sizes(8192))
def test_square_multiply(sess, n):
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)
    da, db, dout = Guarded(sess, a), Guarded(sess, b), Guarded(sess, n=n)
    sess.rdl.rdl_square(sess.h, da.vp, dout.vp, SZ(n))
    same_bits(dout.get(), R.square(a))
    sess.rdl.rdl_multiply(sess.h, dout.vp, da.vp, db.vp, SZ(n))
    same_bits(dout.get(), R.multiply(a, b))
    free(da, db, dout)


@pytest.mark.parametrize("n", sizes(8192))
def test_rms_finish(sess, n):
    d = np.random.default_rng(n).uniform(0, 50, n).astype(F)
    d[0] = 0.0
    dd = Guarded(sess, d)
    norm = 1.0 / 37.3
    sess.rdl.rdl_rms_finish(sess.h, dd.vp, SZ(n), C.c_double(norm))
    same_bits(dd.get(), R.rms_finish(d, norm))
    free(dd)


@pytest.mark.parametrize("n", sizes(8192))
def test_rms_negativity_limit(sess, n):
    rng = np.random.default_rng(n)
    rms = rng.uniform(0, 1, n).astype(F)
    mn = (rng.standard_normal(n) * 2).astype(F)          # negative, positive ...
    mn[rng.random(n) < 0.1] = 0.0                        # ... and zero minima
    eq = rng.random(n) < 0.2                             # rms == lim exactly
    rms[eq] = (np.abs(mn[eq]).astype(np.float64) * (1.5 / 5.0)).astype(F)
    if n > 1:
        mn[-1], rms[-1] = -0.0, 0.0
    drms, dmn = Guarded(sess, rms), Guarded(sess, mn)
    sess.rdl.rdl_rms_negativity_limit(sess.h, drms.vp, dmn.vp, SZ(n))
    same_bits(drms.get(), R.rms_negativity_limit(rms, mn))
    free(drms, dmn)


@pytest.mark.parametrize("zeros", [False, True])
@pytest.mark.parametrize("strength", [1.0, 0.0, 0.5])
@pytest.mark.parametrize("n", sizes(8192))
def test_rms_factor(sess, n, strength, zeros):
    """Strengths 1 and 0 bit-exact; 0.5 within 1 float32 ulp of
    float(pow(stddev / double(v), 0.5)) (the device pow in double is good to a
    few double ulp). With zeros in the image the minimum, and so every factor
    of a non-zero pixel, is 0; the zeros stay zero unless strength is 0."""
    rng = np.random.default_rng(n)
    img = rng.uniform(0.25, 9.0, n).astype(F)
    if zeros:
        img[rng.random(n) < 0.2] = 0.0
        img[0] = 0.0
    d = Guarded(sess, img)
    lowest = C.c_double(-1)
    sess.rdl.rdl_rms_factor(sess.h, d.vp, SZ(n), C.c_double(strength), C.byref(lowest))
    want, low = R.rms_factor(img, strength)
    assert lowest.value == low == float(img.min())
    got = d.get()
    if strength == 0.5:
        assert R.ulp_distance(got, want.astype(F)).max() <= 1
    else:
        same_bits(got, want.astype(F))
    if strength != 0.0:
        same_bits(got[img == 0], np.zeros(int((img == 0).sum()), F))
    else:
        same_bits(got, np.ones(n, F))
    free(d)


def test_rms_factor_negative_input(sess):
    img = np.random.default_rng(2).uniform(0.25, 9.0, 1000).astype(F)
    img[777] = -0.125
    d = Guarded(sess, img)
    lowest = C.c_double(0)
    err_arg(sess.rdl.rdl_rms_factor, sess.h, d.vp, SZ(1000), C.c_double(1.0), C.byref(lowest))
    assert lowest.value == -0.125
    d.get()
    free(d)


@pytest.mark.parametrize("w,h,boxsize", [(8, 8, 1), (33, 20, 7), (64, 64, 64), (300, 200, 151)])
def test_place_gaussian(sess, w, h, boxsize):
    """Unequal pixel scales and a rotated beam. Outside the wrapped box exactly
    0; inside within 1 float32 ulp of the float64 value (the device exp in
    double is good to a few double ulp, which moves a float rounding by at
    most one)."""
    pl, pm, angle = 1.0, 1.5, 0.6
    smaj, smin = max(boxsize / 4.0, 1.0), max(boxsize / 6.0, 0.8)
    d = Guarded(sess, n=w * h)
    sess.rdl.rdl_place_gaussian(sess.h, d.vp, w, h, boxsize, C.c_double(pl), C.c_double(pm),
                                C.c_double(smaj), C.c_double(smin), C.c_double(angle))
    got = d.get((h, w))
    want, written = R.place_gaussian(w, h, boxsize, pl, pm, smaj, smin, angle)
    same_bits(got[~written], np.zeros(int((~written).sum()), F))
    assert R.ulp_distance(got[written], want[written].astype(F)).max() <= 1
    assert got[0, 0] == 1.0
    free(d)


@pytest.mark.parametrize("w,h,window", [(24, 30, 48),       # window / 2 == width
                                         (1500, 1400, 25)])  # beyond 8192 * 256 pixels
def test_sliding_min(sess, orc, w, h, window):
    rng = np.random.default_rng(w)
    img = rng.standard_normal((h, w)).astype(F)
    tied = np.round(img * 2) / 2 + F(0)   # heavily tied, no -0.0 (equal zeros have no order)
    din, dout, dscr = Guarded(sess, img), Guarded(sess, n=w * h), Guarded(sess, n=3 * w * h)
    for x in (img, tied):
        din.dev.upload(np.concatenate([sentinel(GUARD, F), x.ravel(), sentinel(GUARD, F)]))
        sess.rdl.rdl_sliding_min(sess.h, din.vp, dout.vp, dscr.vp, w, h, C.c_uint64(window))
        same_bits(dout.get((h, w)), orc.sliding_minimum(x, window))
        dscr.get()
    free(din, dout, dscr)


# --------------------------------------------------- component optimisation
def model_with_specials(rng, n):
    model = rng.standard_normal(n).astype(F)
    model[rng.random(n) < 0.5] = 0.0
    model[rng.random(n) < 0.05] = -0.0
    model[rng.random(n) < 0.05] = np.nan      # NaN != 0: a component
    return model


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("n", sizes(8192))
def test_masked_copy(sess, n, sign):
    rng = np.random.default_rng(n)
    model, src = model_with_specials(rng, n), rng.standard_normal(n).astype(F)
    dm, ds, dout = Guarded(sess, model), Guarded(sess, src), Guarded(sess, n=n)
    sess.rdl.rdl_masked_copy(sess.h, dm.vp, ds.vp, dout.vp, SZ(n), C.c_float(sign))
    same_bits(dout.get(), R.masked_copy(model, src, sign))
    free(dm, ds, dout)


@pytest.mark.parametrize("n", sizes(8192))
def test_masked_add(sess, n):
    rng = np.random.default_rng(n)
    model, v = model_with_specials(rng, n), rng.standard_normal(n).astype(F)
    model[np.isnan(model)] = 3.0    # NaN + v has no specified payload; masked_copy covers NaN
    dm, dv = Guarded(sess, model), Guarded(sess, v)
    sess.rdl.rdl_masked_add(sess.h, dm.vp, dv.vp, SZ(n))
    same_bits(dm.get(), R.masked_add(model, v))
    free(dm, dv)


# ------------------------------------------------------------ order statistics
def select_input(kind, n, rng):
    v = rng.standard_normal(n).astype(F)
    if kind == "tied":
        v = (np.round(v * 8) / 8).astype(F)
    elif kind == "constant":
        v[:] = F(0.625)
    elif kind == "special":
        for value in (0.0, -0.0, np.inf, -np.inf):
            v[rng.random(n) < 0.1] = value
    return v


def same_value(got, want):
    """Bit-exact, except that equal zeros of either sign are one value: the
    kernel orders -0.0 before +0.0, np.sort does not say."""
    if np.isnan(want):      # the mean of -inf and +inf
        assert np.isnan(got)
        return
    assert got == want and (want == 0 or raw(F(got)) == raw(F(want))), (got, want)


@pytest.mark.parametrize("use_center", [0, 1])
@pytest.mark.parametrize("kind", ["normal", "tied", "constant", "special"])
@pytest.mark.parametrize("n", [1, 2, 1001, 4096, 525289, 525290])   # 2048 * 256 + 1001, odd and even
def test_median_select_kth(sess, n, kind, use_center):
    v = select_input(kind, n, np.random.default_rng(n))
    center = F(0.625) if kind == "constant" else F(0.25)
    d = Guarded(sess, v)
    out = C.c_float()
    sess.rdl.rdl_median(sess.h, d.vp, SZ(n), use_center, C.c_float(center), C.byref(out))
    same_value(out.value, R.median(v, use_center, center))
    for k in sorted({0, n // 2, n - 1}):
        sess.rdl.rdl_select_kth(sess.h, d.vp, SZ(n), use_center, C.c_float(center), SZ(k),
                                C.byref(out))
        same_value(out.value, R.select_kth(v, use_center, center, k))
    err_arg(sess.rdl.rdl_select_kth, sess.h, d.vp, SZ(n), use_center, C.c_float(center), SZ(n),
            C.byref(out))
    free(d)


# ----------------------------------------------------------------- IUWT pieces
def max_abs(sess, d, w, h, xb, yb, allow_negative, dmask):
    p = Peak()
    sess.rdl.rdl_max_abs(sess.h, d.vp, w, h, xb, yb, int(allow_negative),
                         dmask.vp if dmask is not None else None, C.byref(p))
    return p.found, p.x, p.y, F(p.value)


def max_abs_variants(w, h, xb, yb, rng, masked):
    normal = rng.standard_normal((h, w)).astype(F)
    yield "normal", normal
    yield "ties", (np.round(normal * 2) / 2).astype(F)     # many equal maxima
    special = normal.copy()
    for value in (np.nan, np.inf, -np.inf, R.FLT_LOWEST):
        special.ravel()[rng.integers(0, w * h, max(1, w * h // 50))] = value
    yield "special", special
    yield "no finite", np.where(rng.random((h, w)) < 0.5, F(np.nan), F(R.FLT_LOWEST)).astype(F)
    yield "lowest only", np.full((h, w), R.FLT_LOWEST, F)
    hidden = normal.copy()
    hidden[0, 0] = 1e6            # outside the border, or under a zero mask byte
    hidden[h - 1, w - 1] = -2e6
    yield "hidden", hidden


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("w,h,xb,yb", [(1, 1, 0, 0), (64, 64, 32, 32),      # one pixel; an empty box
                                       (300, 200, 7, 3), (1031, 517, 0, 0)])  # beyond 1024 * 256
def test_max_abs(sess, w, h, xb, yb, masked):
    rng = np.random.default_rng(w + 13 * masked)
    mask = (rng.random((h, w)) < 0.6).astype(np.uint8) if masked else None
    if masked:
        mask[0, 0] = mask[h - 1, w - 1] = 0
    dmask = Guarded(sess, mask) if masked else None
    for name, data in max_abs_variants(w, h, xb, yb, rng, masked):
        d = Guarded(sess, data)
        for allow_negative in (True, False):
            found, x, y, value = max_abs(sess, d, w, h, xb, yb, allow_negative, dmask)
            want = R.max_abs(data, xb, yb, allow_negative, mask)
            assert (found, x, y) == want[:3], (name, allow_negative)
            assert raw(value) == raw(F(want[3])), (name, allow_negative)
            if name == "hidden" and (masked or xb or yb):
                assert (x, y) not in ((0, 0), (w - 1, h - 1))
        free(d)
    # nothing qualifies: all-zero mask, and the empty box
    data = rng.standard_normal((h, w)).astype(F)
    d, dzero = Guarded(sess, data), Guarded(sess, np.zeros((h, w), np.uint8))
    found, x, y, value = max_abs(sess, d, w, h, xb, yb, True, dzero)
    assert (found, x, y) == (0, w, h) and raw(value) == raw(F(R.FLT_LOWEST))
    if 2 * xb == w:
        found, x, y, value = max_abs(sess, d, w, h, xb, yb, True, None)
        assert (found, x, y) == (0, w, h) and raw(value) == raw(F(R.FLT_LOWEST))
    free(d, dzero)
    if masked:
        dmask.free()


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("w,h,min_scale,end_scale,xb,yb", [
    (5, 3, 0, 1, 0, 0), (130, 70, 1, 4, 6, 3), (600, 600, 0, 3, 0, 0)])   # 3 * 600^2 > 4096 * 256
def test_iuwt_select(sess, w, h, min_scale, end_scale, xb, yb, with_prior):
    rng = np.random.default_rng(w)
    coeffs = rng.standard_normal((end_scale, h, w)).astype(F)
    prior = (rng.random((h, w)) < 0.7).astype(np.uint8) if with_prior else None
    inside = [(y, x) for y in range(yb, h - yb) for x in range(xb, w - xb)
              if (y, x) != (h // 2, w // 2) and (prior is None or prior[y, x])]
    equal = np.zeros(end_scale, F)
    for s in range(end_scale):      # coefficients exactly at the thresholds used below
        (y0, x0), (y1, x1), (y2, x2) = [inside[(7 * s + i) % len(inside)] for i in (3, 4, 5)]
        coeffs[s, y1, x1], coeffs[s, y2, x2] = F(0.75), F(-0.75)
        equal[s] = coeffs[s, y0, x0] = np.abs(coeffs[s, y0, x0])
    coeffs[:, h // 2, w // 2] = np.nan                     # never selects
    dc = Guarded(sess, coeffs)
    dp = Guarded(sess, prior) if with_prior else None
    dm = Guarded(sess, n=end_scale * w * h, dtype=np.uint8)
    for rotation in range(3):
        thr = np.zeros(end_scale, F)
        for s in range(end_scale):
            # positive; negative (two-sided); exactly a coefficient's value (strict compare)
            thr[s] = [F(0.5), F(-0.75), equal[s]][(s + rotation) % 3]
        area = C.c_uint64(12345)
        sess.rdl.rdl_iuwt_select(sess.h, dc.vp, w, h, min_scale, end_scale,
                                 thr.ctypes.data_as(C.c_void_p), xb, yb,
                                 dp.vp if with_prior else None, dm.vp, C.byref(area))
        want, count = R.iuwt_select(coeffs, min_scale, end_scale, thr, xb, yb, prior)
        got = dm.get((end_scale, h, w))
        np.testing.assert_array_equal(got, want)
        assert not got[:min_scale].any() and not got[:, h // 2, w // 2].any()
        assert area.value == count == int(got.sum())
    free(dc, dm)
    if with_prior:
        dp.free()


@pytest.mark.parametrize("n", sizes(4096))
def test_iuwt_apply_mask(sess, n):
    rng = np.random.default_rng(n)
    scales = 3 if n % 3 == 0 else 1
    coeffs = rng.standard_normal(n).astype(F)
    mask = (rng.random(n) < 0.5).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    dc, dm = Guarded(sess, coeffs), Guarded(sess, mask)
    sess.rdl.rdl_iuwt_apply_mask(sess.h, dc.vp, dm.vp, n // scales, 1, scales)
    same_bits(dc.get(), R.iuwt_apply_mask(coeffs, mask))
    free(dc, dm)


def bbox_variants(w, h, rng):
    yield "zero", np.zeros((h, w), F)
    edges = np.full((h, w), 0.005, F)            # below m * 0.01 with m = 1
    for y in range(h):
        edges[y, [0, w - 1, min(256, w - 1)][y % 3]] = 1.0
    yield "edges", edges
    thr = np.zeros((h, w), F)
    thr[0, 0] = 7.0
    if w * h > 1:
        thr[h - 1, w - 1] = F(0.07)              # kept by the double compare only
    yield "threshold pixel", thr
    neg = (rng.standard_normal((h, w)) * 1e-3).astype(F)
    neg[h // 2, w // 3] = -5.0                   # a negative pixel is the maximum
    if w > 2:
        neg[0, w - 2] = 0.06
    yield "negative maximum", neg
    yield "normal", rng.standard_normal((h, w)).astype(F)


@pytest.mark.parametrize("w,h", [(1, 1), (63, 5), (256, 3), (257, 3), (1000, 37), (700, 1100)])
def test_bbox_rows(sess, w, h):
    rng = np.random.default_rng(w)
    for name, img in bbox_variants(w, h, rng):
        d = Guarded(sess, img)
        first, last = HostGuarded(h, np.int32), HostGuarded(h, np.int32)
        sess.rdl.rdl_bbox_rows(sess.h, d.vp, w, h, first.vp, last.vp)
        want_first, want_last = R.bbox_rows(img)
        np.testing.assert_array_equal(first.get(), want_first, err_msg=name)
        np.testing.assert_array_equal(last.get(), want_last, err_msg=name)
        if name == "zero":
            assert np.all(first.get() == -1) and np.all(last.get() == -1)
        if name == "threshold pixel" and w * h > 1:
            assert last.get()[h - 1] == w - 1
        free(d)


def test_bbox_rows_without_pixels(sess):
    """width * height == 0: RDL_OK, nothing launched, every row at -1."""
    d = Guarded(sess, np.ones(4, F))
    first, last = HostGuarded(3, np.int32), HostGuarded(3, np.int32)
    sess.rdl.rdl_bbox_rows(sess.h, d.vp, 0, 3, first.vp, last.vp)
    assert first.get().tolist() == last.get().tolist() == [-1, -1, -1]
    first, last = HostGuarded(0, np.int32), HostGuarded(0, np.int32)
    sess.rdl.rdl_bbox_rows(sess.h, d.vp, 5, 0, first.vp, last.vp)
    first.get(), last.get()
    free(d)


# ------------------------------------------------------ reductions in double
REDUCTION_SIZES = [1, 63, 64, 65, 255, 256, 257, 262145, 786509]   # 1024 * 256 + 1, 3 * 1024 * 256 + 77


def reduction_inputs(n):
    rng = np.random.default_rng(n)
    yield rng.uniform(1, 2, n).astype(F), rng.uniform(1, 2, n).astype(F)   # float accumulation fails here
    yield rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)


def within(got, terms):
    return abs(got - R.exact_sum(terms)) <= R.reduction_tolerance(terms)


@pytest.mark.parametrize("n", REDUCTION_SIZES)
def test_double_reductions(sess, n):
    """rdl_dot, rdl_dot_pair, rdl_iuwt_snr_sums and rdl_rms against math.fsum of
    the float64 terms, within n * 2^-52 * sum|term|: what any order of summing
    doubles satisfies and a float accumulator does not
    (test_primitive_refs.py::test_reduction_inputs_tell_float_from_double_accumulation)."""
    for a, b in reduction_inputs(n):
        da, db = Guarded(sess, a), Guarded(sess, b)
        x, y = C.c_double(), C.c_double()
        sess.rdl.rdl_dot(sess.h, da.vp, db.vp, SZ(n), C.byref(x))
        assert within(x.value, R.dot_terms(a, b))
        sess.rdl.rdl_dot_pair(sess.h, da.vp, db.vp, SZ(n), C.byref(x), C.byref(y))
        assert within(x.value, R.dot_terms(a, b)) and within(y.value, R.dot_terms(a, a))
        sess.rdl.rdl_iuwt_snr_sums(sess.h, da.vp, db.vp, SZ(n), C.byref(x), C.byref(y))
        model_terms, noise_terms = R.snr_terms(a, b)
        assert within(x.value, model_terms) and within(y.value, noise_terms)
        out = C.c_float()
        sess.rdl.rdl_rms(sess.h, da.vp, SZ(n), C.byref(out))
        assert R.ulp_distance(F(out.value), R.rms(a)) <= 1
        free(da, db)


def test_double_reductions_of_nothing(sess):
    d = Guarded(sess, np.ones(4, F))
    x, y = C.c_double(7), C.c_double(7)
    sess.rdl.rdl_dot(sess.h, d.vp, d.vp, SZ(0), C.byref(x))
    assert x.value == 0.0
    x = C.c_double(7)
    sess.rdl.rdl_dot_pair(sess.h, d.vp, d.vp, SZ(0), C.byref(x), C.byref(y))
    assert (x.value, y.value) == (0.0, 0.0)
    x, y = C.c_double(7), C.c_double(7)
    sess.rdl.rdl_iuwt_snr_sums(sess.h, d.vp, d.vp, SZ(0), C.byref(x), C.byref(y))
    assert (x.value, y.value) == (0.0, 0.0)
    out = C.c_float()
    err_arg(sess.rdl.rdl_rms, sess.h, d.vp, SZ(0), C.byref(out))
    free(d)


# -------------------------------------------------------------------- spectra
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("n", sizes(16384))
def test_spectrum_multiply(sess, n, alias):
    """Where the compiler fuses the two products is not specified: per
    component within 4 * 2^-24 * (|p| + |q|) * |scale| of the float64 product.
    dst aliasing a is how rdl_fft_convolve calls it."""
    rng = np.random.default_rng(n)
    a = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    b = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    scale = F(1.0 / 4096.5)
    da, db = Guarded(sess, a.view(F)), Guarded(sess, b.view(F))
    dd = da if alias else Guarded(sess, n=2 * n)
    sess.rdl.rdl_spectrum_multiply(sess.h, dd.vp, da.vp, db.vp, SZ(n), C.c_float(scale))
    got = dd.get().view(np.complex64).astype(np.complex128)
    ref, tol_re, tol_im = R.spectrum_multiply(a, b, scale)
    assert np.all(np.abs(got.real - ref.real) <= tol_re)
    assert np.all(np.abs(got.imag - ref.imag) <= tol_im)
    db.get()
    free(da, db)
    if not alias:
        dd.free()


@pytest.mark.parametrize("w,h", [(64, 64), (94, 47)])
def test_fft_inverse(sess, w, h):
    """rdl_fft_inverse of the device's own forward spectrum against
    np.fft.irfft2 of that spectrum in float64 (unnormalised: times w * h),
    within 2e-6 * max|x| as test_fft_convolve allows a transform."""
    img = np.random.default_rng(w).standard_normal((h, w)).astype(F)
    f = C.c_void_p()
    sess.rdl.rdl_fft_create(sess.h, w, h, C.byref(f))
    nb = sess.rdl.lib.rdl_fft_spectrum_bytes(f)
    assert nb == (w // 2 + 1) * h * 8
    din, dspec, dout = Guarded(sess, img), Guarded(sess, n=nb // 4), Guarded(sess, n=w * h)
    sess.rdl.rdl_fft_forward(f, din.vp, dspec.vp)
    spectrum = dspec.get().view(np.complex64).reshape(h, w // 2 + 1)
    sess.rdl.rdl_fft_inverse(f, dspec.vp, dout.vp)
    got = dout.get((h, w))
    dspec.get()
    want = R.fft_inverse(spectrum, w, h)
    assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max()
    assert np.abs(got - img.astype(np.float64) * (w * h)).max() <= 2e-6 * np.abs(want).max()
    sess.rdl.rdl_fft_destroy(f)
    free(din, dspec, dout)


# ------------------------------------------ what is done with the loop's model
W, H, N_IMG = 128, 96, 2


def subminor_run(sess, select):
    """One small sub-minor run over two joined images, as
    test_subminor_loop_bit_exact sets it up; -> (handle, positions, models)."""
    from test_gpu_kernels import synthetic
    psf, dirty = synthetic(W, H, 12, 7)
    dirties = np.stack([dirty, dirty * F(1.15) + F(1e-3) * np.roll(dirty, 3, axis=1)]).astype(F)
    integrated = np.abs(R.integrate_linear(dirties, [1, 1])).ravel()
    threshold = F(np.sort(integrated)[-300]) if select else F(10 * integrated.max())
    dres, dpsf = sess.array(dirties), sess.array(np.stack([psf, psf]))
    sm = C.c_void_p()
    sess.rdl.rdl_subminor_create(sess.h, C.byref(sm))
    p = SubminorParams()
    p.width, p.height, p.n_images, p.n_pol = W, H, N_IMG, 1
    p.integ = integration(N_IMG, 1, mode=0)
    p.allow_negative, p.stop_on_negative = 1, 0
    p.threshold, p.gain, p.divergence_limit = threshold, 0.1, 4.0
    p.iteration_start, p.max_iterations = 0, 12
    out = SubminorResult()
    sess.rdl.rdl_subminor_run(sm, dres.vp, dpsf.vp, C.byref(p), C.byref(out), None, C.c_uint64(0))
    n = int(out.n_selected)
    pos, models = np.zeros(n, np.uint32), np.zeros((N_IMG, n), F)
    sess.rdl.rdl_subminor_get(sm, pos.ctypes.data_as(C.c_void_p), models.ctypes.data_as(C.c_void_p),
                              C.c_uint64(n))
    free(dres, dpsf)
    return sm, pos, models


def check_model_calls(sess, sm, pos, models):
    """The four "what is done with the model" calls against NumPy expectations
    built from the run's positions and model values."""
    ox, oy, dw, dh = 5, 3, W + 9, H + 7
    for k in range(N_IMG):
        d64 = Guarded(sess, n=dw * dh, dtype=np.float64)
        sess.rdl.rdl_subminor_model_f64(sm, k, d64.vp, dw, dh, ox, oy)
        same_bits(d64.get((dh, dw)), R.model_plane(pos, models[k], dw, dh, ox, oy, np.float64))
        n_rows = H + oy + 11                                  # longer than height + oy
        drows = Guarded(sess, n=n_rows, dtype=np.uint8)
        sess.rdl.rdl_subminor_model_rows(sm, k, drows.vp, n_rows, oy)
        rows = R.model_rows(pos, models[k], n_rows, oy)
        np.testing.assert_array_equal(drows.get(), rows)
        # the masked scatter reads rows[y + oy] for every destination row y < H + 4
        dest0 = sentinel((H + 4) * (W + 6), F).reshape(H + 4, W + 6)
        ddest = Guarded(sess, dest0)
        if pos.size:
            drows.get()
        else:                      # an empty selection never reads the marks: none to trust
            drows.dev.upload(np.full(n_rows + 2 * GUARD, 1, np.uint8))
        sess.rdl.rdl_subminor_model_masked(sm, k, ddest.vp, W + 6, H + 4, drows.vp, oy)
        got = ddest.get(dest0.shape)
        if pos.size:
            same_bits(got, R.model_masked(dest0, pos, models[k], rows, oy))
            marked = rows[oy:oy + H + 4] != 0
            full = R.model_plane(pos, models[k], W + 6, H + 4, 0, 0, F)
            same_bits(got[marked], full[marked])               # mode 0's rows
            x, y = R.unpack_positions(pos)
            selected = np.zeros(dest0.shape, bool)
            selected[y, x] = True
            keep = ~marked[:, None] & ~selected
            same_bits(got[keep], dest0[keep])                  # sentinel kept
            assert marked.any() and (~marked).any() and (selected & ~marked[:, None]).any()
        else:
            same_bits(got, dest0)
        free(d64, drows, ddest)
    mask0 = (np.random.default_rng(1).random((H, W)) < 0.3).astype(np.uint8)
    dmask = Guarded(sess, mask0)
    sess.rdl.rdl_subminor_update_mask(sm, dmask.vp)
    np.testing.assert_array_equal(dmask.get((H, W)), R.update_mask(mask0, pos, models))
    free(dmask)


def test_subminor_model_calls(sess):
    sm, pos, models = subminor_run(sess, select=True)
    assert 100 < pos.size < 1000
    components = (models != 0).any(axis=0)
    assert 2 <= components.sum() <= 12
    # a row holding only zero-valued selected pixels exists (and must stay unmarked)
    _, y = R.unpack_positions(pos)
    assert set(y.tolist()) - set(y[components].tolist())
    check_model_calls(sess, sm, pos, models)
    sess.rdl.rdl_subminor_destroy(sm)


def test_subminor_model_calls_empty_selection(sess):
    sm, pos, models = subminor_run(sess, select=False)
    assert pos.size == 0
    check_model_calls(sess, sm, pos, models)
    sess.rdl.rdl_subminor_destroy(sm)


# ------------------------------------------------ session calls with no kernel
def test_session_lanes_and_stream(sess):
    """rdl_session_fork / lane / join: work sent to either lane is complete
    after the join; rdl_session_stream names the current lane's stream."""
    n = 100000
    a = np.random.default_rng(1).standard_normal(n).astype(F)
    d0, d1 = Guarded(sess, a), Guarded(sess, a)
    sess.rdl.lib.rdl_session_stream.argtypes = [C.c_void_p]
    home = sess.rdl.lib.rdl_session_stream(sess.h)
    assert home
    sess.rdl.rdl_session_fork(sess.h)
    sess.rdl.rdl_session_lane(sess.h, 1)
    assert sess.rdl.lib.rdl_session_stream(sess.h) not in (None, home)
    sess.rdl.rdl_scale(sess.h, d1.vp, SZ(n), C.c_float(3.0))
    sess.rdl.rdl_session_lane(sess.h, 0)
    assert sess.rdl.lib.rdl_session_stream(sess.h) == home
    sess.rdl.rdl_scale(sess.h, d0.vp, SZ(n), C.c_float(0.5))
    sess.rdl.rdl_session_join(sess.h)
    same_bits(d0.get(), R.scale(a, 0.5))
    same_bits(d1.get(), R.scale(a, 3.0))
    free(d0, d1)


def test_timing_filter_all(sess):
    """rdl_timing_filter_all: only the named family records launches."""
    lib = sess.rdl.lib
    lib.rdl_timing_get_all.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_double)]
    lib.rdl_timing_filter_all.argtypes = [C.c_char_p]

    def launches(family):
        ms, n, b = C.c_double(), C.c_uint64(), C.c_double()
        assert lib.rdl_timing_get_all(family, C.byref(ms), C.byref(n), C.byref(b)) == 0
        return n.value

    a = np.ones(1000, F)
    da, db = Guarded(sess, a), Guarded(sess, a)
    x = C.c_double()
    try:
        lib.rdl_timing_reset_all()
        assert lib.rdl_timing_filter_all(b"dot") == 0
        lib.rdl_timing_enable_all(1)
        sess.rdl.rdl_add(sess.h, da.vp, db.vp, SZ(1000))
        sess.rdl.rdl_dot(sess.h, da.vp, db.vp, SZ(1000), C.byref(x))
        sess.sync()
        assert (launches(b"dot"), launches(b"add")) == (1, 0)
        assert lib.rdl_timing_filter_all(None) == 0
        sess.rdl.rdl_add(sess.h, da.vp, db.vp, SZ(1000))
        sess.sync()
        assert launches(b"add") == 1
    finally:
        lib.rdl_timing_enable_all(0)
        lib.rdl_timing_filter_all(None)
        lib.rdl_timing_reset_all()
    free(da, db)
