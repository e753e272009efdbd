"""Every compile-time FFT plan (csrc/hip/fft_fast_*.hip) against numpy
float64, once as the row plan and once as the column plan of a thin plane.

The plan tables are read from the source (tests/fft_plans.py). A row kernel
handles one row per workgroup and a column kernel a few columns, so the
smallest plane that still exercises plan n is n against the smallest plan of
the other axis: (n, base) puts n on the rows, (base, n) on the columns, base =
1050 (float64) / 1280 (float). Before anything else each plane asserts that
rdl_conv_fast reports the flags the parsed tables predict, which ties the
parse to the binary.

Input: seeded Gaussian noise plus one bright pixel. Reference: numpy float64
rfft / rfft2 / irfft2. The bounds are the ones the suite already asserts for
the same operations (fft_plans.check_*); each plane prints its observed
error / bound per check as

    [fft-plan-error] <length> <role> <check> <error> / <bound> (<plane>)

(profiles/fft_plan_errors.txt is that table from an MI355X run), runs every
check before it fails, and frees what it allocated.

float64 planes: the rows pass alone, the 2-D forward transform,
CorrectResidualDirty's convolve-and-subtract (odd and even windows strictly
inside the plane, a row mask and none, a guard row, the float kernel spectrum
on convolution-column plans), and modes 1 and 2 through
rdl_conv_columns_layout with the kernel in both layouts.
Float tiled planes: rows, forward, modes 1 and 2, rdl_conv_rows_inverse of a
numpy-made spectrum (full plane, odd window, subtract at an even window), the
fused scale search from a windowed rdl_conv_forward_half (real kernel
spectra, 1 and 8 scales per launch, a ninth refused), and
rdl_conv_rows_inverse_peak against numpy's first-index argmax.
Float one-pass columns (width 96 has no row plan): forward, modes 1 and 2.
"""
import ctypes as C

import numpy as np
import pytest

import fft_plans as fp

pytestmark = pytest.mark.gpu

TABLES = fp.plan_tables()
F64_PLANES, F32_PLANES, ONE_PASS_PLANES = fp.planes(TABLES)
CONVD = set(fp.lengths(TABLES, "convd"))
ROW, COL = fp.RDL_CONV_ROW_MAJOR, fp.RDL_CONV_COL_MAJOR

RAN = {"f64": [], "f32": [], "one-pass": []}  # the planes that ran
TABLE = []                                    # (length, role, check, error, bound)


class _Peak(C.Structure):
    _fields_ = [("value", C.c_float), ("x", C.c_uint32), ("y", C.c_uint32),
                ("found", C.c_int32)]


@pytest.fixture(scope="module")
def sess():
    from rdl_lib import Session
    s = Session(0)
    lib = s.rdl.lib
    for name in ("rdl_conv_convolve_subtract_bytes", "rdl_conv_real_kernel_bytes"):
        getattr(lib, name).restype = C.c_size_t
        getattr(lib, name).argtypes = [C.c_void_p]
    yield s
    s.close()


@pytest.fixture(scope="module")
def orc():
    from oracle_lib import get_oracle
    return get_oracle()


class Plane:
    """One conv and the device arrays of one test, all released by close();
    records each check's error and collects the failures."""

    def __init__(self, sess, w, h, f64, kind):
        self.sess, self.w, self.h, self.f64, self.kind = sess, w, h, f64, kind
        self.nu = w // 2 + 1
        self.arrays, self.failures = [], []
        self.c = C.c_void_p()
        sess.rdl.rdl_conv_create_ex(sess.h, w, h, int(f64), 1, C.byref(self.c))
        self.fast = sess.rdl.lib.rdl_conv_fast(self.c)
        self.tiled = bool(self.fast & fp.RDL_CONV_FAST_TILED)
        self.cdt = np.complex128 if f64 else np.complex64
        self.name = f"{kind} {w}x{h}"
        print()  # the table lines start their own line under -s
        # the plans of this plane, by role
        if kind == "f64":
            self.row_role, self.col_role = ("rows-f64", w), ("cols-f64", h)
        elif kind == "f32":
            self.row_role, self.col_role = ("rows-f32", w), ("steps-f32", h)
        else:
            self.row_role, self.col_role = None, ("cols-f32", h)

    def array(self, arr=None, shape=None, dtype=np.float32):
        a = self.sess.array(arr, shape=shape, dtype=dtype)
        self.arrays.append(a)
        return a

    def spectrum(self, poison=False):
        """A spectrum-sized device array; poison: every byte 0xff (NaNs), so
        an element that is never written cannot pass for a result."""
        n = self.sess.rdl.lib.rdl_conv_spectrum_bytes(self.c) // np.dtype(self.cdt).itemsize
        a = self.array(shape=(n,), dtype=self.cdt)
        if poison:
            fill(a)
        return a

    def natural(self, flat):
        """A spectrum buffer's contents as [row][column] (h x w/2+1)."""
        if self.tiled:
            return fp.untile(flat, self.w, self.h)
        return flat[:self.nu * self.h].reshape(self.h, self.nu)

    def check(self, check, roles, fn, *args):
        """Run one comparison helper; print and keep error / bound per plan."""
        what = f"{self.name} {check}"
        try:
            err, bound = fn(*args, what)
        except AssertionError as e:
            self.failures.append(str(e))
            print(f"[fft-plan-FAILED] {e}")
            return
        self.note(check, roles, err, bound)

    def note(self, check, roles, err, bound):
        for role, length in (r for r in roles if r):
            TABLE.append((length, role, check, err, bound))
            print(f"[fft-plan-error] {length} {role} {check} {err:.3g} / {bound:.3g} "
                  f"({self.name})")

    def expect(self, ok, message):
        if not ok:
            self.failures.append(f"{self.name}: {message}")
            print(f"[fft-plan-FAILED] {self.name}: {message}")

    def close(self):
        for a in self.arrays:
            a.free()
        self.sess.rdl.rdl_conv_destroy(self.c)


def fill(a, byte=0xff):
    a.sess.rdl.rdl_memcpy_h2d(a.sess.h, a.vp,
                              np.full(a.nbytes, byte, np.uint8).ctypes.data_as(C.c_void_p),
                              C.c_size_t(a.nbytes))


def small_kernel(w, h, seed):
    """A 7 x 9 noise kernel wrapped around the origin (tests/test_fft_fast.py)."""
    rng = np.random.default_rng(seed)
    ker = np.zeros((h, w), np.float32)
    ker[:7, :9] = rng.standard_normal((7, 9))
    return np.roll(ker, (-3, -4), axis=(0, 1)).copy()


def check_transforms_and_modes(p, rows_check=True):
    """The rows pass alone, the forward transform, and the convolutions of
    mode 1 (in place) and mode 2 (shared spectrum) through
    rdl_conv_columns_layout with kernel (and mode-2 input) in both layouts."""
    rdl, c, w, h = p.sess.rdl, p.c, p.w, p.h
    both = (p.row_role, p.col_role)
    img = fp.noise_image(w, h, 3 * w + h)
    ker = small_kernel(w, h, 5 * w + h)
    img64 = img.astype(np.float64)
    ref_spec = np.fft.rfft2(img64)
    ref_conv = np.fft.irfft2(ref_spec * np.fft.rfft2(ker.astype(np.float64)), s=(h, w))
    di, dk = p.array(img), p.array(ker)
    kspec, kspec_cm, sspec, sspec_cm, work = (p.spectrum() for _ in range(5))
    out = p.array(shape=(h, w))
    one = C.c_double(1.0)
    if rows_check:
        rdl.rdl_conv_rows_forward(c, di.vp, w, h, 0, 0, work.vp)
        p.check("rows", (p.row_role,), fp.check_spectrum, p.natural(work.get()),
                np.fft.rfft(img64, axis=1), w, p.f64)
    for plane, rm, cm in ((dk, kspec, kspec_cm), (di, sspec, sspec_cm)):
        rdl.rdl_conv_forward(c, plane.vp, rm.vp)
        rdl.rdl_conv_rows_forward(c, plane.vp, w, h, 0, 0, work.vp)
        rdl.rdl_conv_columns_layout(c, work.vp, cm.vp, None, 0, one, None, ROW, ROW, COL)
        if p.tiled:  # one layout for every spectrum
            p.expect(np.array_equal(cm.get(), rm.get()), "mode 0: the tiled spectra differ")
        else:
            t = cm.get()[:p.nu * h].reshape(p.nu, h)
            p.expect(np.array_equal(t.T, p.natural(rm.get())),
                     "mode 0: column-major != row-major transposed")
    p.check("forward", both, fp.check_spectrum, p.natural(sspec.get()), ref_spec, w * h, p.f64)
    norm = 1.0 / (w * h) if p.f64 else float(np.float32(1.0 / (w * h)))
    for kern, image, layout, tag in ((kspec, sspec, ROW, "rm"), (kspec_cm, sspec_cm, COL, "cm")):
        rdl.rdl_conv_rows_forward(c, di.vp, w, h, 0, 0, work.vp)
        rdl.rdl_conv_columns_layout(c, work.vp, work.vp, kern.vp, 1, C.c_double(norm), None,
                                    ROW, layout, ROW)
        rdl.rdl_conv_rows_inverse(c, work.vp, out.vp, w, h, 0, 0, 0)
        p.check(f"mode1-{tag}", both, fp.check_image, out.get().astype(np.float64), ref_conv,
                w * h, p.f64)
        fill(work)
        rdl.rdl_conv_columns_layout(c, image.vp, work.vp, kern.vp, 2, C.c_double(norm), None,
                                    layout, layout, ROW)
        rdl.rdl_conv_rows_inverse(c, work.vp, out.vp, w, h, 0, 0, 0)
        p.check(f"mode2-{tag}", both, fp.check_image, out.get().astype(np.float64), ref_conv,
                w * h, p.f64)


def check_correction(p):
    """rdl_conv_convolve_subtract as CorrectResidualDirty runs it."""
    sess, rdl, c, pw, ph = p.sess, p.sess.rdl, p.c, p.w, p.h
    convd = bool(p.fast & fp.RDL_CONV_FAST_CONVD)
    col_role = ("convd-f64", ph) if convd else p.col_role
    rng = np.random.default_rng(7 * pw + ph)
    # the PSF image: a 41 x 41 patch at the centre of an (even-sized) image
    sw, sh = pw - 12, ph - 10
    psf = np.zeros((sh, sw), np.float32)
    psf[sh // 2 - 20:sh // 2 + 21, sw // 2 - 20:sw // 2 + 21] = rng.standard_normal((41, 41))
    kref = np.fft.rfft2(fp.centred_psf_kernel(psf, pw, ph))
    # a sparse model in plane coordinates, inside every window used below
    mp = np.zeros((ph, pw), np.float32)
    ys, xs = rng.integers(6, ph - 7, 300), rng.integers(8, pw - 8, 300)
    mp[ys, xs] = rng.standard_normal(300).astype(np.float32)
    mask = np.zeros(ph, np.uint8)
    mask[np.unique(ys)] = 1
    mspec = np.fft.rfft2(mp.astype(np.float64))
    conv_ref = {0: np.fft.irfft2(mspec * kref, s=(ph, pw))}

    dpsf, dmask = p.array(psf), p.array(mask, dtype=np.uint8)
    kplane = p.array(shape=(ph, pw))
    rows = p.spectrum()
    kspec = p.array(shape=(p.nu, ph), dtype=np.complex128)
    rdl.rdl_prepare_psf_kernel(sess.h, kplane.vp, pw, ph, dpsf.vp, sw, sh)
    rdl.rdl_conv_rows_forward(c, kplane.vp, pw, ph, 0, 0, rows.vp)
    rdl.rdl_conv_columns_ex(c, rows.vp, kspec.vp, None, 0, C.c_double(1.0), None, ROW, COL)
    kerns = {0: kspec}
    if convd:  # the float kernel spectrum; numpy multiplies by the same values
        k32 = p.array(shape=(p.nu, ph), dtype=np.complex64)
        rdl.rdl_complex_narrow(sess.h, k32.vp, kspec.vp, C.c_size_t(p.nu * ph))
        kerns[1] = k32
        conv_ref[1] = np.fft.irfft2(mspec * k32.get().T.astype(np.complex128), s=(ph, pw))
    work = p.array(shape=(sess.rdl.lib.rdl_conv_convolve_subtract_bytes(c),), dtype=np.uint8)
    fill(work)  # rows the passes never write are never read either

    odd = (5, 4, pw - 11, ph - 9)    # ox, oy, img_w, img_h: the scalar stores
    even = (6, 4, pw - 12, ph - 9)   # the float2 stores (and the residual prefetch)
    cases = [("odd-masked", odd, True, 0), ("even-masked", even, True, 0),
             ("odd-dense", odd, False, 0)]
    if convd:
        cases += [("even-masked-kf32", even, True, 1), ("odd-dense-kf32", odd, False, 1)]
    for tag, (ox, oy, iw, ih), masked, kf in cases:
        assert ox > 0 and oy > 0 and ox + iw < pw and oy + ih < ph  # strictly inside
        assert ox % 2 == iw % 2 == (1 if tag.startswith("odd") else 0)
        residual = rng.standard_normal((ih, iw)).astype(np.float32)
        guarded = np.full((ih + 2, iw), 7.0, np.float32)  # guard rows after the window
        guarded[:ih] = residual
        dres = p.array(guarded)
        dmod = p.array(np.ascontiguousarray(mp[oy:oy + ih, ox:ox + iw]))
        rdl.rdl_conv_convolve_subtract(c, dmod.vp, iw, ih, ox, oy, kerns[kf].vp, COL, kf,
                                       C.c_double(1.0 / (pw * ph)),
                                       dmask.vp if masked else None, work.vp, dres.vp)
        got = dres.get()
        p.expect(np.all(got[ih:] == 7.0), f"correction-{tag}: the guard rows were written")
        ref = conv_ref[kf]
        p.check(f"correction-{tag}", (p.row_role, col_role), fp.check_correction, got[:ih],
                residual, ref[oy:oy + ih, ox:ox + iw], float(np.abs(ref).max()))
        for a in (dres, dmod):
            a.free()


@pytest.mark.parametrize("w,h", F64_PLANES, ids=[f"rows{w}-cols{h}" for w, h in F64_PLANES])
def test_f64_plane(sess, w, h):
    p = Plane(sess, w, h, True, "f64")
    try:
        assert p.fast == fp.expected_fast(TABLES, w, h, True), (p.fast, w, h)
        assert p.fast == (fp.RDL_CONV_FAST_ROWS | fp.RDL_CONV_FAST_COLUMNS |
                          (fp.RDL_CONV_FAST_CONVD if h in CONVD else 0))
        RAN["f64"].append((w, h))
        check_transforms_and_modes(p)
        check_correction(p)
    finally:
        p.close()
    assert not p.failures, "\n".join(p.failures)


def check_rows_inverse(p):
    """rdl_conv_rows_inverse of a numpy-made spectrum (uploaded in the tiled
    order) against irfft2: the row pass is irfft2 without its column pass, so
    the spectrum is a plane of row spectra and numpy gets its column
    transform."""
    rdl, c, w, h = p.sess.rdl, p.c, p.w, p.h
    img = fp.noise_image(w, h, 11 * w + h)
    rng = np.random.default_rng(13 * w + h)
    # rounded to what is uploaded; the kernels do not normalise (x w)
    srows = (np.fft.rfft(img.astype(np.float64), axis=1) / w).astype(np.complex64)
    ref = np.fft.irfft2(np.fft.fft(srows.astype(np.complex128), axis=0), s=(h, w)) * w
    spec = p.spectrum()
    spec.upload(fp.tile(srows))
    for tag, (ox, oy, ww, wh), subtract in (("full", (0, 0, w, h), 0),
                                            ("odd-window", (3, 2, w - 7, h - 5), 0),
                                            ("even-subtract", (4, 1, w - 10, h - 3), 1)):
        before = rng.standard_normal((wh, ww)).astype(np.float32)
        guarded = np.full((wh + 1, ww), 7.0, np.float32)  # a guard row
        guarded[:wh] = before
        dout = p.array(guarded)
        rdl.rdl_conv_rows_inverse(c, spec.vp, dout.vp, ww, wh, ox, oy, subtract)
        got = dout.get()
        dout.free()
        p.expect(np.all(got[wh:] == 7.0), f"rows-inverse-{tag}: the guard row was written")
        value = got[:wh].astype(np.float64)
        if subtract:  # out = before - float(result)
            value = before.astype(np.float64) - value
        p.check(f"rows-inverse-{tag}", (p.row_role,), fp.check_image, value,
                ref[oy:oy + wh, ox:ox + ww], w * h, False)


SCALES = (4.0, 6.0, 8.0, 12.0, 16.0, 24.0, 32.0, 48.0)  # kMaxScaleOuts of them


def check_fused_scales(p, orc):
    """rdl_conv_forward_half of a window, rdl_conv_real_kernel,
    rdl_conv_scales with 8 scales and with 1, rdl_conv_scale_finish,
    rdl_conv_rows_inverse(_peak)."""
    sess, rdl, c, w, h = p.sess, p.sess.rdl, p.c, p.w, p.h
    both = (p.row_role, p.col_role)
    ox, oy, iw, ih = 3, 5, w - 10, h - 8
    win = fp.noise_image(iw, ih, 17 * w + h)
    plane = np.zeros((h, w), np.float64)
    plane[oy:oy + ih, ox:ox + iw] = win
    pspec = np.fft.rfft2(plane)
    shapes = [orc.shape_function(s, min(w, h)) for s in SCALES]
    p.expect(len({k.shape for k in shapes}) == len(SCALES), "the shape functions coincide")
    nb = sess.rdl.lib.rdl_conv_real_kernel_bytes(c)
    refs, dks = [], []
    for s, k in zip(SCALES, shapes):
        dk = p.array(shape=(nb // 4,), dtype=np.float32)
        k = np.ascontiguousarray(k, np.float32)
        rdl.rdl_conv_real_kernel(c, k.ctypes.data_as(C.c_void_p), k.shape[0], dk.vp)
        kref = np.fft.rfft2(fp.placed_kernel(k.astype(np.float64), w, h))
        p.check(f"real-kernel-{s:g}", both, fp.check_real_kernel, fp.untile(dk.get(), w, h), kref)
        refs.append(np.fft.irfft2(pspec * kref, s=(h, w)))
        dks.append(dk)
    dwin, half, work = p.array(win), p.spectrum(), p.spectrum()
    outs = [p.spectrum() for _ in SCALES]
    dout = p.array(shape=(h, w))
    # the same window at an even offset through the rows pass alone (8-byte
    # loads; the odd offset below takes the scalar ones)
    fill(work)
    rdl.rdl_conv_rows_forward(c, dwin.vp, iw, ih, ox + 1, oy, work.vp)
    shifted = np.zeros((h, w), np.float64)
    shifted[oy:oy + ih, ox + 1:ox + 1 + iw] = win
    p.check("rows-even-window", (p.row_role,), fp.check_spectrum, p.natural(work.get()),
            np.fft.rfft(shifted, axis=1), w, False)
    rdl.rdl_conv_forward_half(c, dwin.vp, iw, ih, ox, oy, half.vp)
    norm =C.c_double(float(np.float32(1.0 / (w * h))))

    def launch(indices):
        """One rdl_conv_scales launch of these scales into sentinel-filled
        outputs, finished; the images."""
        n = len(indices)
        for o in outs[:n]:
            fill(o)
        kp = (C.c_void_p * n)(*[dks[i].ptr for i in indices])
        op = (C.c_void_p * n)(*[o.ptr for o in outs[:n]])
        rdl.rdl_conv_scales(c, half.vp, n, kp, op, norm)
        images = []
        for o in outs[:n]:
            fill(work)
            rdl.rdl_conv_scale_finish(c, o.vp, work.vp)
            rdl.rdl_conv_rows_inverse(c, work.vp, dout.vp, w, h, 0, 0, 0)
            images.append(dout.get())
        return images

    p.expect(len({o.ptr for o in outs} | {half.ptr, work.ptr}) == len(SCALES) + 2,
             "the outputs are not distinct buffers")
    images = launch(range(len(SCALES)))
    for i, s in enumerate(SCALES):
        p.check(f"scales8-{s:g}", both, fp.check_scale, images[i].astype(np.float64), refs[i])
    p.expect(all(not np.array_equal(images[i], images[j])
                 for i in range(len(images)) for j in range(i)), "two scales gave one image")
    single = launch([3])[0]
    p.check(f"scales1-{SCALES[3]:g}", both, fp.check_scale, single.astype(np.float64), refs[3])
    # a ninth scale is refused before anything is launched
    nine = list(range(len(SCALES))) + [0]
    kp = (C.c_void_p * 9)(*[dks[i].ptr for i in nine])
    op = (C.c_void_p * 9)(*([o.ptr for o in outs] + [work.ptr]))
    rc = sess.rdl.lib.rdl_conv_scales(c, half.vp, 9, kp, op, norm)
    p.expect(rc == fp.RDL_ERR_ARG, f"nine scales returned {rc}, not RDL_ERR_ARG")

    # the peak search fused into the inverse row pass, on scale 3's result
    # (outs[0] holds it): the same image, numpy's first-index argmax
    out_b = p.array(shape=(h, w))
    for tag, (wx, wy, ww, wh), hb, vb, neg in (("full", (0, 0, w, h), 17, 40, 1),
                                               ("odd-window", (3, 2, w - 7, h - 5), 0, 5, 0)):
        rdl.rdl_conv_scale_finish(c, outs[0].vp, work.vp)
        rdl.rdl_conv_rows_inverse(c, work.vp, dout.vp, ww, wh, wx, wy, 0)
        a = dout.get().reshape(-1)[:ww * wh].reshape(wh, ww)
        rdl.rdl_conv_scale_finish(c, outs[0].vp, work.vp)
        fill(out_b)
        rdl.rdl_conv_rows_inverse_peak(c, work.vp, out_b.vp, ww, wh, wx, wy, hb, vb, neg, None, 3)
        got = (_Peak * 4)()
        rdl.rdl_find_peak_collect(sess.h, 4, got)
        b = out_b.get().reshape(-1)[:ww * wh].reshape(wh, ww)
        p.expect(np.array_equal(a.view(np.uint32), b.view(np.uint32)),
                 f"rows-inverse-peak-{tag}: the image differs from rdl_conv_rows_inverse's")
        x, y, value = fp.peak_in_box(a, hb, vb, bool(neg))
        g = got[3]
        p.expect((g.found, g.x, g.y, g.value) == (1, x, y, value),
                 f"rows-inverse-peak-{tag}: peak {(g.found, g.x, g.y, g.value)} != numpy's "
                 f"{(1, x, y, value)}")
        if tag == "full":
            p.check("rows-inverse-peak-image", both, fp.check_scale, a.astype(np.float64), refs[3])


@pytest.mark.parametrize("w,h", F32_PLANES, ids=[f"rows{w}-cols{h}" for w, h in F32_PLANES])
def test_f32_tiled_plane(sess, orc, w, h):
    p = Plane(sess, w, h, False, "f32")
    try:
        assert p.fast == fp.expected_fast(TABLES, w, h, False), (p.fast, w, h)
        assert p.fast == (fp.RDL_CONV_FAST_ROWS | fp.RDL_CONV_FAST_COLUMNS |
                          fp.RDL_CONV_FAST_TILED)
        RAN["f32"].append((w, h))
        check_transforms_and_modes(p)
        check_rows_inverse(p)
        check_fused_scales(p, orc)
    finally:
        p.close()
    assert not p.failures, "\n".join(p.failures)


@pytest.mark.parametrize("w,h", ONE_PASS_PLANES, ids=[f"cols{h}" for _, h in ONE_PASS_PLANES])
def test_f32_one_pass_columns(sess, w, h):
    p = Plane(sess, w, h, False, "one-pass")
    try:
        assert p.fast == fp.expected_fast(TABLES, w, h, False), (p.fast, w, h)
        assert p.fast == fp.RDL_CONV_FAST_COLUMNS
        RAN["one-pass"].append((w, h))
        check_transforms_and_modes(p, rows_check=False)
    finally:
        p.close()
    assert not p.failures, "\n".join(p.failures)


def test_every_plane_ran(request):
    """The parametrisation covers every plan in both roles, and every
    selected plane ran (none skipped); with the whole module selected, every
    plan has its lines in the table."""
    n64, n32 = len(TABLES["rows_f64"]), len(TABLES["rows_f32"])
    assert len(F64_PLANES) == 2 * n64 - 1
    assert len(F32_PLANES) == 2 * n32 - 1
    assert len(ONE_PASS_PLANES) == len(TABLES["cols_f32"])
    selected = {"f64": 0, "f32": 0, "one-pass": 0}
    for item in request.session.items:
        if item.module is request.module:
            for kind, name in (("f64", "test_f64_plane"), ("f32", "test_f32_tiled_plane"),
                               ("one-pass", "test_f32_one_pass_columns")):
                selected[kind] += item.name.startswith(name + "[")
    ran = {k: len(v) for k, v in RAN.items()}
    print(f"[fft-plan-count] float64 planes {ran['f64']} of {len(F64_PLANES)}, float tiled "
          f"{ran['f32']} of {len(F32_PLANES)}, one-pass {ran['one-pass']} of "
          f"{len(ONE_PASS_PLANES)}")
    assert ran == selected, (ran, selected)
    if selected != {"f64": len(F64_PLANES), "f32": len(F32_PLANES),
                    "one-pass": len(ONE_PASS_PLANES)}:
        return  # a subset was asked for
    seen = {(length, role) for length, role, _, _, _ in TABLE}
    for family, role in (("rows_f64", "rows-f64"), ("cols_f64", "cols-f64"),
                         ("convd", "convd-f64"), ("rows_f32", "rows-f32"),
                         ("steps", "steps-f32"), ("cols_f32", "cols-f32")):
        missing = [n for n in fp.lengths(TABLES, family) if (n, role) not in seen]
        assert not missing, (role, missing)
