"""The runtime-plan LDS FFT engine (csrc/hip/lds_fft.hip: RowsForward,
RowsInverse, Columns, ColumnsSplitA/B) over a covering set of its plan space,
against numpy float64.

The lengths are not a hand-kept list. tests/lds_fft_plan_query.cc prints the
planner's own plans (csrc/hip/lds_fft_plan.h); tests/lds_fft_plans.py turns
them into classes, (radix, first pass or later, register slots a thread uses),
and picks a greedy cover, to which the single-pass lengths, the odd lengths,
the largest odd length 10125 and the limit 10240 are added. Each length runs
once as the row length and once as the column length of a thin plane whose
other axis is chosen by rule (lds_fft_plans.height_for_rows /
width_for_columns): at least two workgroups with a partial last one and an
unpaired last row, or more than one column tile per XCD slot with a partial
last tile and idle blocks; one plane of width 2 per precision. The split
(four-step) column passes get a cover of their own classes, and the lengths
without a split are refused.

Mixed dispatch: planes with a compile-time plan (tests/fft_plans.py reads the
tables) on one axis only, so that conv.hip pairs a kernel of fft_fast*.hip
with a runtime kernel: float and float64 compile-time rows with runtime
columns, runtime float64 rows with ColumnsConvD and with ff::Columns<double>.

On planes without compile-time rows rdl_conv_rows_inverse_peak is refused
(RDL_ERR_UNSUPPORTED, nothing launched) and rdl_conv_convolve_subtract_peak
runs the unfused correction and returns RDL_NOT_FUSED, as rdl_hip.h says.
rdl_conv_columns_window is called directly: the window's rows are mode 1's,
and a convolution-column plan leaves every other row unwritten.

Every output is allocated poisoned (0xff bytes) or holds large finite values
(1e30) where a pass may leave rows unwritten, every image is followed by a
guard row, and each plane runs all its checks before it fails. Inputs: seeded
unit Gaussian noise. Bounds: the ones the suite already asserts for the same
operation on this engine: forward transforms eps x 8 sqrt(log2 N) sqrt(N)
(test_lds_fft_forward, eps 2.3e-16 / 1.2e-7), images fft_plans.check_image
(float64: half a float ulp + 1e-12 scale, float: 2e-6 max|ref| sqrt(log2 N),
as test_lds_fft_convolutions), corrections fft_plans.check_correction
(test_lds_fft_correction; also for the float64 subtracting row pass, whose
result is rounded once more at the size of the difference). N: the points of the transforms the check ran (w
for a row pass alone, w h for the plane). Every check prints

    [lds-plan-error] <length> <role> <check> <error> / <bound> (<plane>)

profiles/lds_fft_sweep_errors.txt is that table from an MI355X run.
tests/test_lds_fft_plan.py (CPU) checks the planner itself and that the
comparison helpers used here reject a result one element off.
"""
import atexit
import ctypes as C
import shutil
import tempfile

import numpy as np
import pytest

import fft_plans as fp
import lds_fft_plans as lp

pytestmark = pytest.mark.gpu

ROW, COL = fp.RDL_CONV_ROW_MAJOR, fp.RDL_CONV_COL_MAJOR
RDL_ERR_UNSUPPORTED, RDL_NOT_FUSED = 5, 6
AUTO, SPLIT = 0, 2
PREC = {True: "f64", False: "f32"}
GUARD_ROWS = 2 * 64  # two rows a pair, at most 64 pairs a workgroup
STALE = 1e30  # finite, and large enough that one rounding of it swamps a result

_TMP = tempfile.mkdtemp(prefix="ldsplan")
atexit.register(shutil.rmtree, _TMP, ignore_errors=True)
TABLES = fp.plan_tables()
PLANNER = lp.Planner(lp.compile_query(_TMP))


# --------------------------------------------------------- comparison helpers
check_forward = lp.check_forward


def odd_window(length):
    """(offset, size), both odd, strictly inside [0, length) where it has room."""
    o = 3 if length >= 7 else 1
    size = length - o - 1
    size -= size % 2 == 0
    return o, max(size, 1)


def even_window(length):
    o = 2 if length >= 6 else 0
    size = (length - o - 1) // 2 * 2
    return o, size if size > 0 else length - o


def fill(a, byte=0xff):
    a.sess.rdl.rdl_memcpy_h2d(a.sess.h, a.vp,
                              np.full(a.nbytes, byte, np.uint8).ctypes.data_as(C.c_void_p),
                              C.c_size_t(a.nbytes))


def poisoned(a):
    """The elements of a float array still holding the 0xff fill."""
    return a.view(np.uint32) == 0xffffffff


@pytest.fixture(scope="module")
def sess():
    from rdl_lib import Session
    s = Session(0)
    lib = s.rdl.lib
    lib.rdl_conv_convolve_subtract_bytes.restype = C.c_size_t
    lib.rdl_conv_convolve_subtract_bytes.argtypes = [C.c_void_p]
    yield s
    s.close()


class Plane:
    """One conv and its device arrays, released by close(); prints each
    check's error / bound under every (role, length) and collects failures."""

    def __init__(self, sess, w, h, f64, columns, roles):
        self.sess, self.w, self.h, self.f64, self.roles = sess, w, h, f64, roles
        self.nu = w // 2 + 1
        self.arrays, self.failures, self.guards = [], [], {}
        self.cdt = np.complex128 if f64 else np.complex64
        self.name = f"{PREC[f64]} {w}x{h}" + (" split" if columns == SPLIT else "")
        self.c = C.c_void_p()
        sess.rdl.rdl_conv_create_ex(sess.h, w, h, int(f64), columns, C.byref(self.c))
        self.fast = sess.rdl.lib.rdl_conv_fast(self.c)
        self.split = bool(sess.rdl.lib.rdl_conv_columns_split(self.c))
        self.rng = np.random.default_rng(31 * w + h + int(f64))
        print()

    def noise(self, h, w):
        return self.rng.standard_normal((h, w)).astype(np.float32)

    def array(self, arr=None, shape=None, dtype=np.float32):
        a = self.sess.array(arr, shape=shape, dtype=dtype)
        self.arrays.append(a)
        return a

    def spectrum(self, poison=False, stale=False):
        """A spectrum-sized device array: zero, poisoned (0xff bytes: NaN) or
        stale (large finite values), followed by GUARD_ROWS rows of the same
        fill that release() expects untouched (a row kernel whose last
        workgroup ran its full count would write there)."""
        n = self.sess.rdl.lib.rdl_conv_spectrum_bytes(self.c) // np.dtype(self.cdt).itemsize
        assert n == self.nu * self.h
        rows = self.h + GUARD_ROWS
        if stale:
            a = self.array(np.full((rows, self.nu), STALE * (1 + 1j), self.cdt))
        else:
            a = self.array(shape=(rows, self.nu), dtype=self.cdt)
            if poison:
                fill(a)
        self.guards[a.ptr] = a.get()[self.h:].tobytes()
        return a

    def rows(self, spec):
        """A spectrum array's h rows on the host."""
        return spec.get()[:self.h]

    def release(self, *arrays):
        """Free; for spectra, first check the guard rows."""
        for a in arrays:
            guard = self.guards.pop(a.ptr, None)
            if guard is not None:
                self.expect(a.get()[self.h:].tobytes() == guard,
                            "the rows after a spectrum were written")
            a.free()

    def check(self, check, fn, *args):
        what = f"{self.name} {check}"
        try:
            err, bound = fn(*args, what)
        except AssertionError as e:
            self.failures.append(str(e))
            print(f"[lds-plan-FAILED] {e}")
            return
        for role, length in self.roles:
            print(f"[lds-plan-error] {length} {role} {check} {err:.3g} / {bound:.3g} "
                  f"({self.name})")

    def expect(self, ok, message):
        if not ok:
            self.failures.append(f"{self.name}: {message}")
            print(f"[lds-plan-FAILED] {self.name}: {message}")

    def close(self):
        self.release(*(a for a in self.arrays if a.ptr))
        self.sess.rdl.rdl_conv_destroy(self.c)


def finish(p):
    p.close()
    assert not p.failures, "\n".join(p.failures)


# ------------------------------------------------------------------ the checks
def check_rows_forward(p):
    """rdl_conv_rows_forward alone: the full plane and an odd window at odd
    offsets, against rfft of the zero-padded plane."""
    rdl, c, w, h = p.sess.rdl, p.c, p.w, p.h
    (ox, iw), (oy, ih) = odd_window(w), odd_window(h)
    for tag, (x0, y0, ww, wh) in (("rows-full", (0, 0, w, h)), ("rows-odd-window", (ox, oy, iw, ih))):
        win = p.noise(wh, ww)
        plane = np.zeros((h, w))
        plane[y0:y0 + wh, x0:x0 + ww] = win
        dwin, spec = p.array(win), p.spectrum(poison=True)
        rdl.rdl_conv_rows_forward(c, dwin.vp, ww, wh, x0, y0, spec.vp)
        p.check(tag, check_forward, p.rows(spec), np.fft.rfft(plane, axis=1), w, p.f64)
        p.release(dwin, spec)


def check_rows_inverse(p):
    """rdl_conv_rows_inverse of a numpy-made spectrum against irfft (n = w, so
    odd widths too): the full plane, an odd window at odd offsets, written, an
    even window, subtracted. The imaginary parts of the DC bin and (even w) the
    Nyquist bin are set to values a C2R transform must ignore."""
    rdl, c, w, h = p.sess.rdl, p.c, p.w, p.h
    srows = (np.fft.rfft(p.noise(h, w).astype(np.float64), axis=1) / w).astype(p.cdt)
    clean = srows.astype(np.complex128)
    srows[:, 0] += p.cdt(0.37j)
    if w % 2 == 0:
        srows[:, -1] -= p.cdt(0.21j)
    ref = np.fft.irfft(clean, n=w, axis=1) * w  # the kernels do not normalise
    spec = p.array(srows)
    (ox, iw), (oy, ih) = odd_window(w), odd_window(h)
    (ex, ew), (ey, eh) = even_window(w), even_window(h)
    for tag, (x0, y0, ww, wh), subtract in (("full", (0, 0, w, h), 0),
                                            ("odd-window", (ox, oy, iw, ih), 0),
                                            ("even-subtract", (ex, ey, ew, eh), 1)):
        before = p.noise(wh, ww)
        dout = p.array(shape=(wh + 1, ww))  # a guard row after the image
        fill(dout)
        if subtract:
            guarded = np.full((wh + 1, ww), 7.0, np.float32)
            guarded[:wh] = before
            dout.upload(guarded)
        rdl.rdl_conv_rows_inverse(c, spec.vp, dout.vp, ww, wh, x0, y0, subtract)
        got = dout.get()
        p.release(dout)
        p.expect(np.all(got[wh:] == 7.0) if subtract else poisoned(got[wh:]).all(),
                 f"rows-inverse-{tag}: the guard row was written")
        value = got[:wh].astype(np.float64)
        if subtract:  # out = before - float(result)
            value = before.astype(np.float64) - value
        window = ref[y0:y0 + wh, x0:x0 + ww]
        if subtract and p.f64:
            # before - float(result) rounds once more, at the size of the
            # difference: the bound of the float64 correction, which is this
            # subtraction (test_lds_fft_correction)
            p.check(f"rows-inverse-{tag}", fp.check_correction, got[:wh], before, window,
                    float(np.abs(ref).max()))
        else:
            p.check(f"rows-inverse-{tag}", fp.check_image, value, window, w, p.f64)


def check_forward_and_modes(p):
    """rdl_conv_forward against rfft2; mode 0 written column-major; modes 1
    (in place) and 2 (shared spectrum) through rdl_conv_columns_ex with the
    kernel spectrum in both layouts (split plans: row-major only)."""
    rdl, c, w, h = p.sess.rdl, p.c, p.w, p.h
    img, ker = p.noise(h, w), p.noise(h, w)
    ref_spec = np.fft.rfft2(img.astype(np.float64))
    kref = np.fft.rfft2(ker.astype(np.float64))
    ref_conv = np.fft.irfft2(ref_spec * kref, s=(h, w))
    di, dk = p.array(img), p.array(ker)
    kspec, sspec = p.spectrum(poison=True), p.spectrum(poison=True)
    rdl.rdl_conv_forward(c, dk.vp, kspec.vp)
    rdl.rdl_conv_forward(c, di.vp, sspec.vp)
    p.check("forward", check_forward, p.rows(sspec), ref_spec, w * h, p.f64)
    p.check("forward-kernel", check_forward, p.rows(kspec), kref, w * h, p.f64)
    kerns = [(kspec, ROW, "rm")]
    if not p.split:
        work = p.spectrum(poison=True)
        kspec_cm = p.array(shape=(p.nu, h), dtype=p.cdt)
        fill(kspec_cm)
        rdl.rdl_conv_rows_forward(c, dk.vp, w, h, 0, 0, work.vp)
        rdl.rdl_conv_columns_ex(c, work.vp, kspec_cm.vp, None, 0, C.c_double(1.0), None, ROW, COL)
        p.expect(np.array_equal(kspec_cm.get().T, p.rows(kspec)),
                 "mode 0: column-major != row-major transposed")
        p.release(work)
        kerns.append((kspec_cm, COL, "cm"))
    norm = C.c_double(1.0 / (w * h) if p.f64 else float(np.float32(1.0 / (w * h))))
    for kern, layout, tag in kerns:
        work = p.spectrum(poison=True)
        out = p.array(shape=(h + 1, w))
        for mode in (1, 2):
            fill(out)
            if mode == 1:
                rdl.rdl_conv_rows_forward(c, di.vp, w, h, 0, 0, work.vp)
                rdl.rdl_conv_columns_ex(c, work.vp, work.vp, kern.vp, 1, norm, None, layout, ROW)
            else:
                fill(work)
                rdl.rdl_conv_columns_ex(c, sspec.vp, work.vp, kern.vp, 2, norm, None, layout, ROW)
            rdl.rdl_conv_rows_inverse(c, work.vp, out.vp, w, h, 0, 0, 0)
            got = out.get()
            p.expect(poisoned(got[h:]).all(), f"mode{mode}-{tag}: the guard row was written")
            p.check(f"mode{mode}-{tag}", fp.check_image, got[:h].astype(np.float64), ref_conv,
                    w * h, p.f64)
        p.release(work, out)
    p.release(sspec, di, dk)
    return ker, kspec, kerns[-1][0]


def marked_rows(ih, sparse=False):
    """Every third image row from the second: each marked row's pair partner
    is unmarked (tests/test_stale_state.py). sparse: in the middle third of
    the image only, so that the workgroups of the first and the last rows
    have no marked row and write nothing."""
    if sparse:
        return np.arange(ih // 3, max(2 * ih // 3, ih // 3 + 1), 3)
    return np.arange(min(1, ih - 1), ih, 3)


def stale_model(p, ih, iw, sparse=False):
    """(the model with data in the marked rows only, the same with large
    finite values in every other row)."""
    marked = marked_rows(ih, sparse)
    clean = np.zeros((ih, iw), np.float32)
    clean[marked] = p.noise(marked.size, iw)
    stale = np.full((ih, iw), STALE, np.float32)
    stale[marked] = clean[marked]
    return marked, clean, stale


def check_masked(p, ker, kspec):
    """rdl_conv_rows_forward_masked and the masked column pass: the dense
    result of the marked rows' data, whatever the unmarked image rows and the
    rows of the work buffer that no workgroup writes hold."""
    rdl, c, w, h = p.sess.rdl, p.c, p.w, p.h
    (ox, iw), (oy, ih) = odd_window(w), odd_window(h)
    marked, clean, stale = stale_model(p, ih, iw)
    mask = np.zeros(h + GUARD_ROWS, np.uint8)
    mask[marked + oy] = 1
    plane = np.zeros((h, w))
    plane[oy:oy + ih, ox:ox + iw] = clean
    ref = np.fft.irfft2(np.fft.rfft2(plane) * np.fft.rfft2(ker.astype(np.float64)), s=(h, w))
    dm, dmask = p.array(stale), p.array(mask, dtype=np.uint8)
    work = p.spectrum(stale=True)
    out = p.array(shape=(h + 1, w))
    fill(out)
    norm = C.c_double(1.0 / (w * h) if p.f64 else float(np.float32(1.0 / (w * h))))
    rdl.rdl_conv_rows_forward_masked(c, dm.vp, iw, ih, ox, oy, work.vp, dmask.vp)
    rdl.rdl_conv_columns_ex(c, work.vp, work.vp, kspec.vp, 1, norm, dmask.vp, ROW, ROW)
    rdl.rdl_conv_rows_inverse(c, work.vp, out.vp, w, h, 0, 0, 0)
    got = out.get()
    p.expect(poisoned(got[h:]).all(), "masked: the guard row was written")
    p.check("masked-mode1", fp.check_image, got[:h].astype(np.float64), ref, w * h, p.f64)
    p.release(dm, dmask, work, out)


def check_correction(p, ker, kspec, kspec_cm, windows, peak_refused=False):
    """rdl_conv_convolve_subtract (float64 planes) as CorrectResidualDirty runs
    it: a row mask with stale unmarked rows and none, the kernel in both
    layouts, the work buffer pre-filled with large finite values, a guard row
    after the residual; the float kernel spectrum on convolution-column plans."""
    sess, rdl, c, w, h = p.sess, p.sess.rdl, p.c, p.w, p.h
    kref = {0: np.fft.rfft2(ker.astype(np.float64))}
    kerns = {(0, ROW): kspec, (0, COL): kspec_cm}
    if p.fast & fp.RDL_CONV_FAST_CONVD:  # numpy multiplies by the same float values
        k32 = p.array(shape=(p.nu, h), dtype=np.complex64)
        rdl.rdl_complex_narrow(sess.h, k32.vp, kspec_cm.vp, C.c_size_t(p.nu * h))
        kerns[(1, COL)] = k32
        kref[1] = k32.get().T.astype(np.complex128)
    nbytes = sess.rdl.lib.rdl_conv_convolve_subtract_bytes(c)
    assert nbytes == p.nu * h * 16  # row-major: no tiled correction on these planes
    for tag, (ox, oy, iw, ih) in windows:
        dense = p.noise(ih, iw)
        for masked, (kf, layout) in (("every-third", (0, COL)), (None, (0, ROW)),
                                     ("sparse", (0, COL)), ("every-third", (1, COL)),
                                     (None, (1, COL)), ("sparse", (1, COL))):
            if (kf, layout) not in kerns:
                continue
            model = upload = dense
            if masked:
                marked, model, upload = stale_model(p, ih, iw, masked == "sparse")
                mask = np.zeros(h + GUARD_ROWS, np.uint8)
                mask[marked + oy] = 1
                dmask = p.array(mask, dtype=np.uint8)
            plane = np.zeros((h, w))
            plane[oy:oy + ih, ox:ox + iw] = model
            ref = np.fft.irfft2(np.fft.rfft2(plane) * kref[kf], s=(h, w))
            residual = p.noise(ih, iw)
            guarded = np.full((ih + 1, iw), 7.0, np.float32)
            guarded[:ih] = residual
            dres, dmod, work = p.array(guarded), p.array(upload), p.spectrum(stale=True)
            args = (c, dmod.vp, iw, ih, ox, oy, kerns[(kf, layout)].vp, layout, kf,
                    C.c_double(1.0 / (w * h)), dmask.vp if masked else None, work.vp)
            rdl.rdl_conv_convolve_subtract(*args, dres.vp)
            got = dres.get()
            name = f"correction-{tag}-{masked + '-mask' if masked else 'dense'}" + \
                ("-kf32" if kf else "")
            p.expect(np.all(got[ih:] == 7.0), f"{name}: the guard row was written")
            p.check(name, fp.check_correction, got[:ih], residual,
                    ref[oy:oy + ih, ox:ox + iw], float(np.abs(ref).max()))
            if peak_refused and not masked and kf == 0:
                # no compile-time rows: the correction runs unfused, nothing
                # is queued for the peak, RDL_NOT_FUSED (rdl_hip.h)
                dres.upload(guarded)
                rc = sess.rdl.lib.rdl_conv_convolve_subtract_peak(*args, dres.vp, 0, 0, 1, None, 1, 1)
                p.expect(rc == RDL_NOT_FUSED, f"{name}: the peak form returned {rc}")
                p.expect(np.array_equal(dres.get().view(np.uint32), got.view(np.uint32)),
                         f"{name}: the peak form's residual differs")
            p.release(dres, dmod, work, *((dmask,) if masked else ()))


def check_columns_window(p, kspec):
    """rdl_conv_columns_window into a separate, poisoned output: the window's
    rows are rdl_conv_columns_ex mode 1's, bit for bit; a float64
    convolution-column plan leaves every other row unwritten, any other plan
    writes them all (rdl_hip.h)."""
    rdl, c, w, h = p.sess.rdl, p.c, p.w, p.h
    convd = bool(p.fast & fp.RDL_CONV_FAST_CONVD)
    di = p.array(p.noise(h, w))
    rows, full = p.spectrum(poison=True), p.spectrum(poison=True)
    norm = C.c_double(1.0 / (w * h))
    rdl.rdl_conv_rows_forward(c, di.vp, w, h, 0, 0, rows.vp)
    rdl.rdl_conv_columns_ex(c, rows.vp, full.vp, kspec.vp, 1, norm, None, ROW, ROW)
    f = p.rows(full).view(np.uint8).reshape(h, -1)
    p.expect(not (f == 0xff).all(axis=1).any(), "columns mode 1 left a row unwritten")
    for tag, (oy, ih) in (("odd", odd_window(h)), ("even", even_window(h))):
        win = p.spectrum(poison=True)
        rdl.rdl_conv_columns_window(c, rows.vp, win.vp, kspec.vp, norm, None, ROW, oy, ih, 0)
        g = p.rows(win).view(np.uint8).reshape(h, -1)
        p.release(win)
        inside = np.zeros(h, bool)
        inside[oy:oy + ih] = True
        p.expect(np.array_equal(g[inside], f[inside]),
                 f"columns-window-{tag}: the window's rows differ from mode 1's")
        if convd:
            p.expect((g[~inside] == 0xff).all(),
                     f"columns-window-{tag}: a row outside the window was written")
        else:
            p.expect(np.array_equal(g[~inside], f[~inside]),
                     f"columns-window-{tag}: the rows outside the window differ from mode 1's")
    p.release(di, rows, full)


def check_peak_refused(p):
    """rdl_conv_rows_inverse_peak needs compile-time rows: refused before any
    launch (the output keeps its fill)."""
    spec, out = p.spectrum(), p.array(shape=(p.h, p.w))
    fill(out)
    rc = p.sess.rdl.lib.rdl_conv_rows_inverse_peak(p.c, spec.vp, out.vp, p.w, p.h, 0, 0, 0, 0, 1,
                                                   None, 1)
    p.expect(rc == RDL_ERR_UNSUPPORTED, f"rdl_conv_rows_inverse_peak returned {rc}")
    p.expect(poisoned(out.get()).all(), "rdl_conv_rows_inverse_peak wrote its output")
    p.release(spec, out)


def windows_of(w, h):
    (ox, iw), (oy, ih) = odd_window(w), odd_window(h)
    return ox, oy, iw, ih


# ------------------------------------------------------------------- the sweep
def sweep_cases():
    out = []
    for f64 in (False, True):
        _, cover, chosen = lp.sweep_lengths(PLANNER, f64, TABLES)
        for n in chosen:
            out.append(("rows", n, n, lp.height_for_rows(PLANNER, TABLES, n, f64), f64))
            out.append(("cols", n, lp.width_for_columns(PLANNER, TABLES, n, f64), n, f64))
        out.append(("cols", cover[0], 2, cover[0], f64))  # two columns: idle blocks
    return out


SWEEP = sweep_cases()


@pytest.mark.parametrize("axis,n,w,h,f64", SWEEP,
                         ids=[f"{PREC[f64]}-{axis}{n}-{w}x{h}" for axis, n, w, h, f64 in SWEEP])
def test_runtime_plan(sess, axis, n, w, h, f64):
    plan = PLANNER.plane(w, h, f64)
    assert plan.ok and fp.expected_fast(TABLES, w, h, f64) == 0
    if axis == "rows":  # two workgroups at least, the last partial, an unpaired last row
        pairs = (h + 1) // 2
        assert h % 2 == 1 and pairs > plan.row_count and (pairs % plan.row_count or
                                                          plan.row_count == 1)
    elif w > 2:         # more than a tile per XCD slot, a partial last tile, idle blocks
        tiles = -(-(w // 2 + 1) // plan.col_count)
        assert tiles > 8 and (plan.col_count == 1 or (w // 2 + 1) % plan.col_count)
    p = Plane(sess, w, h, f64, AUTO, [(f"{axis}-{PREC[f64]}", n)])
    try:
        assert p.fast == 0 and not p.split
        check_rows_forward(p)
        check_rows_inverse(p)
        ker, kspec, kspec_cm = check_forward_and_modes(p)
        check_masked(p, ker, kspec)
        if f64:
            check_correction(p, ker, kspec, kspec_cm, [("odd", windows_of(w, h))])
        check_peak_refused(p)
    finally:
        finish(p)


def test_sweep_covers_every_class():
    k = PLANNER.constants()
    for f64 in (False, True):
        acc = PLANNER.accepted(f64)
        classes, cover, chosen = lp.sweep_lengths(PLANNER, f64, TABLES)
        for axis in ("rows", "cols"):
            ran = [n for a, n, w, h, f in SWEEP if a == axis and f == f64]
            assert set().union(*(lp.pass_classes(acc[n], k) for n in ran)) == classes
            assert set(lp.ALWAYS) <= set(ran)
        sclasses, scover = lp.split_lengths(PLANNER, TABLES, f64)
        assert set().union(*(lp.split_classes(PLANNER, acc[n], TABLES) for n in scover)) == sclasses


# ------------------------------------------------------------ the split passes
def split_cases():
    out = []
    for f64 in (False, True):
        acc = PLANNER.accepted(f64)
        for n in lp.split_lengths(PLANNER, TABLES, f64)[1]:
            out.append((n, lp.split_width(acc[n], TABLES), f64))
    return out


SPLITS = split_cases()


@pytest.mark.parametrize("n,w,f64", SPLITS, ids=[f"{PREC[f64]}-{n}-w{w}" for n, w, f64 in SPLITS])
def test_split_columns(sess, n, w, f64):
    plan = PLANNER.plane(w, n, f64, SPLIT)
    assert plan.ok and plan.split
    p = Plane(sess, w, n, f64, SPLIT, [(f"splitcols-{PREC[f64]}", n)])
    try:
        assert p.fast == 0 and p.split
        check_forward_and_modes(p)
    finally:
        finish(p)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_split_refused_without_two_factors(sess, f64):
    acc = PLANNER.accepted(f64)
    refused = [n for n, q in acc.items() if not q.can_split]
    assert set(refused) >= {2, 3, 5, 7, 9, 15} and len(refused) == 15
    for n in refused:
        c = C.c_void_p()
        rc = sess.rdl.lib.rdl_conv_create_ex(sess.h, 64, n, int(f64), SPLIT, C.byref(c))
        assert rc == RDL_ERR_UNSUPPORTED and not c.value, (n, rc)


# -------------------------------------------------------------- mixed dispatch
def mixed_cases():
    """(w, h, f64, the runtime axis, role): one axis on a compile-time plan,
    the smallest of its family, the other on runtime lengths 30 and 45."""
    rows32, rows64 = fp.lengths(TABLES, "rows_f32")[0], fp.lengths(TABLES, "rows_f64")[0]
    convd = fp.lengths(TABLES, "convd")[0]
    plain = sorted(set(fp.lengths(TABLES, "cols_f64")) - set(fp.lengths(TABLES, "convd")))
    out = []
    for n in (30, 45):
        out.append((rows32, n, False, "cols", "cols-f32|fast-rows"))
        out.append((rows64, n, True, "cols", "cols-f64|fast-rows"))
        out.append((n, convd, True, "rows", "rows-f64|convd"))
    if plain:
        out.append((30, plain[0], True, "rows", "rows-f64|fast-cols"))
    return out


MIXED = mixed_cases()


@pytest.mark.parametrize("w,h,f64,axis,role", MIXED,
                         ids=[f"{role.replace('|', '-')}-{w}x{h}" for w, h, f64, axis, role in MIXED])
def test_mixed_dispatch(sess, w, h, f64, axis, role):
    p = Plane(sess, w, h, f64, AUTO, [(role, h if axis == "cols" else w)])
    try:
        expected = fp.expected_fast(TABLES, w, h, f64)
        assert p.fast == expected, (p.fast, expected)
        if axis == "cols":   # compile-time rows, not tiled; runtime columns
            assert p.fast == fp.RDL_CONV_FAST_ROWS
        else:                # runtime rows; compile-time columns
            assert p.fast & fp.RDL_CONV_FAST_COLUMNS and not p.fast & fp.RDL_CONV_FAST_ROWS
            assert bool(p.fast & fp.RDL_CONV_FAST_CONVD) == role.endswith("convd")
        check_rows_forward(p)
        check_rows_inverse(p)
        ker, kspec, kspec_cm = check_forward_and_modes(p)
        if f64:
            (ox, iw), (oy, ih) = odd_window(w), odd_window(h)
            assert oy % 2 == 1 and ih % 2 == 1
            windows = [("odd-oy", (ox, oy, iw, ih)), ("even-oy", (ox, oy + 1, iw, ih - 2))]
            check_correction(p, ker, kspec, kspec_cm, windows, peak_refused=axis == "rows")
            check_columns_window(p, kspec)
        if axis == "rows":
            check_peak_refused(p)
    finally:
        finish(p)
