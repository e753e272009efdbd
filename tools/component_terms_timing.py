"""The spectral fit of ComponentList.write on the host (fitter.fit per
component, the reference's loop) against the batched device fit
(rdl_component_terms), on synthetic lists of the sizes a deep joined clean
leaves: 109,233 components of 8 channels on a 4096^2 image (the joined C3 run
to threshold) and 937,217 on 8192^2 (the tiled run), for the log-polynomial,
polynomial and forced fits of 3 terms. The forced fit reads two term planes of
the image's size, as a Radler's does.

Per mode and size, after a warm-up of each path:
  host    wall clock of ComponentList.fit_terms(fitter): the loop alone;
  device  wall clock of ComponentList.fit_terms(fitter, device=True): the
          transposition, the copies to the device, the kernel, the copy back
          (it ends in a synchronous copy) and, for the forced fit, the
          upload of the term planes, which a write does once, and
  kernel  HIP-event time of rdl_component_terms alone on resident data (the
          C-ABI's timing family), for the share the copies take;
  write   wall clock of the whole ComponentList.write, fit and text, through
          each path (one run after a warm-up), for the share the fit takes.
The host loop runs nothing on the GPU and the device path ends in a
synchronous copy, so both are timed by the host clock; HIP events time the
kernel. ComponentList.write_sources fits on the device because `device` beats
`host` in every mode at the smaller size.

    python tools/component_terms_timing.py [--out FILE] [--reps K]
"""
import argparse
import ctypes as C
import math
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from radler_import import radler as rd  # noqa: E402
from rdl_lib import Session, logpoly  # noqa: E402

SIZES = {109_233: 4096, 937_217: 8192}  # components: image side
N_CH, N_TERMS = 8, 3
FREQS = [1.0e8 + 1.0e7 * c for c in range(N_CH)]
WEIGHTS = [1.0] * N_CH


class ForcedTerms(C.Structure):
    _fields_ = [("d_planes", C.c_void_p), ("plane_stride", C.c_size_t), ("pitch", C.c_uint32),
                ("rows", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32),
                ("weights", C.c_float * 16)]


def make_list(n, W, seed):
    """n components on distinct pixels of a W x W image; power-law spectra
    with 1 % noise."""
    rng = np.random.default_rng(seed)
    pixels = np.sort(rng.choice(W * W, n, replace=False))
    lg = np.log10(np.asarray(FREQS) / np.mean(FREQS))[None, :]
    values = rng.uniform(0.01, 2.0, (n, 1)) * 10.0 ** (rng.uniform(-1.5, 0.5, (n, 1)) * lg)
    values = (values * (1.0 + 0.01 * rng.standard_normal(values.shape))).astype(np.float32)
    cl = rd.ComponentList(W, W, 1, N_CH)
    for p, v in zip(pixels.tolist(), values.tolist()):
        cl.add(p % W, p // W, 0, v)
    cl.merge_duplicates()
    assert cl.component_count(0) == n
    return cl, pixels, values


def fitter_of(mode, planes):
    f = rd.SpectralFitter(getattr(rd.SpectralFittingMode, mode), N_TERMS, FREQS, WEIGHTS)
    if mode == "forced_terms":
        f.set_forced_terms(list(planes))
    return f


def timed(fn, reps):
    fn()  # warm-up
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t), float(np.median(t))


def kernel_time(sess, mode, fitter, pixels, values, planes, W, reps):
    """HIP-event milliseconds per call of rdl_component_terms on resident data"""
    lib, n = sess.rdl.lib, len(values)
    lib.rdl_timing_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    d_v = sess.array(np.ascontiguousarray(values.T))
    d_t = sess.array(shape=(N_TERMS, n))
    fit_map = np.ascontiguousarray(fitter.fit_matrix, np.float64)
    fitted = np.ones(N_CH, np.uint8)
    lp = logpoly(FREQS, WEIGHTS, N_TERMS)
    for c in range(N_CH):
        lp.lg[c] = math.log10(FREQS[c] / fitter.reference_frequency)
    forced, d_p = ForcedTerms(), None
    x = np.ascontiguousarray(pixels % W, np.uint32)
    y = np.ascontiguousarray(pixels // W, np.uint32)
    if mode == "forced_terms":
        d_p = sess.array(planes)
        forced.d_planes, forced.plane_stride, forced.pitch, forced.rows = d_p.ptr, W * W, W, W
        for c in range(N_CH):
            forced.weights[c] = WEIGHTS[c]
    code = {"polynomial": 0, "log_polynomial": 1, "forced_terms": 2}[mode]
    u32 = C.POINTER(C.c_uint32)

    def call():
        sess.rdl.rdl_component_terms(
            sess.h, C.c_uint32(code), C.c_uint32(N_CH), C.c_uint32(N_TERMS),
            fit_map.ctypes.data_as(C.POINTER(C.c_double)) if code == 0 else None,
            fitted.ctypes.data_as(C.POINTER(C.c_uint8)) if code == 0 else None,
            C.byref(lp) if code else None, C.byref(forced) if code == 2 else None,
            C.c_uint32(W), C.c_uint32(W), x.ctypes.data_as(u32), y.ctypes.data_as(u32),
            d_v.vp, C.c_size_t(n), C.c_size_t(n), d_t.vp, C.c_size_t(n))

    call()
    sess.sync()
    sess.rdl.rdl_timing_enable(sess.h, 1)
    lib.rdl_timing_reset(sess.h)
    for _ in range(reps):
        call()
    sess.sync()
    ms, k, b = C.c_double(), C.c_uint64(), C.c_double()
    lib.rdl_timing_get(sess.h, b"component_terms", C.byref(ms), C.byref(k), C.byref(b))
    sess.rdl.rdl_timing_enable(sess.h, 0)
    terms = d_t.get().T.copy()
    for a in (d_v, d_t, d_p):
        if a is not None:
            a.free()
    return ms.value / max(k.value, 1), terms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    sess = Session(0)
    rng = np.random.default_rng(1)
    say(f"# spectral fit of ComponentList.write: {N_CH} channels, {N_TERMS} terms; seconds are "
        f"min / median of {args.reps} runs after a warm-up")
    say("# host = fitter.fit per component; device = transpose + H2D + rdl_component_terms + "
        "D2H + transpose; kernel = HIP events around rdl_component_terms alone")
    say(f"{'mode':15s} {'components':>10s} {'image':>6s} {'host s':>17s} {'device s':>17s} {'kernel ms':>10s} "
        f"{'host/device':>11s} {'max |dev-host|':>14s} {'write host s':>12s} {'write dev s':>11s}")
    for n in args.sizes:
        W = SIZES.get(n, 1024)
        planes = rng.uniform(-1.2, 0.4, (N_TERMS - 1, W, W)).astype(np.float32)
        cl, pixels, values = make_list(n, W, seed=n)
        for mode in ("log_polynomial", "polynomial", "forced_terms"):
            fitter = fitter_of(mode, planes)
            host = timed(lambda: cl.fit_terms(0, fitter), max(2, args.reps // 2))
            device = timed(lambda: cl.fit_terms(0, fitter, device=True), args.reps)
            t_host = cl.fit_terms(0, fitter)
            t_dev = cl.fit_terms(0, fitter, device=True)
            k_ms, t_k = kernel_time(sess, mode, fitter, pixels, values, planes, W, args.reps)
            assert np.array_equal(t_k, t_dev)  # the same kernel on the same values
            err = float(np.max(np.abs(t_dev.astype(np.float64) - t_host.astype(np.float64))))
            with tempfile.TemporaryDirectory() as tmp:
                path, scale = os.path.join(tmp, "sources.txt"), math.pi / 180.0 / 3600.0
                write = [timed(lambda: cl.write(path, fitter, [0.0], scale, scale, 0.3, 0.4,
                                                device=dev), 1)[0] for dev in (False, True)]
            say(f"{mode:15s} {n:10d} {W:6d} {host[0]:8.4f}/{host[1]:8.4f} {device[0]:8.4f}/"
                f"{device[1]:8.4f} {k_ms:10.3f} {host[0] / device[0]:11.2f} {err:14.3g} "
                f"{write[0]:12.3f} {write[1]:11.3f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
