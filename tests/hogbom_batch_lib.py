"""ctypes mirrors, inputs and the two runners shared by the tests of
rdl_hogbom_batch_run (test_hogbom_batch_api.py, test_hogbom_batch_gpu.py).

run_batch() calls the batch entry point over stacks whose plane strides are
larger than a plane, with sentinel values in the gaps; run_loop() cleans the
same planes one at a time with rdl_find_peak + rdl_hogbom_run, the path the
batch must reproduce bit for bit. Both return a Run.

Run as a program (python hogbom_batch_lib.py OUT.npz) it runs resume_case()
through the batch and saves the Run: the child process of the resume test,
which sets RDL_HOGBOM_BATCH_CHUNK in its environment.
"""
import ctypes as C
import sys
import types

import numpy as np

from rdl_lib import HogbomParams, HogbomResult, Peak, integration

FILL = 0xffffffff        # the trace buffers before a call
OUT_FILL = 0xab          # every byte of the result slots before a call
GAP = np.float32(12345.0)  # between the planes of a stack
GAP_MASK = 7             # non-zero: a mask read from a gap allows the pixel
PAD = 37                 # elements between two planes
MAX_PIXELS = 1 << 20
LOAD_RULE = 1            # RDL_HOGBOM_BATCH_LOAD_RULE


class BatchParams(C.Structure):
    """rdl_hogbom_batch_params (include/rdl_hip.h)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("n_planes", C.c_uint32),
                ("flags", C.c_uint32),
                ("d_residuals", C.c_void_p), ("residual_stride", C.c_size_t),
                ("d_models", C.c_void_p), ("model_stride", C.c_size_t),
                ("d_psfs", C.c_void_p), ("psf_stride", C.c_size_t),
                ("d_mask", C.c_void_p), ("mask_stride", C.c_size_t),
                ("gain", C.c_float), ("major_loop_gain", C.c_float),
                ("divergence_limit", C.c_float), ("allow_negative", C.c_int32),
                ("stop_on_negative", C.c_int32), ("h_border", C.c_uint32),
                ("v_border", C.c_uint32)]


class BatchOut(C.Structure):
    """rdl_hogbom_batch_out."""
    _fields_ = [("result", HogbomResult), ("start", Peak), ("first_threshold", C.c_float),
                ("reserved", C.c_uint32)]


assert C.sizeof(BatchOut) == 56 and C.sizeof(BatchParams) == 112

# the compared fields of a BatchOut, as one row of uint64 (floats by their bits)
OUT_FIELDS = ("iteration", "peak", "x", "y", "found", "diverging", "start_value", "start_x",
              "start_y", "start_found", "first_threshold")


def f32bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def out_row(result, start, first_threshold):
    return [int(result.iteration), f32bits(result.peak), int(result.x), int(result.y),
            int(result.found) & 0xffffffff, int(result.diverging) & 0xffffffff,
            f32bits(start.value), int(start.x), int(start.y), int(start.found) & 0xffffffff,
            f32bits(first_threshold)]


def first_threshold(threshold, start_value, major_loop_gain):
    """generic_clean.cc:138-142 in float with MajorIterationThreshold() = 0."""
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        by_gain = f32(abs(f32(start_value)) * f32(f32(1.0) - f32(major_loop_gain)))
    major = by_gain if f32(0.0) < by_gain else f32(0.0)  # std::max(0.0f, by_gain)
    return major if major > f32(threshold) else f32(threshold)


def options(**kw):
    """The shared parameters of a batch, with the defaults of these tests."""
    o = dict(gain=0.1, major_loop_gain=1.0, divergence_limit=4.0, allow_negative=1,
             stop_on_negative=0, h_border=0, v_border=0)
    assert set(kw) <= set(o), kw
    o.update(kw)
    return types.SimpleNamespace(**o)


def make_psf(w, h, seed=0):
    """A peak of exactly 1 at (w / 2, h / 2) over decaying ripples of both
    signs, a little different for every seed."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    dx, dy = xx - w // 2, yy - h // 2
    r2 = dx * dx + dy * dy
    psf = np.exp(-r2 / 4.5) + 0.08 * np.cos(0.9 * dx + 0.4 * dy + 0.1 * seed) * np.exp(
        -r2 / (2.0 * (0.2 * max(w, h) + 1.0) ** 2))
    psf[h // 2, w // 2] = 1.0
    return psf.astype(np.float32)


def make_planes(w, h, n_planes, seed=1):
    """n_planes residual planes: a few sources of both signs, each the PSF
    shifted, over noise; no two planes alike."""
    rng = np.random.default_rng(seed)
    psf = make_psf(w, h).astype(np.float64)
    planes = np.empty((n_planes, h, w), np.float32)
    for b in range(n_planes):
        img = 0.03 * rng.standard_normal((h, w))
        for _ in range(1 + (w * h > 16) * 5):
            amp = rng.uniform(0.4, 1.5) * (1.0 if rng.random() < 0.7 else -1.0)
            img += amp * np.roll(psf, (int(rng.integers(h)), int(rng.integers(w))), axis=(0, 1))
        planes[b] = img
    return planes


class Run:
    """What one side produced: residual and model [B, h, w], out [B, 11]
    uint64 (OUT_FIELDS), trace [B, cap, 2] uint32, and for the batch the raw
    bytes of every result slot."""

    def __init__(self, residual, model, out, trace, raw=None):
        self.residual, self.model, self.out, self.trace, self.raw = residual, model, out, trace, raw

    def field(self, name):
        return self.out[:, OUT_FIELDS.index(name)]

    def iterations(self):
        return self.field("iteration").astype(np.int64)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, planes=None):
    """Bit for bit: residual, model, trace and every result field."""
    sel = slice(None) if planes is None else planes
    for b, (g, w_) in enumerate(zip(got.out[sel], want.out[sel])):
        assert list(g) == list(w_), (b, dict(zip(OUT_FIELDS, zip(g, w_))))
    assert np.array_equal(got.trace[sel], want.trace[sel])
    assert np.array_equal(bits(got.residual[sel]), bits(want.residual[sel]))
    assert np.array_equal(bits(got.model[sel]), bits(want.model[sel]))


def per_plane(v, n_planes, dtype):
    a = np.empty(n_planes, dtype)
    a[:] = v
    return a


def stack(planes, n_planes, dtype, gap):
    """[B, h, w] as rows of h * w + PAD elements, or one shared plane (stride 0)."""
    planes = np.ascontiguousarray(planes, dtype)
    if planes.ndim == 2:
        return planes.reshape(1, -1).copy(), 0
    n = planes.shape[1] * planes.shape[2]
    s = np.full((n_planes, n + PAD), gap, dtype)
    s[:, :n] = planes.reshape(n_planes, n)
    return s, n + PAD


def run_batch(sess, residuals, models, psfs, masks, opt, thresholds, iteration_start,
              max_iterations, active=1, trace_cap=64, null_trace=False, flags=0):
    """rdl_hogbom_batch_run over padded stacks. psfs and masks: [h, w] for one
    shared plane or [B, h, w]; masks None for no mask. The per-plane values
    may be scalars. Asserts that the gaps between the planes come back as
    they were and that nothing reads as written outside the stacks."""
    n_planes, h, w = residuals.shape
    n = w * h
    keep = []

    def dev(a):
        keep.append(sess.array(a, dtype=a.dtype))
        return keep[-1]

    try:
        res, res_stride = stack(residuals, n_planes, np.float32, GAP)
        mod, mod_stride = stack(models, n_planes, np.float32, GAP)
        psf, psf_stride = stack(psfs, n_planes, np.float32, GAP)
        p = BatchParams()
        p.width, p.height, p.n_planes, p.flags = w, h, n_planes, flags
        dres, dmod, dpsf = dev(res), dev(mod), dev(psf)
        p.d_residuals, p.residual_stride = dres.ptr, res_stride
        p.d_models, p.model_stride = dmod.ptr, mod_stride
        p.d_psfs, p.psf_stride = dpsf.ptr, psf_stride
        if masks is not None:
            msk, p.mask_stride = stack(masks, n_planes, np.uint8, GAP_MASK)
            dmsk = dev(msk)
            p.d_mask = dmsk.ptr
        p.gain, p.major_loop_gain = opt.gain, opt.major_loop_gain
        p.divergence_limit = opt.divergence_limit
        p.allow_negative, p.stop_on_negative = opt.allow_negative, opt.stop_on_negative
        p.h_border, p.v_border = opt.h_border, opt.v_border
        thr = per_plane(thresholds, n_planes, np.float32)
        it0 = per_plane(iteration_start, n_planes, np.uint64)
        cap = per_plane(max_iterations, n_planes, np.uint64)
        act = per_plane(active, n_planes, np.uint8)
        out = (BatchOut * n_planes)()
        C.memset(out, OUT_FILL, C.sizeof(out))
        trace = np.full((n_planes, max(trace_cap, 1), 2), FILL, np.uint32)
        sess.rdl.rdl_hogbom_batch_run(
            sess.h, C.byref(p), thr.ctypes.data_as(C.c_void_p), it0.ctypes.data_as(C.c_void_p),
            cap.ctypes.data_as(C.c_void_p), act.ctypes.data_as(C.c_void_p), out,
            None if null_trace else trace.ctypes.data_as(C.c_void_p), C.c_uint64(trace_cap))
        res_back, mod_back = dres.get(), dmod.get()
        assert np.all(res_back[:, n:] == GAP) and np.all(mod_back[:, n:] == GAP)
        assert np.array_equal(bits(dpsf.get()), bits(psf))
        if masks is not None:
            assert np.array_equal(dmsk.get(), msk)
        rows = np.array([out_row(o.result, o.start, o.first_threshold) for o in out], np.uint64)
        raw = np.frombuffer(bytes(out), np.uint8).reshape(n_planes, C.sizeof(BatchOut))
        return Run(res_back[:, :n].reshape(n_planes, h, w).copy(),
                   mod_back[:, :n].reshape(n_planes, h, w).copy(), rows, trace, raw)
    finally:
        for a in keep:
            a.free()


def run_loop(sess, residuals, models, psfs, masks, opt, thresholds, iteration_start,
             max_iterations, active=1, trace_cap=64, null_trace=False):
    """The same planes one at a time: rdl_find_peak, the threshold of
    generic_clean.cc:138-142, rdl_hogbom_run. An inactive plane is returned
    as given, with an all-zero result row."""
    n_planes, h, w = residuals.shape
    thr = per_plane(thresholds, n_planes, np.float32)
    it0 = per_plane(iteration_start, n_planes, np.uint64)
    cap = per_plane(max_iterations, n_planes, np.uint64)
    act = per_plane(active, n_planes, np.uint8)
    res_out, mod_out = np.array(residuals, np.float32), np.array(models, np.float32)
    rows = np.zeros((n_planes, len(OUT_FIELDS)), np.uint64)
    traces = np.full((n_planes, max(trace_cap, 1), 2), FILL, np.uint32)
    for b in range(n_planes):
        if not act[b]:
            continue
        psf = psfs if psfs.ndim == 2 else psfs[b]
        mask = None if masks is None else masks if masks.ndim == 2 else masks[b]
        dres, dmod, dpsf = sess.array(res_out[b]), sess.array(mod_out[b]), sess.array(psf)
        dmask = None if mask is None else sess.array(np.ascontiguousarray(mask, np.uint8),
                                                     dtype=np.uint8)
        try:
            found, x, y, value = sess.find_peak(dres, w, h, opt.allow_negative,
                                                hb=opt.h_border, vb=opt.v_border, dmask=dmask)
            start = Peak(value, x, y, int(found))
            first = first_threshold(thr[b], value, opt.major_loop_gain)
            p = HogbomParams()
            p.width, p.height, p.n_images, p.n_pol = w, h, 1, 1
            p.integ = integration(1, 1, None, 1.0, mode=1)
            p.gain, p.threshold = opt.gain, first
            p.initial_max = abs(np.float32(value))
            p.divergence_limit = opt.divergence_limit
            p.iteration_start, p.max_iterations = int(it0[b]), int(cap[b])
            p.allow_negative, p.stop_on_negative = opt.allow_negative, opt.stop_on_negative
            p.h_border, p.v_border = opt.h_border, opt.v_border
            p.d_mask = None if dmask is None else dmask.ptr
            p.start_x, p.start_y, p.start_value, p.start_found = x, y, value, int(found)
            r = HogbomResult()
            sess.rdl.rdl_hogbom_run(
                sess.h, dres.vp, dmod.vp, dpsf.vp, C.byref(p), C.byref(r),
                None if null_trace else traces[b].ctypes.data_as(C.c_void_p),
                C.c_uint64(trace_cap))
            res_out[b], mod_out[b] = dres.get(), dmod.get()
            rows[b] = out_row(r, start, first)
        finally:
            for a in (dres, dmod, dpsf, dmask):
                if a is not None:
                    a.free()
    return Run(res_out, mod_out, rows, traces)


def resume_case():
    """The case of the resume test: five 40 x 33 planes with a shared mask
    that stop after different counts, some of them far above any chunk the
    test sets."""
    w, h, n_planes = 40, 33, 5
    residuals = make_planes(w, h, n_planes, seed=31)
    mask = np.ones((h, w), np.uint8)
    mask[::5, ::3] = 0
    return dict(residuals=residuals, models=np.zeros_like(residuals), psfs=make_psf(w, h),
                masks=mask, opt=options(h_border=2, v_border=1),
                thresholds=[0.0, 0.2, 0.0, 0.05, 0.0], iteration_start=[0, 3, 0, 0, 9],
                max_iterations=[23, 60, 1, 45, 16], trace_cap=32)


def main(path):
    from rdl_lib import Session
    sess = Session(0)
    try:
        run = run_batch(sess, **resume_case())
    finally:
        sess.close()
    np.savez(path, residual=run.residual, model=run.model, out=run.out, trace=run.trace)


if __name__ == "__main__":
    main(sys.argv[1])
