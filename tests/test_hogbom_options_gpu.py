"""The Högbom loop under every option of rdl_hogbom_run.

rdl_hogbom_run (HogbomPass<NI> + HogbomStep, csrc/hip/clean.hip) against the
oracle's Högbom branch of GenericClean (OracleAlgorithm kind 0 without the
sub-minor loop) for each HogbomPass instantiation (1, 4, 16 and 64 images),
more than one row per block, and each option of the ABI: mask, borders, RMS
factors, the sign rules, divergence, the iteration window, the trace cap and a
NULL trace, the three integration modes with polarizations and weights, the
spectral map, and the log-polynomial and forced-term fits; the in-loop "no
qualifying pixel" branches with and without a mask; a NaN pixel; and runs
that end one side or the other of the host's batch of 32 queued iterations.

One helper (run_case, a Pair stepped once) runs a case on both sides. The
device call's start peak is computed on the CPU (the linear integration, the
RMS factors, the oracle's peak finder) and asserted to be the oracle run's
starting peak, so the comparison isolates the loop. Asserted bit for bit:
iteration, found, diverging, the final peak and its position when found, the
trace (every entry past min(components, trace_cap) still holding the fill
value), every residual plane and every model plane. The log-polynomial and
forced-term fits: identical trace, planes and peak within 2e-5 x
max|dirties| (test_spectral.py's bound for that fitter), valid because every
decision of the oracle's run keeps a relative margin of 1e-4 (asserted).
Each case asserts on the oracle's result alone that its option did
something.

Not covered, and why:
* pol_mask other than all polarizations: the oracle has no
  linked-polarization form to compare with.
* Forced terms that vary over the image, and tiled origins beyond one padded
  plane: test_forced_terms.py runs those through Radler::Perform.
* RDL_INTEGRATE_SQUARED_JOINS and n_pol > 1 together with the
  log-polynomial fits: the fits are tested with n_pol = 1 and the linear
  join only.
* Images of more than 2^31 pixels and the workload's own sizes: every case
  here is a few hundred launches on at most 74 k pixels.
"""
import ctypes as C
import types

import numpy as np
import pytest

from hogbom_cases import border, mask_image, mixed, rms_image, single
from oracle_lib import OracleAlgorithm, get_oracle
from rdl_lib import ForcedLogPoly, HogbomParams, HogbomResult, Session, integration, logpoly

pytestmark = pytest.mark.gpu

LOGPOLY = 2  # oracle/spectral.h SpectralFit::mode
FILL = 0xffffffff  # what the trace buffer holds before the call


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def sess():
    s = Session(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def orc():
    return get_oracle()


@pytest.fixture
def ctx(sess, orc):
    return dict(sess=sess, orc=orc)


def FREQS(n):
    return 1.0e8 + 1.0e7 * np.arange(n)


def projector(n_ch, terms, weights, n_pol=1):
    """The weighted polynomial fit-and-evaluate over n_ch channels as a
    matrix (float64 numpy, rounded to float32 once), not symmetric for
    unequal weights; n_pol > 1: its Kronecker product with the identity,
    images ordered channel-major. The channels are spaced geometrically:
    mixed()'s planes are linear in the channel number, and a two-term fit
    over evenly spaced channels would give them back unchanged."""
    wts = np.asarray(weights, np.float64)
    f = 1.0e8 * 1.25 ** np.arange(n_ch)
    x = f / (np.sum(f * wts) / np.sum(wts)) - 1.0
    v = np.vander(x, terms, increasing=True)
    p = v @ np.linalg.inv(v.T @ (wts[:, None] * v)) @ (v.T * wts)
    if n_pol > 1:
        p = np.kron(p, np.eye(n_pol))
    p = np.ascontiguousarray(p, np.float32)
    assert not np.array_equal(p, p.T)
    return p


def forced_map(n_ch, weights, term):
    """The forced-term fit of two terms with the same second term at every
    pixel (csrc/hip/logpoly.h ForcedFit) is linear in the values:
    S[c][q] = f_c w_q / sum_j w_j f_j with f_c = 10^(term lg_c)."""
    wts = np.asarray(weights, np.float64)
    lp = logpoly(FREQS(n_ch), wts, 2)
    f = 10.0 ** (term * np.array([lp.lg[c] for c in range(n_ch)]))
    return np.ascontiguousarray(np.outer(f, wts) / np.sum(wts * f), np.float32)


class Pair:
    """One image set cleaned by the oracle and by rdl_hogbom_run side by
    side. step() runs one major iteration's loop on both and compares; a
    second step continues on the same buffers (the oracle's iteration count
    becomes the device call's iteration_start).

    fit: None, ("logpoly", n_terms) or ("forced", term): the second term's
    plane holds `term` at every pixel, which makes the fit the linear map
    forced_map() that the oracle then applies."""

    def __init__(self, ctx, dirties, psfs, *, name=None, n_pol=1, weights=None, pol_factor=1.0,
                 squared_joins=False, mask=None, border_ratio=0.0, rms=None, allow_negative=1,
                 stop_on_negative=0, divergence_limit=4.0, gain=0.1, threshold=0.0, smap=None,
                 fit=None, device=True):
        self.sess, self.orc, self.name = ctx["sess"], ctx["orc"], name
        self.n_img, self.h, self.w = dirties.shape
        self.n_pol, self.n_ch = n_pol, self.n_img // n_pol
        assert psfs.shape == (self.n_ch, self.h, self.w)
        self.wts = None if weights is None else np.asarray(weights, np.float32)
        self.pol_factor, self.squared_joins = pol_factor, squared_joins
        self.mask, self.rms, self.border_ratio = mask, rms, border_ratio
        # GenericClean::ExecuteMajorIteration: stop_on_negative sets allow_negative
        self.allow_negative = 1 if stop_on_negative else allow_negative
        self.stop_on_negative = stop_on_negative
        self.divergence_limit, self.gain, self.threshold = divergence_limit, gain, threshold
        self.smap, self.fit, self.device = smap, fit, device
        self.psfs = np.ascontiguousarray(psfs, np.float32)
        self.res_o = np.array(dirties, np.float32)
        self.mod_o = np.zeros_like(self.res_o)
        self.scale = float(np.nanmax(np.abs(dirties)))
        self.alg = None
        self.iteration = 0
        self.keep = []
        if device:
            self.dres, self.dmod = self.dev(self.res_o), self.dev(self.mod_o)
            self.dpsf = self.dev(self.psfs)

    def dev(self, a, dtype=np.float32):
        self.keep.append(self.sess.array(np.ascontiguousarray(a, dtype), dtype=dtype))
        return self.keep[-1]

    def close(self):
        for a in self.keep:
            a.free()
        self.keep = []

    # ------------------------------------------------------------- oracle
    def settings(self, max_iterations):
        # major_loop_gain = 1 and major_iteration_threshold = 0: the loop's
        # threshold is float(threshold)
        return dict(threshold=self.threshold, major_iteration_threshold=0.0, major_loop_gain=1.0,
                    minor_loop_gain=self.gain, border_ratio=self.border_ratio,
                    divergence_limit=self.divergence_limit, max_iterations=max_iterations,
                    allow_negative=self.allow_negative, stop_on_negative=self.stop_on_negative,
                    use_sub_minor=0, clean_mask=self.mask)

    def oracle_execute(self, max_iterations):
        if self.alg is None:
            self.alg = OracleAlgorithm(self.orc, 0, **self.settings(max_iterations))
            self.alg.set_rms(self.rms)
            if self.fit is not None and self.fit[0] == "logpoly":
                self.alg.set_spectral_fitter(LOGPOLY, self.fit[1], FREQS(self.n_ch),
                                             np.ones(self.n_ch, np.float32))
            elif self.fit is not None:
                self.alg.set_spectral_map(forced_map(self.n_ch, self.wts, self.fit[1]))
            else:
                self.alg.set_spectral_map(self.smap)
        else:
            self.alg.update(**self.settings(max_iterations))
        return self.alg.execute(self.res_o, self.mod_o, self.psfs, self.wts,
                                pol_factor=self.pol_factor, squared_joins=self.squared_joins)

    def find_peak(self, square):
        """GenericClean::FindPeak of the oracle-side residual on the CPU."""
        integ = self.orc.integrate(self.res_o, self.wts, self.n_pol, self.pol_factor,
                                   square=square, squared_joins=self.squared_joins)
        if self.rms is not None:
            integ = integ * self.rms
        has, x, y, v = self.orc.find_peak(integ, bool(self.allow_negative),
                                          hb=border(self.w, self.border_ratio),
                                          vb=border(self.h, self.border_ratio), mask=self.mask)
        return has, x, y, np.float32(v)

    # ------------------------------------------------------------- device
    def device_run(self, start, iteration_start, max_iterations, trace, trace_cap):
        w, h = self.w, self.h
        p = HogbomParams()
        p.width, p.height, p.n_images, p.n_pol = w, h, self.n_img, self.n_pol
        p.integ = integration(self.n_ch, self.n_pol, self.wts, self.pol_factor,
                              mode=2 if self.squared_joins else 1)
        p.gain, p.threshold = self.gain, np.float32(self.threshold)
        p.initial_max = abs(start[3]) if start[0] else 0.0
        p.divergence_limit = self.divergence_limit
        p.iteration_start, p.max_iterations = iteration_start, max_iterations
        p.allow_negative, p.stop_on_negative = self.allow_negative, self.stop_on_negative
        p.h_border, p.v_border = border(w, self.border_ratio), border(h, self.border_ratio)
        if start[0]:
            p.start_found, p.start_x, p.start_y, p.start_value = 1, *start[1:]
        if self.mask is not None:
            p.d_mask = self.dev(self.mask, np.uint8).ptr
        if self.rms is not None:
            p.d_rms = self.dev(self.rms).ptr
        if self.smap is not None:
            p.d_spectral = self.dev(self.smap).ptr
        if self.fit is not None and self.fit[0] == "logpoly":
            lp = logpoly(FREQS(self.n_ch), np.ones(self.n_ch, np.float32), self.fit[1])
            p.logpoly = C.addressof(lp)
        elif self.fit is not None:
            # the term plane inside a larger allocation whose padding holds a
            # value no fit survives: a wrong pitch or origin reads it
            plane = np.full((h + 5, w + 9), 50.0, np.float32)
            plane[3:3 + h, 5:5 + w] = self.fit[1]
            lp = ForcedLogPoly()
            lp.fit = logpoly(FREQS(self.n_ch), self.wts, 2)
            lp.fit.reserved = 1  # RDL_LOGPOLY_FORCED
            t = lp.terms
            t.d_planes, t.plane_stride = self.dev(plane).ptr, plane.size
            t.pitch, t.rows, t.x0, t.y0 = w + 9, h + 5, 5, 3
            for c in range(self.n_ch):
                t.weights[c] = self.wts[c]
            p.logpoly = C.addressof(lp)
        out = HogbomResult()
        self.sess.rdl.rdl_hogbom_run(
            self.sess.h, self.dres.vp, self.dmod.vp, self.dpsf.vp, C.byref(p), C.byref(out),
            None if trace is None else trace.ctypes.data_as(C.c_void_p), C.c_uint64(trace_cap))
        return out, self.dres.get(), self.dmod.get()

    # --------------------------------------------------------------- step
    def step(self, max_iterations, trace_cap=None, null_trace=False, compare_peak=True):
        """Runs to max_iterations on both sides and compares. trace_cap: the
        cap handed to the device call (default: every component fits); the
        buffer always has room for every component. Returns the oracle's run:
        iteration, trace [n, 2], diverging, found, final_peak, start, and the
        planes residual / model (the Pair's own, updated by later steps)."""
        iteration_start = self.iteration
        start = self.find_peak(square=False)
        r, trace_o = self.oracle_execute(max_iterations)
        trace_o = trace_o[:, :2]
        n_it = int(r.iteration_number) - iteration_start
        assert n_it == len(trace_o)
        assert bool(r.has_starting_peak) == start[0]
        if start[0]:
            assert bits(r.starting_peak) == bits(start[3]), (r.starting_peak, start[3])
        # the peak the oracle's loop ended on: its last search, redone here
        end = self.find_peak(square=True) if n_it else start
        if end[0]:
            assert bits(r.final_peak) == bits(end[3])
        self.iteration = int(r.iteration_number)
        o = types.SimpleNamespace(iteration=self.iteration, trace=trace_o,
                                  components=[tuple(t) for t in trace_o.tolist()],
                                  diverging=int(r.is_diverging), found=int(end[0]),
                                  final_peak=np.float32(r.final_peak), start=start,
                                  residual=self.res_o, model=self.mod_o, alg=self.alg)
        if not self.device:
            return o

        rows = max(n_it, max_iterations - iteration_start, trace_cap or 0, 1)
        trace = np.full((rows, 2), FILL, np.uint32)
        cap = rows if trace_cap is None else trace_cap
        out, res, mod = self.device_run(start, iteration_start, max_iterations,
                                        None if null_trace else trace, cap)
        o.out = out
        assert int(out.iteration) == o.iteration
        assert int(out.found) == o.found
        assert int(out.diverging) == o.diverging
        n_tr = 0 if null_trace else min(n_it, cap)
        assert np.array_equal(trace[:n_tr], trace_o[:n_tr])
        assert np.all(trace[n_tr:] == FILL)  # nothing past the last component or the cap
        nan = np.isnan(self.res_o)
        assert np.array_equal(np.isnan(res), nan) and not np.isnan(mod).any()
        if self.fit is None:
            assert np.array_equal(bits(res)[~nan], bits(self.res_o)[~nan])
            assert np.array_equal(bits(mod), bits(self.mod_o))
            if o.found and compare_peak:
                assert bits(out.peak) == bits(end[3]), (out.peak, end[3])
                assert (out.x, out.y) == end[1:3]
        else:
            # test_spectral.py's bound for the log-polynomial fitter (device
            # exp vs host pow); the peak is a residual value (same bound there)
            tol = 2e-5 * self.scale
            deviation = max(float(np.abs(res - self.res_o).max()),
                            float(np.abs(mod - self.mod_o).max()),
                            abs(float(out.peak) - float(end[3])))
            print(f"{self.name}: largest deviation {deviation:.3e}, bound {tol:.3e}")
            assert deviation <= tol
            assert (out.x, out.y) == end[1:3]
            # the traces are comparable only where no decision was closer than
            # the engines may differ: asserted on the oracle's margins
            margins, values = self.alg.margins()
            assert len(margins) == n_it + 1
            assert float(np.min(margins / values)) >= 1e-4
        return o


def run_case(ctx, dirties, psfs, max_iterations, *, trace_cap=None, null_trace=False,
             compare_peak=True, **options):
    """One loop on both sides (Pair.step); returns the oracle's run."""
    pair = Pair(ctx, dirties, psfs, **options)
    try:
        return pair.step(max_iterations, trace_cap, null_trace, compare_peak)
    finally:
        pair.close()


def oracle_case(ctx, dirties, psfs, max_iterations, **options):
    """The oracle's run alone, for a case's precondition."""
    return Pair(ctx, dirties, psfs, device=False, **options).step(max_iterations)


def distinct(o):
    return len(set(o.components))


# --------------------------------------------------------------------- cases
@pytest.mark.parametrize("w,h", [(96, 80), (61, 75), (300, 70), (36, 2049)])
def test_plain_geometry(ctx, w, h):
    """Odd halves and a width that is no multiple of 4 (61 x 75), a width
    above the pass's 256-thread x stride (300), and 2049 rows:
    rows_per_block = 2 with a last block of one row."""
    o = run_case(ctx, *single(w, h), 150)
    assert o.iteration == 150 and distinct(o) >= 15
    if h == 2049:
        ys = o.trace[:, 1].astype(int)
        assert (ys % 2 == 0).any() and (ys % 2 == 1).any()
        assert ys.max() - ys.min() > h // 2


@pytest.mark.parametrize("n_img", [2, 4, 5, 16, 17, 64])
def test_image_counts(ctx, n_img):
    """Both ends of HogbomPass<4>, <16> and <64>: the select chain that picks
    image k's value out of the register array."""
    o = run_case(ctx, *mixed(64, 48, n_img), 80)
    assert o.iteration == 80 and distinct(o) >= 8


def test_two_polarizations(ctx):
    """3 channels x 2 polarizations in RDL_INTEGRATE_SQUARE."""
    planes, psfs = mixed(96, 80, 6, 2)
    o = run_case(ctx, planes, psfs, 120, n_pol=2, pol_factor=0.5)
    # the same planes as six channels: the polarizations are joined otherwise
    linear = oracle_case(ctx, planes, np.repeat(psfs, 2, axis=0), 120)
    assert distinct(o) >= 8 and o.components != linear.components


def test_squared_joins_with_weights(ctx):
    """RDL_INTEGRATE_SQUARED_JOINS, 3 weighted channels x 2 polarizations."""
    planes, psfs = mixed(96, 80, 6, 2)
    kw = dict(n_pol=2, pol_factor=0.5)
    o = run_case(ctx, planes, psfs, 120, weights=[1.0, 2.0, 0.5], squared_joins=True, **kw)
    plain = oracle_case(ctx, planes, psfs, 120, **kw)
    weighted = oracle_case(ctx, planes, psfs, 120, weights=[1.0, 2.0, 0.5], **kw)
    assert distinct(o) >= 8
    assert o.components != plain.components and o.components != weighted.components


def test_zero_weight_channel(ctx):
    planes, psfs = mixed(96, 80, 3)
    o = run_case(ctx, planes, psfs, 120, weights=[1.0, 0.0, 2.0])
    plain = oracle_case(ctx, planes, psfs, 120)
    assert distinct(o) >= 8 and o.components != plain.components
    assert o.model[1].any()  # the unweighted image still gets its components


@pytest.mark.parametrize("rms", [False, True], ids=["mask", "mask-rms"])
def test_mask_and_borders(ctx, rms):
    """The border box against the subtraction window: a row can lie in one,
    in both or in neither, and the pass skips those in neither."""
    w, h = 96, 80
    dirties, psfs = single(w, h)
    mask = mask_image(w, h)
    kw = dict(rms=rms_image(w, h)) if rms else {}
    o = run_case(ctx, dirties, psfs, 120, mask=mask, border_ratio=0.1, **kw)
    plain = oracle_case(ctx, dirties, psfs, 120, **kw)
    assert distinct(o) >= 8 and o.components != plain.components
    hb, vb = border(w, 0.1), border(h, 0.1)
    assert (hb, vb) == (10, 8)
    for x, y in o.components:
        assert mask[y, x] and hb <= x < w - hb and vb <= y < h - vb
    # some component's window leaves rows above or below both it and the box
    assert any(y - h // 2 > vb or y + h // 2 < h - vb for _, y in o.components)


def test_rms_factor(ctx):
    dirties, psfs = single(96, 80)
    o = run_case(ctx, dirties, psfs, 120, rms=rms_image(96, 80))
    plain = oracle_case(ctx, dirties, psfs, 120)
    assert distinct(o) >= 8 and o.components[0] != plain.components[0]


def test_rms_factor_negative_peak(ctx):
    """A weighted negative peak is taken as a component."""
    o = run_case(ctx, *single(96, 80, "neg"), 120, rms=rms_image(96, 80))
    assert distinct(o) >= 8 and o.model.min() < 0 < o.model.max()


def test_positive_components_only(ctx):
    dirties, psfs = single(96, 80, "neg")
    o = run_case(ctx, dirties, psfs, 120, allow_negative=0)
    both = oracle_case(ctx, dirties, psfs, 120)
    assert distinct(o) >= 8 and o.model.min() >= 0
    assert o.components != both.components


def test_stop_on_negative(ctx):
    o = run_case(ctx, *single(96, 80, "neg"), 120, stop_on_negative=1)
    assert 0 < o.iteration < 120 and o.final_peak < 0 and not o.diverging


def test_divergence(ctx):
    """PSFs times -0.5: every component grows its pixel by 5 %, so the peak
    passes 4 x the first after 29 components."""
    o = run_case(ctx, *single(96, 80, "div"), 120)
    assert o.diverging and 3 < o.iteration < 120


def test_divergence_limit_zero(ctx):
    o = run_case(ctx, *single(96, 80, "div"), 40, divergence_limit=0.0)
    assert o.iteration == 40 and not o.diverging
    assert abs(o.final_peak) > 4.0 * abs(o.start[3])  # past the default limit


def test_threshold_stop(ctx):
    dirties, psfs = single(96, 80)
    thr = 0.3 * float(np.abs(dirties).max())
    o = run_case(ctx, dirties, psfs, 400, threshold=thr)
    assert 10 < o.iteration < 400 and abs(o.final_peak) <= np.float32(thr)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_batch_boundary(ctx, n):
    """The host queues 32 pass + step pairs and then reads the state: runs
    that end inside the first batch, on its last pair, and one pair later."""
    o = run_case(ctx, *single(96, 80), n)
    assert o.iteration == n and len(o.trace) == n


def test_iteration_window(ctx):
    """A second call on the same buffers continues at iteration 40; its trace
    starts at index 0 again."""
    pair = Pair(ctx, *single(96, 80))
    try:
        first = pair.step(40)
        assert first.iteration == 40
        model_after_first = first.model.copy()
        second = pair.step(100)
        assert second.iteration == 100 and len(second.trace) == 60
        assert distinct(second) >= 8
        assert not np.array_equal(second.model, model_after_first)
    finally:
        pair.close()


@pytest.mark.parametrize("max_iterations", [40, 30], ids=["equal", "past"])
def test_empty_iteration_window(ctx, max_iterations):
    """iteration_start >= max_iterations: nothing changes."""
    pair = Pair(ctx, *single(96, 80))
    try:
        pair.step(40)
        residual, model = pair.res_o.copy(), pair.mod_o.copy()
        o = pair.step(max_iterations)
        assert o.iteration == 40 and len(o.trace) == 0 and o.found == 1
        assert np.array_equal(bits(pair.res_o), bits(residual))
        assert np.array_equal(bits(pair.mod_o), bits(model))
    finally:
        pair.close()


def test_no_starting_peak(ctx):
    """start_found = 0 (an empty mask): nothing changes."""
    dirties, psfs = single(96, 80)
    o = run_case(ctx, dirties, psfs, 50, mask=np.zeros((80, 96), np.uint8))
    assert not o.start[0] and o.found == 0 and o.iteration == 0
    assert np.array_equal(bits(o.residual), bits(dirties)) and not o.model.any()


@pytest.mark.parametrize("variant", ["cap", "null", "cap0"])
def test_trace_variants(ctx, variant):
    """A cap below the number of components, a NULL trace with a cap, and a
    trace with cap 0: the planes are those of the full-trace run."""
    dirties, psfs = single(96, 80)
    kw = dict(cap=dict(trace_cap=10), null=dict(null_trace=True), cap0=dict(trace_cap=0))
    o = run_case(ctx, dirties, psfs, 50, **kw[variant])
    full = oracle_case(ctx, dirties, psfs, 50)
    assert o.iteration == 50 and distinct(o) >= 8
    assert np.array_equal(bits(o.residual), bits(full.residual))
    assert np.array_equal(bits(o.model), bits(full.model))


def test_no_qualifying_pixel_without_mask(ctx):
    """Every pixel negative and allow_negative = 0: the peak finder falls
    back to pixel 0, which stays a found peak."""
    dirties, psfs = single(96, 80)
    negative = -(np.abs(dirties) + np.float32(0.01))
    o = run_case(ctx, negative, psfs, 10, allow_negative=0)
    assert o.iteration == 10 and o.found == 1
    assert o.components == [(0, 0)] * 10 and o.final_peak < 0


def test_no_qualifying_pixel_with_mask(ctx):
    """A mask of one pixel and a gain of 1: the first component zeroes the
    only allowed pixel, and the next search finds nothing."""
    dirties, psfs = single(96, 80)
    y, x = np.unravel_index(np.argmax(dirties[0]), dirties[0].shape)
    mask = np.zeros((80, 96), np.uint8)
    mask[y, x] = 1
    o = run_case(ctx, dirties, psfs, 10, mask=mask, allow_negative=0, gain=1.0,
                 compare_peak=False)
    assert o.iteration == 1 and o.components == [(x, y)] and o.found == 0
    assert bits(o.residual[0, y, x]) == 0


def test_nan_pixel(ctx):
    dirties, psfs = single(96, 80)
    dirties = dirties.copy()
    dirties[0, 40, 48] = np.nan
    o = run_case(ctx, dirties, psfs, 120)
    assert distinct(o) >= 8 and (48, 40) not in o.components
    assert np.isnan(o.residual).sum() == 1 and np.isnan(o.residual[0, 40, 48])
    # some component's window covered the pixel
    assert any(abs(x - 48) < 48 and abs(y - 40) < 40 for x, y in o.components)


@pytest.mark.parametrize("n_ch,n_pol", [(4, 1), (3, 2)])
def test_spectral_map(ctx, n_ch, n_pol):
    """d_spectral's own arithmetic (fmaf over q ascending, then the gain)
    against the oracle's map form, bit for bit. The join's weights are not
    the fit's: a weighted fit keeps the sum under its own weights, so with
    n_pol = 1 the integrated peak would move as it does without the map."""
    wts = [1.0, 0.5, 2.0, 1.0][:n_ch]
    planes, psfs = mixed(96, 80, n_ch * n_pol, n_pol)
    kw = dict(n_pol=n_pol, weights=[2.0, 1.0, 1.0, 0.5][:n_ch], pol_factor=1.0 / n_pol)
    o = run_case(ctx, planes, psfs, 120, smap=projector(n_ch, 2, wts, n_pol), **kw)
    plain = oracle_case(ctx, planes, psfs, 120, **kw)
    assert distinct(o) >= 8 and o.components != plain.components


@pytest.mark.parametrize("planes", ["positive", "signed"])
def test_log_polynomial_fit(ctx, planes):
    """4 channels, 2 terms, against the oracle's own log-polynomial fitter."""
    dirties, psfs = mixed(96, 80, 4)
    if planes == "positive":
        dirties = np.abs(dirties) + np.float32(0.5)
    # as far as every decision of the oracle's run keeps a relative margin
    # of 1e-4 (asserted in Pair.step)
    n_it = 40 if planes == "positive" else 60
    o = run_case(ctx, dirties, psfs, n_it, fit=("logpoly", 2), name=f"logpoly-{planes}")
    plain = oracle_case(ctx, dirties, psfs, n_it)
    assert o.iteration == n_it and not np.array_equal(plain.model, o.model)


def test_forced_terms(ctx):
    """4 weighted channels, 2 terms, the second term 0.7 at every pixel of a
    plane stored with a pitch, an origin and poisoned padding."""
    dirties, psfs = mixed(96, 80, 4)
    wts = [1.0, 2.0, 0.5, 1.0]
    n_it = 60
    o = run_case(ctx, dirties, psfs, n_it, weights=wts, fit=("forced", 0.7), name="forced")
    plain = oracle_case(ctx, dirties, psfs, n_it, weights=wts)
    assert o.iteration == n_it and not np.array_equal(plain.model, o.model)


def test_everything_at_once(ctx):
    """3 channels x 2 polarizations, weights, mask, borders, RMS factors and
    the spectral map on 61 x 75."""
    w, h = 61, 75
    wts = [1.0, 0.5, 2.0]
    planes, psfs = mixed(w, h, 6, 2)
    o = run_case(ctx, planes, psfs, 120, n_pol=2, weights=wts, pol_factor=0.5,
                 mask=mask_image(w, h), border_ratio=0.1, rms=rms_image(w, h),
                 smap=projector(3, 2, wts, 2))
    assert o.iteration == 120 and distinct(o) >= 8
