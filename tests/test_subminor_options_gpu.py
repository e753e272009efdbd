"""Every sub-minor loop kernel under every option of rdl_subminor_run.

rdl_subminor_run against the oracle's SubMinorLoop::Run (Oracle.subminor_run)
for each loop kernel PlanSubminorLoop can choose (Lds, Reg, Wave, Big, Tab,
TabN; one workgroup and grid; Reg / Wave / Big also reading the pairwise PSF
table, which is what mode 0 runs when an RMS image, a spectral map or
n_pol > 1 rules the table kernels out) and for each option the kernels
handle in their own copy of the code: RMS-factor weighting, mask and borders
(every selection mode), allow_negative = 0, stop_on_negative, divergence, the
iteration window, image sizes with an odd half and a width that is no
multiple of 4, polarizations and channel weights, the spectral map, and the
log-polynomial and forced-term fits (Lds only); and for the paths two
per-run environment switches choose (one-workgroup Tab through the wave slots,
TabN's grid exchange through agent-scope stores) and exact |value| ties.

One helper (run_case) runs a case on both sides and asserts n_selected, the
positions, the iteration count, the trace, every image's model values, peak,
diverging, flux_cleaned and iteration, bit for bit (the log-polynomial fits:
identical trace, model within 2e-5 x max|dirties|, test_spectral.py's bound).
It also asks PlanSubminorLoop itself (tests/subminor_plan_query.cc, compiled
here) which kernel the run's selection, flags and CU count lead to, and
asserts the kind, the grid form and build_table the case is meant for. Each
option's precondition is asserted on the oracle's result alone.

Not tested: the Lds kernel's global-scratch form (use_lds = 0). It needs
more than 150 KiB per workgroup after the selection has spread over every
CU, far more pixels than a seconds-long test selects.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle_lib import get_oracle
from rdl_lib import (ForcedLogPoly, Session, SubminorParams, SubminorResult, integration,
                     logpoly)
from subminor_cases import joined, synthetic
from test_subminor_plan import _host_build

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KIND_NAMES = ["Lds", "Reg", "Wave", "Big", "Tab", "TabN"]  # rdl::LoopKind
LOGPOLY = 2  # oracle/spectral.h SpectralFit::mode
# the grid of images(..., "ties"): the finest power of two at which the
# oracle's runs of the 256 x 256 images choose a component on an exact tie
# (2^-12 ... 2^-8 show none: after the first component every pixel the PSF
# reaches is off the grid)
TIE_QUANTUM = 2.0 ** -7


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def sess():
    s = Session(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def orc():
    return get_oracle()


@pytest.fixture(scope="module")
def n_cus(sess):
    """hipDeviceProp_t::multiProcessorCount of device 0, which the session
    hands the plan as SubminorShape::n_cus."""
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    n = C.c_int(0)
    attribute = 63  # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)
    assert hip.hipDeviceGetAttribute(C.byref(n), attribute, 0) == 0
    assert 8 <= n.value <= 1024, n.value
    return n.value


@pytest.fixture(scope="module")
def plan_query(tmp_path_factory):
    """PlanSubminorLoop's own answer: tests/subminor_plan_query.cc compiled
    the way test_subminor_plan.py compiles its dump."""
    b = _host_build()
    exe = str(tmp_path_factory.mktemp("plan") / "subminor_plan_query")
    subprocess.run([b.CXX, *b.CXX_FLAGS, os.path.join(HERE, "subminor_plan_query.cc"), "-o", exe],
                   check=True)

    @functools.lru_cache(maxsize=None)
    def query(*args):
        out = subprocess.run([exe, *map(str, args)], check=True, capture_output=True, text=True)
        error, kind, n_blocks, build_table, use_lds, threads, items = map(int, out.stdout.split())
        return dict(error=error, kind=KIND_NAMES[kind], n_blocks=n_blocks,
                    build_table=bool(build_table), use_lds=bool(use_lds))
    return query


@pytest.fixture
def ctx(sess, orc, n_cus, plan_query):
    return dict(sess=sess, orc=orc, n_cus=n_cus, plan=plan_query)


# -------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def images(w, h, n_img, n_pol, variant):
    """Residual planes [n_img, h, w] (channel-major) and PSFs
    [n_img // n_pol, h, w]. variant "neg": a negative copy of every source at
    0.6 of its flux, so the largest |value| turns negative after a few
    components; "div": PSFs times -0.5, so subtracting a component grows it;
    "edge": two more sources, 2 pixels from the left edge and 5 from the top
    (synthetic() keeps its own 8 pixels from every edge); "ties": every value
    rounded to a multiple of TIE_QUANTUM, both signs, so exact |value| ties
    occur among the integrated values."""
    psf, dirty = synthetic(w, h, 60, 7)
    if variant == "edge":
        for x, y, flux in ((2, h // 3, 0.8), (w // 3, 5, 0.7)):
            dirty = dirty + np.float32(flux) * np.roll(psf, (y - h // 2, x - w // 2), axis=(0, 1))
    if variant == "neg":
        dirty = (dirty - np.float32(0.6) * np.roll(dirty, (37, 53), axis=(0, 1))).astype(np.float32)
    if n_img == 1:
        dirties, psfs = dirty[None].copy(), psf[None].copy()
    else:
        dirties, psfs = joined(dirty, psf, n_img, n_pol)
    if variant == "div":
        psfs = (psfs * np.float32(-0.5)).astype(np.float32)
    if variant == "ties":
        dirties = (np.round(dirties / TIE_QUANTUM) * TIE_QUANTUM).astype(np.float32)
        psfs = (np.round(psfs / TIE_QUANTUM) * TIE_QUANTUM).astype(np.float32)
    dirties.setflags(write=False)
    psfs.setflags(write=False)
    return dirties, psfs


@functools.lru_cache(maxsize=None)
def rms_image(w, h):
    """Smooth, positive, spanning [0.25, 4]."""
    yy, xx = np.mgrid[0:h, 0:w]
    e = 2.0 * np.sin(2 * np.pi * xx / w * 1.5 + 0.3) * np.cos(2 * np.pi * yy / h + 0.2)
    img = (2.0 ** e).astype(np.float32)
    assert img.min() < 0.3 and img.max() > 3.5 and img.min() > 0.2
    return img


@functools.lru_cache(maxsize=None)
def mask_image(w, h):
    return (np.random.default_rng(w * 3 + h).random((h, w)) < 0.7).astype(np.uint8)


def FREQS(n):
    return 1.0e8 + 1.0e7 * np.arange(n)


def projector(n_ch, terms, weights=None, n_pol=1):
    """The weighted polynomial fit-and-evaluate over n_ch channels as a
    matrix (float64 numpy, rounded to float32 once); n_pol > 1: its Kronecker
    product with the identity, images ordered channel-major."""
    wts = np.ones(n_ch) if weights is None else np.asarray(weights, np.float64)
    f = FREQS(n_ch)
    x = f / (np.sum(f * wts) / np.sum(wts)) - 1.0
    v = np.vander(x, terms, increasing=True)
    p = v @ np.linalg.inv(v.T @ (wts[:, None] * v)) @ (v.T * wts)
    if n_pol > 1:
        p = np.kron(p, np.eye(n_pol))
    return np.ascontiguousarray(p, np.float32)


# ------------------------------------------------------------------- kernels
# name -> (set_tuning mode, target, selection for n_img images, kind, grid)
KERNELS = {
    "lds1": (1, 0, lambda ni: 600, "Lds", False),
    "ldsG": (1, 0, lambda ni: 9000, "Lds", True),          # >= 3 workgroups
    "wave": (3, 0, lambda ni: 100, "Wave", False),
    "reg1": (2, 0, lambda ni: min(600, 2000 // ni), "Reg", False),  # n_sel x n_img <= 2048
    "regG": (2, 512, lambda ni: 3000, "Reg", True),
    "big1": (4, 0, lambda ni: 1500, "Big", False),
    "bigG": (5, 1024, lambda ni: 3000, "Big", True),
    "tab1": (6, 1 << 20, lambda ni: 1500, "Tab", False),
    "tabG": (6, 512, lambda ni: 3000, "Tab", True),
    "tabn1": (0, 0, lambda ni: 600, "TabN", False),
    "tabnG": (0, 0, lambda ni: 3000, "TabN", True),
}
GENERAL = ["lds1", "ldsG", "wave", "reg1", "regG", "big1", "bigG"]
TAB = ["tab1", "tabG"]
TABN = [(k, ni) for ni in (2, 4, 8) for k in ("tabn1", "tabnG")]
# every form with the image count it runs by default
ALL_FORMS = [(k, 1) for k in GENERAL + TAB] + TABN
FORM_IDS = [f"{k}-{ni}img" for k, ni in ALL_FORMS]


def device_run(sess, spec):
    """rdl_subminor_run of one case: (n_selected, positions, model values
    [n_img, n_selected], the result struct, the trace buffer)."""
    w, h, n_ch, n_pol, wts = (spec[k] for k in ("w", "h", "n_ch", "n_pol", "wts"))
    n_img = n_ch * n_pol
    fit, smap, mask_img, rms_img = (spec[k] for k in ("fit", "smap", "mask_img", "rms_img"))
    iteration_start, max_iterations = spec["iteration_start"], spec["max_iterations"]
    uniform = np.ones(n_ch, np.float32)
    keep = []

    def dev(a, dtype=np.float32):
        keep.append(sess.array(np.ascontiguousarray(a, dtype), dtype=dtype))
        return keep[-1]

    env = {}
    if spec["table_max"] is not None:
        env["RDL_SUBMINOR_TABLE_MAX"] = str(spec["table_max"])
    if spec["select"] is not None:
        env["RDL_SUBMINOR_SELECT"] = str(spec["select"])
    sm = C.c_void_p()
    os.environ.update(env)
    try:
        sess.rdl.rdl_subminor_create(sess.h, C.byref(sm))
    finally:
        for k in env:
            del os.environ[k]
    try:
        sess.rdl.rdl_subminor_set_tuning(sm, spec["mode"], spec["target"])
        p = SubminorParams()
        p.width, p.height, p.n_images, p.n_pol = w, h, n_img, n_pol
        p.integ = integration(n_ch, n_pol, wts, spec["pol_factor"], mode=0)
        p.h_border, p.v_border = spec["h_border"], spec["v_border"]
        p.allow_negative, p.stop_on_negative = spec["allow_negative"], spec["stop_on_negative"]
        p.threshold, p.gain = spec["thr"], spec["gain"]
        p.divergence_limit = spec["divergence_limit"]
        p.iteration_start, p.max_iterations = iteration_start, max_iterations
        if mask_img is not None:
            p.d_mask = dev(mask_img, np.uint8).ptr
        if rms_img is not None:
            p.d_rms = dev(rms_img).ptr
        if smap is not None:
            p.d_spectral = dev(smap).ptr
        if fit is not None and fit[0] == "logpoly":
            lp = logpoly(FREQS(n_ch), uniform, fit[1])
            p.logpoly = C.addressof(lp)
        elif fit is not None:
            lp = ForcedLogPoly()
            lp.fit = logpoly(FREQS(n_ch), uniform, 2)
            lp.fit.reserved = 1  # RDL_LOGPOLY_FORCED
            t = lp.terms
            t.d_planes, t.plane_stride = dev(np.zeros((h, w), np.float32)).ptr, w * h
            t.pitch, t.rows, t.x0, t.y0 = w, h, 0, 0
            for c in range(n_ch):
                t.weights[c] = 1.0
            p.logpoly = C.addressof(lp)
        out = SubminorResult()
        cap = max(max_iterations - iteration_start, 1)
        trace = np.full((cap, 2), 0xffffffff, np.uint32)
        dres, dpsf = dev(spec["dirties"]), dev(spec["psfs"])
        before = {k: os.environ.get(k) for k in spec["env"]}
        os.environ.update(spec["env"])  # switches rdl_subminor_run reads per run
        try:
            sess.rdl.rdl_subminor_run(sm, dres.vp, dpsf.vp, C.byref(p), C.byref(out),
                                      trace.ctypes.data_as(C.c_void_p), C.c_uint64(cap))
        finally:
            for k, v in before.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        n = int(out.n_selected)
        pos = np.zeros(max(n, 1), np.uint32)
        mod = np.zeros((n_img, max(n, 1)), np.float32)
        sess.rdl.rdl_subminor_get(sm, pos.ctypes.data_as(C.c_void_p),
                                  mod.ctypes.data_as(C.c_void_p), C.c_uint64(n))
    finally:
        sess.rdl.rdl_subminor_destroy(sm)
        for a in keep:
            a.free()
    return n, pos, mod, out, trace


def run_case(ctx, kernel, *, w=256, h=256, n_ch=1, n_pol=1, weights=None, pol_factor=1.0,
             variant="plain", n_sel=None, rms=False, mask=False, h_border=0, v_border=0,
             allow_negative=1, stop_on_negative=0, divergence_limit=4.0, gain=0.1,
             iteration_start=0, max_iterations=300, smap=None, fit=None, table_max=None,
             select=None, expect=None, custom=None, env=None):
    """Runs one case on the device and in the oracle, asserts that they agree
    and that PlanSubminorLoop sends the run to the kernel the case is for.
    kernel: a KERNELS name, or "auto" (mode 0) with expect = (kind, grid,
    build_table). fit: None, ("logpoly", terms) or ("forced",). custom:
    (dirties, psfs, mask, threshold) in place of the generated images and of
    the threshold that selects about n_sel pixels. env: environment switches
    set around rdl_subminor_run alone. Returns the oracle's run
    with .inputs (dirties, psfs, threshold, oracle kwargs) and .plan for the
    caller's preconditions."""
    sess, orc = ctx["sess"], ctx["orc"]
    n_img = n_ch * n_pol
    if kernel == "auto":
        mode, target = 0, 0
        kind, grid, build_table = expect
    else:
        mode, target, sel_of, kind, grid = KERNELS[kernel]
        n_sel = sel_of(n_img) if n_sel is None else n_sel
        build_table = kind in ("Tab", "TabN")  # forced modes 1-5 never build it
    wts = None if weights is None else np.asarray(weights, np.float32)
    rms_img = rms_image(w, h) if rms else None
    if custom is not None:
        dirties, psfs, mask_img, thr = custom
        assert dirties.shape == (n_img, h, w)
    else:
        dirties, psfs = images(w, h, n_img, n_pol, variant)
        mask_img = mask_image(w, h) if mask else None
        # the threshold: the n_sel-th largest eligible value of the integrated image
        integ = orc.integrate(dirties, wts, n_pol, pol_factor) if n_img > 1 else dirties[0].copy()
        if rms:
            integ = integ * rms_img
        value = np.abs(integ) if allow_negative else integ
        eligible = np.ones((h, w), bool) if mask_img is None else mask_img != 0
        if h_border or v_border:
            box = np.zeros((h, w), bool)
            box[v_border:h - v_border, h_border:w - h_border] = True
            eligible &= box
        thr = np.float32(np.sort(value[eligible])[-n_sel])
        assert thr > 0

    okw = dict(gain=gain, divergence_limit=divergence_limit, h_border=h_border,
               v_border=v_border, iteration_start=iteration_start,
               max_iterations=max_iterations, allow_negative=bool(allow_negative),
               stop_on_negative=bool(stop_on_negative), mask=mask_img, rms_factor=rms_img,
               spectral_map=smap, n_pol=n_pol, weights=wts, pol_factor=pol_factor)
    uniform = np.ones(n_ch, np.float32)
    if fit is not None:
        # the forced fit with zero term planes is the weighted mean; the
        # oracle's one-term log-polynomial fit is the plain mean: equal for
        # the uniform weights these cases use
        assert wts is None
        okw["spectral"] = (LOGPOLY, fit[1] if fit[0] == "logpoly" else 1, FREQS(n_ch), uniform)
    o = orc.subminor_run(dirties, psfs, thr, **okw)
    o.inputs = (dirties, psfs, thr, okw)
    assert abs(o.n_selected - n_sel) <= n_sel // 10 + 2  # exact ties only
    empty = o.n_selected == 0  # no loop runs: nothing to plan

    spec = dict(w=w, h=h, n_ch=n_ch, n_pol=n_pol, wts=wts, pol_factor=pol_factor, mode=mode,
                target=target, dirties=dirties, psfs=psfs, thr=thr, gain=gain,
                divergence_limit=divergence_limit, h_border=h_border, v_border=v_border,
                allow_negative=allow_negative, stop_on_negative=stop_on_negative,
                iteration_start=iteration_start, max_iterations=max_iterations,
                mask_img=mask_img, rms_img=rms_img, smap=smap, fit=fit, table_max=table_max,
                select=select, env=env or {})
    n, pos, mod, out, trace = device_run(sess, spec)

    # ---- which kernel ran: PlanSubminorLoop's answer for this launch (an
    # empty selection launches no loop)
    if not empty:
        plan = ctx["plan"](mode, target, n, n_img, n_pol, 0, int(n_img == 1), int(rms),
                           int(smap is not None), int(fit is not None), ctx["n_cus"], 0,
                           -1 if table_max is None else table_max)
        o.plan = plan
        assert plan["error"] == 0
        assert plan["kind"] == kind, plan
        assert (plan["n_blocks"] > 1) == grid, plan
        if kernel == "ldsG":
            assert plan["n_blocks"] >= 3, plan
        if kind == "Lds":
            assert plan["use_lds"], plan  # the global-scratch form is out of reach (docstring)
        assert plan["build_table"] == build_table, plan

    # ---- the comparison
    n_it = o.iteration - iteration_start
    assert n == o.n_selected
    assert np.array_equal(pos[:n], o.positions)
    assert int(out.iteration) == o.iteration
    assert np.array_equal(trace[:n_it], o.trace)
    assert np.all(trace[n_it:] == 0xffffffff)  # nothing past the last component
    assert int(out.has_peak) == o.has_peak and int(out.diverging) == o.diverging
    if fit is None:
        assert np.array_equal(bits(mod[:, :n]), bits(o.model))
        assert bits(out.peak) == bits(o.peak), (out.peak, o.peak)
        assert bits(out.flux_cleaned) == bits(o.flux_cleaned), (out.flux_cleaned, o.flux_cleaned)
    else:
        # test_spectral.py's bound for the log-polynomial fitter (device exp
        # vs host pow): model within 2e-5 x max|dirties|; the peak is a
        # residual value (same bound there), the flux a sum of n_it peaks x gain
        tol = 2e-5 * float(np.abs(dirties).max())
        assert np.abs(mod[:, :n] - o.model).max() <= tol
        assert abs(float(out.peak) - float(o.peak)) <= tol
        assert abs(float(out.flux_cleaned) - float(o.flux_cleaned)) <= \
            n_it * gain * tol + n_it * 1.2e-7 * abs(float(o.flux_cleaned))
        # the trace is only comparable where no decision was closer than the
        # engines may differ: asserted on the oracle's margins
        assert float(np.min(o.margins / o.values)) >= 1e-4
    return o


def components(o):
    return [tuple(t) for t in o.trace]


# --------------------------------------------------------------------- cases
@pytest.mark.parametrize("kernel,n_img", ALL_FORMS, ids=FORM_IDS)
def test_plain(ctx, kernel, n_img):
    """No option: what the existing kernel tests run, with the outputs they
    do not compare (positions, peak, diverging, flux_cleaned)."""
    o = run_case(ctx, kernel, n_ch=n_img)
    assert len(o.trace) >= 20 and not o.diverging


@pytest.mark.parametrize("kernel", GENERAL)
def test_rms_factor(ctx, kernel):
    o = run_case(ctx, kernel, rms=True)
    dirties, psfs, thr, okw = o.inputs
    plain = ctx["orc"].subminor_run(dirties, psfs, thr, **dict(okw, rms_factor=None))
    assert len(o.trace) >= 20 and components(o)[:20] != components(plain)[:20]


@pytest.mark.parametrize("kernel", GENERAL)
def test_rms_factor_negative_peak(ctx, kernel):
    """The run ends on a negative peak, so the loop's last RMS-weighted value
    (rebuilt from the argmax key in the register kernels) carries a sign."""
    o = run_case(ctx, kernel, rms=True, variant="neg", stop_on_negative=1)
    assert 0 < len(o.trace) < 300 and o.peak < 0


@pytest.mark.parametrize("kernel,n_img", ALL_FORMS, ids=FORM_IDS)
def test_negative_zero_peak_does_not_stop(ctx, kernel, n_img):
    """stop_on_negative tests `peak >= 0`, which -0.0 passes. Every pixel is
    -0.0 and the threshold is negative, so the first peak is -0.0 (selection
    index 0 wins the tie) and the loop must go on to max_iterations; a mask of
    the first n_sel pixels sets the selection's size."""
    w = h = 128
    n_sel = KERNELS[kernel][2](n_img)
    dirties = np.full((n_img, h, w), -0.0, np.float32)
    psfs = images(w, h, n_img, 1, "plain")[1]
    mask = (np.arange(w * h) < n_sel).reshape(h, w).astype(np.uint8)
    o = run_case(ctx, kernel, w=w, h=h, n_ch=n_img, stop_on_negative=1, max_iterations=5,
                 custom=(dirties, psfs, mask, np.float32(-1.0)))
    dirties, psfs, thr, okw = o.inputs
    first = ctx["orc"].subminor_run(dirties, psfs, thr, **dict(okw, max_iterations=0))
    assert bits(first.peak) == 0x80000000 and o.n_selected == n_sel
    assert len(o.trace) == 5 and components(o)[0] == (0, 0)


@pytest.mark.parametrize("kernel", ["lds1", "reg1", "tab1"])
def test_empty_selection(ctx, kernel):
    """A threshold above every pixel: no selection, no peak, and the
    iteration stays at iteration_start."""
    dirties, psfs = images(256, 256, 1, 1, "plain")
    o = run_case(ctx, kernel, n_sel=0, iteration_start=17, max_iterations=40,
                 custom=(dirties, psfs, None, np.float32(1e9)))
    assert (o.n_selected, o.has_peak, o.iteration, o.diverging) == (0, 0, 17, 0)


def _mask_preconditions(orc, o):
    """The mask, the left / right border and the top / bottom border each
    keep pixels out that the threshold alone would select."""
    dirties, psfs, thr, okw = o.inputs
    for off in (dict(mask=None), dict(h_border=0), dict(v_border=0)):
        more = orc.subminor_run(dirties, psfs, thr, **dict(okw, max_iterations=0, **off))
        assert more.n_selected > o.n_selected, off
    assert len(o.trace) >= 20


@pytest.mark.parametrize("kernel,n_img", ALL_FORMS, ids=FORM_IDS)
def test_mask_and_borders(ctx, kernel, n_img):
    o = run_case(ctx, kernel, n_ch=n_img, mask=True, h_border=5, v_border=11, variant="edge")
    _mask_preconditions(ctx["orc"], o)


@pytest.mark.parametrize("select", [None, 4, 1, 3])
@pytest.mark.parametrize("joined3,rms", [(False, False), (True, False), (False, True),
                                         (True, True)])
def test_mask_and_borders_selection_modes(ctx, select, joined3, rms):
    """The sparse selection (16-byte and scalar loads), the single pass and
    count + scan + scatter, with IntegratePixel over 3 weighted images and
    with the RMS factor in the selection."""
    kw = dict(n_ch=3, weights=[1.0, 0.5, 2.0]) if joined3 else {}
    o = run_case(ctx, "big1", mask=True, h_border=5, v_border=11, rms=rms, select=select,
                 n_sel=1000 if joined3 else None, variant="edge", **kw)
    _mask_preconditions(ctx["orc"], o)


@pytest.mark.parametrize("kernel", GENERAL + TAB)
def test_positive_components_only(ctx, kernel):
    o = run_case(ctx, kernel, allow_negative=0, variant="neg")
    dirties, psfs, thr, okw = o.inputs
    both = ctx["orc"].subminor_run(dirties, psfs, thr, **dict(okw, allow_negative=True))
    assert both.n_selected > o.n_selected  # negative pixels above the threshold exist


@pytest.mark.parametrize("kernel,n_img", ALL_FORMS, ids=FORM_IDS)
def test_stop_on_negative(ctx, kernel, n_img):
    o = run_case(ctx, kernel, n_ch=n_img, stop_on_negative=1, variant="neg")
    _, _, thr, _ = o.inputs
    assert 0 < len(o.trace) and o.iteration < 300
    assert o.peak < 0 and abs(o.peak) > thr and not o.diverging


@pytest.mark.parametrize("kernel,n_img", ALL_FORMS, ids=FORM_IDS)
def test_divergence(ctx, kernel, n_img):
    """PSFs times -0.5: every component grows its pixel by 5 %, so the peak
    passes 1.5 x the first after nine components."""
    o = run_case(ctx, kernel, n_ch=n_img, variant="div", divergence_limit=1.5)
    assert o.diverging and 3 < len(o.trace) < 300


@pytest.mark.parametrize("kernel,n_img", ALL_FORMS, ids=FORM_IDS)
def test_iteration_window(ctx, kernel, n_img):
    """A gain of 0.02 keeps even the 100-pixel selection above its threshold
    for 137 components."""
    o = run_case(ctx, kernel, n_ch=n_img, gain=0.02, iteration_start=1000, max_iterations=1137)
    assert len(o.trace) == 137 and o.iteration == 1137


@pytest.mark.parametrize("kernel,n_img", ALL_FORMS, ids=FORM_IDS)
def test_empty_iteration_window(ctx, kernel, n_img):
    o = run_case(ctx, kernel, n_ch=n_img, iteration_start=300, max_iterations=300)
    dirties, psfs, thr, okw = o.inputs
    first = ctx["orc"].subminor_run(dirties, psfs, thr,
                                    **dict(okw, iteration_start=0, max_iterations=1))
    assert len(o.trace) == 0 and o.has_peak == 1 and o.iteration == 300
    assert not o.model.any() and o.flux_cleaned == 0
    assert bits(o.peak) == bits(first.values[0] * np.sign(o.peak)) and abs(o.peak) > thr


@pytest.mark.parametrize("w,h", [(201, 150), (150, 201)])
@pytest.mark.parametrize("kernel,n_img", ALL_FORMS, ids=FORM_IDS)
def test_odd_geometry(ctx, kernel, n_img, w, h):
    """Odd W/2 or H/2, and a width that is no multiple of 4 (the selection's
    scalar loads). Some component and selected pixel are further apart than
    the PSF plane reaches: the offset test of the gathers, kOutsideBits in the
    pairwise table."""
    o = run_case(ctx, kernel, n_ch=n_img, w=w, h=h)
    xs, ys = (o.positions & 0xffff).astype(int), (o.positions >> 16).astype(int)
    outside = False
    for cx, cy in components(o):
        dx, dy = xs - int(cx) + w // 2, ys - int(cy) + h // 2
        outside = outside or bool(np.any((dx < 0) | (dx >= w) | (dy < 0) | (dy >= h)))
    assert outside


@pytest.mark.parametrize("kernel", GENERAL)
def test_two_polarizations(ctx, kernel):
    run_case(ctx, kernel, n_ch=2, n_pol=2, weights=[1.0, 0.5], pol_factor=0.5)


@pytest.mark.parametrize("kernel", GENERAL)
def test_zero_weight_channel(ctx, kernel):
    o = run_case(ctx, kernel, n_ch=3, weights=[1.0, 0.0, 2.0])
    assert o.model[1].any()  # the unweighted image still gets its components


@pytest.mark.parametrize("n_img", [3, 5, 7])
@pytest.mark.parametrize("kernel", GENERAL + ["tabn1", "tabnG"])
def test_image_counts_between_templates(ctx, kernel, n_img):
    """The kernels are instantiated for 1, 2, 4 and 8 images; 3, 5 and 7 run
    in the next larger one with the spare images switched off."""
    run_case(ctx, kernel, n_ch=n_img, weights=list(1.0 + 0.5 * np.arange(n_img)))


@pytest.mark.parametrize("n_img", [12, 20])
@pytest.mark.parametrize("kernel", ["lds1", "ldsG"])
def test_more_than_eight_images(ctx, kernel, n_img):
    """Only the Lds kernel takes more than 8 images (its 16- and 64-image
    instantiations)."""
    o = run_case(ctx, kernel, n_ch=n_img // 2, n_pol=2, pol_factor=0.5,
                 weights=list(1.0 + 0.25 * np.arange(n_img // 2)))
    assert len(o.trace) >= 20


@pytest.mark.parametrize("kernel,n_img", TABN, ids=[f"{k}-{ni}img" for k, ni in TABN])
def test_joined_table_weights(ctx, kernel, n_img):
    weights = {2: [1.0, 0.5], 4: [1.0, 0.0, 2.0, 0.5],
               8: [1.0, 0.5, 2.0, 0.0, 1.0, 1.5, 0.25, 1.0]}[n_img]
    run_case(ctx, kernel, n_ch=n_img, weights=weights)


@pytest.mark.parametrize("n_pol", [1, 2])
@pytest.mark.parametrize("kernel", GENERAL)
def test_spectral_map(ctx, kernel, n_pol):
    """The polynomial projector of 4 channels and 2 terms as d_spectral."""
    wts = [1.0, 0.5, 2.0, 1.0]
    smap = projector(4, 2, wts, n_pol)
    o = run_case(ctx, kernel, n_ch=4, n_pol=n_pol, weights=wts, smap=smap)
    dirties, psfs, thr, okw = o.inputs
    plain = ctx["orc"].subminor_run(dirties, psfs, thr, **dict(okw, spectral_map=None))
    assert not np.array_equal(plain.model, o.model)


@pytest.mark.parametrize("kernel", ["lds1", "ldsG"])
@pytest.mark.parametrize("fit", [("logpoly", 2), ("forced",)], ids=["logpoly", "forced"])
def test_log_polynomial_fits(ctx, kernel, fit):
    """The log-polynomial fit and the forced-term fit (zero term planes: the
    mean) run in the Lds kernel only. 60 and 25 components: as far as every
    decision of the oracle's run keeps a relative margin of 1e-4 (asserted in
    run_case)."""
    n_it = 60 if fit[0] == "logpoly" else 25
    o = run_case(ctx, kernel, n_ch=4, fit=fit, max_iterations=n_it)
    dirties, psfs, thr, okw = o.inputs
    plain = ctx["orc"].subminor_run(dirties, psfs, thr, **dict(okw, spectral=None))
    assert len(o.trace) == n_it and not np.array_equal(plain.model, o.model)


@pytest.mark.parametrize("kernel", GENERAL)
def test_everything_at_once(ctx, kernel):
    """RMS, mask, borders, n_pol = 2, weights, the map and iteration_start."""
    wts = [1.0, 0.5, 2.0, 1.0]
    o = run_case(ctx, kernel, n_ch=4, n_pol=2, weights=wts, pol_factor=0.5, rms=True, mask=True,
                 h_border=5, v_border=11, smap=projector(4, 2, wts, 2), iteration_start=1000,
                 max_iterations=1200)
    assert len(o.trace) == 200


@pytest.mark.parametrize("kernel,n_img", [(k, 1) for k in TAB] + TABN,
                         ids=[f"{k}-{ni}img" for k, ni in [(k, 1) for k in TAB] + TABN])
def test_everything_the_table_kernels_take(ctx, kernel, n_img):
    """Mask, borders, weights, iteration_start and stop_on_negative."""
    weights = None if n_img == 1 else list(1.0 + 0.25 * np.arange(n_img))
    o = run_case(ctx, kernel, n_ch=n_img, weights=weights, mask=True, h_border=5, v_border=11,
                 iteration_start=1000, max_iterations=1300, stop_on_negative=1, variant="neg")
    assert 0 < len(o.trace) < 300 and o.peak < 0


# the product path: mode 0 with an option the table kernels do not take, so
# Wave / Big / Reg read the pairwise table; the kind depends on n_sel x n_img
WTS4 = (1.0, 0.5, 2.0, 1.0)  # (weights that make the projector asymmetric)
PRODUCT = [
    ("rms", dict(rms=True), 100, "Wave"),
    ("rms", dict(rms=True), 1500, "Big"),
    ("rms", dict(rms=True, n_ch=4), 3000, "Reg"),
    ("map", dict(n_ch=4, weights=WTS4, smap=(4, 2, WTS4, 1)), 30, "Wave"),
    ("map", dict(n_ch=4, weights=WTS4, smap=(4, 2, WTS4, 1)), 800, "Big"),
    ("map", dict(n_ch=4, weights=WTS4, smap=(4, 2, WTS4, 1)), 3000, "Reg"),
    ("pol", dict(n_ch=2, n_pol=2, weights=[1.0, 0.5], pol_factor=0.5), 30, "Wave"),
    ("pol", dict(n_ch=2, n_pol=2, weights=[1.0, 0.5], pol_factor=0.5), 800, "Big"),
    ("pol", dict(n_ch=2, n_pol=2, weights=[1.0, 0.5], pol_factor=0.5), 3000, "Reg"),
]


@pytest.mark.parametrize("table", [True, False], ids=["table", "gathers"])
@pytest.mark.parametrize("option,kw,n_sel,kind", PRODUCT,
                         ids=[f"{o}-{k}" for o, _, _, k in PRODUCT])
def test_product_path(ctx, option, kw, n_sel, kind, table):
    """RDL_SUBMINOR_TABLE_MAX=0 runs the same kernels on PSF gathers."""
    kw = dict(kw)
    if "smap" in kw:
        kw["smap"] = projector(*kw["smap"])
    o = run_case(ctx, "auto", n_sel=n_sel, expect=(kind, kind == "Reg", table),
                 table_max=None if table else 0, **kw)
    assert o.plan["kind"] != "TabN" and len(o.trace) >= 20


# ------------------------------------------------- paths the options share
def tie_selection(orc, kernel, n_img=1):
    """The kernel's selection size, grown to the whole group of equal values
    its threshold (the n_sel-th largest |integrated value|) falls in on the
    TIE_QUANTUM grid."""
    dirties, _ = images(256, 256, n_img, 1, "ties")
    integ = orc.integrate(dirties, None, 1, 1.0) if n_img > 1 else dirties[0]
    value = np.sort(np.abs(integ).ravel())
    return int(np.count_nonzero(value >= value[-KERNELS[kernel][2](n_img)]))


def assert_exact_ties(o):
    """On the oracle alone: some component was chosen with a decision margin
    of 0, i.e. its runner-up held exactly the same |integrated value|."""
    assert np.any(o.margins[:len(o.trace)] == 0), float(o.margins[:len(o.trace)].min())


@pytest.mark.parametrize("option", ["plain", "positive", "ties"])
def test_table_wave_slots_one_workgroup(ctx, option):
    """RDL_SUBMINOR_ATOMIC=0: one-workgroup Tab reduces through the wave
    slots, the form its grids run, in place of the LDS atomic cells."""
    kw = dict(plain={}, positive=dict(allow_negative=0, variant="neg"),
              ties=dict(variant="ties", n_sel=tie_selection(ctx["orc"], "tab1")))[option]
    o = run_case(ctx, "tab1", env={"RDL_SUBMINOR_ATOMIC": "0"}, **kw)
    assert len(o.trace) >= 20
    if option == "ties":
        assert_exact_ties(o)


@pytest.mark.parametrize("n_img", [2, 8])
def test_joined_table_agent_exchange(ctx, n_img):
    """RDL_SUBMINOR_EXCHANGE=agent: the grid's records of 3 + n_img granules
    through agent-scope stores."""
    o = run_case(ctx, "tabnG", n_ch=n_img, env={"RDL_SUBMINOR_EXCHANGE": "agent"})
    assert len(o.trace) >= 20


TIES = [("tabn1", 2), ("tabn1", 4), ("tabnG", 2), ("tabnG", 4), ("reg1", 1), ("regG", 1)]


@pytest.mark.parametrize("kernel,n_img", TIES, ids=[f"{k}-{ni}img" for k, ni in TIES])
def test_exact_value_ties(ctx, kernel, n_img):
    """Values on a TIE_QUANTUM grid, both signs: among equal |integrated
    values| the lowest selection index wins, within a thread, a wave, a
    workgroup and a grid."""
    o = run_case(ctx, kernel, n_ch=n_img, variant="ties",
                 n_sel=tie_selection(ctx["orc"], kernel, n_img))
    assert len(o.trace) >= 20
    assert_exact_ties(o)
