"""rdl_hogbom_batch_run (csrc/hip/clean_batch.hip) against the path it
replaces, plane by plane and bit for bit.

Every case cleans the same planes twice: once with one batch call over
stacks whose planes lie PAD elements apart (hogbom_batch_lib.run_batch, which
also asserts that the gaps, the PSFs and the masks come back untouched), once
with rdl_find_peak + rdl_hogbom_run per plane (run_loop). Compared bit for
bit: every residual and model plane, the trace (entries past
min(components, trace_cap) still holding the fill value), and the eleven
fields of the result: iteration, peak, x, y, found, diverging, the start
peak's value, x, y, found, and first_threshold. Each case asserts on the
loop's answer alone that its option did something.

Shapes: 1 x 1, 5 x 3 and 17 x 9 (planes far below a workgroup), 64 x 64 and
65 x 64 (the last size of the 64-thread workgroup and the first of the
256-thread one), 255 x 257, 256 x 256 and 257 x 256 (the last size of the
256-thread workgroup and the first of the 1024-thread one: one pixel more per
thread somewhere), 1024 x 1024 once with a dozen components, and 1025 x 1024,
which is refused. Plane counts 1, 2, 3, 257 and, at 16 x 16, 1025.

Which case catches which wrong kernel:
* a dropped last row: test_shapes (every size: the sources and the noise
  reach the last row, which the window of nearly every component covers) and
  test_borders[none];
* a stale winner value (the peak read before the sweep's stores are
  visible): test_shapes and test_stops_differ, through peak, the factors that
  follow from it (model and residual bits) and the threshold stops;
* a plane that keeps running after done: test_stops_differ (iteration, the
  model and the trace of the planes that stop early) and test_resume (a plane
  done in the first launch is launched again unless the host drops it);
* a shared-PSF stride applied as per-plane: every case with a shared PSF and
  more than one plane (the second plane would read past the one PSF plane);
  test_psfs[shared] by name.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import hogbom_batch_lib as hb
from hogbom_batch_lib import (FILL, OUT_FILL, assert_same, bits, make_planes, make_psf, options,
                              run_batch, run_loop)
from hogbom_cases import border
from oracle_lib import OracleAlgorithm, get_oracle
from rdl_lib import RdlError, Session

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sess():
    s = Session(0)
    yield s
    s.close()


def both(sess, **case):
    """The case through the batch and through the loop, compared; returns the
    loop's Run."""
    got = run_batch(sess, **case)
    want = run_loop(sess, **case)
    assert_same(got, want)
    return want


def plain_case(w, h, n_planes, max_iterations, seed=1, **kw):
    residuals = make_planes(w, h, n_planes, seed)
    case = dict(residuals=residuals, models=np.zeros_like(residuals), psfs=make_psf(w, h),
                masks=None, opt=options(), thresholds=0.0, iteration_start=0,
                max_iterations=max_iterations, trace_cap=max(int(np.max(max_iterations)), 1))
    case.update(kw)
    return case


# -------------------------------------------------------------------- shapes
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (17, 9), (64, 64), (65, 64), (255, 257),
                                 (256, 256), (257, 256)])
def test_shapes(sess, w, h):
    want = both(sess, **plain_case(w, h, 3, [30, 17, 24]))
    assert list(want.iterations()) == [30, 17, 24]
    if w * h > 16:
        for b in range(3):
            n = int(want.iterations()[b])
            assert len({tuple(t) for t in want.trace[b, :n].tolist()}) >= 4
        # components in the last row and column of some plane's window: the
        # residual's last row and column changed
        assert not np.array_equal(want.residual[:, -1, :], make_planes(w, h, 3)[:, -1, :])
        assert not np.array_equal(want.residual[:, :, -1], make_planes(w, h, 3)[:, :, -1])


def test_largest_plane(sess):
    """1024 x 1024, the cap itself, a dozen components on two planes."""
    want = both(sess, **plain_case(1024, 1024, 2, 12))
    assert list(want.iterations()) == [12, 12]


def test_plane_above_the_cap_is_refused(sess):
    residuals = np.zeros((1, 1024, 1025), np.float32)
    with pytest.raises(RdlError, match="2\\^20"):
        run_batch(sess, residuals=residuals, models=residuals.copy(), psfs=residuals[0],
                  masks=None, opt=options(), thresholds=0.0, iteration_start=0,
                  max_iterations=3)


# -------------------------------------------------------------- plane counts
@pytest.mark.parametrize("n_planes", [1, 2, 257])
def test_plane_counts(sess, n_planes):
    caps = 4 + np.arange(n_planes) % 13
    want = both(sess, **plain_case(40, 24, n_planes, caps, seed=5))
    assert np.array_equal(want.iterations(), caps)


def test_more_planes_than_workgroup_slots(sess):
    """1025 planes of 16 x 16: 64-thread workgroups, more of them than one
    launch holds at once on a few CUs; every plane its own cap."""
    caps = 1 + np.arange(1025) % 7
    want = both(sess, **plain_case(16, 16, 1025, caps, seed=6))
    assert np.array_equal(want.iterations(), caps)


# ------------------------------------------------------------------- options
def signed_case(**kw):
    """Six 48 x 40 planes with sources of both signs; plane 4's largest
    pixel is negative."""
    w, h = 48, 40
    residuals = make_planes(w, h, 6, seed=11)
    if residuals[4].flat[np.argmax(np.abs(residuals[4]))] > 0:
        residuals[4] = -residuals[4]
    case = plain_case(w, h, 6, 60, residuals=residuals, models=np.zeros_like(residuals))
    case.update(kw)
    return case


@pytest.mark.parametrize("allow_negative", [0, 1])
@pytest.mark.parametrize("stop_on_negative", [0, 1])
def test_sign_rules(sess, allow_negative, stop_on_negative):
    want = both(sess, **signed_case(opt=options(allow_negative=allow_negative,
                                                stop_on_negative=stop_on_negative)))
    it, peak = want.iterations(), want.field("peak").astype(np.uint32).view(np.float32)
    if stop_on_negative and allow_negative:
        assert it[4] == 0 and peak[4] < 0 and it.max() > 0
    elif allow_negative:
        assert (it == 60).all() and want.model.min() < 0 < want.model.max()
    else:
        assert (it == 60).all() and want.model[:4].min() >= 0


@pytest.mark.parametrize("name,hb,vb", [("none", 0, 0), ("small", 3, 2), ("no-columns", 24, 2),
                                        ("no-rows", 3, 20), ("narrow", 21, 17),
                                        ("beyond", 50, 45)])
def test_borders(sess, name, hb, vb):
    """The box against the subtraction window (about 48 x 40 around each
    component): no box columns or rows at all (the start peak is pixel 0,
    found, as rdl_find_peak says without a mask), and a box of 6 x 6, far
    narrower than the window."""
    want = both(sess, **signed_case(opt=options(h_border=hb, v_border=vb)))
    it = want.iterations()
    xs, ys = want.trace[:, :, 0], want.trace[:, :, 1]
    taken = xs != FILL
    if name in ("no-columns", "no-rows", "beyond"):
        assert (want.field("start_found") == 1).all() and (want.field("start_x") == 0).all()
        assert (xs[taken] == 0).all() and (ys[taken] == 0).all()
    else:
        assert (it == 60).all()
        assert (xs[taken] >= hb).all() and (xs[taken] < 48 - hb).all()
        assert (ys[taken] >= vb).all() and (ys[taken] < 40 - vb).all()


def checker(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx // 4 + yy // 4) % 2 == 0).astype(np.uint8)


@pytest.mark.parametrize("kind", ["shared", "per-plane", "bool-like"])
def test_masks(sess, kind):
    """A shared mask; per-plane masks of which plane 2's excludes everything
    (no start peak: nothing of that plane changes) and plane 3's allows one
    pixel (gain 1 zeroes it and the next search finds nothing)."""
    w, h = 48, 40
    case = signed_case(opt=options(gain=1.0 if kind == "per-plane" else 0.1, allow_negative=0))
    if kind == "shared":
        case["masks"] = checker(w, h)
    elif kind == "bool-like":
        case["masks"] = checker(w, h) * np.uint8(200)  # any non-zero byte allows
    else:
        masks = np.stack([np.roll(checker(w, h), b, axis=1) for b in range(6)])
        masks[2] = 0
        masks[3] = 0
        y, x = np.unravel_index(np.argmax(case["residuals"][3]), (h, w))
        masks[3, y, x] = 1
        case["masks"] = masks
    case["max_iterations"] = 25
    want = both(sess, **case)
    found, it = want.field("found"), want.iterations()
    if kind == "per-plane":
        assert want.field("start_found")[2] == 0 and it[2] == 0 and found[2] == 0
        assert (want.field("start_x")[2], want.field("start_y")[2]) == (w, h)
        assert np.array_equal(bits(want.residual[2]), bits(case["residuals"][2]))
        assert it[3] == 1 and found[3] == 0 and bits(want.residual[3, y, x]) == 0
        assert (found[[0, 1, 4, 5]] == 1).all()
    else:
        assert (it == 25).all()
    for b in range(6):
        m = case["masks"] if case["masks"].ndim == 2 else case["masks"][b]
        for x_, y_ in want.trace[b, :int(it[b])].tolist():
            assert m[y_, x_]
    plain = run_loop(sess, **dict(case, masks=None))
    assert not np.array_equal(plain.trace, want.trace)


@pytest.mark.parametrize("kind", ["shared", "per-plane"])
def test_psfs(sess, kind):
    w, h = 48, 40
    case = signed_case()
    if kind == "per-plane":
        case["psfs"] = np.stack([make_psf(w, h, seed=3 * b) for b in range(6)])
    want = both(sess, **case)
    assert (want.iterations() == 60).all()
    if kind == "per-plane":
        shared = run_loop(sess, **dict(case, psfs=case["psfs"][0]))
        assert np.array_equal(bits(shared.residual[0]), bits(want.residual[0]))
        assert all(not np.array_equal(shared.residual[b], want.residual[b]) for b in range(1, 6))


@pytest.mark.parametrize("major_loop_gain", [1.0, 0.8])
def test_major_loop_gain(sess, major_loop_gain):
    want = both(sess, **signed_case(opt=options(major_loop_gain=major_loop_gain),
                                    max_iterations=500, trace_cap=64))
    first = want.field("first_threshold").astype(np.uint32).view(np.float32)
    start = want.field("start_value").astype(np.uint32).view(np.float32)
    if major_loop_gain == 1.0:
        assert (first == 0).all() and (want.iterations() == 500).all()
    else:
        assert np.allclose(first, 0.2 * np.abs(start), rtol=1e-6) and (first > 0).all()
        it = want.iterations()
        assert (it > 0).all() and (it < 500).all() and len(set(it.tolist())) >= 3
        peak = want.field("peak").astype(np.uint32).view(np.float32)
        assert (np.abs(peak) <= first).all()


def test_iteration_start(sess):
    """Loops that count on from 5, 0 and 17; the third is already at its cap
    (zero components), the sixth past it."""
    want = both(sess, **signed_case(iteration_start=[5, 0, 17, 2, 40, 30],
                                    max_iterations=[30, 12, 17, 3, 41, 29]))
    assert list(want.iterations()) == [30, 12, 17, 3, 41, 30]
    taken = (want.trace[:, :, 0] != FILL).sum(axis=1)
    assert list(taken) == [25, 12, 0, 1, 1, 0]
    assert not want.model[2].any() and not want.model[5].any()


def stops_differ_case():
    """Eight 48 x 40 planes with per-plane PSFs that end for eight reasons:
    0 the iteration cap, 1 a threshold, 2 a cap of zero, 3 all zeros (the
    start peak is pixel 0 with value 0), 4 inactive, 5 divergence (its PSF
    alone has a sidelobe of -1.6 two pixels from the centre), 6 a threshold
    above the start peak, 7 a later cap."""
    w, h = 48, 40
    residuals = make_planes(w, h, 8, seed=21)
    residuals[3] = 0.0
    psfs = np.stack([make_psf(w, h, seed=b) for b in range(8)])
    psfs[5, h // 2, w // 2 + 2] = -1.6
    return dict(residuals=residuals, models=np.zeros_like(residuals), psfs=psfs, masks=None,
                opt=options(gain=0.2), thresholds=[0.0, 0.35, 0.0, 0.0, 0.0, 0.0, 50.0, 0.01],
                iteration_start=0, max_iterations=[40, 400, 0, 40, 40, 400, 40, 90],
                active=[1, 1, 1, 1, 0, 1, 1, 1], trace_cap=100)


def test_stops_differ(sess):
    case = stops_differ_case()
    got = run_batch(sess, **case)
    want = run_loop(sess, **case)
    on = [0, 1, 2, 3, 5, 6, 7]
    assert_same(got, want, on)
    it = want.iterations()
    assert it[0] == 40 and 0 < it[1] < 400 and it[2] == 0 and it[3] == 0 and it[6] == 0
    assert it[7] == 90
    diverging = want.field("diverging")
    assert diverging[5] == 1 and 0 < it[5] < 400 and diverging[on].sum() == 1
    assert want.field("start_found")[3] == 1 and want.field("start_value")[3] == 0
    # the inactive plane: not written, its result slot and trace rows as given
    assert np.array_equal(bits(got.residual[4]), bits(case["residuals"][4]))
    assert not got.model[4].any()
    assert (got.raw[4] == OUT_FILL).all() and (got.trace[4] == FILL).all()
    assert not (got.raw[on] == OUT_FILL).all(axis=1).any()


def test_no_active_plane(sess):
    case = stops_differ_case()
    got = run_batch(sess, **dict(case, active=0))
    assert np.array_equal(bits(got.residual), bits(case["residuals"])) and not got.model.any()
    assert (got.raw == OUT_FILL).all() and (got.trace == FILL).all()


@pytest.mark.parametrize("variant", ["below", "above", "zero", "null"])
def test_trace_caps(sess, variant):
    kw = dict(below=dict(trace_cap=10), above=dict(trace_cap=200), zero=dict(trace_cap=0),
              null=dict(trace_cap=10, null_trace=True))[variant]
    case = dict(stops_differ_case(), **kw)
    got = run_batch(sess, **case)
    want = run_loop(sess, **case)
    assert_same(got, want, [0, 1, 2, 3, 5, 6, 7])
    full = run_loop(sess, **stops_differ_case())
    assert np.array_equal(bits(full.residual), bits(want.residual))
    filled = (want.trace[:, :, 0] != FILL).sum(axis=1)
    expect = dict(below=np.minimum(full.iterations(), 10),
                  above=np.minimum(full.iterations(), 200), zero=0 * filled,
                  null=0 * filled)[variant]
    if variant == "above":
        assert (full.iterations() < 200).sum() >= 5
    assert np.array_equal(filled, expect)


def test_nan_and_infinities(sess):
    """Plane 1 holds a NaN, a +Inf and a -Inf pixel inside the box. NaN is
    never a peak; +Inf is the start peak, and the component it makes turns
    its window into NaN and infinities, which the loop goes on taking as
    peaks. The other planes are as without them."""
    case = signed_case(max_iterations=20)
    clean = run_loop(sess, **case)
    residuals = case["residuals"].copy()
    residuals[1, 7, 9] = np.nan
    residuals[1, 20, 30] = np.inf
    residuals[1, 33, 3] = -np.inf
    case = dict(case, residuals=residuals)
    with np.errstate(invalid="ignore"):
        want = both(sess, **case)
    assert want.field("start_value")[1] == hb.f32bits(np.inf)
    assert (want.field("start_x")[1], want.field("start_y")[1]) == (30, 20)
    assert np.isnan(want.residual[1]).sum() > 1
    others = [0, 2, 3, 4, 5]
    assert np.array_equal(bits(want.residual[others]), bits(clean.residual[others]))
    assert np.array_equal(want.out[others], clean.out[others])


def test_load_rule(sess):
    """RDL_HOGBOM_BATCH_LOAD_RULE: the -0 pixels of the active planes'
    residuals and models become +0 (a plane as ImageSet::LoadAndAverage would
    have loaded it), and nothing else changes; the inactive plane keeps its."""
    case = stops_differ_case()
    residuals, models = case["residuals"].copy(), case["models"].copy()
    residuals[:, 5, 7:11] = -0.0
    residuals[:, 0, 0] = -0.0
    models[:, 9, 3:30] = -0.0
    case.update(residuals=residuals, models=models)
    got = run_batch(sess, flags=hb.LOAD_RULE, **case)
    loaded = dict(case, residuals=residuals + np.float32(0.0), models=models + np.float32(0.0))
    assert not (bits(loaded["residuals"]) == 0x80000000).any()
    assert not (bits(loaded["models"]) == 0x80000000).any()
    on = [0, 1, 2, 3, 5, 6, 7]
    assert_same(got, run_loop(sess, **loaded), on)
    assert np.array_equal(bits(got.residual[4]), bits(residuals[4]))
    assert np.array_equal(bits(got.model[4]), bits(models[4]))
    # without the flag the zeros keep their sign where nothing touches them
    plain = run_batch(sess, **case)
    assert_same(plain, run_loop(sess, **case), on)
    assert (bits(plain.model[2]) == 0x80000000).sum() == 27
    assert (bits(got.model[2]) == 0x80000000).sum() == 0


# -------------------------------------------------------------- independence
def test_exact_strides(sess, monkeypatch):
    """Planes back to back (stride = width x height), as a (B, H, W) array is."""
    monkeypatch.setattr(hb, "PAD", 0)
    case = stops_differ_case()
    assert_same(run_batch(sess, **case), run_loop(sess, **case), [0, 1, 2, 3, 5, 6, 7])


def test_permuted_planes(sess):
    """The planes in another order give the same outputs in that order."""
    case = stops_differ_case()
    perm = np.array([5, 2, 7, 0, 4, 6, 1, 3])
    permuted = dict(case)
    for key in ("residuals", "models", "psfs"):
        permuted[key] = case[key][perm]
    for key in ("thresholds", "max_iterations", "active"):
        permuted[key] = list(np.array(case[key])[perm])
    a, b = run_batch(sess, **case), run_batch(sess, **permuted)
    assert np.array_equal(bits(a.residual[perm]), bits(b.residual))
    assert np.array_equal(bits(a.model[perm]), bits(b.model))
    assert np.array_equal(a.trace[perm], b.trace) and np.array_equal(a.raw[perm], b.raw)


# ------------------------------------------------------------------ resuming
@pytest.fixture(scope="module")
def resume_default(sess):
    case = hb.resume_case()
    run = run_batch(sess, **case)
    assert_same(run, run_loop(sess, **case))
    it = run.iterations()
    assert it[0] == 23 and it[2] == 1 and it[4] == 16 and len(set(it.tolist())) == 5
    return run


@pytest.mark.parametrize("chunk", [1, 2, 7])
def test_resume(resume_default, tmp_path, chunk):
    """A child process whose launches end after `chunk` components per plane
    gives the bits of the default, which runs every plane in one launch."""
    out = tmp_path / "run.npz"
    env = dict(os.environ, RDL_HOGBOM_BATCH_CHUNK=str(chunk))
    subprocess.run([sys.executable, hb.__file__, str(out)], env=env, check=True, timeout=120,
                   cwd=os.path.dirname(hb.__file__))
    child = np.load(out)
    assert np.array_equal(child["out"], resume_default.out)
    assert np.array_equal(child["trace"], resume_default.trace)
    assert np.array_equal(bits(child["residual"]), bits(resume_default.residual))
    assert np.array_equal(bits(child["model"]), bits(resume_default.model))


# -------------------------------------------------------------------- oracle
def test_against_the_oracle(sess):
    """One plane of a batch against the oracle's Högbom branch of
    GenericClean (kind 0 without the sub-minor loop), driven as
    test_hogbom_options_gpu.py drives it: mask, borders, major loop gain 0.8."""
    w, h = 61, 45
    residuals = make_planes(w, h, 3, seed=41)
    psf = make_psf(w, h)
    mask = checker(w, h)
    ratio = 0.1
    opt = options(major_loop_gain=0.8, h_border=border(w, ratio), v_border=border(h, ratio))
    got = run_batch(sess, residuals=residuals, models=np.zeros_like(residuals), psfs=psf,
                    masks=mask, opt=opt, thresholds=0.01, iteration_start=0, max_iterations=300,
                    trace_cap=300)
    orc = get_oracle()
    for b in range(3):
        res_o, mod_o = residuals[b][None].copy(), np.zeros((1, h, w), np.float32)
        alg = OracleAlgorithm(orc, 0, threshold=0.01, major_iteration_threshold=0.0,
                              major_loop_gain=0.8, minor_loop_gain=0.1, border_ratio=ratio,
                              divergence_limit=4.0, max_iterations=300, allow_negative=1,
                              stop_on_negative=0, use_sub_minor=0, clean_mask=mask)
        r, trace = alg.execute(res_o, mod_o, psf[None])
        n = int(r.iteration_number)
        assert 5 < n < 300 and int(got.iterations()[b]) == n
        assert np.array_equal(got.trace[b, :n], trace[:n, :2])
        assert (got.trace[b, n:] == FILL).all()
        assert np.array_equal(bits(got.residual[b]), bits(res_o[0]))
        assert np.array_equal(bits(got.model[b]), bits(mod_o[0]))
        assert got.field("start_value")[b] == hb.f32bits(r.starting_peak)
        assert got.field("peak")[b] == hb.f32bits(r.final_peak)
        assert got.field("diverging")[b] == int(r.is_diverging) == 0
