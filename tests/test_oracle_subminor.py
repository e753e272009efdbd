"""The oracle's direct sub-minor loop entry (orc_subminor_run, bound as
Oracle.subminor_run) on the CPU: it reproduces the loop GenericClean's Clark
path runs, and its map path equals a plain float32 restatement.
"""
import numpy as np
import pytest

from oracle_lib import OracleAlgorithm, get_oracle
from subminor_cases import fma32, joined, numpy_subminor_map_loop, synthetic


@pytest.fixture(scope="module")
def orc():
    return get_oracle()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fma32_rounds_once():
    """fma32 against exact rational arithmetic, on values built to land the
    float64 sum on float32 ties and near them."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = rng.standard_normal(4000).astype(np.float32)
    # ties: c = (a float32 tie) - a*b rounded, so that a*b + c is close to a tie
    base = rng.standard_normal(2000).astype(np.float32)
    half_ulp = (np.nextafter(base, np.float32(np.inf)) - base).astype(np.float64) / 2
    tie = base.astype(np.float64) + half_ulp
    c[:2000] = (tie - a[:2000].astype(np.float64) * b[:2000].astype(np.float64)).astype(np.float32)
    got = fma32(a, b, c)

    def round32(x):  # Fraction -> nearest float32, ties to even
        lo = np.float32(float(x))
        cands = {lo, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf))}
        best = min(cands, key=lambda f: (abs(Fraction(float(f)) - x),
                                         int(np.float32(f).view(np.uint32)) & 1))
        return np.float32(best)

    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert bits(got[i]) == bits(round32(exact)), i


@pytest.mark.parametrize("w,n_src,threshold_frac,mgain,max_iter,n_ch", [
    (128, 10, 0.0, 0.8, 300, 1),     # SUBMINOR_CASES[0] of test_gpu_kernels.py
    (200, 30, 0.002, 0.9, 800, 2),   # its first joined case
])
def test_entry_reproduces_generic_clean(orc, w, n_src, threshold_frac, mgain, max_iter, n_ch):
    """Given the threshold GenericClean derives, the entry takes the same
    components as OracleAlgorithm(kind 0, use_sub_minor=1): iteration count,
    trace and every image's model."""
    h = w
    psf, dirty = synthetic(w, h, n_src, 7)
    dirties = np.stack([dirty * np.float32(1.0 + 0.15 * k) + np.float32(1e-3 * k) *
                        np.roll(dirty, 3 * k, axis=1) for k in range(n_ch)]).astype(np.float32)
    psfs = np.stack([psf] * n_ch)
    integ = orc.integrate(dirties) if n_ch > 1 else dirties[0]
    thr = threshold_frac * float(np.abs(integ).max())
    res_o, mod_o = dirties.copy(), np.zeros((n_ch, h, w), np.float32)
    alg = OracleAlgorithm(orc, 0, threshold=thr, max_iterations=max_iter, border_ratio=0.0,
                          use_sub_minor=1, major_loop_gain=mgain)
    r, trace_o = alg.execute(res_o, mod_o, psfs)
    _, _, _, v = orc.find_peak(integ, True)
    # generic_clean.cc:99-112 in float arithmetic
    first = max(np.float32(thr), np.float32(abs(v)) * (np.float32(1.0) - np.float32(mgain)))
    run = orc.subminor_run(dirties, psfs, first, gain=0.1, divergence_limit=4.0,
                           max_iterations=max_iter)
    assert run.iteration == r.iteration_number and run.iteration > 20
    assert np.array_equal(run.trace, trace_o[:, :2])
    assert run.has_peak == 1 and bits(run.peak) == bits(r.final_peak)
    assert run.margins.shape == (run.iteration + 1,) and np.all(run.margins >= 0)
    ys, xs = run.positions >> 16, run.positions & 0xffff
    for k in range(n_ch):
        full = np.zeros((h, w), np.float32)
        full[ys, xs] = run.model[k]
        assert np.array_equal(bits(full), bits(mod_o[k])), k


def test_entry_options_reach_the_loop(orc):
    """Borders, the mask, the iteration window and an empty selection."""
    w, h = 64, 48
    psf, dirty = synthetic(w, h, 12, 5)
    thr = float(np.sort(np.abs(dirty).ravel())[-200])
    rng = np.random.default_rng(1)
    mask = rng.random((h, w)) < 0.7
    run = orc.subminor_run(dirty[None], psf[None], thr, h_border=5, v_border=11, mask=mask,
                           iteration_start=1000, max_iterations=1010)
    ys, xs = (run.positions >> 16).astype(int), (run.positions & 0xffff).astype(int)
    keep = (np.abs(dirty) >= np.float32(thr)) & mask
    keep[:11] = keep[h - 11:] = False
    keep[:, :5] = keep[:, w - 5:] = False
    ey, ex = np.nonzero(keep)
    assert np.array_equal(ys, ey) and np.array_equal(xs, ex) and run.n_selected == ey.size
    assert run.iteration == 1010 and len(run.trace) == 10
    none = orc.subminor_run(dirty[None], psf[None], 1e9)
    assert (none.n_selected, none.has_peak, none.iteration) == (0, 0, 0)
    stay = orc.subminor_run(dirty[None], psf[None], thr, iteration_start=7, max_iterations=7)
    assert stay.has_peak == 1 and len(stay.trace) == 0 and not stay.model.any()
    assert abs(stay.peak) == np.abs(dirty).max()


def test_map_path_equals_numpy_restatement(orc):
    """24 x 16, 3 images, 30 selected pixels: the spectral map path of the
    oracle against the loop written out in numpy float32 (one rounding per
    operation, fused multiply-adds where the oracle has them)."""
    w, h, n_img = 24, 16, 3
    psf, dirty = synthetic(w, h, 6, 11, margin=3)
    dirties, psfs = joined(dirty, psf, n_img)
    weights = np.array([1.0, 0.5, 2.0], np.float32)
    rng = np.random.default_rng(2)
    smap = (np.eye(n_img) * 0.7 + 0.3 * rng.random((n_img, n_img)) / n_img).astype(np.float32)
    integ = orc.integrate(dirties, weights)
    thr = np.float32(np.sort(np.abs(integ).ravel())[-30])
    run = orc.subminor_run(dirties, psfs, thr, gain=0.1, divergence_limit=0.0,
                           max_iterations=60, spectral_map=smap, weights=weights)
    pos, trace, model, peak, flux = numpy_subminor_map_loop(dirties, psfs, weights, smap, thr,
                                                            0.1, 60)
    assert run.n_selected == 30
    assert np.array_equal(run.positions & 0xffff, pos[:, 0])
    assert np.array_equal(run.positions >> 16, pos[:, 1])
    assert len(trace) > 20 and np.array_equal(run.trace, trace)
    assert np.array_equal(bits(run.model), bits(model))
    assert bits(run.peak) == bits(peak) and bits(run.flux_cleaned) == bits(flux)
    # the map matters: without it the model differs
    plain = orc.subminor_run(dirties, psfs, thr, gain=0.1, divergence_limit=0.0,
                             max_iterations=60, weights=weights)
    assert not np.array_equal(plain.model, run.model)
