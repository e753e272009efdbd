"""radler.PlaneBatch against a loop of radler.Radler over the same planes.

Plane b of a batch must behave as a Radler over that plane alone
(algorithm_type generic_clean, generic.use_sub_minor_optimization False)
whose perform() is called for as long as it returns True. Every case runs
three perform calls on both sides and compares, after each call, the flags
and the iteration numbers, and at the end the residual and model bits. The
Radler side always works on numpy arrays (the unchanged path); the batch
side on numpy stacks or on radler.gpu.to_device stacks, read back through
.numpy() to check that they were updated in place. The inputs hold no -0.

Shapes: 48 x 40 with 5 planes and 128 x 128 with 33. Each case asserts on the
Radler side alone that its setting did something (planes that drop out at
different calls, caps that bite, a mask that excludes components).
"""
import numpy as np
import pytest

from hogbom_batch_lib import bits, make_psf
from radler_import import radler as rd

pytestmark = pytest.mark.gpu

PIXEL_SCALE = np.pi / (180.0 * 3600.0)
SHAPES = [(48, 40, 5), (128, 128, 33)]
CALLS = 3


def settings(w, h, **kw):
    s = rd.Settings()
    s.algorithm_type = rd.AlgorithmType.generic_clean
    s.generic.use_sub_minor_optimization = False
    s.trimmed_image_width, s.trimmed_image_height = w, h
    s.pixel_scale.x = s.pixel_scale.y = PIXEL_SCALE
    s.minor_iteration_count = 2000
    s.major_loop_gain = 0.8
    for name, value in kw.items():
        setattr(s, name, value)
    return s


def inputs(w, h, n_planes, per_plane_psf=False):
    """Planes of six sources of both signs over noise of 0.004; the fluxes
    grow by a factor 40 from the first plane to the last, so that the planes
    reach a threshold after different numbers of calls. Plane 1 is all zeros."""
    rng = np.random.default_rng(51)
    psf = make_psf(w, h).astype(np.float64)
    residuals = np.empty((n_planes, h, w), np.float32)
    for b in range(n_planes):
        img = 0.004 * rng.standard_normal((h, w))
        for _ in range(6):
            amp = 0.15 * 40.0 ** (b / (n_planes - 1)) * rng.uniform(0.4, 1.0)
            amp *= 1.0 if rng.random() < 0.7 else -1.0
            img += amp * np.roll(psf, (int(rng.integers(h)), int(rng.integers(w))), axis=(0, 1))
        residuals[b] = img
    residuals[1] = 0.0
    assert not (bits(residuals) == 0x80000000).any()
    psfs = (np.stack([make_psf(w, h, seed=b) for b in range(n_planes)]) if per_plane_psf
            else make_psf(w, h))
    return psfs, residuals, np.zeros_like(residuals)


def radler_loop(make_settings, psfs, residuals, models, masks, tmp_path):
    """One Radler per plane, perform(k) for k = 1.. while it returns True.
    Returns flags [CALLS, B], iteration numbers [CALLS, B], residuals, models."""
    n_planes, h, w = residuals.shape
    residuals, models = residuals.copy(), models.copy()
    flags = np.zeros((CALLS, n_planes), bool)
    iterations = np.zeros((CALLS, n_planes), np.uint64)
    for b in range(n_planes):
        s = make_settings()
        if masks is not None:
            mask = masks if masks.ndim == 2 else masks[b]
            path = str(tmp_path / f"mask{b}.fits")
            rd.io.write_fits(path, mask.astype(np.float32), PIXEL_SCALE, PIXEL_SCALE)
            s.fits_mask = path
        psf = psfs if psfs.ndim == 2 else psfs[b]
        radler = rd.Radler(s, psf, residuals[b], models[b], 0.0)
        another = True
        for k in range(CALLS):
            if another:
                another = radler.perform(k + 1)
            flags[k, b] = another
            iterations[k, b] = radler.iteration_number
        del radler
    return flags, iterations, residuals, models


def batch_run(make_settings, psfs, residuals, models, masks, on_device):
    residuals, models = residuals.copy(), models.copy()
    if on_device:
        d_psfs, d_residuals, d_models = (rd.gpu.to_device(a) for a in (psfs, residuals, models))
        batch = rd.PlaneBatch(make_settings(), d_psfs, d_residuals, d_models, masks)
    else:
        batch = rd.PlaneBatch(make_settings(), psfs, residuals, models, masks)
    n_planes = residuals.shape[0]
    assert batch.n_planes == n_planes
    flags = np.zeros((CALLS, n_planes), bool)
    iterations = np.zeros((CALLS, n_planes), np.uint64)
    for k in range(CALLS):
        flags[k] = batch.perform(k + 1)
        iterations[k] = batch.iteration_numbers
    if on_device:
        assert np.array_equal(bits(d_psfs.numpy()), bits(psfs))
        return flags, iterations, d_residuals.numpy(), d_models.numpy()
    return flags, iterations, residuals, models


def compare(make_settings, w, h, n_planes, tmp_path, on_device, masks=None, per_plane_psf=False):
    psfs, residuals, models = inputs(w, h, n_planes, per_plane_psf)
    want = radler_loop(make_settings, psfs, residuals, models, masks, tmp_path)
    got = batch_run(make_settings, psfs, residuals, models, masks, on_device)
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(bits(got[2]), bits(want[2]))
    assert np.array_equal(bits(got[3]), bits(want[3]))
    return want


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("w,h,n_planes", SHAPES)
def test_absolute_threshold_three_calls(tmp_path, w, h, n_planes, on_device):
    """major_loop_gain 0.8 and an absolute threshold: the faint planes are
    done after the first call, others after the second, the bright ones need
    all three."""
    flags, iterations, _, models = compare(lambda: settings(w, h, absolute_threshold=0.05),
                                           w, h, n_planes, tmp_path, on_device)
    assert not flags[:, 1].any() and iterations[-1, 1] == 0 and not models[1].any()
    calls_needed = flags.sum(axis=0)
    assert set(calls_needed.tolist()) >= {0, 1, 2} and not flags[0].all()
    assert (iterations[-1] > iterations[0])[flags[0]].all()


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("w,h,n_planes", SHAPES)
def test_auto_threshold(tmp_path, w, h, n_planes, on_device):
    """The threshold of every plane and call from that plane's own median
    and MAD; per-plane PSFs."""
    flags, iterations, _, _ = compare(
        lambda: settings(w, h, auto_threshold_sigma=5.0, absolute_threshold=1e-4),
        w, h, n_planes, tmp_path, on_device, per_plane_psf=True)
    assert flags[0].any() and iterations[-1].max() > 20
    fixed = radler_loop(lambda: settings(w, h, absolute_threshold=1e-4),
                        *inputs(w, h, n_planes, True), None, tmp_path)
    assert not np.array_equal(fixed[1], iterations)


@pytest.mark.parametrize("cap", ["minor", "major", "gain-1"])
@pytest.mark.parametrize("w,h,n_planes", SHAPES)
def test_caps(tmp_path, w, h, n_planes, cap):
    """minor_iteration_count = 30 ends every bright plane at 30 components
    with its flag False; major_iteration_count = 2 turns the flags of the
    second call False; major_loop_gain = 1 cleans to the threshold in one
    call."""
    kw = dict(minor=dict(minor_iteration_count=30), major=dict(major_iteration_count=2),
              **{"gain-1": dict(major_loop_gain=1.0)})[cap]
    flags, iterations, _, _ = compare(lambda: settings(w, h, absolute_threshold=0.02, **kw),
                                      w, h, n_planes, tmp_path, cap == "major")
    free = radler_loop(lambda: settings(w, h, absolute_threshold=0.02),
                       *inputs(w, h, n_planes), None, tmp_path)
    if cap == "minor":
        assert iterations.max() == 30 and (iterations[-1] == 30).sum() >= 2
        assert not flags[-1].any() and free[1].max() > 30
    elif cap == "major":
        assert flags[0].any() and not flags[1].any() and free[0][1].any()
    else:
        assert not flags.any() and iterations[0].max() > 30
        assert np.array_equal(iterations[0], iterations[-1])


@pytest.mark.parametrize("kind", ["shared", "per-plane"])
@pytest.mark.parametrize("w,h,n_planes", SHAPES)
def test_masks(tmp_path, w, h, n_planes, kind):
    """The masks argument against the same masks as fits_mask files; with
    per-plane masks plane 2's excludes everything. Options on top: a border,
    positive components only."""
    yy, xx = np.mgrid[0:h, 0:w]
    shared = ((xx // 5 + yy // 3) % 2 == 0)
    if kind == "shared":
        masks = shared
    else:
        masks = np.stack([np.roll(shared, b, axis=1) for b in range(n_planes)]).astype(np.uint8)
        masks[2] = 0

    def make():
        return settings(w, h, absolute_threshold=0.05, border_ratio=0.08,
                        allow_negative_components=False)
    flags, iterations, _, models = compare(make, w, h, n_planes, tmp_path, kind == "per-plane",
                                           masks=masks)
    assert iterations[-1].max() > 20
    for b in range(n_planes):
        mask = masks if masks.ndim == 2 else masks[b]
        assert not models[b][mask == 0].any()
    if kind == "per-plane":
        assert iterations[-1, 2] == 0 and not flags[:, 2].any()
    free = radler_loop(make, *inputs(w, h, n_planes), None, tmp_path)
    assert not np.array_equal(free[1], iterations)


def test_stop_on_negative_and_divergence(tmp_path):
    """stop_on_negative_components, and a plane whose PSF alone makes it
    diverge: Radler's answers for both."""
    w, h, n_planes = 48, 40, 5
    psfs, residuals, models = inputs(w, h, n_planes, per_plane_psf=True)
    psfs[3, h // 2, w // 2 + 2] = -1.6
    residuals[4] = -np.abs(residuals[4])

    def make():
        return settings(w, h, absolute_threshold=0.01, stop_on_negative_components=True,
                        minor_loop_gain=0.2)
    want = radler_loop(make, psfs, residuals, models, None, tmp_path)
    got = batch_run(make, psfs, residuals, models, None, False)
    for g, w_ in zip(got[:2], want[:2]):
        assert np.array_equal(g, w_), (g, w_)
    assert np.array_equal(bits(got[2]), bits(want[2]))
    assert np.array_equal(bits(got[3]), bits(want[3]))
    assert want[1][-1, 4] == 0 and want[1][-1, 3] > 0 and not want[0][:, 3].any()
