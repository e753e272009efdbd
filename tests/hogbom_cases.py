"""Inputs and a plain restatement shared by the Högbom loop's direct tests
(test_oracle.py on the CPU, test_hogbom_options_gpu.py on the GPU).
"""
import functools

import numpy as np

from subminor_cases import fma32, linear_integrate, synthetic


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def single(w, h, variant="plain"):
    """One residual plane [1, h, w] and its PSF [1, h, w]. variant "neg": a
    negative copy of every source at 0.6 of its flux, so negative pixels
    become the largest after a few components; "div": the PSF times -0.5, so
    subtracting a component grows its pixel by 5 %."""
    psf, dirty = synthetic(w, h, 60, 7)
    if variant == "neg":
        dirty = (dirty - np.float32(0.6) * np.roll(dirty, (37, 53), axis=(0, 1))).astype(np.float32)
    if variant == "div":
        psf = (psf * np.float32(-0.5)).astype(np.float32)
    return _frozen(dirty[None].copy(), psf[None].copy())


@functools.lru_cache(maxsize=None)
def mixed(w, h, n_img, n_pol=1):
    """n_img residual planes (image = channel * n_pol + pol) that slide from
    one sky to another, A (1 - k/n) + B (k/n) for image k of n, the B part
    negated on odd polarizations; the n_img // n_pol PSFs differ by a scale
    only. The integrated peak then moves between the two skies' sources as
    the weights, the join and the components change, where row-shifted PSFs
    keep a run of many images on one or two pixels."""
    psf, a = synthetic(w, h, 60, 7)
    _, b = synthetic(w, h, 60, 11)
    planes = []
    for k in range(n_img):
        t = np.float32(k / n_img)
        sign = np.float32(-1.0 if (k % n_pol) % 2 else 1.0)
        planes.append(a * (np.float32(1.0) - t) + sign * b * t)
    psfs = [psf * np.float32(1.0 - 0.002 * c) for c in range(n_img // n_pol)]
    return _frozen(np.stack(planes).astype(np.float32), np.stack(psfs).astype(np.float32))


@functools.lru_cache(maxsize=None)
def rms_image(w, h):
    """Smooth, positive, spanning about [0.5, 3.5]."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = 2.0 + 1.5 * np.sin(2 * np.pi * xx / w * 1.5 + 0.3) * np.cos(2 * np.pi * yy / h + 0.2)
    img = img.astype(np.float32)
    assert 0.5 <= img.min() < 0.6 and 3.4 < img.max() <= 3.5
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def mask_image(w, h):
    """The checkerboard of 8 x 8 squares, (0, 0) inside."""
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((xx // 8 + yy // 8) % 2 == 0).astype(np.uint8)
    m.setflags(write=False)
    return m


def border(n, ratio):
    """peak_finder.h:99-107 as GenericClean::FindPeak calls it: round()."""
    return int(np.floor(n * ratio + 0.5))


def numpy_hogbom_map_loop(residual, psfs, weights, smap, threshold, gain, max_iterations):
    """The Högbom branch of GenericClean::ExecuteMajorIteration
    (generic_clean.cc:163-207) in float32 numpy for n_pol = 1, non-zero
    weights, allow_negative, no mask / borders / RMS / divergence, with the
    n_img x n_img map `smap` as the spectral fit: f[i] = (fmaf over q
    ascending of S[i][q] r[q], from 0) * gain. Returns (trace [k, 2] x y,
    residual, model, peak)."""
    n_img, h, w = residual.shape
    f32 = np.float32
    r = residual.astype(f32).reshape(n_img, -1).copy()
    model = np.zeros_like(r)
    trace = []

    def find_peak():
        integ = linear_integrate(r, weights)  # (the square integration of n_pol = 1 is linear)
        idx = int(np.argmax(np.abs(integ)))   # the first of equal values
        assert abs(integ[idx]) > np.finfo(f32).tiny
        return idx, integ[idx]

    idx, peak = find_peak()
    while abs(peak) > f32(threshold) and len(trace) < max_iterations:
        cx, cy = idx % w, idx // w
        trace.append((cx, cy))
        values = r[:, idx].copy()
        x0, x1 = max(cx - w // 2, 0), min(cx + w // 2, w)
        y0, y1 = max(cy - h // 2, 0), min(cy + h // 2, h)
        for i in range(n_img):
            acc = f32(0)
            for q in range(n_img):
                acc = fma32(smap[i, q], values[q], acc)
            f = f32(f32(acc) * f32(gain))
            model[i, idx] += f
            img = r[i].reshape(h, w)
            pv = psfs[i][y0 - cy + h // 2:y1 - cy + h // 2, x0 - cx + w // 2:x1 - cx + w // 2]
            img[y0:y1, x0:x1] = fma32(-pv, f, img[y0:y1, x0:x1])
        idx, peak = find_peak()
    return (np.array(trace, np.int64).reshape(-1, 2), r.reshape(n_img, h, w),
            model.reshape(n_img, h, w), peak)
