"""Inputs and plain restatements shared by the sub-minor loop's direct tests
(test_oracle_subminor.py on the CPU, test_subminor_options_gpu.py on the GPU).
"""
import numpy as np


def synthetic(w, h, n_src, seed, psf_fwhm=3.0, margin=8):
    """Small deterministic sky convolved with an analytic PSF whose peak is
    exactly 1.0 at (w // 2, h // 2); any w, h. Sources keep `margin` pixels
    from the edges."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    s = psf_fwhm / 2.355
    r2 = ((xx - w // 2) ** 2 + (yy - h // 2) ** 2)
    psf = np.exp(-r2 / (2 * s * s)) + \
        0.05 * np.cos(2 * np.pi * np.sqrt(r2) / 9.0) * np.exp(-np.sqrt(r2) / 20.0)
    psf = (psf / psf[h // 2, w // 2]).astype(np.float32)
    sky = np.zeros((h, w))
    xs = rng.integers(margin, w - margin, n_src)
    ys = rng.integers(margin, h - margin, n_src)
    fl = np.exp(rng.uniform(np.log(0.01), np.log(1.0), n_src))
    for x, y, f in zip(xs, ys, fl):
        sky[y, x] += f
    shifted = np.roll(psf.astype(np.float64), (-(h // 2), -(w // 2)), axis=(0, 1))
    dirty = np.real(np.fft.ifft2(np.fft.fft2(sky) * np.fft.fft2(shifted)))
    dirty += 1e-3 * rng.standard_normal((h, w))
    return psf, dirty.astype(np.float32)


def joined(dirty, psf, n_img, n_pol=1):
    """n_img residual planes (channel-major: image = channel * n_pol + pol)
    that differ in scale and by a shifted copy, and n_img // n_pol PSFs that
    differ by a row shift and a scale."""
    dirties = np.stack([dirty * np.float32(1.0 + 0.15 * k) + np.float32(1e-3 * k) *
                        np.roll(dirty, 3 * k, axis=1) for k in range(n_img)]).astype(np.float32)
    psfs = np.stack([np.roll(psf, k, axis=0) * np.float32(1.0 - 0.02 * k)
                     for k in range(n_img // n_pol)]).astype(np.float32)
    return dirties, psfs


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: a * b is exact in float64; the sum is
    rounded to float64 and then to float32, and the one case where the two
    roundings differ from a single one (the float64 sum lands on a float32
    tie that the discarded part breaks) is nudged off the tie first."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    t = p + c
    bb = t - p
    err = (p - (t - bb)) + (c - bb)  # TwoSum: p + c == t + err exactly
    tie = (np.atleast_1d(t).view(np.uint64) & np.uint64(0x1fffffff)) == np.uint64(0x10000000)
    tie = tie.reshape(np.shape(t))
    toward = np.where(err > 0, np.inf, -np.inf)
    t = np.where(tie & (err != 0), np.nextafter(t, toward), t)
    return t.astype(np.float32)


def linear_integrate(values, weights):
    """ImageSet::GetLinearIntegrated of n_pol = 1 images with non-zero weights
    (cpp/image_set.cc:423-462): values [n_img, n]."""
    w = np.asarray(weights, np.float32)
    if len(w) == 1:
        return values[0].copy()
    acc = values[0] * w[0]
    for k in range(1, len(w)):
        acc = fma32(values[k], w[k], acc)
    return acc * np.float32(1.0 / float(np.sum(w.astype(np.float64))))


def numpy_subminor_map_loop(residual, psfs, weights, smap, threshold, gain, max_iterations):
    """SubMinorLoop::Run in float32 numpy for n_pol = 1, allow_negative, no
    mask / borders / RMS / divergence, with the n_img x n_img map `smap` as
    the spectral fit. Returns (positions [n, 2] x y, trace [k, 2], model
    [n_img, n], peak, flux)."""
    n_img, h, w = residual.shape
    f32 = np.float32
    integ = linear_integrate(residual.reshape(n_img, -1), weights).reshape(h, w)
    ys, xs = np.nonzero(np.abs(integ) >= f32(threshold))
    r = residual[:, ys, xs].astype(f32)
    model = np.zeros_like(r)
    trace = []
    flux = f32(0)
    scratch = linear_integrate(r, weights)
    c = int(np.argmax(np.abs(scratch)))
    while abs(scratch[c]) > f32(threshold) and len(trace) < max_iterations:
        vals = r[:, c] * f32(gain)
        flux = f32(flux + scratch[c] * f32(gain))
        trace.append((xs[c], ys[c]))
        comp = np.zeros(n_img, f32)
        for k in range(n_img):
            acc = f32(0)
            for q in range(n_img):
                acc = fma32(smap[k, q], vals[q], acc)
            comp[k] = acc
        model[:, c] += comp
        px = xs - xs[c] + w // 2
        py = ys - ys[c] + h // 2
        inside = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        for k in range(n_img):
            pv = psfs[k][py[inside], px[inside]]
            r[k, inside] = fma32(-pv, comp[k], r[k, inside])
        scratch = linear_integrate(r, weights)
        c = int(np.argmax(np.abs(scratch)))
    return (np.stack([xs, ys], axis=1), np.array(trace, np.int64).reshape(-1, 2), model,
            scratch[c], flux)
