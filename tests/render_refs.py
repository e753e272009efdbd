"""numpy float64 references for rendering a component list into model images
(ComponentList.render) and restoring them (radler.restore), with the bounds
their tests use. Hand checks: tests/test_render_api.py.

A list is given per scale as (positions (n, 2) int [x, y], values (n, n_planes)).
"""
import math

import numpy as np

from primitive_refs import place_gaussian

# the float32-transform error of one scale convolution, relative to the
# convolved image's peak: the project's measured bound (tests/test_configs_gpu.py)
RTOL = 1e-6


def shape_kernels(oracle, scale_sizes, width, height, shape=0):
    """The oracle's n x n shape kernel of every non-zero scale (None for 0)."""
    return [None if s == 0.0 else
            oracle.shape_function(float(s), min(width, height), shape).astype(np.float64)
            for s in scale_sizes]


def delta_planes(width, height, positions, values):
    """(n_planes, height, width) float64 with values[i] at positions[i]."""
    values = np.asarray(values, np.float64).reshape(len(positions), -1)
    out = np.zeros((values.shape[1], height, width), np.float64)
    for (x, y), v in zip(positions, values):
        out[:, y, x] += v
    return out


def circular_convolve(plane, kernel):
    """plane (h, w) convolved circularly with the odd n x n kernel centred at
    (n/2, n/2): MultiScaleTransforms::Transform in float64."""
    h, w = plane.shape
    n = kernel.shape[0]
    placed = np.zeros((h, w), np.float64)
    for ky in range(n):
        for kx in range(n):
            placed[(ky - n // 2) % h, (kx - n // 2) % w] += kernel[ky, kx]
    return np.fft.irfft2(np.fft.rfft2(plane) * np.fft.rfft2(placed), s=(h, w))


def render(width, height, kernels, lists):
    """-> (planes (n_planes, h, w), peak): the sum over the scales of the delta
    planes convolved with the scale's kernel (added as they are where the
    kernel is None), and peak = max_s max |K_s (*) |D_s||, which bounds every
    scale-convolved plane of the computation."""
    total, peak = None, 0.0
    for kernel, (positions, values) in zip(kernels, lists):
        if len(positions) == 0:
            continue
        deltas = delta_planes(width, height, positions, values)
        if kernel is None:
            conv, conv_abs = deltas, np.abs(deltas)
        else:
            conv = np.stack([circular_convolve(d, kernel) for d in deltas])
            conv_abs = np.stack([circular_convolve(np.abs(d), np.abs(kernel)) for d in deltas])
        total = conv if total is None else total + conv
        peak = max(peak, float(np.max(conv_abs)))
    return total, peak


def lists_of(component_list):
    """The per-scale (positions, values) of a radler.ComponentList."""
    out = []
    for s in range(component_list.n_scales):
        comps = [component_list.get_component(s, i)
                 for i in range(component_list.component_count(s))]
        out.append((np.asarray([(x, y) for x, y, _ in comps], np.int64).reshape(-1, 2),
                    np.asarray([v for _, _, v in comps], np.float64).reshape(
                        len(comps), component_list.n_frequencies)))
    return out


# ---------------------------------------------------------------- restore
def beam_kernel(width, height, beam_major, beam_minor, beam_pa, pixel_scale_l, pixel_scale_m):
    """RestoreImage's kernel (csrc/host/restore.h) -> (box x box float32 as the
    device stores it, box): sigma = FWHM / (2 sqrt(2 ln 2)), angle = pa + pi/2,
    box = ceil(40 sigma_max / min pixel scale) made even, at most the smaller
    image side."""
    to_sigma = 1.0 / (2.0 * math.sqrt(2.0 * math.log(2.0)))
    sigma_major, sigma_minor = beam_major * to_sigma, beam_minor * to_sigma
    angle = beam_pa + 0.5 * math.pi
    sigma_max = max(abs(sigma_major * math.cos(angle)), abs(sigma_major * math.sin(angle)))
    min_dim = min(width, height)
    box = min(int(math.ceil(sigma_max * 40.0 / min(pixel_scale_l, pixel_scale_m))), min_dim)
    if box % 2:
        box += 1
    box = min(box, min_dim)
    side = 2 * box
    placed, _ = place_gaussian(side, side, box, pixel_scale_l, pixel_scale_m, sigma_major,
                               sigma_minor, angle)
    idx = (np.arange(box) - box // 2) % side
    return placed[np.ix_(idx, idx)].astype(np.float32), box


def linear_convolve(model, kernel):
    """Exact 'same' linear convolution of the float model with the box kernel
    whose centre is (box/2, box/2): out[y, x] = sum model[y - dy, x - dx] *
    kernel[dy + c, dx + c], nothing wrapping. float64 products of floats, summed
    over the model's non-zero pixels."""
    h, w = model.shape
    box = kernel.shape[0]
    c = box // 2
    k = kernel.astype(np.float64)
    out = np.zeros((h, w), np.float64)
    for y, x in zip(*np.nonzero(model)):
        y0, y1 = max(0, y - c), min(h, y - c + box)
        x0, x1 = max(0, x - c), min(w, x - c + box)
        out[y0:y1, x0:x1] += float(model[y, x]) * k[y0 - y + c:y1 - y + c, x0 - x + c:x1 - x + c]
    return out


def restore_bound(residual, conv, model):
    """|got - (residual + conv)| per pixel: two float roundings (the
    convolution, then the sum) and a loose cover of the float64 transform."""
    r = residual.astype(np.float64)
    return 2.0 ** -24 * (np.abs(r + conv) + np.abs(conv)) + \
        1e-12 * float(np.sum(np.abs(model.astype(np.float64))))
