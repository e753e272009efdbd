"""rdl_draw_sources on the MI355X, through ctypes: a catalogue of points and
sub-pixel Gaussians against the contract's sum in numpy float64.

Per pixel, with s the float64 sum in source order and d the destination:
  |got - (d + s)| <= 2^-24 (|s| + |d + s|) + 1e-13 sum_i |a_i g_i|
the two float roundings the contract allows (the sum, then the addition), and
the device's double exp against numpy's. The plane is 70 x 50: no multiple of
the 64 x 16 tile in either direction, 2 x 4 tiles."""
import ctypes as C
import math

import numpy as np
import pytest

import sources_lib as L

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 70, 50
TILE_W, TILE_H = 64, 16


@pytest.fixture(scope="module")
def sess():
    s = L.Session()
    yield s
    s.close()


def gaussian(x0, y0, fwhm_major, fwhm_minor, angle):
    cov = L.pixel_covariance(fwhm_major, fwhm_minor, angle, 1.0, 1.0)
    return L.shape_of(cov, x0, y0, W, H)


def point(x0, y0):
    return (x0, y0, 0.0, 0.0, 0.0, 0, 0)


def make_catalogue():
    rng = np.random.default_rng(17)
    shapes = [point(0, 0), point(W - 1, H - 1), point(TILE_W - 1, TILE_H - 1),
              point(TILE_W, TILE_H), point(TILE_W - 0.5, 2 * TILE_H - 0.5),  # rounds up
              point(TILE_W + 0.49, 3 * TILE_H - 0.51), point(W, 10), point(-1, 3),
              point(12, H + 0.2), point(5.3, 7.8), point(5.3, 7.8)]  # two on one pixel
    for _ in range(12):  # sub-pixel Gaussians, FWHM 1.5 to 9 px, any angle
        major = rng.uniform(1.5, 9.0)
        shapes.append(gaussian(rng.uniform(0, W), rng.uniform(0, H), major,
                               rng.uniform(1.5, major), rng.uniform(-math.pi, math.pi)))
    shapes.append(gaussian(-4.0, 20.3, 6.0, 3.0, 0.4))     # centred outside, the box reaches in
    shapes.append(gaussian(30.2, H + 3.6, 5.0, 5.0, 0.0))
    shapes.append(gaussian(33.7, 24.1, 90.0, 60.0, 1.1))   # wider than the plane
    # 300 sources inside one tile: more than one LDS chunk of 256
    for k in range(300):
        x0, y0 = rng.uniform(1, TILE_W - 2), rng.uniform(TILE_H + 1, 2 * TILE_H - 2)
        shapes.append(point(x0, y0) if k % 3 == 0 else (x0, y0, 0.9, 0.2 * (k % 2), 1.3, 3, 2))
    return shapes


def amplitudes_of(n_planes, n, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.05, 2.0, (n_planes, n)) * rng.choice([-1.0, 1.0], (n_planes, n))).astype(F)


SHAPES = make_catalogue()
REFERENCE = {}


def reference(n_planes):
    """The contract's sum for the first n_planes amplitude rows, computed once."""
    if n_planes not in REFERENCE:
        amplitudes = amplitudes_of(5, len(SHAPES))[:n_planes]
        REFERENCE[n_planes] = (amplitudes, *L.contract_sum(SHAPES, amplitudes, W, H))
    return REFERENCE[n_planes]


def test_catalogue_covers_the_cases():
    assert len(SHAPES) > 300
    wide = [s for s in SHAPES if s[5] >= max(W, H)]
    assert wide and all(s[5] == max(W, H) for s in wide)
    assert any(s[0] < 0 and s[5] > 4 for s in SHAPES)
    _, total, _ = reference(1)
    assert total[0, 0, 0] != 0 and total[0, H - 1, W - 1] != 0


@pytest.mark.parametrize("n_planes", [1, 3, 5])
@pytest.mark.parametrize("zeroed", [True, False])
def test_against_the_contract_sum(sess, n_planes, zeroed):
    amplitudes, total, absolute = reference(n_planes)
    rng = np.random.default_rng(n_planes)
    dest = np.zeros((n_planes, H, W), F) if zeroed else \
        rng.standard_normal((n_planes, H, W)).astype(F)
    d = sess.array(dest)
    L.draw_sources(sess, SHAPES, amplitudes, d, n_planes, W, H)
    got = d.get()
    d.free()
    want = dest.astype(np.float64) + total
    bound = L.contract_bound(dest, total, absolute)
    err = np.abs(got.astype(np.float64) - want)
    touched = absolute > 0
    worst = float(np.max(err[touched] / bound[touched]))
    print(f"draw sources, {n_planes} planes, zeroed={zeroed}: max |got - want| = "
          f"{np.max(err):.3g}, max error / bound = {worst:.3g}, max |want| = "
          f"{np.max(np.abs(want)):.3g}")
    assert np.all(err <= bound)
    # a pixel inside no box keeps its bits
    assert np.array_equal(got[~touched].view(np.uint32), dest[~touched].view(np.uint32))
    assert np.count_nonzero(touched) > 0.9 * touched.size  # the wide source


def test_points_land_on_their_pixels(sess):
    shapes = [point(0, 0), point(W - 1, H - 1), point(TILE_W - 0.5, TILE_H - 0.5),
              point(W - 0.5, 4), point(3, -0.51), point(3.49, -0.5), point(1e300, 2),
              point(-1e300, 2)]
    amplitudes = np.arange(1, len(shapes) + 1, dtype=F)[None]
    d = sess.array(np.zeros((H, W), F))
    L.draw_sources(sess, shapes, amplitudes, d, 1, W, H)
    got = d.get()
    d.free()
    want = np.zeros((H, W), F)
    want[0, 0], want[H - 1, W - 1], want[TILE_H, TILE_W], want[0, 3] = 1.0, 2.0, 3.0, 6.0
    assert np.array_equal(got, want)


def test_two_runs_and_a_larger_stride_give_the_same_bits(sess):
    n_planes = 3
    amplitudes, _, _ = reference(n_planes)
    rng = np.random.default_rng(8)
    dest = rng.standard_normal((n_planes, H, W)).astype(F)
    runs = []
    for _ in range(2):
        d = sess.array(dest)
        L.draw_sources(sess, SHAPES, amplitudes, d, n_planes, W, H)
        runs.append(d.get())
        d.free()
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
    # the planes embedded at a stride that breaks the rows' 16-byte alignment
    stride = W * H + 37
    padded = np.full(n_planes * stride, 7.0, F)
    for g in range(n_planes):
        padded[g * stride:g * stride + W * H] = dest[g].ravel()
    d = sess.array(padded)
    L.draw_sources(sess, SHAPES, amplitudes, d, n_planes, W, H, stride=stride)
    got = d.get()
    d.free()
    for g in range(n_planes):
        plane = got[g * stride:g * stride + W * H].reshape(H, W)
        assert np.array_equal(plane.view(np.uint32), runs[0][g].view(np.uint32))
        assert np.all(got[g * stride + W * H:(g + 1) * stride] == 7.0)


def test_an_empty_list_leaves_the_planes_untouched(sess):
    rng = np.random.default_rng(2)
    dest = rng.standard_normal((2, H, W)).astype(F)
    dest[0, 0, 0] = -0.0
    d = sess.array(dest)
    L.draw_sources(sess, [], None, d, 2, W, H)
    L.draw_sources(sess, None, None, d, 2, W, H, n_sources=0)
    assert np.array_equal(d.get().view(np.uint32), dest.view(np.uint32))
    # every box misses the plane: nothing is launched
    L.draw_sources(sess, [point(-3, -3), gaussian(-40.0, -40.0, 3.0, 2.0, 0.3)],
                   np.ones((2, 2), F), d, 2, W, H)
    assert np.array_equal(d.get().view(np.uint32), dest.view(np.uint32))
    d.free()


def test_argument_errors(sess):
    d = sess.array(np.zeros((2, H, W), F))
    good, amp = [point(1, 1), gaussian(20.5, 20.5, 3.0, 2.0, 0.3)], np.ones((2, 2), F)
    lib = sess.rdl.lib
    lib.rdl_last_error.restype = C.c_char_p

    def refused(call, word):
        with pytest.raises(L.RdlError) as e:
            call()
        assert "rc=1" in str(e.value) and word in str(e.value), str(e.value)

    refused(lambda: L.draw_sources(sess, good, amp, None, 2, W, H), "NULL")
    refused(lambda: L.draw_sources(sess, None, amp, d, 2, W, H, n_sources=2), "NULL")
    refused(lambda: L.draw_sources(sess, good, None, d, 2, W, H), "NULL")
    refused(lambda: sess.rdl.rdl_draw_sources(None, 0, None, None, 1, W, H, d.vp,
                                              C.c_size_t(W * H)), "NULL")
    refused(lambda: L.draw_sources(sess, good, amp, d, 0, W, H), "plane count")
    refused(lambda: L.draw_sources(sess, good, np.ones((65, 2), F), d, 65, W, H), "plane count")
    refused(lambda: L.draw_sources(sess, good, amp, d, 2, 0, H), "plane size")
    refused(lambda: L.draw_sources(sess, good, amp, d, 2, W, 0), "plane size")
    refused(lambda: L.draw_sources(sess, good, amp, d, 2, W, H, stride=W * H - 1), "overlap")
    for field in range(5):
        for bad in (math.nan, math.inf, -math.inf):
            shape = list(good[1])
            shape[field] = bad
            refused(lambda: L.draw_sources(sess, [good[0], tuple(shape)], amp, d, 2, W, H),
                    "non-finite")
    assert not np.any(d.get())  # nothing was drawn
    d.free()
