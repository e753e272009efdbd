"""Rendering and restoring, the part that needs no device: the new entry
points are exported, refuse bad arguments before any device call, and
ComponentList.render reports a bad request before it asks for a session. The
numpy references of the GPU tests (tests/render_refs.py) are checked by hand."""
import ctypes as C

import numpy as np
import pytest

import render_refs as R
from radler_import import radler as rd
from rdl_lib import HIP_SO, declared_symbols

POLYNOMIAL, LOGPOLY, FORCED, VALUES = 0, 1, 2, 3
ERR_ARG = 1
MODE = rd.SpectralFittingMode


def test_new_entry_points_are_declared_and_exported():
    lib = C.CDLL(HIP_SO)
    for name in ("rdl_render_components", "rdl_spectrum_multiply_add"):
        assert name in declared_symbols()
        assert hasattr(lib, name)


def render_status(session=True, mode=VALUES, n_in=2, n=3, x=(0, 1, 2), y=(0, 0, 0), width=4,
                  height=3, n_out=2, h_out=None, planes=True):
    """rdl_render_components' status for arguments it must refuse. The
    session and the device pointers are dummies: a refused call reads none."""
    lib = C.CDLL(HIP_SO)
    lib.rdl_last_error.restype = C.c_char_p
    dummy = C.create_string_buffer(4096)
    xs, ys = (C.c_uint32 * len(x))(*x), (C.c_uint32 * len(y))(*y)
    out = None if h_out is None else (C.c_double * len(h_out))(*h_out)
    rc = lib.rdl_render_components(
        C.cast(dummy, C.c_void_p) if session else None, C.c_uint32(mode), C.c_uint32(n_in),
        C.cast(dummy, C.c_void_p), C.c_size_t(n), C.c_size_t(n), xs, ys, C.c_uint32(width),
        C.c_uint32(height), out, C.c_uint32(n_out),
        C.cast(dummy, C.c_void_p) if planes else None, C.c_size_t(width * height))
    return rc, lib.rdl_last_error().decode()


def test_render_components_refuses_bad_arguments_without_a_device():
    assert render_status(session=False)[0] == ERR_ARG
    assert render_status(planes=False)[0] == ERR_ARG
    rc, why = render_status(n_in=65, n_out=65)
    assert rc == ERR_ARG and "out of range" in why
    rc, why = render_status(mode=POLYNOMIAL, n_out=65, h_out=[0.0] * 65)
    assert rc == ERR_ARG and "output count" in why
    rc, why = render_status(x=(0, 4, 2))  # x == width
    assert rc == ERR_ARG and "outside the image" in why
    rc, why = render_status(y=(0, 3, 0))  # y == height
    assert rc == ERR_ARG and "outside the image" in why
    rc, why = render_status(x=(1, 2, 1))  # two equal positions
    assert rc == ERR_ARG and "share a position" in why
    rc, why = render_status(mode=VALUES, n_in=2, n_out=3)
    assert rc == ERR_ARG and "one plane per row" in why
    rc, why = render_status(mode=POLYNOMIAL, h_out=None)  # terms need the outputs
    assert rc == ERR_ARG
    rc, why = render_status(mode=LOGPOLY, n_in=9, h_out=[0.0, 0.1])
    assert rc == ERR_ARG and "term count" in why
    assert render_status(mode=4)[0] == ERR_ARG


def test_spectrum_multiply_add_refuses_null_arguments():
    lib = C.CDLL(HIP_SO)
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    call = lib.rdl_spectrum_multiply_add
    assert call(None, dummy, dummy, dummy, C.c_size_t(1), C.c_float(1.0)) == ERR_ARG
    assert call(dummy, None, dummy, dummy, C.c_size_t(1), C.c_float(1.0)) == ERR_ARG
    assert call(dummy, dummy, dummy, None, C.c_size_t(1), C.c_float(1.0)) == ERR_ARG


def small_list(n_frequencies=2):
    cl = rd.ComponentList(16, 12, 2, n_frequencies)
    cl.add(3, 4, 0, [1.0] * n_frequencies)
    cl.add(5, 6, 1, [2.0] * n_frequencies)
    return cl


def fitter(n=2):
    return rd.SpectralFitter(MODE.polynomial, 2, [1.0e8 + 1.0e7 * c for c in range(n)],
                             [1.0] * n)


def test_render_reports_a_bad_request_before_it_needs_a_session():
    cl = small_list()
    with pytest.raises(RuntimeError, match="unmerged"):
        cl.render(fitter(), [0.0, 4.0])
    cl.merge_duplicates()
    with pytest.raises(RuntimeError, match="1 scale sizes given for 2 scales"):
        cl.render(fitter(), [0.0])
    with pytest.raises(RuntimeError, match="3 scale sizes given for 2 scales"):
        cl.render(fitter(), [0.0, 4.0, 9.0])
    for bad in (0.0, -1.0e8, float("nan")):
        with pytest.raises(RuntimeError, match="not positive"):
            cl.render(fitter(), [0.0, 4.0], [1.0e8, bad])
    with pytest.raises(RuntimeError, match="2 frequencies, the spectral fitter has 3"):
        cl.render(fitter(3), [0.0, 4.0], [1.0e8])
    with pytest.raises(RuntimeError, match="2 frequencies, the spectral fitter has 3"):
        cl.render(fitter(3), [0.0, 4.0])
    none = rd.SpectralFitter(MODE.no_fitting, 0, [], [])
    with pytest.raises(RuntimeError, match="spectral fitting"):
        cl.render(none, [0.0, 4.0], [1.0e8])


def test_restore_reports_mismatched_shapes_without_a_device():
    image = np.zeros((4, 5), np.float32)
    with pytest.raises(RuntimeError, match="differ in shape"):
        rd.restore(image, np.zeros((5, 4), np.float32), 0.0, 0.0, 0.0, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="differ in shape"):
        rd.restore(image, np.zeros((1, 4, 5), np.float32), 0.0, 0.0, 0.0, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="2-D images or 3-D stacks"):
        rd.restore(np.zeros(5, np.float32), np.zeros(5, np.float32), 0.0, 0.0, 0.0, 1.0, 1.0)


# ------------------------------------------------- the references, by hand
def test_circular_convolution_reference_by_hand():
    plane = np.zeros((4, 5))
    plane[0, 0], plane[2, 3] = 2.0, -1.0
    kernel = np.arange(1.0, 10.0).reshape(3, 3)  # centre (1, 1) holds 5
    got = R.circular_convolve(plane, kernel)
    want = np.zeros((4, 5))
    for (y, x), v in (((0, 0), 2.0), ((2, 3), -1.0)):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                want[(y + dy) % 4, (x + dx) % 5] += v * kernel[dy + 1, dx + 1]
    np.testing.assert_allclose(got, want, atol=1e-13)
    # the corner source wraps: its upper-left neighbour is the far corner,
    # which is also the lower-right neighbour of the source at (2, 3)
    assert abs(got[3, 4] - (2.0 * kernel[0, 0] - kernel[2, 2])) < 1e-13


def test_render_reference_by_hand():
    kernel = np.full((3, 3), 0.1)
    kernel[1, 1] = 0.2
    lists = [(np.array([[1, 1]]), np.array([[3.0, -6.0]])),
             (np.array([[0, 2], [2, 0]]), np.array([[1.0, 2.0], [-1.0, 0.0]]))]
    planes, peak = R.render(3, 3, [None, kernel], lists)
    # a 3 x 3 kernel on a 3 x 3 plane covers every pixel once
    want0 = np.full((3, 3), 0.1 * 1.0 - 0.1 * 1.0)
    want0[2, 0] += 0.1
    want0[0, 2] -= 0.1
    want0[1, 1] += 3.0
    np.testing.assert_allclose(planes[0], want0, atol=1e-13)
    want1 = np.full((3, 3), 0.2)
    want1[2, 0] += 0.2
    want1[1, 1] -= 6.0
    np.testing.assert_allclose(planes[1], want1, atol=1e-13)
    # the largest scale-convolved plane of absolute values: |-6| at scale 0
    assert peak == 6.0
    assert R.delta_planes(3, 3, [(0, 2)], [[1.0, 2.0]])[1, 2, 0] == 2.0


def test_linear_convolution_reference_by_hand():
    model = np.zeros((4, 5), np.float32)
    model[0, 0], model[3, 4] = 1.0, 2.0
    kernel = np.arange(1.0, 17.0, dtype=np.float32).reshape(4, 4)  # centre (2, 2) holds 11
    got = R.linear_convolve(model, kernel)
    want = np.zeros((4, 5))
    for (y, x), v in (((0, 0), 1.0), ((3, 4), 2.0)):
        for dy in range(-2, 2):
            for dx in range(-2, 2):
                if 0 <= y + dy < 4 and 0 <= x + dx < 5:
                    want[y + dy, x + dx] += v * kernel[dy + 2, dx + 2]
    np.testing.assert_array_equal(got, want)
    assert got[0, 0] == 11.0 and got[1, 1] == 16.0 and got[1, 2] == 2.0 * 1.0
    assert got[0, 4] == 0.0  # nothing wraps: (3, 4) reaches rows 1..3 only


def test_beam_kernel_reference_by_hand():
    # FWHM 3 x 2 pixels at pa 0: the major axis lies along m (y), peak 1
    fwhm_to_sigma = 1.0 / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    kernel, box = R.beam_kernel(64, 48, 3.0, 2.0, 0.0, 1.0, 1.0)
    # angle pi/2: sigma_max = sigma_major, box = ceil(40 * 1.27398) = 51 -> 52, clipped to 48
    assert box == 48 and kernel.shape == (48, 48)
    c = box // 2
    assert kernel[c, c] == 1.0
    assert abs(kernel[c + 1, c] - np.exp(-0.5 / (3.0 * fwhm_to_sigma) ** 2)) < 1e-7
    assert abs(kernel[c, c + 1] - np.exp(-0.5 / (2.0 * fwhm_to_sigma) ** 2)) < 1e-7
    # half the peak at half the FWHM along each axis
    small, box = R.beam_kernel(64, 48, 4.0, 2.0, 0.0, 1.0, 1.0)
    assert abs(small[box // 2 + 2, box // 2] - 0.5) < 1e-7
    assert abs(small[box // 2, box // 2 - 1] - 0.5) < 1e-7
    # a pixel 1.5 times as tall: the same beam spans fewer pixels in y
    tall, box = R.beam_kernel(64, 48, 3.0, 2.0, 0.0, 1.0, 1.5)
    assert abs(tall[box // 2 + 1, box // 2] - 0.5) < 1e-7


def test_restore_bound_by_hand():
    residual = np.array([[1.0, -2.0]], np.float32)
    conv = np.array([[3.0, 2.0]])
    model = np.array([[4.0, -4.0]], np.float32)
    bound = R.restore_bound(residual, conv, model)
    np.testing.assert_allclose(bound, 2.0 ** -24 * np.array([[7.0, 2.0]]) + 8e-12, rtol=1e-12)
