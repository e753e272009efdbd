"""rdl_average_planes against the chain it replaces, bit for bit.

The oracle is the chain ImageSet::LoadAndAverage / LoadAndAveragePsfs run
before (and still run for host accessors), on the same device buffers:
rdl_memset_zero, one rdl_axpy (mode 0) or rdl_axpy_f64 (mode 1) per source in
the order given, then rdl_scale / rdl_axpy_f64(mode 1). Results are compared
as uint32 words: signs of zero, NaNs and infinities included.

Launch constants of the kernel (csrc/hip/elementwise.hip): 256 threads, at
most 1024 blocks, 16 sources per launch. One grid pass therefore covers
1024 * 256 = 262144 float4 items on the 16-byte path and 262144 floats on the
scalar path. n = 1031 * 1021 = 1052651 is odd (a scalar tail of 3 after the
float4 body) and is 263162 float4 items, 1018 past one pass, so the grid
stride runs on both paths; 4099 is past one block with a tail of 3; 17 sources
cross one argument chunk, with the running value carried in the destination.
"""
import ctypes as C

import numpy as np
import pytest

from rdl_lib import Session
from test_primitives_gpu import F, SZ, Guarded, err_arg, free, same_bits

pytestmark = pytest.mark.gpu

BIG = 1031 * 1021
SIZES = [1, 3, 255, 1024, 4099, BIG]
SPECIALS = np.array([-0.0, 0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, -5e-40,
                     np.finfo(F).max, -np.finfo(F).max, np.nan], F)


@pytest.fixture(scope="module")
def sess():
    s = Session(0)
    yield s
    s.close()


def planes(n_sources, n, seed, extra=0):
    """n_sources planes of n + extra floats: normal values with every special
    sprinkled over each plane (first and last elements included)."""
    rng = np.random.default_rng(seed)
    out = rng.standard_normal((n_sources, n + extra)).astype(F)
    for k in range(n_sources):
        at = np.unique(np.concatenate([[0, n + extra - 1],
                                       rng.integers(0, n + extra, 3 * SPECIALS.size)]))
        out[k, at] = SPECIALS[rng.integers(0, SPECIALS.size, at.size)]
    return out


def weights_for(n_sources, seed):
    w = np.random.default_rng(seed + 1).uniform(0.1, 3.0, n_sources)
    if n_sources > 1:
        w[1] = -w[1]                                    # a negative weight
    return w


def chain(sess, dest, sources, weights, factor, mode, n):
    rdl = sess.rdl
    rdl.rdl_memset_zero(sess.h, dest, SZ(4 * n))
    for src, w in zip(sources, weights):
        if mode == 0:
            rdl.rdl_axpy(sess.h, dest, src, SZ(n), C.c_float(F(w)), 0)
        else:
            rdl.rdl_axpy_f64(sess.h, dest, src, SZ(n), C.c_double(w), 0)
    if mode == 0:
        rdl.rdl_scale(sess.h, dest, SZ(n), C.c_float(F(factor)))
    else:
        rdl.rdl_axpy_f64(sess.h, dest, None, SZ(n), C.c_double(factor), 1)


def fused(sess, dest, sources, weights, factor, mode, n):
    g = len(sources)
    pointers = (C.c_void_p * g)(*[s.value for s in sources]) if g else None
    w = (C.c_double * g)(*[float(x) for x in weights]) if g else None
    sess.rdl.rdl_average_planes(sess.h, pointers, w, C.c_uint32(g), C.c_double(factor),
                                C.c_int(mode), dest, SZ(n))


def check(sess, data, weights, factor, mode, n, dest_off=0, src_off=None):
    """Both ways into guarded destinations (sentinel-filled: a start from
    anything but +0 would show), compared word for word. dest_off / src_off
    (index, elements) move a pointer off 16-byte alignment."""
    srcs = [Guarded(sess, row) for row in data]
    pointers = [s.at(src_off[1] if src_off and src_off[0] == k else 0)
                for k, s in enumerate(srcs)]
    want, got = Guarded(sess, n=n + dest_off), Guarded(sess, n=n + dest_off)
    if dest_off == 0 and src_off is None:
        assert all(p.value % 16 == 0 for p in pointers + [want.vp, got.vp])
    else:
        assert any(p.value % 16 == 4 for p in pointers + [got.at(dest_off)])
    chain(sess, want.at(dest_off), pointers, weights, factor, mode, n)
    fused(sess, got.at(dest_off), pointers, weights, factor, mode, n)
    w, g = want.get(), got.get()                        # guards checked
    same_bits(g, w)
    free(want, got, *srcs)
    return g[dest_off:]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("n_sources", [0, 1, 5, 17])
@pytest.mark.parametrize("mode", [0, 1])
def test_matches_the_chain(sess, mode, n_sources, n):
    data = planes(n_sources, n, seed=n + n_sources)
    w = weights_for(n_sources, n)
    factor = 1.0 / w.sum() if n_sources else 0.5
    check(sess, data, w, factor, mode, n)


@pytest.mark.parametrize("n", [4099, BIG])
@pytest.mark.parametrize("which", ["dest", "first", "last"])
@pytest.mark.parametrize("mode", [0, 1])
def test_a_pointer_four_bytes_off(sess, mode, which, n):
    """Tensor slices are 4-byte aligned only: the destination or one source one
    float off takes the scalar path."""
    data = planes(5, n, seed=n, extra=1)
    w = weights_for(5, n)
    if which == "dest":
        check(sess, data, w, 1.0 / w.sum(), mode, n, dest_off=1)
    else:
        check(sess, data, w, 1.0 / w.sum(), mode, n, src_off=(0 if which == "first" else 4, 1))


def test_chunk_with_one_misaligned_source_after_an_aligned_chunk(sess):
    """17 sources, the 17th one float off: the first launch takes the float4
    path, the second the scalar one, over the same destination."""
    n = 4099
    data = planes(17, n, seed=5, extra=1)
    w = weights_for(17, 5)
    for mode in (0, 1):
        check(sess, data, w, 1.0 / w.sum(), mode, n, src_off=(16, 1))


def test_zero_weight_on_a_plane_of_nans_mode_1(sess):
    """The kernel skips nothing (LoadAndAveragePsfs skips nothing): 0 * NaN
    reaches every element, as in the chain."""
    n = 1024
    data = planes(3, n, seed=3)
    data[1] = np.nan
    out = check(sess, data, np.array([1.5, 0.0, 2.0]), 1.0 / 3.5, 1, n)
    assert np.isnan(out).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_signed_zero_denormals_and_infinities(sess, mode):
    n = 4 * SPECIALS.size + 3
    data = np.stack([np.resize(SPECIALS, n), np.resize(SPECIALS[::-1], n),
                     np.full(n, -0.0, F)])
    check(sess, data, np.array([2.0, -0.5, 1.0]), -0.4, mode, n)
    # planes of -0.0 only: +0 from the start value, -0 after a negative factor
    out = check(sess, np.full((2, n), -0.0, F), np.array([1.0, 3.0]), -0.25, mode, n)
    assert np.signbit(out).all() and (out == 0).all()


@pytest.mark.parametrize("factor", [0.0, np.inf])
@pytest.mark.parametrize("n_sources", [0, 2])
@pytest.mark.parametrize("mode", [0, 1])
def test_factor_zero_and_infinity(sess, mode, n_sources, factor):
    """The host's factor for a weight sum of 0: inf for images (1 / 0), 0 for
    PSFs."""
    n = 259
    check(sess, planes(n_sources, n, seed=9), weights_for(n_sources, 9), factor, mode, n)


def test_argument_errors(sess):
    n = 16
    src, dest = Guarded(sess, np.ones(n, F)), Guarded(sess, n=n)
    one = (C.c_void_p * 1)(src.vp.value)
    null = (C.c_void_p * 2)(src.vp.value, None)
    w = (C.c_double * 2)(1.0, 1.0)
    call = sess.rdl.rdl_average_planes
    err_arg(call, sess.h, one, w, C.c_uint32(1), C.c_double(1.0), 0, None, SZ(n))
    err_arg(call, sess.h, null, w, C.c_uint32(2), C.c_double(1.0), 0, dest.vp, SZ(n))
    err_arg(call, sess.h, one, w, C.c_uint32(1), C.c_double(1.0), 2, dest.vp, SZ(n))
    err_arg(call, sess.h, one, w, C.c_uint32(1), C.c_double(1.0), -1, dest.vp, SZ(n))
    assert b"mode" in sess.rdl.lib.rdl_last_error()
    # nothing to do is no error, and nothing is written
    sess.rdl.rdl_average_planes(sess.h, one, w, C.c_uint32(1), C.c_double(1.0), 0, None, SZ(0))
    dest.get()
    free(src, dest)
