"""IUWT à-trous decomposition.

CPU: the oracle's decomposition/recomposition round trip reproduces the
input within float rounding; the aliased form (input used as scratch, as the
reference's IUWT deconvolution calls it) differs from the plain one and
overwrites the input.
GPU: rdl_iuwt_decompose / rdl_iuwt_recompose are bit-exact with the oracle
(tap order per boundary region and FMA contraction of the reference build),
aliased and not, with and without the approximation plane; from
test_oracle_equals_float64_zero_boundary_filter on, at the shapes of
tests/iuwt_cases.py where the dispatch of csrc/hip/iuwt.hip changes its kernel
family, under every RDL_IUWT_FUSED mode, between sentinel guards.
"""
import os
import ctypes as C

import numpy as np
import pytest

import iuwt_cases as K
from iuwt_cases import image
from oracle_lib import get_oracle, iuwt_decompose, iuwt_recompose

CASES = [(64, 64, 3), (100, 80, 3), (256, 256, 6), (300, 260, 5), (1024, 512, 6)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("w,h,n", CASES[:4])
def test_oracle_round_trip(w, h, n):
    orc = get_oracle()
    img = image(w, h, w)
    coeffs, after = iuwt_decompose(orc, img, n)
    assert np.array_equal(after, img)  # not aliased: input untouched
    back = iuwt_recompose(orc, coeffs, n)
    assert np.abs(back - img).max() <= 1e-5 * np.abs(img).max()
    # without the approximation the recomposition is the detail sum only
    no_approx = iuwt_recompose(orc, coeffs, n, include_largest=False)
    assert np.abs(no_approx - back).max() > 0
    aliased, clobbered = iuwt_decompose(orc, img, n, aliased=True)
    assert not np.array_equal(aliased[0], coeffs[0])
    assert not np.array_equal(clobbered, img)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,n", CASES)
@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("include_largest", [True, False])
def test_gpu_iuwt_bit_exact(w, h, n, aliased, include_largest):
    from rdl_lib import Session
    orc = get_oracle()
    img = image(w, h, w + n)
    coeffs_o, after_o = iuwt_decompose(orc, img, n, aliased, include_largest)
    s = Session(0)
    d_in = s.array(img)
    d_scratch = d_in if aliased else s.array(shape=(h, w))
    d_coeffs = s.array(shape=(n + 1, h, w))
    s.rdl.rdl_iuwt_decompose(s.h, d_in.vp, d_scratch.vp, w, h, n, d_coeffs.vp,
                             int(include_largest))
    got = d_coeffs.get()
    for k in range(n + 1):
        assert np.array_equal(bits(got[k]), bits(coeffs_o[k])), k
    if aliased:
        assert np.array_equal(bits(d_in.get()), bits(after_o))
    d_out = s.array(shape=(h, w))
    s.rdl.rdl_iuwt_recompose(s.h, d_coeffs.vp, w, h, n, int(include_largest), d_out.vp)
    expect = iuwt_recompose(orc, coeffs_o, n, include_largest)
    assert np.array_equal(bits(d_out.get()), bits(expect))
    for x in {id(a): a for a in (d_in, d_scratch, d_coeffs, d_out)}.values():
        x.free()
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,n", [(4096, 4096, 6), (1000, 37, 6), (8192, 64, 6),
                                   (260, 300, 7), (2048, 1500, 8)])
@pytest.mark.parametrize("include_largest", [True, False])
@pytest.mark.parametrize("mode", ["2", "3", "1"])
def test_gpu_iuwt_fused_equal_four_pass(w, h, n, include_largest, mode):
    """The fused kernels against the four-pass kernels (RDL_IUWT_FUSED=0),
    bit for bit: mode 2 (the default) the fused row decomposition
    (IuwtDecomposeRows, the intermediate row in LDS) and the row-chain
    recomposition (IuwtRecomposeChain: one launch per scale, five filtered
    rows per chain in LDS), mode 3 the row chains for the decomposition too
    (IuwtDecomposeChain), mode 1 the fused rows with the four-pass
    recomposition; at the C4 size, at
    heights and widths below the larger spacings (d = 63, 127, 255 against 37,
    64, 260 and 300 rows) and with partial column strips. At n = 8 with the
    approximation plane, PlanChain refuses the recomposition at d = 255 and
    every mode recomposes on the four-pass kernels, and mode 3 decomposes on
    the fused rows (d = 255 is refused there too): those comparisons run the
    same recomposition kernels on both sides, and mode 3's equals mode 2's."""
    from rdl_lib import Session
    img = image(w, h, 77)
    s = Session(0)
    outs = []
    for fused in (mode, "0"):
        os.environ["RDL_IUWT_FUSED"] = fused
        try:
            d_in, d_scratch = s.array(img), s.array(shape=(h, w))
            d_coeffs = s.array(shape=(n + 1, h, w))
            d_out = s.array(shape=(h, w))
            s.rdl.rdl_iuwt_decompose(s.h, d_in.vp, d_scratch.vp, w, h, n, d_coeffs.vp,
                                     int(include_largest))
            s.rdl.rdl_iuwt_recompose(s.h, d_coeffs.vp, w, h, n, int(include_largest),
                                     d_out.vp)
            outs.append((d_coeffs.get(), d_out.get(), d_in.get()))
            for x in (d_in, d_scratch, d_coeffs, d_out):
                x.free()
        finally:
            del os.environ["RDL_IUWT_FUSED"]
    s.close()
    for k in range(n + 1):
        assert np.array_equal(bits(outs[0][0][k]), bits(outs[1][0][k])), k
    assert np.array_equal(bits(outs[0][1]), bits(outs[1][1]))
    assert np.array_equal(bits(outs[0][2]), bits(img))  # the input is not written


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,n", [(4096, 512, 6), (1000, 37, 6), (260, 300, 7), (64, 64, 3)])
def test_gpu_iuwt_aliased_recurrences_equal_row_kernel(w, h, n):
    """The aliased decomposition (input as its own scratch, as the IUWT
    deconvolution calls it): its first horizontal pass is a recursive
    in-place filter. The recurrence kernel (IuwtHorizontalInPlaceChains, one
    thread per row and residue, taps in registers) against the
    one-thread-per-row kernel (RDL_IUWT_FUSED=0), bit for bit, including the
    overwritten input."""
    from rdl_lib import Session
    img = image(w, h, 91)
    s = Session(0)
    outs = []
    for fused in ("2", "0"):
        os.environ["RDL_IUWT_FUSED"] = fused
        try:
            d_in = s.array(img)
            d_coeffs = s.array(shape=(n + 1, h, w))
            s.rdl.rdl_iuwt_decompose(s.h, d_in.vp, d_in.vp, w, h, n, d_coeffs.vp, 0)
            outs.append((d_coeffs.get(), d_in.get()))
            for x in (d_in, d_coeffs):
                x.free()
        finally:
            del os.environ["RDL_IUWT_FUSED"]
    s.close()
    for k in range(n + 1):
        assert np.array_equal(bits(outs[0][0][k]), bits(outs[1][0][k])), k
    assert np.array_equal(bits(outs[0][1]), bits(outs[1][1]))


# ---- the transform against the oracle at every dispatch edge (iuwt_cases.py)

ALL_SHAPES = sorted(set(K.EDGE_CASES + [K.ALIGN_CASE] + K.WS_CASES))


def same_values(got, want, what):
    """Bit for bit; where the oracle has a NaN (the special-values image),
    a NaN of any payload."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.flatnonzero((bits(got) != bits(want)).ravel() & ~nan.ravel())
    assert bad.size == 0, (what, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])


_ORACLE_CACHE = {}


def oracle_case(w, h, n, kind, aliased, include_largest):
    """(image, coefficients, input after the call, recomposition) of the
    oracle; the last few are kept, the GPU cases of one shape being adjacent."""
    key = (w, h, n, kind, aliased, include_largest)
    if key not in _ORACLE_CACHE:
        while len(_ORACLE_CACHE) >= 16:
            _ORACLE_CACHE.pop(next(iter(_ORACLE_CACHE)))
        orc = get_oracle()
        img = dict(K.IMAGES)[kind](w, h, w + n)
        coeffs, after = iuwt_decompose(orc, img, n, aliased, include_largest)
        back = iuwt_recompose(orc, coeffs, n, include_largest)
        for a in (img, coeffs, after, back):
            a.setflags(write=False)
        _ORACLE_CACHE[key] = (img, coeffs, after, back)
    return _ORACLE_CACHE[key]


@pytest.mark.parametrize("w,h,n", ALL_SHAPES)
@pytest.mark.parametrize("kind", [k for k, _ in K.IMAGES])
def test_oracle_equals_float64_zero_boundary_filter(w, h, n, kind):
    """The oracle defines the transform where the reference does not (width
    or height below 4 d: its region loops overrun), by zero-filled taps. Its
    non-aliased planes and recompositions against the zero-boundary à-trous
    filter in float64, within the bounds derived in iuwt_cases.py; for the
    special-values image the non-finite pixels must be the same ones and the
    bound holds on the others, with the largest finite |pixel|."""
    img, coeffs, after, _ = oracle_case(w, h, n, kind, False, True)
    assert np.array_equal(bits(after), bits(img))
    m = np.abs(img[np.isfinite(img)]).max() if np.isfinite(img).any() else 0.0
    ref = K.decompose64(img, n)
    bounds = K.decompose_bounds(n, float(m))
    for s in range(n + 1):
        fin = np.isfinite(ref[s])
        assert np.array_equal(np.isnan(coeffs[s]), np.isnan(ref[s])), s
        assert np.array_equal(coeffs[s][~fin & ~np.isnan(ref[s])],
                              ref[s][~fin & ~np.isnan(ref[s])]), s
        err = np.abs(coeffs[s].astype(np.float64)[fin] - ref[s][fin])
        assert err.size == 0 or err.max() <= bounds[s], (s, err.max(), bounds[s])
    for il in (True, False):
        c = coeffs.copy()
        if not il:
            c[n] = 0
        back = iuwt_recompose(get_oracle(), c, n, il)
        ref_back = K.recompose64(c, n, il)
        fin = np.isfinite(ref_back)
        assert np.array_equal(np.isnan(back), np.isnan(ref_back)), il
        err = np.abs(back.astype(np.float64)[fin] - ref_back[fin])
        bound = K.recompose_bound(c, n, il)
        assert err.size == 0 or err.max() <= bound, (il, err.max(), bound)


def test_cases_reach_every_reachable_chain_kernel():
    """The shapes of the GPU comparison against the census of
    tests/test_iuwt_chain_plan.py (profiles/iuwt_chain_plan_census.txt):
    they launch every instantiation of the row-chain kernels that any call can
    launch, meet every refusal of PlanChain that occurs, run a chain launch
    with more than 64 KiB of LDS, and take every kernel family in both
    directions."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "profiles", "iuwt_chain_plan_census.txt")
    reachable, refusals = set(), set()
    for line in open(path):
        f = line.split()
        if line.startswith("inst ") and "unreachable" not in line:
            reachable.add((f[1], int(f[2][3:]), int(f[3][3:]), int(f[4][3:])))
        if line.startswith("refusal ") and "no call meets it" not in line:
            refusals.add((f[1], int(f[2])))
    assert len(reachable) >= 10 and refusals
    launched, refused, families = set(), set(), set()
    for dec, rec in K.all_dispatches():
        for side, direction in ((dec, "dec"), (rec, "rec")):
            launched |= side["launches"]
            families.add((direction, side["family"]))
            if side["refused"]:
                refused.add((side["refused"][0], side["refused"][2]))
    assert launched == reachable, (reachable - launched, launched - reachable)
    assert refused == refusals, (refusals - refused, refused - refusals)
    assert families == {("dec", "four-pass"), ("dec", "fused-rows"), ("dec", "chain"),
                        ("rec", "four-pass"), ("rec", "chain"), ("rec", "chain-copy")}
    # one pointer off: that direction alone leaves the vector kernels
    w, h, n = K.ALIGN_CASE
    fam = {m: tuple(side["family"] for side in K.dispatch(w, h, n, 3, True, False, misaligned=m))
           for m in (None,) + K.MISALIGNED}
    assert fam == {None: ("chain", "chain"), "input": ("four-pass", "chain"),
                   "coeffs": ("four-pass", "four-pass"), "out": ("chain", "four-pass")}
    p = K.chain_scales(512, 30, 7, True)
    assert not p["refusal"].any() and p["lds"].max() > 64 * 1024


class Plane:
    """A device buffer of floats between sentinel guards (Guarded of
    test_primitives_gpu.py), its body `off` floats into the guarded area:
    off = 1 puts it 4 bytes off a 16-byte boundary."""

    def __init__(self, sess, data=None, n=None, off=0):
        from test_primitives_gpu import Guarded, sentinel
        self.off = off
        if data is not None:
            host = sentinel(data.size + off, np.float32)
            host[off:] = np.asarray(data, np.float32).ravel()
            self.g = Guarded(sess, host)
        else:
            self.g = Guarded(sess, n=n + off, dtype=np.float32)

    @property
    def vp(self):
        return self.g.at(self.off)

    def get(self, shape):
        from test_primitives_gpu import same_bits, sentinel
        body = self.g.get()  # checks the guards
        same_bits(body[:self.off], sentinel(self.off, np.float32))  # the float before
        return body[self.off:].reshape(shape)

    def free(self):
        self.g.free()


def run_and_compare(s, w, h, n, kind, aliased, include_largest, misaligned=None):
    """One decomposition and recomposition under the environment as it is,
    every plane, the recomposition and the input after the call against the
    oracle; outputs start as sentinels, so an unwritten pixel shows."""
    img, coeffs_o, after_o, back_o = oracle_case(w, h, n, kind, aliased, include_largest)
    d_in = Plane(s, data=img, off=int(misaligned == "input"))
    d_scratch = d_in if aliased else Plane(s, n=h * w)
    d_coeffs = Plane(s, n=(n + 1) * h * w, off=int(misaligned == "coeffs"))
    d_out = Plane(s, n=h * w, off=int(misaligned == "out"))
    try:
        assert d_in.vp.value % 16 == (4 if misaligned == "input" else 0)
        s.rdl.rdl_iuwt_decompose(s.h, d_in.vp, d_scratch.vp, w, h, n, d_coeffs.vp,
                                 int(include_largest))
        got = d_coeffs.get((n + 1, h, w))
        for k in range(n + 1):
            same_values(got[k], coeffs_o[k], ("plane", k))
        same_values(d_in.get((h, w)), after_o if aliased else img, "input after the call")
        if not aliased:
            d_scratch.get((h, w))  # its guards
        s.rdl.rdl_iuwt_recompose(s.h, d_coeffs.vp, w, h, n, int(include_largest), d_out.vp)
        same_values(d_out.get((h, w)), back_o, "recomposition")
        same_values(d_coeffs.get((n + 1, h, w)), got, "coefficients after the recomposition")
    finally:
        for x in {id(a): a for a in (d_in, d_scratch, d_coeffs, d_out)}.values():
            x.free()


class iuwt_env:
    """RDL_IUWT_FUSED / RDL_IUWT_CHAIN_WS around a call (None: unset)."""

    def __init__(self, mode=None, ws=None):
        self.vars = {"RDL_IUWT_FUSED": mode, "RDL_IUWT_CHAIN_WS": ws}

    def __enter__(self):
        for k, v in self.vars.items():
            assert k not in os.environ
            if v is not None:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k in self.vars:
            os.environ.pop(k, None)


@pytest.fixture(scope="module")
def sess():
    from rdl_lib import Session
    s = Session(0)
    yield s
    s.close()


EDGE_PARAMS = [(w, h, n, il, aliased, mode)
               for (w, h, n) in K.EDGE_CASES
               for il in (True, False) for aliased in (False, True) for mode in K.MODES]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,n,include_largest,aliased,mode", EDGE_PARAMS)
def test_gpu_iuwt_edges_bit_exact(sess, w, h, n, include_largest, aliased, mode):
    """Every kernel family at the shapes where the dispatch changes
    (iuwt_cases.EDGE_CASES), under RDL_IUWT_FUSED unset, 0, 1 and 3, against
    the oracle, with the noise image and the special-values image."""
    for kind, _ in K.IMAGES:
        with iuwt_env(mode):
            run_and_compare(sess, w, h, n, kind, aliased, include_largest)


@pytest.mark.gpu
@pytest.mark.parametrize("misaligned", K.MISALIGNED)
@pytest.mark.parametrize("include_largest", [True, False])
@pytest.mark.parametrize("mode", K.MODES)
def test_gpu_iuwt_misaligned_pointer_bit_exact(sess, misaligned, include_largest, mode):
    """A vectorizable shape with one pointer 4 bytes off a 16-byte boundary:
    the dispatcher must take the scalar kernels for that direction (a float4
    access there would fault or read shifted columns)."""
    w, h, n = K.ALIGN_CASE
    for kind, _ in K.IMAGES:
        with iuwt_env(mode):
            run_and_compare(sess, w, h, n, kind, False, include_largest, misaligned)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,n", K.WS_CASES)
@pytest.mark.parametrize("ws", K.WS_VALUES)
@pytest.mark.parametrize("include_largest", [True, False])
@pytest.mark.parametrize("mode", [2, 3])
def test_gpu_iuwt_strip_width_override_bit_exact(sess, w, h, n, ws, include_largest, mode):
    """RDL_IUWT_CHAIN_WS = 256, 768, 1024: the NO = 4 instantiations and
    strips of another width, recomposition (mode 2) and both directions
    (mode 3)."""
    for kind, _ in K.IMAGES:
        with iuwt_env(mode, ws):
            run_and_compare(sess, w, h, n, kind, False, include_largest)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [2, 3])
def test_gpu_iuwt_session_reuse(mode):
    """One session, large then smallest then large again: the scratch of
    s->iuwt grows and is reused, the dummy area behind its first plane moves
    with the size, and the opt-in for more than 64 KiB of LDS (mode 3,
    (520, 200, 7) at d = 127) happens once."""
    from rdl_lib import Session
    s = Session(0)
    try:
        for (w, h, n) in [(16388, 8, 3), (520, 200, 7), (4, 1, 3), (520, 200, 7), (16388, 8, 3)]:
            for aliased in (False, True):
                with iuwt_env(mode):
                    run_and_compare(s, w, h, n, "noise", aliased, True)
    finally:
        s.close()
