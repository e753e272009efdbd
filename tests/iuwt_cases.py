"""Shapes, images and references of the IUWT transform tests
(tests/test_iuwt.py, tests/test_iuwt_chain_plan.py).

* plan_chain: PlanChain (csrc/hip/iuwt_chain_plan.h) restated on numpy
  arrays, with the reason of a refusal; test_iuwt_chain_plan.py holds it
  against the C++ function over a sweep.
* dispatch: which kernel family rdl_iuwt_decompose / rdl_iuwt_recompose
  (csrc/hip/iuwt.hip) take for a call, from the same conditions.
* EDGE_CASES / WS_CASES: the shapes of the GPU comparison with the oracle.
* image / special_image: the two images of every shape.
* decompose64 / recompose64 and the error bounds: the zero-boundary à-trous
  transform in float64, the yardstick of the oracle where the reference
  itself is undefined (width or height below 4 d).
"""
import numpy as np

# ---------------------------------------------------------------- PlanChain

REFUSALS = {0: "planned",
            1: "row slot: wa4 > 512 float4 per row",
            2: "halo strip: ni > no + 2",
            3: "more than 2^30 workgroups",
            4: "LDS above 160 KiB"}


def plan_chain(w, h, d, decompose, ws_override=0):
    """PlanChain for arrays (or scalars) of widths, heights, spacings,
    directions and strip-width overrides (0: none). Returns a dict of int64
    arrays: refusal (a key of REFUSALS; the other fields are meaningful only
    where it is 0), ws, n_strips, n_seg, n_res, blocks, lds, na, no, ni."""
    w, h, d, decompose, ov = np.broadcast_arrays(
        *[np.asarray(v, np.int64) for v in (w, h, d, decompose, ws_override)])
    decompose = decompose != 0
    ws = np.where((ov >= 256) & (ov <= 1024) & (ov % 256 == 0), ov, 512)
    ws = np.minimum(ws, (w + 3) // 4 * 4)
    halo = np.where(decompose, 4 * d, 2 * d)
    wa4 = (ws + 2 * halo + 6) // 4
    na = np.where(wa4 <= 256, 1, 2)
    no = (ws + 255) // 256
    no = np.where(no == 3, 4, no)
    wi = ws + 4 * d
    ni = np.maximum(no, (wi + 255) // 256)
    n_strips = (w + ws - 1) // ws
    n_res = np.minimum(d, h)
    k_max = (h + d - 1) // d
    n_seg = np.minimum((k_max + 23) // 24, (1536 + n_res * n_strips - 1) // (n_res * n_strips))
    n_seg = np.maximum(1, np.minimum(n_seg, k_max))
    n_blocks = n_res * n_seg * n_strips
    blocks = 8 * ((n_blocks + 7) // 8)
    slots = 2 * 1024 * na
    lds = np.where(decompose, slots + 7 * wi + 11 * ws, slots + 5 * ws) * 4
    refusal = np.select([wa4 > 512, ni > no + 2, n_blocks > 1 << 30, lds > 160 * 1024],
                        [1, 2, 3, 4], 0)
    return dict(refusal=refusal, ws=ws, n_strips=n_strips, n_seg=n_seg, n_res=n_res,
                blocks=blocks, lds=lds, na=na, no=no, ni=ni)


def chain_scales(w, h, n_scales, decompose, ws_override=0):
    """The plans of spacings 1, 3, .. 2^n_scales - 1, one array entry each."""
    d = (1 << np.arange(1, n_scales + 1)) - 1
    return plan_chain(w, h, d, decompose, ws_override)


K_FUSED_MAX_WIDTH = 16384  # kIuwtFusedMaxWidth


def dispatch(w, h, n, mode, include_largest, aliased, misaligned=None, ws_override=0):
    """(decomposition, recomposition) of one call pair as
    (family, launches): family one of "four-pass", "fused-rows", "chain";
    launches the chain instantiations (direction, na, no, ni - no) it runs,
    and for a family reached through a refused plan, refused = (direction, d,
    refusal); "chain-copy" is the chain recomposition of no scale at all
    (n = 1 without the approximation plane: one copy). mode: None (unset,
    = 2), 0, 1, 2, 3. misaligned: None or the pointer 4 bytes off a 16-byte
    boundary, "input", "coeffs" or "out": the decomposition needs d_input and
    d_coeffs aligned, the recomposition d_coeffs and d_out."""
    m = 2 if mode is None else mode
    assert misaligned in (None, "input", "coeffs", "out")
    vec_dec = w % 4 == 0 and misaligned not in ("input", "coeffs")
    vec_rec = w % 4 == 0 and misaligned not in ("coeffs", "out")

    def chains(count, dec):
        p = chain_scales(w, h, count, dec, ws_override)
        bad = np.flatnonzero(p["refusal"])
        if bad.size:
            s = int(bad[0])
            return None, ("dec" if dec else "rec", (1 << (s + 1)) - 1, int(p["refusal"][s]))
        return {("dec" if dec else "rec", int(p["na"][s]), int(p["no"][s]),
                 int(p["ni"][s] - p["no"][s]) if dec else 0) for s in range(count)}, None

    dec = dict(family="four-pass", launches=set(), refused=None)
    if vec_dec and not aliased:
        if m == 3:
            launches, refused = chains(n, True)
            if launches is not None:
                dec = dict(family="chain", launches=launches, refused=None)
            else:
                dec["refused"] = refused
        if dec["family"] != "chain" and m != 0 and w <= K_FUSED_MAX_WIDTH:
            dec["family"] = "fused-rows"
    rec = dict(family="four-pass", launches=set(), refused=None)
    if vec_rec and m >= 2:
        first = n if include_largest else n - 1
        launches, refused = chains(first, False)
        if launches is not None:
            rec = dict(family="chain" if first else "chain-copy", launches=launches,
                       refused=None)
        else:
            rec["refused"] = refused
    return dec, rec


# -------------------------------------------------------------------- shapes

# (w, h, n_scales), by what they are there for
EDGE_CASES = [
    # width % 4 != 0: the scalar kernels; widths and heights below d, 2d and
    # 4d; a single row, a single column
    (1, 1, 2), (1, 7, 3), (5, 3, 4), (13, 9, 5), (63, 64, 6), (255, 131, 7), (1001, 37, 6),
    # the smallest vectorizable images; (4, 1, 8): the one strip width whose
    # decomposition is refused by the halo-strip check (d = 255), not by the
    # row slot
    (4, 1, 3), (8, 5, 4), (4, 1, 8),
    # one scale: without the approximation plane the chain recomposition has
    # no scale to run and copies the detail plane
    (8, 5, 1),
    # overlapping boundary regions with width % 4 == 0; (64, 48): h < d at
    # d = 63 and 127
    (1000, 37, 6), (260, 300, 7), (300, 260, 7), (64, 48, 7),
    # column strips whose last is 4 columns wide
    (516, 40, 4), (1028, 25, 6),
    # wider than kIuwtFusedMaxWidth
    (16388, 8, 3),
    # a refused plan: d = 255 (recomposition, with the approximation plane),
    # d up to 4095
    (260, 300, 8), (64, 48, 12),
    # a chain decomposition with more than 64 KiB of LDS (mode 3, d = 127)
    (512, 30, 7),
]
ALIGN_CASE = (256, 64, 4)  # with one of d_input, d_coeffs, d_out 4 bytes off
MISALIGNED = ("input", "coeffs", "out")
# x RDL_IUWT_CHAIN_WS; (776, 1, 7) with 1024 is the census's smallest case of
# IuwtDecomposeChain<2,4,6>, which the first three do not launch; (516, 1, 9)
# with 768 is the smallest call whose recomposition passes d = 255 (NO = 4)
# and is refused by the row slot at d = 511
WS_CASES = [(516, 40, 4), (1028, 25, 6), (520, 200, 7), (776, 1, 7), (516, 1, 9)]
WS_VALUES = (256, 768, 1024)
MODES = (None, 0, 1, 3)  # RDL_IUWT_FUSED


def all_dispatches():
    """Every (decomposition, recomposition) dispatch of the GPU test's list."""
    out = []
    for (w, h, n) in EDGE_CASES:
        for mode in MODES:
            for il in (True, False):
                for aliased in (False, True):
                    out.append(dispatch(w, h, n, mode, il, aliased))
    w, h, n = ALIGN_CASE
    for mode in MODES:
        for il in (True, False):
            for misaligned in MISALIGNED:
                out.append(dispatch(w, h, n, mode, il, False, misaligned=misaligned))
    for (w, h, n) in WS_CASES:
        for ws in WS_VALUES:
            for mode in (2, 3):
                for il in (True, False):
                    out.append(dispatch(w, h, n, mode, il, False, ws_override=ws))
    return out


# -------------------------------------------------------------------- images

def image(w, h, seed):
    """Noise plus a Gaussian source."""
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((h, w)).astype(np.float32) * np.float32(1e-2)
    yy, xx = np.mgrid[0:h, 0:w]
    img += np.exp(-((xx - w / 3) ** 2 + (yy - h / 2) ** 2) / (2 * 6.0 ** 2)).astype(np.float32)
    return img


def special_image(w, h, seed):
    """image() with, left of the middle, a block of +0.0 above a block of -0.0
    (the deconvolution recomposes planes that rdl_iuwt_apply_mask zeroed
    almost everywhere), in its middle a patch of subnormals (1e-41) beside
    one of values whose 1/16 tap is subnormal (1e-37), both with alternating
    signs, and one +Inf pixel and one NaN pixel in opposite corners (top
    right, bottom left): w - 1 columns and h - 1 rows apart, the most a shape
    allows along both axes, so that along the longer axis the Inf spreads
    through the planes without the NaN for as long as the shape lets it. (A
    NaN in the Inf's row or column would turn every later Inf into a NaN,
    which is compared as a mask only.) A block that does not fit a tiny shape
    is empty or overwritten by the next; a single pixel has neither Inf nor
    NaN."""
    img = image(w, h, seed)
    z0, z1 = w // 8, w // 8 + w // 4
    img[:max(1, h // 2), z0:z1] = np.float32(0.0)
    img[max(1, h // 2):, z0:z1] = np.float32(-0.0)
    sign = np.where((np.add.outer(np.arange(h), np.arange(w)) & 1) == 0, 1.0, -1.0)
    y0, x0 = h // 3, w // 2
    for dx, v in ((0, 1e-41), (5, 1e-37)):
        sl = (slice(y0, y0 + 3), slice(x0 + dx, min(x0 + dx + 5, w)))
        img[sl] = (sign[sl] * v).astype(np.float32)
    if w > 1 or h > 1:
        img[0, w - 1] = np.inf
        img[h - 1, 0] = np.nan
    return img


IMAGES = (("noise", image), ("special", special_image))

# ----------------------------------------------------------- float64 yardstick

TAPS = np.array([1, 4, 6, 4, 1], np.float64) / 16


def _filter64(a, d, axis):
    """Σ_k TAPS[k] a[i + (k - 2) d] along axis, taps outside the image zero."""
    n = a.shape[axis]
    out = np.zeros_like(a)
    for k in range(5):
        s = (k - 2) * d
        lo, hi = max(0, -s), min(n, n - s)
        if lo >= hi:
            continue
        dst = [slice(None)] * 2
        src = [slice(None)] * 2
        dst[axis], src[axis] = slice(lo, hi), slice(lo + s, hi + s)
        out[tuple(dst)] += TAPS[k] * a[tuple(src)]
    return out


def _smooth64(a, d):
    return _filter64(_filter64(a, d, 1), d, 0)


def decompose64(img, n_scales):
    """The non-aliased DecomposeMt in float64: n_scales detail planes and the
    approximation plane."""
    with np.errstate(invalid="ignore"):
        a = np.asarray(img, np.float64)
        planes = []
        for s in range(n_scales):
            d = (1 << (s + 1)) - 1
            i1 = _smooth64(a, d)
            planes.append(a - _smooth64(i1, d))
            a = i1
        planes.append(a)
    return np.stack(planes)


def recompose64(coeffs, n_scales, include_largest):
    with np.errstate(invalid="ignore"):
        c = np.asarray(coeffs, np.float64)
        first = n_scales if include_largest else n_scales - 1
        out = c[first].copy()
        for s in range(first - 1, -1, -1):
            out = _smooth64(out, (1 << (s + 1)) - 1) + c[s]
    return out


U = 2.0 ** -24  # float32 unit roundoff
TINY = 2.0 ** -150  # a rounding in the subnormal range errs by half of 2^-149


def decompose_bounds(n_scales, m):
    """Error bounds of the float32 planes against decompose64, m = max|image|.
    Every filter is a convex combination (no value grows), and a tap sum makes
    at most 5 roundings. Detail plane s is reached through 4 (s + 1) filter
    passes, then one subtraction of values up to 2 m: (5 * 4 (s + 1) + 2) u m;
    the approximation plane through 2 n passes: 5 * 2 n u m. Where a result is
    subnormal (the special-values image) a rounding errs by TINY instead of
    by u times the value, so each rounding is given both. With m near 1, as
    in every image but one, TINY is 2e-38 of the bound and decides nothing;
    it decides at (1, 1, 2) alone, whose special image is a single subnormal
    pixel (m = 1e-41), where u m is below what float32 can resolve."""
    return ([(5 * 4 * (s + 1) + 2) * (U * m + TINY) for s in range(n_scales)]
            + [5 * 2 * n_scales * (U * m + TINY)])


def recompose_bound(coeffs, n_scales, include_largest):
    """Each of at most n steps filters twice (10 roundings) and adds (1); no
    intermediate exceeds Σ_s max|c_s| over the planes that enter (TINY: as in
    decompose_bounds)."""
    first = n_scales if include_largest else n_scales - 1
    c = np.asarray(coeffs, np.float64)[:first + 1]
    c = np.where(np.isfinite(c), c, 0.0)
    return 11 * n_scales * (U * np.abs(c).reshape(first + 1, -1).max(axis=1).sum() + TINY)
