"""The plan tables of the compile-time-planned FFT engine (csrc/hip/
fft_fast_*.hip), read from the source, and the comparison helpers of
tests/test_fft_plans.py.

Every table entry is a macro invocation followed by its length in a comment:

    RDL_FAST_ROWS(double, 512, 7, 9, 9, 8),      // 9072
    RDL_FAST_COLS(double, 1024, true, 7, 9, 9, 4, 4),        // 9072
    RDL_CONV_D(1024, 7, 9, 9, 4, 4),        // 9072
    RDL_FAST_STEPS(64, 128, 4, 2, RDL_R(8, 8), RDL_R(16, 8)),  // 8192

The tables are parsed, not typed in, so a plan added later is tested without
an edit here. The helpers take plain numpy arrays: the CPU tests drive them
with doctored inputs (tests/test_fft_plan_tables.py), the GPU tests with what
the kernels wrote.
"""
import collections
import os
import re

import numpy as np

HIP_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "ska-sdp-func-radler_amd", "csrc", "hip")
SOURCES = ("fft_fast_rows_f64.hip", "fft_fast_rows.hip", "fft_fast_cols.hip",
           "fft_fast_convd.hip", "fft_fast_steps.hip")

# rdl_hip.h
RDL_CONV_FAST_COLUMNS, RDL_CONV_FAST_ROWS, RDL_CONV_FAST_TILED, RDL_CONV_FAST_CONVD = 1, 2, 4, 8
RDL_CONV_ROW_MAJOR, RDL_CONV_COL_MAJOR = 0, 1
RDL_ERR_ARG = 1

RTOL = 1e-6  # tests/test_configs_gpu.py

Plan = collections.namedtuple("Plan", "length precision threads radices")
# a four-step plan: radices = (radices of N1, radices of N2)
Steps = collections.namedtuple("Steps", "length precision threads radices n1 n2 ga gb")
Entry = collections.namedtuple("Entry", "family plan comment file line")

_CALL = re.compile(r"^\s*(RDL_FAST_ROWS|RDL_FAST_COLS|RDL_CONV_D|RDL_FAST_STEPS)\((.*)\),?\s*"
                   r"(?://\s*(\d+))?\s*$")
_PRECISION = {"double": "f64", "float": "f32"}


def _product(values):
    p = 1
    for v in values:
        p *= v
    return p


def _ints(text):
    return tuple(int(t) for t in text.split(",") if t.strip())


def _parse_call(macro, args):
    """(family, plan) of one invocation's argument text."""
    if macro == "RDL_FAST_STEPS":
        m = re.fullmatch(r"\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*RDL_R\(([^)]*)\),\s*"
                         r"RDL_R\(([^)]*)\)\s*", args)
        if not m:
            raise ValueError(f"unreadable RDL_FAST_STEPS({args})")
        n1, n2, ga, gb = (int(m.group(i)) for i in range(1, 5))
        # the kernels are instantiated with 256 threads (the macro's body)
        return "steps", Steps(n1 * n2, "f32", 256, (_ints(m.group(5)), _ints(m.group(6))),
                              n1, n2, ga, gb)
    parts = [p.strip() for p in args.split(",")]
    if macro == "RDL_CONV_D":
        radices = tuple(int(p) for p in parts[1:])
        return "convd", Plan(_product(radices), "f64", int(parts[0]), radices)
    precision = _PRECISION[parts[0]]
    if macro == "RDL_FAST_ROWS":
        radices = tuple(int(p) for p in parts[2:])
        return "rows_" + precision, Plan(2 * _product(radices), precision, int(parts[1]), radices)
    radices = tuple(int(p) for p in parts[3:])  # T, TH, PF, radices
    return "cols_" + precision, Plan(_product(radices), precision, int(parts[1]), radices)


def parse_entries(hip_dir=HIP_DIR):
    """Every table entry of the five files, in source order."""
    out = []
    for name in SOURCES:
        with open(os.path.join(hip_dir, name)) as f:
            for number, line in enumerate(f, 1):
                if line.lstrip().startswith("#"):  # the macro's #define / #undef
                    continue
                m = _CALL.match(line)
                if not m:
                    if re.search(r"\bRDL_(FAST_ROWS|FAST_COLS|CONV_D|FAST_STEPS)\(", line):
                        raise ValueError(f"{name}:{number}: unreadable plan entry: {line!r}")
                    continue
                family, plan = _parse_call(m.group(1), m.group(2))
                comment = int(m.group(3)) if m.group(3) else None
                out.append(Entry(family, plan, comment, name, number))
    return out


FAMILIES = ("rows_f64", "cols_f64", "convd", "rows_f32", "steps", "cols_f32")


def plan_tables(hip_dir=HIP_DIR):
    """{family: [plan, ...]} with (length, precision, threads, radices) per
    plan; families: rows_f64, cols_f64, convd, rows_f32, steps, cols_f32."""
    tables = {f: [] for f in FAMILIES}
    for e in parse_entries(hip_dir):
        tables[e.family].append(e.plan)
    return tables


def lengths(tables, family):
    return sorted(p.length for p in tables[family])


def planes(tables):
    """The thin planes of tests/test_fft_plans.py: per length n of a family
    (n, base) puts plan n on the rows and (base, n) on the columns, base the
    family's smallest length; the base x base plane once. Returns
    (f64 planes, float tiled planes, float one-pass planes) as (w, h)."""
    def thin(ns):
        base = min(ns)
        out = [(base, base)]
        for n in sorted(ns):
            if n != base:
                out += [(n, base), (base, n)]
        return out
    return (thin(lengths(tables, "rows_f64")), thin(lengths(tables, "rows_f32")),
            [(ONE_PASS_WIDTH, n) for n in lengths(tables, "cols_f32")])


ONE_PASS_WIDTH = 96  # a width without a float row plan: Columns<float> runs


def expected_fast(tables, w, h, f64):
    """rdl_conv_fast's mask for a w x h plane, from the tables (conv.hip
    rdl_conv_create_ex)."""
    if f64:
        rows = w in lengths(tables, "rows_f64")
        cols = h in lengths(tables, "cols_f64")
        return ((RDL_CONV_FAST_ROWS if rows else 0) | (RDL_CONV_FAST_COLUMNS if cols else 0) |
                (RDL_CONV_FAST_CONVD if h in lengths(tables, "convd") else 0))
    rows = w in lengths(tables, "rows_f32")
    cols = h in lengths(tables, "cols_f32")
    tiled = rows and h in lengths(tables, "steps")
    return ((RDL_CONV_FAST_ROWS if rows else 0) | (RDL_CONV_FAST_COLUMNS if cols else 0) |
            (RDL_CONV_FAST_TILED if tiled else 0))


# ------------------------------------------------------------- spectrum layout
TILE = 16


def tile(natural):
    """A natural [row][column] spectrum (h x w/2+1) in the tiled order
    (element (y, k) at ((k / 16) * h + y) * 16 + k % 16), the last tile
    zero-padded: what a RDL_CONV_FAST_TILED plan reads."""
    h, nu = natural.shape
    nt = (nu + TILE - 1) // TILE
    padded = np.zeros((h, nt * TILE), natural.dtype)
    padded[:, :nu] = natural
    return np.ascontiguousarray(padded.reshape(h, nt, TILE).transpose(1, 0, 2)).reshape(-1)


def untile(flat, w, h):
    """tile()'s inverse for a w x h plane: the natural h x (w/2+1) array."""
    nu = w // 2 + 1
    nt = (nu + TILE - 1) // TILE
    t = np.asarray(flat).reshape(nt, h, TILE)
    return t.transpose(1, 0, 2).reshape(h, nt * TILE)[:, :nu]


# ------------------------------------------------------------------ references
def noise_image(w, h, seed, bright=50.0):
    """Seeded Gaussian noise plus one bright pixel."""
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((h, w)).astype(np.float32)
    img[h // 3, w // 5] = bright
    return img


def placed_kernel(k, w, h):
    """PrepareSmallConvolutionKernel: an n x n kernel with its centre at the
    origin of a w x h plane (float64)."""
    n = k.shape[0]
    ker = np.zeros((h, w), np.float64)
    ker[:n, :n] = k
    return np.roll(ker, (-(n // 2), -(n // 2)), axis=(0, 1))


def centred_psf_kernel(psf, pw, ph):
    """rdl_prepare_psf_kernel: psf centred in a zero pw x ph plane, shifted
    so that (pw/2, ph/2) lands at the origin (float64)."""
    h, w = psf.shape
    ox, oy = (pw - w) // 2, (ph - h) // 2
    kp = np.zeros((ph, pw))
    kp[oy:oy + h, ox:ox + w] = psf
    return np.roll(kp, (-(ph // 2), -(pw // 2)), axis=(0, 1))


def mixed_radix_dft(x, radices, skip_twiddles=None):
    """The forward DFT along axis 0 as the kernels' passes compute it (pass p
    of radix R over span NS = the product of the earlier radices: twiddle
    W_N^{r k N / (NS R)}, an R-point DFT, outputs NS apart), in complex128.
    skip_twiddles: the index of a pass whose twiddles are left out (a broken
    transform, for the negative controls)."""
    x = np.asarray(x, np.complex128)
    n = x.shape[0]
    assert _product(radices) == n
    flat = x.reshape(n, -1)
    ns = 1
    for p, r in enumerate(radices):
        nb = n // r
        j = np.arange(nb)
        k = j % ns
        v = flat.reshape(r, nb, -1).copy()  # v[q, j] = x[j + q nb]
        if p != skip_twiddles:
            e = np.arange(r)[:, None] * k[None, :] * (n // (ns * r))
            v *= np.exp(-2j * np.pi * e / n)[:, :, None]
        q = np.arange(r)
        dft = np.exp(-2j * np.pi * np.outer(q, q) / r)
        v = np.einsum("ab,bjc->ajc", dft, v)
        d = (j // ns) * ns * r + k
        out = np.empty_like(flat)
        out[(d[None, :] + q[:, None] * ns).reshape(-1)] = v.reshape(r * nb, -1)
        flat = out
        ns *= r
    return flat.reshape(x.shape)


def peak_in_box(img, h_border, v_border, allow_negative):
    """peak_finder::Find on the whole image (rdl_find_peak with start_y 0,
    end_y h, no mask): the first index of the largest value (of |value| with
    allow_negative) inside the borders. Returns (x, y, value)."""
    h, w = img.shape
    box = img[v_border:h - v_border, h_border:w - h_border]
    key = np.abs(box) if allow_negative else box
    i = int(np.argmax(key))  # numpy's argmax returns the first of equal values
    y, x = divmod(i, box.shape[1])
    return x + h_border, y + v_border, float(box[y, x])


# ------------------------------------------------------------------ the checks
# Each returns (error, bound) and asserts error <= bound; `what` names the
# plan in the message. The bounds are the ones the suite already asserts for
# the same operation (tests/test_fft_fast.py, tests/test_scale_convs.py).
def transform_scale(n_points):
    return np.sqrt(n_points) * np.sqrt(np.log2(n_points))


def check_spectrum(got, ref, n_points, f64, what):
    """A forward spectrum of unit noise over n_points points (w h for the
    2-D transform, w for the rows pass alone), as
    test_fast_forward_matches_numpy: 1e-13 (float64) / 2e-6 (float) x
    sqrt(n) sqrt(log2 n)."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    bound = (1e-13 if f64 else 2e-6) * transform_scale(n_points)
    assert err <= bound, f"{what}: |spectrum - numpy| {err:.3g} > {bound:.3g}"
    return err, bound


def check_image(got, ref, n_points, f64, what):
    """A convolved float image, as test_fast_convolutions_match_numpy:
    float64 plans give the exact result rounded to float (half a float ulp +
    1e-12 x scale), float plans 2e-6 x scale; scale = max |ref| x
    sqrt(log2 n)."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = np.abs(ref).max() * np.sqrt(np.log2(n_points))
    d = np.abs(got - ref)
    if f64:
        half_ulp = 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        ratio = float((d / (half_ulp + 1e-12 * scale)).max())
        assert ratio <= 1.0, f"{what}: |image - numpy| is {ratio:.3g} x (half ulp + 1e-12 scale)"
        return ratio, 1.0
    err, bound = float(d.max()), 2e-6 * scale
    assert err <= bound, f"{what}: |image - numpy| {err:.3g} > {bound:.3g}"
    return err, bound


def check_correction(got, residual, conv_window, conv_peak, what):
    """CorrectResidualDirty's residual -= float(convolution window), as
    test_fast_masked_correction: 2.4e-7 x max(|conv|, |residual|)."""
    expect = residual - conv_window.astype(np.float32)
    assert got.shape == expect.shape, (what, got.shape, expect.shape)
    err = float(np.abs(got - expect).max())
    bound = 2.4e-7 * max(conv_peak, float(np.abs(residual).max()))
    assert err <= bound, f"{what}: |residual - numpy| {err:.3g} > {bound:.3g}"
    return err, bound


def check_scale(got, ref, what):
    """One scale convolution against float64, as test_scales_against_float64:
    RTOL / 2 x the convolved image's peak."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    peak = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    bound = RTOL / 2 * peak
    assert err <= bound, f"{what}: |float32 - float64| {err:.3g} > {bound:.3g}"
    return err, bound


def check_real_kernel(got, ref, what):
    """rdl_conv_real_kernel against rfft2 of the placed kernel, as
    test_real_kernel_spectrum: numpy's imaginary part <= 1e-12 x peak, the
    real part within 1.2e-7 x peak."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    peak = float(np.abs(ref).max())
    imag = float(np.abs(ref.imag).max())
    assert imag <= 1e-12 * peak, f"{what}: the reference spectrum is not real ({imag:.3g})"
    err = float(np.abs(got - ref.real).max())
    bound = 1.2e-7 * peak
    assert err <= bound, f"{what}: |K - Re rfft2| {err:.3g} > {bound:.3g}"
    return err, bound
