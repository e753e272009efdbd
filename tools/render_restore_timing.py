"""Timing record of ComponentList.render and radler.restore at 8192^2
(profiles/render_restore_timing.txt): a 4-scale, 100,000-component,
single-frequency list rendered into its model image, and that image restored
onto a noise residual. Times by the rdl_timing kernel families (HIP events
around every launch, with the launch counts) and by a host clock around the
whole call.

    python tools/render_restore_timing.py [--out FILE] [--size N] [--reps K]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-func-radler_amd"))
import radler as rd  # noqa: E402

SEED = 2026
SCALES = [0.0, 8.0, 16.0, 32.0]
N_PER_SCALE = 25_000
FAMILIES = ["render_components", "extend", "conv_rows", "conv_cols", "fft", "spectrum_multiply",
            "spectrum_multiply_add", "add", "box", "conv64_rows", "conv64_cols", "fft64",
            "spectrum_multiply64", "trim_subtract", "rms_elementwise", "axpy"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    w = args.size
    lib = C.CDLL(os.path.join(ROOT, "ska-sdp-func-radler_amd", "lib", "librdl_hip.so"))
    lib.rdl_timing_get_all.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_double)]
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        lib.rdl_timing_reset_all()
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        fams = {}
        for fam in FAMILIES:
            ms, n, b = C.c_double(), C.c_uint64(), C.c_double()
            lib.rdl_timing_get_all(fam.encode(), C.byref(ms), C.byref(n), C.byref(b))
            if n.value:
                fams[fam] = (ms.value, n.value)
        return wall, fams

    def report(name, runs):
        say(f"{name}:")
        for wall, fams in runs:
            device = sum(ms for ms, _ in fams.values())
            say(f"  wall {wall:8.1f} ms, device kernels {device:7.2f} ms: " +
                ", ".join(f"{k} {ms:.2f} ms / {n}" for k, (ms, n) in fams.items()))

    rng = np.random.default_rng(SEED)
    cl = rd.ComponentList(w, w, len(SCALES), 1)
    for s in range(len(SCALES)):
        pixels = rng.choice(w * w, N_PER_SCALE, replace=False)
        values = rng.uniform(0.01, 1.0, N_PER_SCALE) * rng.choice([-1.0, 1.0], N_PER_SCALE)
        for p, v in zip(pixels.tolist(), values.tolist()):
            cl.add(p % w, p // w, s, [v])
    cl.merge_duplicates()
    counts = [cl.component_count(s) for s in range(len(SCALES))]
    no_fit = rd.SpectralFitter(rd.SpectralFittingMode.no_fitting, 0, [], [])
    shape = rd.MultiscaleShape.tapered_quadratic

    say(f"ComponentList.render and radler.restore at {w} x {w}, one MI355X: 'ms / launches' per")
    say("rdl_timing kernel family (HIP events around every launch) and a host clock around the")
    say("whole call (staging, uploads and the copy of the planes back included).")
    say(f"List: single frequency, scale sizes {SCALES}, components per scale {counts}, positions")
    say(f"drawn without replacement per scale by numpy default_rng({SEED}), tapered quadratic shape.")
    say()
    lib.rdl_timing_enable_all(1)
    planes = cl.render(no_fit, SCALES, [], shape)  # warm up: plans, code objects
    report("render (3 kernel spectra and the size-0 kernel's, 3 forward transforms, 1 inverse)",
           [timed(lambda: cl.render(no_fit, SCALES, [], shape)) for _ in range(args.reps)])
    say()
    pix = 1.0 / 3600.0 * np.pi / 180.0
    residual = (1e-4 * rng.standard_normal((w, w))).astype(np.float32)
    beam = (3.0 * pix, 2.0 * pix, np.radians(30.0), pix, pix)
    rd.restore(residual, planes[0], *beam)  # warm up
    report("restore, beam 3 x 2 pixels FWHM at 30 degrees (box 46, float64 transforms at "
           f"{rd.utils.calculate_good_fft_size(w + 46)}^2)",
           [timed(lambda: rd.restore(residual, planes[0], *beam)) for _ in range(args.reps)])
    lib.rdl_timing_enable_all(0)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
