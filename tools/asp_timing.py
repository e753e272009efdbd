"""Where a component of the adaptive-scale-pixel algorithm spends its time.

The extended-source case of tests/test_asp_gpu.py scaled to 1024^2 with the
source widths x 8: a PSF of FWHM 32 px (peak 1), a Gaussian of FWHM 96 px and
flux 10 plus a point of flux 1, gain 0.1, threshold 5 % of the start peak, at
most 300 components. One Radler.perform after a warm-up perform on a copy.

Per component, split into four parts:
  peak searches    the linear integration, the scale-0 search and the fused
                   multi-scale transforms with their searches
  fit              rdl_gaussian_fit_sums (one launch pair and one 224-byte
                   read per Levenberg-Marquardt evaluation)
  weighted values  rdl_gaussian_weighted_values
  correction       rdl_draw_gaussian (model and scratch), the padded float64
                   convolve-and-subtract, rdl_subtract_psf for point sources
`device ms` is HIP-event time of the kernel families (rdl_timing_*_all; the
setup of the major iteration, the scales' PSF peaks and the padded PSF
spectrum, falls into the first and last part and is divided over the
components like everything else); `host ms` is the wall clock of the host
sections (RADLER_HOST_PROFILE's), which includes every wait for the device:
the fit's reads, the searches' collect. The correction is queued without a
wait, so its device time shows up in the host time of the next searches.

    python tools/asp_timing.py [--out FILE] [--size N]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import asp_lib as A  # noqa: E402
from radler_import import radler as rd  # noqa: E402

PARTS = {
    "peak searches": ["integrate", "find_peak", "conv_rows", "conv_cols", "fft",
                      "spectrum_multiply", "extend", "rms_elementwise"],
    "fit": ["gaussian_fit"],
    "weighted values": ["gaussian_weighted"],
    "correction": ["gaussian_draw", "conv64_rows", "conv64_cols", "conv64_rows_sparse",
                   "conv64_cols_sparse", "fft64", "trim_subtract", "subtract_psf"],
}
SECTIONS = {"peak searches": "asp.find_maxima", "fit": "asp.fit",
            "weighted values": "asp.weighted_values", "correction": "asp.correct_and_model"}


def problem(n):
    k = n / 128.0
    yy, xx = np.mgrid[0:n, 0:n]
    psf = A.gaussian(xx, yy, n // 2, n // 2, 4.0 * k, 4.0 * k, 0.0)
    sky = 10.0 * A.unit_norm(12.0 * k, 12.0 * k) * A.gaussian(xx, yy, 70.0 * k, 60.0 * k,
                                                             12.0 * k, 12.0 * k, 0.0)
    sky[int(90 * k), int(30 * k)] += 1.0
    dirty = np.fft.irfft2(np.fft.rfft2(sky) * np.fft.rfft2(np.fft.ifftshift(psf)), s=(n, n))
    return psf.astype(np.float32), dirty.astype(np.float32), 4.0 * k


def perform(n, psf, dirty, beam_px):
    pixel_scale = 1.0 / 60.0 * (np.pi / 180.0)
    s = rd.Settings()
    s.algorithm_type = rd.AlgorithmType.adaptive_scale_pixel
    s.trimmed_image_width = s.trimmed_image_height = n
    s.pixel_scale.x = s.pixel_scale.y = pixel_scale
    s.minor_iteration_count = 300
    s.minor_loop_gain = 0.1
    s.absolute_threshold = 0.05 * float(dirty.max())
    residual, model = dirty.copy(), np.zeros_like(dirty)
    r = rd.Radler(s, psf, residual, model, beam_px * pixel_scale, rd.Polarization.stokes_i)
    t0 = time.perf_counter()
    r.perform(0)
    return r.iteration_number, time.perf_counter() - t0, residual, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    lib = C.CDLL(os.path.join(ROOT, "ska-sdp-func-radler_amd", "lib", "librdl_hip.so"))
    lib.rdl_timing_get_all.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_double)]
    n = args.size
    psf, dirty, beam_px = problem(n)
    perform(n, psf, dirty, beam_px)  # warm-up: plans, kernels, allocations
    lib.rdl_timing_enable_all(1)
    lib.rdl_timing_reset_all()
    rd.gpu.host_profile_enable(True)
    rd.gpu.host_profile_reset()
    components, seconds, residual, model = perform(n, psf, dirty, beam_px)
    host = rd.gpu.host_profile()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# adaptive scale pixel, {n}^2, PSF FWHM {beam_px:g} px: {components} components in "
        f"{seconds * 1e3:.1f} ms ({seconds * 1e3 / max(components, 1):.3f} ms per component); "
        f"residual peak {float(np.abs(residual).max()):.4g} of {float(dirty.max()):.4g}, model "
        f"flux {float(model.sum()):.4g}")
    say("# HIP-event timing of every launch is on, which lengthens the run itself")
    say(f"{'part':16s} {'device ms':>10s} {'launches':>9s} {'device ms/comp':>15s} "
        f"{'host ms':>9s} {'calls':>6s} {'host ms/comp':>13s}")
    for part, families in PARTS.items():
        ms_total, launches = 0.0, 0
        for fam in families:
            ms, k, b = C.c_double(), C.c_uint64(), C.c_double()
            lib.rdl_timing_get_all(fam.encode(), C.byref(ms), C.byref(k), C.byref(b))
            ms_total += ms.value
            launches += k.value
        calls, host_s = host.get(SECTIONS[part], (0, 0.0))
        say(f"{part:16s} {ms_total:10.3f} {launches:9d} {ms_total / max(components, 1):15.4f} "
            f"{host_s * 1e3:9.2f} {calls:6d} {host_s * 1e3 / max(components, 1):13.4f}")
    for name in ("asp.point_source", "asp.convolve_psfs", "fit.gaussian_centred", "asp.execute"):
        calls, host_s = host.get(name, (0, 0.0))
        say(f"# host section {name}: {calls} calls, {host_s * 1e3:.2f} ms")
    lib.rdl_timing_enable_all(0)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
