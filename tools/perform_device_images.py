"""What device images save a Radler.perform, and what the fused average costs
(profiles/perform_device_images.txt).

Perform cost: the host-profile sections perform.load, perform.load_psfs,
perform.store and perform.total of one perform() over numpy arrays and over
the same data as radler.gpu.to_device arrays, in one process, for the h8k
problem (8192^2, one image) and the joined 8 x 4096^2 problem (c3) of
tests/config_problems.py. A warm-up run of each kind comes first. The minor
iteration count is capped (--iterations): the load and store cost does not
depend on it.

Kernel time: rdl_average_planes against the chain it replaces
(rdl_memset_zero, G x rdl_axpy / rdl_axpy_f64, rdl_scale / rdl_axpy_f64 mode
1) for G = 1 and G = 8 source planes of 4096^2, both modes, by a host clock
around runs queued back to back on the session's stream, with the fused kernel's
fraction of the 6.29 TB/s float4 copy rate for its (G + 1) * 4n bytes.

    python tools/perform_device_images.py [--out FILE] [--iterations K] [--reps K]
                                          [--skip-perform] [--skip-kernel]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-func-radler_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import radler as rd  # noqa: E402

import config_problems as cp  # noqa: E402
from rdl_lib import Session  # noqa: E402

SECTIONS = ["perform.load", "perform.load_psfs", "perform.store", "perform.total"]
COPY_ROOF = 6.29e12  # bytes / s, float4 copy
SZ = C.c_size_t


def multiscale_settings(size, max_scales, threshold, iterations):
    s = rd.Settings()
    s.algorithm_type = rd.AlgorithmType.multiscale
    s.trimmed_image_width = s.trimmed_image_height = size
    s.pixel_scale.x = s.pixel_scale.y = cp.PIXEL_SCALE
    s.minor_iteration_count = iterations
    s.absolute_threshold = threshold
    s.minor_loop_gain = 0.1
    s.major_loop_gain = 1.0
    s.allow_negative_components = True
    s.border_ratio = 0.0
    s.multiscale.max_scales = max_scales
    return s


def perform_costs(say, title, settings, psf, dirty, extra):
    beam = cp.BEAM_PX * cp.PIXEL_SCALE
    rows, finals = {}, {}
    for kind in ("host arrays", "device arrays"):
        for run in ("warm-up", "timed"):
            arrays = [psf.copy(), dirty.copy(), np.zeros_like(dirty)]
            if kind == "device arrays":
                arrays = [rd.gpu.to_device(a) for a in arrays]
            radler = rd.Radler(settings, *arrays, beam, **extra)
            rd.gpu.host_profile_reset()
            rd.gpu.host_profile_enable(True)
            try:
                radler.perform(0)
            finally:
                rd.gpu.host_profile_enable(False)
            profile = rd.gpu.host_profile()
            if run == "timed":
                rows[kind] = {k: profile.get(k, (0, 0.0))[1] for k in SECTIONS}
                residual = arrays[1] if kind == "host arrays" else arrays[1].numpy()
                finals[kind] = (rd.gpu.total_iteration_number(radler), residual)
            del radler, arrays
    same = (finals["host arrays"][0] == finals["device arrays"][0] and
            np.array_equal(finals["host arrays"][1].view(np.uint32),
                           finals["device arrays"][1].view(np.uint32)))
    say(f"{title}: {finals['host arrays'][0]} components; residual bits "
        f"{'identical' if same else 'DIFFER'} between the two runs")
    say(f"  {'section':<20}{'host arrays':>14}{'device arrays':>16}")
    for k in SECTIONS:
        h, d = rows["host arrays"][k], rows["device arrays"][k]
        verdict = "below" if d < h else "NOT BELOW"
        say(f"  {k:<20}{h * 1e3:>11.2f} ms{d * 1e3:>13.2f} ms   ({verdict})")
    say()


def kernel_times(say, reps):
    n = 4096 * 4096
    sess = Session(0)
    rdl = sess.rdl
    rng = np.random.default_rng(7)
    sources = [sess.array(rng.standard_normal(n).astype(np.float32)) for _ in range(8)]
    chain_dest, fused_dest = sess.array(shape=(n,)), sess.array(shape=(n,))
    say(f"rdl_average_planes against the chain, n = 4096^2, mean of {reps} runs queued back to back (host clock, one sync):")
    say(f"  {'mode':<6}{'G':>3}{'chain':>12}{'fused':>12}{'speed-up':>10}{'fused GB/s':>12}"
        f"{'of 6.29 TB/s':>14}{'  bits'}")
    for mode in (0, 1):
        for g in (1, 8):
            weights = [0.5 + 0.25 * k for k in range(g)]
            factor = 1.0 / sum(weights)
            pointers = (C.c_void_p * g)(*[s.ptr for s in sources[:g]])
            w = (C.c_double * g)(*weights)

            def chain():
                rdl.rdl_memset_zero(sess.h, chain_dest.vp, SZ(4 * n))
                for k in range(g):
                    if mode == 0:
                        rdl.rdl_axpy(sess.h, chain_dest.vp, sources[k].vp, SZ(n),
                                     C.c_float(weights[k]), 0)
                    else:
                        rdl.rdl_axpy_f64(sess.h, chain_dest.vp, sources[k].vp, SZ(n),
                                         C.c_double(weights[k]), 0)
                if mode == 0:
                    rdl.rdl_scale(sess.h, chain_dest.vp, SZ(n), C.c_float(factor))
                else:
                    rdl.rdl_axpy_f64(sess.h, chain_dest.vp, None, SZ(n), C.c_double(factor), 1)

            def fused():
                rdl.rdl_average_planes(sess.h, pointers, w, C.c_uint32(g), C.c_double(factor),
                                       mode, fused_dest.vp, SZ(n))

            times = {}
            for name, run in (("chain", chain), ("fused", fused)):
                run()
                sess.sync()
                t0 = time.perf_counter()
                for _ in range(reps):
                    run()
                sess.sync()
                times[name] = (time.perf_counter() - t0) * 1e3 / reps
            same = np.array_equal(chain_dest.get().view(np.uint32),
                                  fused_dest.get().view(np.uint32))
            rate = (g + 1) * 4.0 * n / (times["fused"] * 1e-3)
            say(f"  {mode:<6}{g:>3}{times['chain'] * 1e3:>9.1f} us{times['fused'] * 1e3:>9.1f} us"
                f"{times['chain'] / times['fused']:>9.2f}x{rate * 1e-9:>12.0f}"
                f"{100.0 * rate / COPY_ROOF:>13.1f}%  {'same' if same else 'DIFFER'}")
    say()
    sess.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-perform", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("Radler.perform over host arrays and over device arrays, and rdl_average_planes against")
    say("the kernel chain it replaces, one MI355X.")
    say()
    if not args.skip_kernel:
        kernel_times(say, args.reps)
    if not args.skip_perform:
        say(f"Host-profile sections of one perform() (multiscale, at most {args.iterations} "
            "components), after a warm-up run of each kind:")
        t0 = time.perf_counter()
        c = cp.CONFIGS["h8k"]
        psfs, dirty = cp.problem("h8k")
        print(f"[h8k generated in {time.perf_counter() - t0:.0f} s]", file=sys.stderr, flush=True)
        perform_costs(say, "h8k, 8192^2, one image",
                      multiscale_settings(c["size"], c["max_scales"], c["threshold"],
                                          args.iterations), psfs[0], dirty[0], {})
        del psfs, dirty
        c = cp.CONFIGS["c3"]
        psfs, dirty = cp.problem("c3")
        frequencies = np.array([[f, f] for f in cp.C3_FREQUENCIES], np.float64)
        perform_costs(say, "c3, 8 joined channels of 4096^2",
                      multiscale_settings(c["size"], c["max_scales"], c["threshold"],
                                          args.iterations), psfs, dirty,
                      dict(frequencies=frequencies, weights=np.ones(len(frequencies))))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
