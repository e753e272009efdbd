"""What rdl_draw_sources costs on a deep catalogue.

10^3, 10^5 and 10^6 sources drawn into one 4096^2 plane and into 4 planes:
half points, half Gaussians of FWHM 2 to 20 px (axis ratio 0.5 to 1, any
angle), numpy seed 2026. Two fields: uniform, and clustered with 90 % of the
sources inside a square of 5 % of the area. Per case, the mean of --reps calls
after a warm-up call:
  bin ms      the host's binning of the boxes into tiles (wall clock inside
              the call, timing family draw_sources_bin)
  upload ms   shapes, amplitudes and tile lists to the device (HIP events
              around the three copies, family draw_sources_upload)
  kernel ms   HIP events around the launches (family draw_sources)
  call ms     the host clock around the whole call, which waits for the device
  Gexp/s      exp evaluations (pixels of the clipped boxes, once per chunk of
              up to 4 planes) per second of kernel time
  floor ms    reading and writing every plane once at 6.3 TB/s
At 10^3 sources the same Gaussians also go through a loop of
rdl_draw_gaussian calls, one launch each, one plane at a time: the only device
path before rdl_draw_sources (wall clock around the loop and a sync).

    python tools/draw_sources_timing.py [--out FILE] [--size N] [--reps K]
"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sources_lib as L  # noqa: E402

SHAPE = np.dtype([("x0", "f8"), ("y0", "f8"), ("qa", "f8"), ("qb", "f8"), ("qc", "f8"),
                  ("half_w", "u4"), ("half_h", "u4")])
assert SHAPE.itemsize == C.sizeof(L.SourceShape)
HBM = 6.3e12  # bytes/s, a float4 copy


def catalogue(n, size, clustered, rng):
    """(shapes, (fwhm_major, fwhm_minor, pa) of the Gaussians): the first half
    points, the second half Gaussians."""
    xy = rng.uniform(0.0, size, (n, 2))
    if clustered:  # 90 % inside a square of 5 % of the area
        side = size * math.sqrt(0.05)
        k = int(0.9 * n)
        inside = rng.permutation(n)[:k]
        xy[inside] = 0.3 * size + rng.uniform(0.0, side, (k, 2))
    shapes = np.zeros(n, SHAPE)
    shapes["x0"], shapes["y0"] = xy[:, 0], xy[:, 1]
    g = np.arange(n) >= n // 2
    major = rng.uniform(2.0, 20.0, n)
    minor = major * rng.uniform(0.5, 1.0, n)
    pa = rng.uniform(-math.pi / 2, math.pi / 2, n)
    sa, sb = (major * L.FWHM_TO_SIGMA) ** 2, (minor * L.FWHM_TO_SIGMA) ** 2
    cs, sn = np.cos(pa), np.sin(pa)
    # covariance of rdl_draw_gaussian's ellipse (pa from +x towards +y), inverted
    cxx, cxy, cyy = sa * cs * cs + sb * sn * sn, (sa - sb) * cs * sn, sa * sn * sn + sb * cs * cs
    det = cxx * cyy - cxy * cxy
    shapes["qa"][g], shapes["qb"][g], shapes["qc"][g] = (cyy / det)[g], (-cxy / det)[g], (cxx / det)[g]
    half = np.ceil(6.0 * major * L.FWHM_TO_SIGMA).astype(np.uint32)
    shapes["half_w"][g] = shapes["half_h"][g] = half[g]
    return shapes, (major[g], minor[g], pa[g])


def exp_count(shapes, size):
    cx, cy = np.floor(shapes["x0"] + 0.5), np.floor(shapes["y0"] + 0.5)
    w = np.minimum(cx + shapes["half_w"], size - 1) - np.maximum(cx - shapes["half_w"], 0) + 1
    h = np.minimum(cy + shapes["half_h"], size - 1) - np.maximum(cy - shapes["half_h"], 0) + 1
    return float(np.sum(np.maximum(w, 0) * np.maximum(h, 0)))


def family(sess, name):
    ms, k, b = C.c_double(), C.c_uint64(), C.c_double()
    sess.rdl.rdl_timing_get(sess.h, name.encode(), C.byref(ms), C.byref(k), C.byref(b))
    return ms.value, k.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    size, reps = args.size, args.reps
    sess = L.Session()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def draw(shapes, amplitudes, planes, n_planes):
        sess.rdl.rdl_draw_sources(sess.h, C.c_uint32(len(shapes)),
                                  shapes.ctypes.data_as(C.c_void_p),
                                  amplitudes.ctypes.data_as(C.c_void_p), C.c_uint32(n_planes),
                                  C.c_uint32(size), C.c_uint32(size), planes.vp,
                                  C.c_size_t(size * size))

    say(f"# rdl_draw_sources, {size}^2 planes, half points and half Gaussians of FWHM 2-20 px; "
        f"mean of {reps} calls after a warm-up call; HIP-event timing on")
    say(f"{'sources':>8s} {'planes':>6s} {'field':>9s} {'bin ms':>9s} {'upload ms':>10s} "
        f"{'kernel ms':>10s} {'call ms':>9s} {'Gexp/s':>8s} {'floor ms':>9s} {'longest list':>13s}")
    kernel_ms = {}
    for n in (1000, 100000, 1000000):
        for clustered in (False, True):
            rng = np.random.default_rng(2026)
            shapes, ellipses = catalogue(n, size, clustered, rng)
            exps = exp_count(shapes, size)
            # the longest tile list, as the host bins it (64 x 16 tiles): the skew
            tiles = np.zeros(((size + 15) // 16, (size + 63) // 64), np.int64)
            cx, cy = np.floor(shapes["x0"] + 0.5), np.floor(shapes["y0"] + 0.5)
            x0 = np.maximum(cx - shapes["half_w"], 0).astype(np.int64) // 64
            x1 = np.minimum(cx + shapes["half_w"], size - 1).astype(np.int64) // 64
            y0 = np.maximum(cy - shapes["half_h"], 0).astype(np.int64) // 16
            y1 = np.minimum(cy + shapes["half_h"], size - 1).astype(np.int64) // 16
            ok = (x0 <= x1) & (y0 <= y1)
            for dy in range(int(np.max(y1 - y0)) + 1):
                for dx in range(int(np.max(x1 - x0)) + 1):
                    m = ok & (y0 + dy <= y1) & (x0 + dx <= x1)
                    np.add.at(tiles, (y0[m] + dy, x0[m] + dx), 1)
            for n_planes in (1, 4):
                amplitudes = rng.uniform(0.1, 1.0, (n_planes, n)).astype(np.float32)
                planes = sess.array(shape=(n_planes, size, size))
                draw(shapes, amplitudes, planes, n_planes)  # warm-up
                sess.sync()
                sess.rdl.rdl_timing_enable(sess.h, 1)
                sess.rdl.rdl_timing_reset(sess.h)
                t0 = time.perf_counter()
                for _ in range(reps):
                    draw(shapes, amplitudes, planes, n_planes)
                sess.sync()
                call = (time.perf_counter() - t0) * 1e3 / reps
                bin_ms = family(sess, "draw_sources_bin")[0] / reps
                upload = family(sess, "draw_sources_upload")[0] / reps
                kernel = family(sess, "draw_sources")[0] / reps
                sess.rdl.rdl_timing_enable(sess.h, 0)
                kernel_ms[(n, n_planes, clustered)] = kernel
                floor = 2.0 * 4.0 * size * size * n_planes / HBM * 1e3
                say(f"{n:8d} {n_planes:6d} {'clustered' if clustered else 'uniform':>9s} "
                    f"{bin_ms:9.3f} {upload:10.3f} {kernel:10.3f} {call:9.3f} "
                    f"{exps / (kernel * 1e-3) / 1e9:8.2f} {floor:9.3f} {int(tiles.max()):13d}")
                if n == 1000:
                    major, minor, pa = ellipses
                    gx, gy = shapes["x0"][n // 2:], shapes["y0"][n // 2:]

                    def loop():
                        for g in range(n_planes):
                            plane = planes.offset(g * size * size * 4)
                            for i in range(len(major)):
                                sess.rdl.rdl_draw_gaussian(
                                    sess.h, plane, C.c_uint32(size), C.c_uint32(size),
                                    C.c_double(gx[i]), C.c_double(gy[i]), C.c_double(major[i]),
                                    C.c_double(minor[i]), C.c_double(pa[i]),
                                    C.c_double(float(amplitudes[g, n // 2 + i])))
                        sess.sync()
                    loop()  # warm-up
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        loop()
                    loop_ms = (time.perf_counter() - t0) * 1e3 / reps
                    say(f"#   the same {len(major)} Gaussians by a loop of {len(major) * n_planes} "
                        f"rdl_draw_gaussian calls: {loop_ms:.3f} ms (ctypes calls included); "
                        f"rdl_draw_sources' whole call {call:.3f} ms")
                planes.free()
    for n in (1000, 100000, 1000000):
        for n_planes in (1, 4):
            ratio = kernel_ms[(n, n_planes, True)] / kernel_ms[(n, n_planes, False)]
            say(f"# clustered / uniform kernel time, {n} sources, {n_planes} planes: {ratio:.2f}")
    sess.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
