"""Components per second of rdl_hogbom_batch_run against the loop it replaces
(profiles/hogbom_batch_timing.txt).

For planes of 64^2, 128^2, 256^2 and 512^2 and B = 1, 16, 256 and 1024 planes:
the batch call over the whole stack, and beside it a loop of rdl_find_peak +
rdl_hogbom_run over the same planes in the same process (the only way without
the batch call; that code is unchanged). Both work on stacks that are already
in device memory, so neither side pays an upload. Every plane takes the same
number of components (threshold 0, a cap of --components), shared PSF, no
mask. One more row times a single 1024^2 plane, the largest the batch call
takes: its time per component sets the default chunk of clean_batch.hip.

Method: a host clock around calls that end in a stream synchronise (both
entry points do). Each (size, B) cell: the stacks are uploaded afresh before
every run, one warm-up run of each side, then --reps timed runs of each side,
alternating; the table gives the median and the spread (max / min) of each
side. After the last pair the residual and model stacks of both sides are
compared bit for bit.

    python tools/hogbom_batch_timing.py [--out FILE] [--components K] [--reps K] [--quick]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hogbom_batch_lib import (BatchOut, BatchParams, HogbomParams, HogbomResult,  # noqa: E402
                              first_threshold, make_planes, make_psf)
from rdl_lib import Session, integration  # noqa: E402

DISTINCT = 16  # distinct planes of a stack; the rest repeat them


class Problem:
    def __init__(self, sess, size, n_planes, components):
        self.sess, self.size, self.n_planes, self.components = sess, size, n_planes, components
        base = make_planes(size, size, min(n_planes, DISTINCT), seed=size)
        self.residuals = np.ascontiguousarray(
            np.tile(base, (-(-n_planes // len(base)), 1, 1))[:n_planes])
        self.n = size * size
        self.d_res = sess.array(self.residuals)
        self.d_mod = sess.array(shape=self.residuals.shape)
        self.d_psf = sess.array(make_psf(size, size))

    def reset(self):
        self.d_res.upload(self.residuals)
        self.sess.rdl.rdl_memset_zero(self.sess.h, self.d_mod.vp, C.c_size_t(self.d_mod.nbytes))
        self.sess.sync()

    def free(self):
        for a in (self.d_res, self.d_mod, self.d_psf):
            a.free()

    def batch(self):
        p = BatchParams()
        p.width = p.height = self.size
        p.n_planes = self.n_planes
        p.d_residuals, p.residual_stride = self.d_res.ptr, self.n
        p.d_models, p.model_stride = self.d_mod.ptr, self.n
        p.d_psfs, p.psf_stride = self.d_psf.ptr, 0
        p.gain, p.major_loop_gain, p.divergence_limit, p.allow_negative = 0.1, 1.0, 0.0, 1
        b = self.n_planes
        thr, it0 = np.zeros(b, np.float32), np.zeros(b, np.uint64)
        cap, act = np.full(b, self.components, np.uint64), np.ones(b, np.uint8)
        out = (BatchOut * b)()
        t0 = time.perf_counter()
        self.sess.rdl.rdl_hogbom_batch_run(
            self.sess.h, C.byref(p), thr.ctypes.data_as(C.c_void_p),
            it0.ctypes.data_as(C.c_void_p), cap.ctypes.data_as(C.c_void_p),
            act.ctypes.data_as(C.c_void_p), out, None, C.c_uint64(0))
        dt = time.perf_counter() - t0
        assert all(o.result.iteration == self.components for o in out)
        return dt

    def loop(self):
        sess, size = self.sess, self.size
        plane_bytes = self.n * 4
        p = HogbomParams()
        p.width = p.height = size
        p.n_images = p.n_pol = 1
        p.integ = integration(1, 1, None, 1.0, mode=1)
        p.gain, p.divergence_limit, p.allow_negative = 0.1, 0.0, 1
        p.max_iterations = self.components
        r = HogbomResult()
        view = types_view(self.d_res)
        t0 = time.perf_counter()
        for b in range(self.n_planes):
            view.ptr = self.d_res.ptr + b * plane_bytes
            found, x, y, value = sess.find_peak(view, size, size, True)
            p.threshold = first_threshold(0.0, value, 1.0)
            p.initial_max = abs(np.float32(value))
            p.start_x, p.start_y, p.start_value, p.start_found = x, y, value, int(found)
            sess.rdl.rdl_hogbom_run(sess.h, C.c_void_p(view.ptr),
                                    C.c_void_p(self.d_mod.ptr + b * plane_bytes),
                                    self.d_psf.vp, C.byref(p), C.byref(r), None, C.c_uint64(0))
            assert r.iteration == self.components
        return time.perf_counter() - t0

    def bits(self):
        return self.d_res.get().view(np.uint32), self.d_mod.get().view(np.uint32)


class types_view:
    """A plane inside a stack, for Session.find_peak (which reads .vp)."""

    def __init__(self, array):
        self.ptr = array.ptr

    @property
    def vp(self):
        return C.c_void_p(self.ptr)


def measure(problem, reps):
    times = {"batch": [], "loop": []}
    for name in ("batch", "loop"):  # warm-up
        problem.reset()
        getattr(problem, name)()
    finals = {}
    for _ in range(reps):
        for name in ("batch", "loop"):
            problem.reset()
            times[name].append(getattr(problem, name)())
            finals[name] = problem.bits()
    same = all(np.array_equal(a, b) for a, b in zip(finals["batch"], finals["loop"]))
    return times, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hogbom_batch_timing.txt"))
    ap.add_argument("--components", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="64^2 and 128^2, B up to 16 (rehearsal)")
    args = ap.parse_args()
    sizes, counts = ([64, 128], [1, 16]) if args.quick else ([64, 128, 256, 512],
                                                             [1, 16, 256, 1024])
    cells = [(s, b) for s in sizes for b in counts] + ([] if args.quick else [(1024, 1)])
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    sess = Session(0)
    say("rdl_hogbom_batch_run against a loop of rdl_find_peak + rdl_hogbom_run")
    say(f"{args.components} components per plane, shared PSF, no mask, stacks in device memory;")
    say(f"host clock around synchronising calls, median of {args.reps} alternating runs "
        "after one warm-up of each")
    say()
    say(f"{'plane':>9} {'B':>5} | {'batch ms':>9} {'spread':>6} {'comp/s':>10} {'us/comp/plane':>13} | "
        f"{'loop ms':>9} {'spread':>6} {'comp/s':>10} | {'batch/loop':>10} {'bits':>5}")
    for size, n_planes in cells:
        problem = Problem(sess, size, n_planes, args.components)
        try:
            times, same = measure(problem, args.reps)
        finally:
            problem.free()
        total = n_planes * args.components
        tb, tl = np.median(times["batch"]), np.median(times["loop"])
        say(f"{size:>4}^2 {n_planes:>7} | {tb * 1e3:>9.2f} {max(times['batch']) / min(times['batch']):>6.2f} "
            f"{total / tb:>10.0f} {tb / args.components * 1e6:>13.2f} | "
            f"{tl * 1e3:>9.2f} {max(times['loop']) / min(times['loop']):>6.2f} {total / tl:>10.0f} | "
            f"{tl / tb:>9.2f}x {'same' if same else 'DIFF':>5}")
    say()
    say("us/comp/plane: batch time over the components of one plane (the planes run side by")
    say("side); for B = 1 it is the time one workgroup takes per component.")
    sess.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
