"""Runs a peak-search Group of tests/boxed_cases.py on the device, between
sentinel guards; and, as a program, the two-launch form of the search:

    RDL_PEAK_FINISH=0 python tests/boxed_peak_child.py RESULTS.npy

RDL_PEAK_FINISH is read once per process, so the separate FindPeakFinal launch
needs a process of its own: tests/test_boxed_primitives_gpu.py starts this one
with the variable set, and compares RESULTS.npy (one row of found, x, y, value
bits for every query of boxed_cases.representative_subset) with what the same
calls gave in the pytest process.
"""
import ctypes as C
import sys

import numpy as np

import boxed_cases as B
from rdl_lib import Peak, Session
from test_primitives_gpu import Guarded, sentinel

F = np.float32
U32 = C.c_uint32


class DeviceGroup:
    """A Group's image and mask on the device, each between guards; the bytes
    that misalign a pointer are sentinel too."""

    def __init__(self, sess, g):
        self.g = g
        self.img = Guarded(sess, np.concatenate([sentinel(g.img_off, F), g.img.ravel()]))
        assert self.img.vp.value % 16 == 0
        self.mask = None
        if g.mask is not None:
            self.mask = Guarded(sess, np.concatenate([sentinel(g.mask_off, np.uint8),
                                                      g.mask.ravel()]))
            assert self.mask.vp.value % 16 == 0

    def args(self, q):
        """The arguments of rdl_find_peak / _enqueue between the session and
        the result."""
        h, w = self.g.img.shape
        mask = self.mask.at(self.g.mask_off) if self.mask is not None and q.masked else None
        return (self.img.at(self.g.img_off), U32(w), U32(h), U32(q.start_y), U32(q.end_y),
                U32(q.hb), U32(q.vb), int(q.allow_negative), mask, int(q.avx))

    def find(self, sess, q):
        """rdl_find_peak -> (found, x, y, value bits)."""
        p = Peak()
        sess.rdl.rdl_find_peak(sess.h, *self.args(q), C.byref(p))
        return peak_tuple(np.frombuffer(p, np.uint32))

    def close(self):
        """Checks the guards and frees."""
        self.img.get()
        self.img.free()
        if self.mask is not None:
            self.mask.get()
            self.mask.free()


def peak_tuple(words):
    """An rdl_peak as four 32-bit words (value, x, y, found)."""
    return (int(np.int32(words[3])), int(words[1]), int(words[2]), int(words[0]))


def run_groups(sess, groups):
    """Every query of every group -> an (n, 4) array of found, x, y, bits."""
    rows = []
    for g in groups:
        dev = DeviceGroup(sess, g)
        rows += [dev.find(sess, q) for q in g.queries]
        dev.close()
    return np.array(rows, np.int64)


if __name__ == "__main__":
    session = Session(0)
    np.save(sys.argv[1], run_groups(session, B.representative_subset()))
    session.close()
