"""DeconvolutionAlgorithm::PeakBorders (csrc/host/clean_border.h), the border
the peak searches and the sub-minor loops leave out at each side of an image,
against its closed form

    border = max(round(size * ratio), ceil(scale * 0.5))

with the product formed in float32 and rounded half away from zero
(std::round, not Python's round-half-to-even), and scale * 0.5 in float64.

The function replaced fourteen spellings in two cast orders, transcribed
below as they stood: uint32(round(size * ratio)) where no scale takes part,
and uint32(max(size_t(round(size * ratio)), size_t(ceil(scale * 0.5)))) where
one does. The two agree with each other at scale 0 and with the function for
every input here.

tests/clean_border_dump.cc prints the borders for widths and heights of 1, 2,
3, 64, 100, 1000 and 8192 in every pairing, six ratios and six scales.
"""
import math
import os
import subprocess

import numpy as np

from test_subminor_plan import _host_build

HERE = os.path.dirname(os.path.abspath(__file__))
SIDES = [1, 2, 3, 64, 100, 1000, 8192]
RATIOS = [0.0, 0.01, 0.05, 0.125, 0.25, 0.5]
SCALES = [0.0, 1.0, 4.5, 5.0, 37.2, 300.0]
U32 = 0xffffffff


def _round_half_away(x):
    """std::round of a non-negative float32, exact in float64."""
    return math.floor(float(x) + 0.5)


def _product(size, ratio):
    return np.float32(size) * np.float32(ratio)  # size_t * float: a float product


def _closed_form(size, ratio, scale):
    half_scale = math.ceil(float(np.float32(scale)) * 0.5)
    return max(_round_half_away(_product(size, ratio)), half_scale)


def _old_without_scale(size, ratio):
    return int(_round_half_away(_product(size, ratio))) & U32  # uint32_t(std::round(..))


def _old_with_scale(size, ratio, scale):
    border = int(_round_half_away(_product(size, ratio)))      # size_t(std::round(..))
    border_scale = int(math.ceil(float(np.float32(scale)) * 0.5))  # size_t(std::ceil(..))
    return max(border, border_scale) & U32                      # uint32_t(std::max<size_t>(..))


def test_borders_are_the_closed_form(tmp_path):
    assert _round_half_away(np.float32(0.5)) == 1 and round(0.5) == 0
    assert _round_half_away(np.float32(2.5)) == 3 and round(2.5) == 2
    b = _host_build()
    exe = str(tmp_path / "clean_border_dump")
    subprocess.run([b.CXX, *b.CXX_FLAGS, os.path.join(HERE, "clean_border_dump.cc"), "-o", exe],
                   check=True)
    text = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = [tuple(int(v) for v in line.split()) for line in text.splitlines()]
    expect = [(w, h, r, s) for w in SIDES for h in SIDES
              for r in range(len(RATIOS)) for s in range(len(SCALES))]
    assert [row[:4] for row in rows] == expect
    n_half, n_scale_wins = 0, 0
    for w, h, r, s, horizontal, vertical in rows:
        ratio, scale = RATIOS[r], SCALES[s]
        for size, border in ((w, horizontal), (h, vertical)):
            where = (size, ratio, scale)
            assert border == _closed_form(size, ratio, scale), where
            assert border == _old_with_scale(size, ratio, scale), where
            if scale == 0.0:
                assert border == _old_without_scale(size, ratio), where
            frac = float(_product(size, ratio)) % 1.0
            n_half += frac == 0.5
            n_scale_wins += border > _old_without_scale(size, ratio)
    # the inputs reach a product that ends in .5 (100 * 0.125 = 12.5 -> 13, where
    # Python's round gives 12) and borders that the scale decides
    assert n_half > 0 and n_scale_wins > 0
    assert _closed_form(100, 0.125, 0.0) == 13 and _closed_form(2, 0.25, 0.0) == 1
    assert _closed_form(64, 0.05, 37.2) == 19 and _closed_form(64, 0.05, 4.5) == 3
