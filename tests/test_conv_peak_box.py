"""rdl::MakePeakBox (csrc/hip/conv_peak_box.h), the search box of the peak
searches fused into the inverse row pass, against its closed form:

    xs = hb,  xe = w - hb if hb <= w and w - hb > hb else hb   (y alike)

which is the box of rdl_find_peak(start_y 0, end_y h) (peak_finder.cc:27-32)
for every border that fits the image and an empty box (xe == xs) beyond. The
row kernels form xe - xs in unsigned arithmetic, so xs <= xe must hold for
every input, a border wider than the image included.

The function replaced two hand-written copies, transcribed below in 32-bit
unsigned arithmetic as they stood: that of rdl_conv_convolve_subtract_peak
(clamp, clamp, re-clamp), which it equals for every input, and that of
rdl_conv_rows_inverse_peak (no re-clamp), which it equals wherever the
borders fit the image (hb <= w, vb <= h).

tests/conv_peak_box_dump.cc prints the box for w, h in 0..6 and (64, 48),
borders 0..side+2 and 0xffffffff.
"""
import os
import subprocess

from test_subminor_plan import _host_build

HERE = os.path.dirname(os.path.abspath(__file__))
U32 = 0xffffffff


def _end(n, border):
    return n - border if border <= n and n - border > border else border


def _old_convolve_subtract_peak(w, h, hb, vb):
    xs, xe = hb, (w - hb) & U32
    ys = vb
    ye = h if h < ((h - vb) & U32) else (h - vb) & U32
    if xe < xs:
        xe = xs
    if ye < ys:
        ye = ys
    if xe > w:
        xe = w
    if ye > h:
        ye = h
    if xe < xs:
        xe = xs
    if ye < ys:
        ye = ys
    return xs, xe, ys, ye


def _old_rows_inverse_peak(w, h, hb, vb):
    xs, xe = hb, (w - hb) & U32
    ys, ye = vb, (h - vb) & U32
    if xe < xs:
        xe = xs
    if ye < ys:
        ye = ys
    if xe > w:
        xe = w
    if ye > h:
        ye = h
    return xs, xe, ys, ye


def test_peak_box_is_the_closed_form(tmp_path):
    b = _host_build()
    exe = str(tmp_path / "conv_peak_box_dump")
    subprocess.run([b.CXX, *b.CXX_FLAGS, os.path.join(HERE, "conv_peak_box_dump.cc"), "-o", exe],
                   check=True)
    text = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = [tuple(int(v) for v in line.split()) for line in text.splitlines()]
    sizes = [(w, h) for w in range(7) for h in range(7)] + [(64, 48)]
    expect = [(w, h, hb, vb)
              for w, h in sizes
              for hb in [*range(w + 3), U32]
              for vb in [*range(h + 3), U32]]
    assert [r[:4] for r in rows] == expect
    n_fit = 0
    for w, h, hb, vb, xs, xe, ys, ye in rows:
        box = (xs, xe, ys, ye)
        assert box == (hb, _end(w, hb), vb, _end(h, vb)), (w, h, hb, vb)
        assert xs <= xe and ys <= ye, (w, h, hb, vb)
        assert box == _old_convolve_subtract_peak(w, h, hb, vb), (w, h, hb, vb)
        if hb <= w and vb <= h:
            n_fit += 1
            assert box == _old_rows_inverse_peak(w, h, hb, vb), (w, h, hb, vb)
    assert 0 < n_fit < len(rows)
