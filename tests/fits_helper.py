"""FITS files written with numpy alone, for the tests of the product's own
reader (csrc/host/fits_image.cc): 80-byte cards, big-endian data, 2880-byte
blocks."""
import numpy as np

BLOCK = 2880


def card(key, value=None, quote=False):
    if value is None:
        text = key
    elif quote:
        text = f"{key:<8}= '{value:<8}'"
    elif isinstance(value, bool):
        text = f"{key:<8}= {'T' if value else 'F':>20}"
    else:
        text = f"{key:<8}= {value!r:>20}" if isinstance(value, float) else \
            f"{key:<8}= {value:>20}"
    assert len(text) <= 80
    return text.ljust(80).encode("ascii")


def header_bytes(cards, end=True):
    raw = b"".join(cards) + (card("END") if end else b"")
    return raw + b" " * (-len(raw) % BLOCK)


def fits_bytes(data, bitpix=-32, ctypes=None, bscale=None, bzero=None):
    """The file for `data` (numpy axes slowest first: data[..., y, x]) stored
    as `bitpix`; for integer BITPIX the values stored are round((data - bzero)
    / bscale). Returns (bytes, the float32 planes a reader must give)."""
    data = np.asarray(data)
    dtype = {8: ">u1", 16: ">i2", 32: ">i4", -32: ">f4", -64: ">f8"}[bitpix]
    if bitpix > 0:
        stored = np.round((data.astype(np.float64) - (bzero or 0.0)) / (bscale or 1.0))
    else:
        stored = data
    stored = stored.astype(dtype)
    cards = [card("SIMPLE", True), card("BITPIX", bitpix), card("NAXIS", data.ndim)]
    for i, n in enumerate(reversed(data.shape)):
        cards.append(card(f"NAXIS{i + 1}", n))
    if bscale is not None:
        cards.append(card("BSCALE", float(bscale)))
    if bzero is not None:
        cards.append(card("BZERO", float(bzero)))
    for i, name in enumerate(ctypes or []):
        cards.append(card(f"CTYPE{i + 1}", name, quote=True))
    cards.append(card("COMMENT written by the test suite"))
    raw = stored.tobytes()
    expect = stored.astype(np.float64)
    if bscale is not None or bzero is not None:
        expect = (bzero or 0.0) + (bscale or 1.0) * expect
    h, w = data.shape[-2:]
    return (header_bytes(cards) + raw + b"\0" * (-len(raw) % BLOCK),
            expect.astype(np.float32).reshape(-1, h, w))


def write_fits(path, data, **kw):
    raw, expect = fits_bytes(data, **kw)
    with open(path, "wb") as f:
        f.write(raw)
    return expect
