"""Cases and plain NumPy references for the boxed primitives: the peak search
(rdl_find_peak*), the PSF subtraction (rdl_subtract_psf) and the image-set
integration (rdl_integrate).

tests/test_boxed_primitives_gpu.py runs every case on the device;
tests/test_boxed_cases.py runs the same cases through the models below and
through models that are wrong on purpose (`mutant=`), to show that the cases
can fail. Nothing here touches the device.

A peak case is a Group: one image (and perhaps a mask), the way its pointers
are to be misaligned, and the Queries to ask of it. A Query's `expect` is the
answer fixed by how the image was made, (found, x, y, value bits), or None
where the oracle alone decides.
"""
import numpy as np

F = np.float32
FLT_MIN = np.finfo(F).tiny                  # 2^-126: not a peak (strict '>')
ABOVE_MIN = np.nextafter(FLT_MIN, F(1))     # the smallest peak
BIG = F(1e6)                                # well below the guards' 6e18
TARGET_BLOCKS = 2048                        # LaunchFindPeak (peak.hip)
PEAK_SLOTS = 64                             # RDL_PEAK_SLOTS
NAN_BITS = 0x7FC00123


def bits(v):
    return int(np.asarray(v, F).reshape(1).view(np.uint32)[0])


def payload_nan():
    return np.array([NAN_BITS], np.uint32).view(F)[0]


class Query:
    def __init__(self, start_y, end_y, hb, vb, allow_negative, avx, expect=None, masked=True,
                 oracle=True):
        self.start_y, self.end_y, self.hb, self.vb = start_y, end_y, hb, vb
        self.allow_negative, self.avx = bool(allow_negative), bool(avx)
        self.expect, self.masked, self.oracle = expect, masked, oracle

    def __repr__(self):
        return (f"Query(y {self.start_y}..{self.end_y}, border {self.hb}/{self.vb}, "
                f"neg={self.allow_negative}, avx={self.avx}, masked={self.masked})")


class Group:
    def __init__(self, name, img, queries, mask=None, img_off=0, mask_off=0):
        self.name, self.img, self.queries = name, np.array(img, F), queries      # copies
        self.mask = None if mask is None else np.array(mask, np.uint8)
        self.img_off, self.mask_off = img_off, mask_off     # floats / bytes off 16-byte alignment

    def mask_of(self, q):
        return self.mask if q.masked else None


# ------------------------------------------------------------- the peak model
def box(w, h, start_y, end_y, hb, vb):
    """peak_finder.cc:27-32 in plain integers: borders beyond the image leave
    an empty box (the reference's unsigned bounds wrap there)."""
    xs, xe = hb, max(w - hb, hb)
    ys = max(start_y, vb)
    ye = max(min(end_y, h - vb), ys)
    return min(xs, w), min(xe, w), min(ys, h), min(ye, h)


def nothing_found(img, mask, avx):
    """peak_finder.cc:202,250-252: the AVX search without a mask reports
    pixel 0; FindWithMask and the simple search report (width, height)."""
    h, w = img.shape
    if avx and mask is None:
        return (1, 0, 0, bits(img[0, 0]))
    return (0, w, h, 0)


BOX_MUTANTS = {"left wider": (-1, 0, 0, 0), "left narrower": (1, 0, 0, 0),
               "right wider": (0, 1, 0, 0), "right narrower": (0, -1, 0, 0),
               "top wider": (0, 0, -1, 0), "top narrower": (0, 0, 1, 0),
               "bottom wider": (0, 0, 0, 1), "bottom narrower": (0, 0, 0, -1)}
PEAK_MUTANTS = list(BOX_MUTANTS) + [
    "end_y ignored", "start_y ignored", ">= FLT_MIN", "last index on ties", "NaN qualifies",
    "-Inf does not qualify", "last row of a block dropped (2)", "last row of a block dropped (3)",
    "mask read one byte on"]


def find_peak(img, q, mask=None, mutant=None):
    """(found, x, y, value bits) of the search `q` over `img`."""
    h, w = img.shape
    start_y = 0 if mutant == "start_y ignored" else q.start_y
    end_y = h if mutant == "end_y ignored" else q.end_y
    xs, xe, ys, ye = box(w, h, start_y, end_y, q.hb, q.vb)
    if mutant in BOX_MUTANTS and xs < xe and ys < ye:
        d = BOX_MUTANTS[mutant]
        xs, xe = min(max(xs + d[0], 0), w), min(max(xe + d[1], 0), w)
        ys, ye = min(max(ys + d[2], 0), h), min(max(ye + d[3], 0), h)
    if xs < xe and ys < ye:
        sub = img[ys:ye, xs:xe]
        key = np.abs(sub) if q.allow_negative else sub.copy()
        with np.errstate(invalid="ignore"):
            ok = key >= FLT_MIN if mutant == ">= FLT_MIN" else key > FLT_MIN
        if mutant == "NaN qualifies":
            ok = ok | np.isnan(sub)
            key = np.where(np.isnan(sub), F(np.inf), key)
        if mutant == "-Inf does not qualify":
            ok = ok & ~np.isneginf(sub)
        if mask is not None:
            m = mask.ravel()
            if mutant == "mask read one byte on":
                m = np.concatenate([m[1:], [1]]).astype(np.uint8)
            ok = ok & (m.reshape(h, w)[ys:ye, xs:xe] != 0)
        if mutant and mutant.startswith("last row of a block dropped"):
            rpb = -(-(ye - ys) // TARGET_BLOCKS)
            if rpb == int(mutant[-2]):
                ok = ok.copy()
                for y0 in range(ys, ye, rpb):
                    ok[min(ye, y0 + rpb) - 1 - ys] = False
        if ok.any():
            k = np.where(ok, key, F(-1)).ravel()
            i = int(np.argmax(k))
            if mutant == "last index on ties":
                i = k.size - 1 - int(np.argmax(k[::-1]))
            y, x = ys + i // (xe - xs), xs + i % (xe - xs)
            return (1, x, y, bits(img[y, x]))
    return nothing_found(img, mask, q.avx)


def same_peak(got, want):
    """found, x, y and the value's bits; two NaNs count as equal. The value of
    a search that found nothing is not compared."""
    if tuple(got[:3]) != tuple(want[:3]):
        return False
    if not want[0]:
        return True
    a, b = np.array([got[3], want[3]], np.uint32).view(F)
    return got[3] == want[3] or (np.isnan(a) and np.isnan(b))


# --------------------------------------------------------- planted box edges
def noise(w, h, seed):
    return np.random.default_rng(seed).uniform(-0.9, 0.9, (h, w)).astype(F)


def box_positions(xs, xe, ys, ye):
    """The four corners and four edge midpoints of a box, without repeats."""
    xm, ym = (xs + xe - 1) // 2, (ys + ye - 1) // 2
    out = []
    for p in [(xs, ys), (xm, ys), (xe - 1, ys), (xs, ym), (xe - 1, ym),
              (xs, ye - 1), (xm, ye - 1), (xe - 1, ye - 1)]:
        if p not in out:
            out.append(p)
    return out


def other_pixel(xs, xe, ys, ye, px, py):
    """A box pixel that is not (px, py): the opposite one, else any other."""
    cand = [(xs + xe - 1 - px, ys + ye - 1 - py), (xs, ys), (xe - 1, ye - 1)]
    for c in cand:
        if c != (px, py):
            return c
    return None


def planted(name, w, h, start_y, end_y, hb, vb, mask_kind=None, img_off=0, mask_off=0):
    """BIG on each corner and edge midpoint of the box, 2 * BIG on the four
    pixels just outside the box on its row and column, 1.0 on another box
    pixel (the runner-up) and noise of |v| <= 0.9 elsewhere; then the same with
    every planted sign reversed. mask_kind: None, "ones", "hide" (zero exactly
    at the planted maximum: the runner-up wins) or "only" (zero everywhere but
    at the planted maximum)."""
    xs, xe, ys, ye = box(w, h, start_y, end_y, hb, vb)
    assert xs < xe and ys < ye
    base = noise(w, h, w * 131 + h * 7 + hb * 3 + vb)
    for n_pos, (px, py) in enumerate(box_positions(xs, xe, ys, ye)):
        runner = other_pixel(xs, xe, ys, ye, px, py)
        for sign in (1, -1):
            img = base.copy()
            if runner is not None:
                img[runner[1], runner[0]] = 1.0
            img[py, px] = sign * BIG
            for ox, oy in ((xs - 1, py), (xe, py), (px, ys - 1), (px, ye)):
                if 0 <= ox < w and 0 <= oy < h:
                    img[oy, ox] = sign * 2 * BIG
            mask = None
            if mask_kind == "ones":
                mask = np.ones((h, w), np.uint8)
            elif mask_kind == "hide":
                mask = np.ones((h, w), np.uint8)
                mask[py, px] = 0
            elif mask_kind == "only":
                mask = np.zeros((h, w), np.uint8)
                mask[py, px] = 1
            queries = []
            for allow_negative in (True, False):
                avx = (n_pos + allow_negative) % 2 == 0
                plant_visible = mask_kind != "hide" and (sign > 0 or allow_negative)
                runner_visible = runner is not None and mask_kind != "only"
                if plant_visible:
                    expect = (1, px, py, bits(sign * BIG))
                elif runner_visible:
                    expect = (1, runner[0], runner[1], bits(1.0))
                else:           # all else is masked, or the box is its one pixel
                    expect = nothing_found(img, mask, avx)
                queries.append(Query(start_y, end_y, hb, vb, allow_negative, avx, expect))
            yield Group(f"{name} {w}x{h} box x {xs}..{xe} y {ys}..{ye} at ({px},{py}) sign {sign}"
                        f" mask {mask_kind}", img, queries, mask, img_off, mask_off)


H_PLANT = 7
# (start_y, end_y, v_border): the border decides both limits; start_y / end_y
# decide both; one each way, both ways round
Y_VARIANTS = [(0, 7, 2), (3, 5, 1), (2, 7, 1), (0, 4, 2)]
ONE_ROW = [(3, 4, 0), (0, 7, 3)]
VECTOR_WIDTHS = [8, 64, 1028, 2052]     # 1028 / 4 = 257 and 2052 / 4 = 513 float4 a row: the
                                        # 256-thread loop takes a second / third, partial trip


def planted_vector():
    """Aligned, width % 4 == 0: h_border 0..3 puts xs % 4 and xe % 4 through
    every residue; boxes 2 and 4 pixels wide (width - 2 * h_border is even on
    this path) and one-row boxes."""
    for wi, w in enumerate(VECTOR_WIDTHS):
        for hb in range(4):
            yield from planted("vector", w, H_PLANT, *Y_VARIANTS[(wi + hb) % 4][:2], hb,
                               Y_VARIANTS[(wi + hb) % 4][2])
    yield from planted("vector narrow", 8, H_PLANT, *ONE_ROW[0][:2], 3, ONE_ROW[0][2])     # 2 wide
    yield from planted("vector narrow", 64, H_PLANT, *ONE_ROW[1][:2], 30, ONE_ROW[1][2])   # 4 wide
    yield from planted("vector narrow", 64, H_PLANT, *Y_VARIANTS[1][:2], 31, Y_VARIANTS[1][2])
    yield from planted("vector narrow", 2052, H_PLANT, *ONE_ROW[0][:2], 1024, ONE_ROW[0][2])


def planted_scalar():
    """The scalar kernel, reached three ways: width % 4 != 0 (257 and 513: a
    thread's loop takes a second / third trip; boxes 1, 3 and 5 wide), the
    image 4 bytes off, the mask 1, 2 and 3 bytes off."""
    for w, borders in ((5, (0, 1, 2)), (257, (0, 126, 127, 128)), (513, (0, 1, 254))):
        for i, hb in enumerate(borders):
            sy, ey, vb = (Y_VARIANTS + ONE_ROW)[(i + w) % 6]
            yield from planted("scalar width", w, H_PLANT, sy, ey, hb, vb)
    for w, hb in ((8, 1), (1028, 2)):
        yield from planted("scalar image + 4 bytes", w, H_PLANT, *Y_VARIANTS[2][:2], hb,
                           Y_VARIANTS[2][2], img_off=1)
    for w, off in ((8, 1), (1028, 2), (64, 3)):
        yield from planted("scalar mask off", w, H_PLANT, *Y_VARIANTS[0][:2], 1,
                           Y_VARIANTS[0][2], mask_kind="hide", mask_off=off)


def planted_masked():
    for kind in ("ones", "hide", "only"):
        for i, w in enumerate(VECTOR_WIDTHS + [257]):
            sy, ey, vb = Y_VARIANTS[i % 4]
            yield from planted("masked", w, H_PLANT, sy, ey, 1 + i % 3, vb, mask_kind=kind)


# ------------------------------------------------------- rows to workgroups
def rows_cases():
    """Box rows 2048 / 2049 / 4097 (rows_per_block 1 / 2 / 3; 2048 / 1025 /
    1366 blocks, the last holding 1 / 1 / 2 rows) of width 8 (vector) and 5
    (scalar), through the border and through start_y / end_y. The maximum on
    the first and on the last row of a block and on the last row of the box,
    2 * BIG one row before and one row past the box; then equal maxima in two
    blocks and inside one float4 (the lower index wins)."""
    for w in (8, 5):
        for rows in (2048, 2049, 4097):
            rpb = -(-rows // TARGET_BLOCKS)
            for through_border in (True, False):
                if through_border:
                    h, sy, ey, vb = rows + 2, 0, rows + 2, 1
                else:
                    h, sy, ey, vb = rows + 7, 3, rows + 3, 0
                ys, ye = max(sy, vb), min(ey, h - vb)
                assert ye - ys == rows
                base = noise(w, h, rows + w)
                block = 700
                plants = {"first row of a block": ys + block * rpb,
                          "last row of a block": ys + block * rpb + rpb - 1,
                          "last row of the box": ye - 1}
                for what, py in plants.items():
                    img = base.copy()
                    px = (py * 3) % w
                    img[py, px] = BIG
                    img[ys - 1, px] = img[ye, px] = 2 * BIG
                    q = [Query(sy, ey, 0, vb, an, an, (1, px, py, bits(BIG)))
                         for an in (True, False)]
                    yield Group(f"rows {rows} w {w} border {through_border}: {what}", img, q)
                img = base.copy()
                ya, yb = ys + 5 * rpb + rpb - 1, ys + 900 * rpb        # different blocks
                img[ya, w - 1] = img[yb, 0] = -BIG
                img[ys - 1, 0] = img[ye, 0] = -2 * BIG
                q = [Query(sy, ey, 0, vb, True, False, (1, w - 1, ya, bits(-BIG)))]
                yield Group(f"rows {rows} w {w} border {through_border}: equal maxima in two "
                            "blocks", img, q)
                img = base.copy()
                img[ye - 1, 1] = img[ye - 1, 2] = img[ye - 1, 3] = BIG  # one float4
                q = [Query(sy, ey, 0, vb, False, True, (1, 1, ye - 1, bits(BIG)))]
                yield Group(f"rows {rows} w {w} border {through_border}: equal maxima in a float4",
                            img, q)


# ------------------------------------------------------------ special values
def special_cases():
    nan, inf = payload_nan(), F(np.inf)
    for w, h in ((12, 3), (5, 3), (260, 2)):     # vector, scalar, a longer vector row
        at = (min(w - 2, 6), h - 2)              # inside every box below; not the box's first pixel
        for hb, vb in ((0, 0), (1, 0)):
            def ask(img, want_on, want_off, mask=None, name=""):
                """want_*: a pixel (x, y) or None for nothing found."""
                q = []
                for an, want in ((True, want_on), (False, want_off)):
                    for avx in (True, False):
                        expect = ((1, want[0], want[1], bits(img[want[1], want[0]]))
                                  if want is not None else nothing_found(img, mask, avx))
                        q.append(Query(0, h, hb, vb, an, avx, expect))
                return Group(f"special {w}x{h} border {hb}/{vb}: {name}", img, q, mask)

            ones = np.ones((h, w), np.uint8)
            for value in (F(2.0), F(-2.0), ABOVE_MIN, -ABOVE_MIN):
                neg = value < 0
                img = np.full((h, w), nan, F)
                img[at[1], at[0]] = value
                yield ask(img, at, None if neg else at, name=f"{value} among NaN")
                yield ask(img, at, None if neg else at, ones, name=f"{value} among NaN, masked")
                img = np.tile(np.array([-0.0, 1e-40, -1e-40, 0.0, -FLT_MIN / 2], F), w * h)[:w * h]
                img = img.reshape(h, w).copy()
                img[at[1], at[0]] = value
                yield ask(img, at, None if neg else at, name=f"{value} among -0 and subnormals")
                img = np.full((h, w), FLT_MIN, F)
                img[1::2] = -FLT_MIN
                img[at[1], at[0]] = value
                yield ask(img, at, None if neg else at, name=f"{value} among +-FLT_MIN")
            base = noise(w, h, w)
            first, second = (hb + 1, 0), at
            img = base.copy()
            img[at[1], at[0]] = inf
            yield ask(img, at, at, name="+Inf against finite values")
            img[first[1], first[0]] = inf
            yield ask(img, first, first, name="two +Inf")
            img = base.copy()
            img[first[1], first[0]] = 0.5
            img[first[1], first[0] + 1] = 0.95           # the largest finite value
            img[at[1], at[0]] = -inf
            yield ask(img, at, (first[0] + 1, first[1]), name="-Inf against finite values")
            img[first[1], first[0]] = -inf
            img[at[1], at[0]] = inf
            yield ask(img, first, at, name="-Inf before +Inf")
            img = base.copy()
            img[first[1], first[0] + 1] = 0.95
            img[at[1], at[0]] = nan
            yield ask(img, (first[0] + 1, first[1]), (first[0] + 1, first[1]), name="one NaN")
            for fill, name in ((nan, "all NaN"), (F(0), "all zero"), (FLT_MIN, "all FLT_MIN")):
                img = np.full((h, w), fill, F)
                yield ask(img, None, None, name=name)
                yield ask(img, None, None, ones, name=name + ", masked")


# ------------------------------------------------- small shapes, exhaustively
SMALL_WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16]


def small_cases():
    """Every box of every small image, images a random permutation of distinct
    values of mixed sign; the semantics rotate through AVX / simple / masked
    from one query to the next. Answers are the oracle's."""
    count = 0
    for w in SMALL_WIDTHS:
        for h in range(1, 6):
            rng = np.random.default_rng(w * 16 + h)
            values = (np.arange(1, w * h + 1) * rng.choice([-1, 1], w * h)).astype(F) / 4
            img = rng.permutation(values).reshape(h, w)
            mask = (rng.random((h, w)) < 0.6).astype(np.uint8)
            queries = []
            ranges = [(s, e) for s in range(h + 1) for e in range(s, h + 1)]
            ranges += [(h, 0), (1, 0), (0, h + 1), (0, h + 9)][:4]      # start > end; end > height
            for hb in range(w // 2 + 2):
                for vb in range(h // 2 + 2):
                    for s, e in ranges:
                        for an in (True, False):
                            queries.append(Query(s, e, hb, vb, an, count % 3 != 1,
                                                 masked=count % 3 == 2))
                            count += 1
            yield Group(f"small {w}x{h}", img, queries, mask)


# -------------------------------------------------- borders beyond the image
def beyond_cases():
    """h_border >= width, v_border > height, start_y > height: the reference
    reads past the image there (no oracle value); the answer is the empty
    box's. start_y = 2^32 - 1 with end_y = height is where clamping ye to the
    height after raising it to ys leaves ye < ys and `rows` wraps to a small
    count, whose workgroups then search rows of the image."""
    for w, h in ((8, 6), (5, 4), (64, 3)):
        img = noise(w, h, w)
        img[h // 2, w // 2] = BIG
        mask = np.ones((h, w), np.uint8)
        u = 2 ** 32
        boxes = [(0, h, w, 0), (0, h, w + 1, 0), (0, h, u - 1, 0), (0, h, u - w, 0),
                 (0, h, 0, h + 1), (0, h, 0, 2 * h + 3), (0, h, 0, u - 1), (0, u - 1, 0, h + 1),
                 (h + 1, h, 0, 0), (h + 1, h + 5, 0, 0), (h + 1, u - 1, 0, 0), (2 ** 21, h, 0, 0),
                 (u - 1, h, 0, 0), (u - 2, h, 0, 0), (u - h, h, 0, 0), (u - 1, u - 1, 0, 0),
                 (u - 3, h, 0, 1)]
        queries = []
        for sy, ey, hb, vb in boxes:
            for an in (True, False):
                for avx, masked in ((True, False), (False, False), (True, True)):
                    expect = nothing_found(img, mask if masked else None, avx)
                    queries.append(Query(sy, ey, hb, vb, an, avx, expect, masked, oracle=False))
        yield Group(f"beyond {w}x{h}", img, queries, mask)


def representative_subset():
    """The two-launch form's cases: one planted-edge shape per dispatch path,
    the 2049-row case and the nothing-found table."""
    out = list(planted("vector", 1028, H_PLANT, 0, 7, 1, 2))
    out += list(planted("scalar width", 257, H_PLANT, 3, 5, 2, 1))
    out += list(planted("scalar image + 4 bytes", 8, H_PLANT, 2, 7, 1, 1, img_off=1))
    out += list(planted("scalar mask off", 64, H_PLANT, 0, 7, 1, 2, mask_kind="hide", mask_off=3))
    out += list(planted("masked", 64, H_PLANT, 0, 7, 2, 2, mask_kind="only"))
    out += [g for g in rows_cases() if g.name.startswith("rows 2049 ")]
    out += [g for g in special_cases() if "all " in g.name]
    return out


def deferred_round(which):
    """PEAK_SLOTS single searches of different shapes, boxes, masks, semantics
    and dispatch paths: (group, query) pairs. Round 1 takes other images."""
    pool = []
    for gen in (planted_vector, planted_scalar, planted_masked, rows_cases, special_cases,
                beyond_cases):
        pairs = [(g, q) for g in gen() for q in g.queries]
        step = (len(pairs) - 1 - which) // 10
        pool += pairs[which::step][:11]
    assert len(pool) >= PEAK_SLOTS
    return pool[:PEAK_SLOTS]


# --------------------------------------------------------------- subtraction
def subtract_window(w, h, x, y):
    """simple_clean.cc:96-131: x - W/2 .. min(x + W/2, W), likewise in y."""
    return max(x - w // 2, 0), min(x + w // 2, w), max(y - h // 2, 0), min(y + h // 2, h)


def fma32(a, b, c):
    """float(a * b + c) of float32 inputs: the product is exact in float64
    (48 bits), the sum is rounded to double and then to float."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64)
            + np.asarray(c, np.float64)).astype(F)


SUBTRACT_MUTANTS = ["(W + 1) / 2 window", "(W + 1) / 2 PSF offset", "x loop stops after 2048"]


def subtract(img, psf, x, y, factor, mutant=None):
    """image -= psf * factor over the window, PSF centre at (W/2, H/2), one
    fused multiply-add a pixel. In place."""
    h, w = img.shape
    hw, hh = ((w + 1) // 2, (h + 1) // 2) if mutant == "(W + 1) / 2 window" else (w // 2, h // 2)
    x0, x1, y0, y1 = max(x - hw, 0), min(x + hw, w), max(y - hh, 0), min(y + hh, h)
    if mutant == "x loop stops after 2048":
        x1 = min(x1, x0 + 2048)
    if x1 <= x0 or y1 <= y0:
        return
    ox, oy = w // 2, h // 2
    if mutant == "(W + 1) / 2 PSF offset":
        ox, oy = (w + 1) // 2, (h + 1) // 2
    py = np.clip(np.arange(y0, y1) - (y - oy), 0, h - 1)
    px = np.clip(np.arange(x0, x1) - (x - ox), 0, w - 1)
    img[y0:y1, x0:x1] = fma32(-psf[np.ix_(py, px)], factor, img[y0:y1, x0:x1])


def subtract_images(w, h, seed=0):
    """An image in [1, 2) and a PSF of 0.5 <= |p| < 1.5: with |factor| >= 2^-3
    every window pixel changes by far more than an ulp."""
    rng = np.random.default_rng(w * 10007 + h + seed)
    img = rng.uniform(1, 2, (h, w)).astype(F)
    psf = (rng.uniform(0.5, 1.5, (h, w)) * rng.choice([-1, 1], (h, w))).astype(F)
    return img, psf


def subtract_cases():
    """(w, h, [(x, y, factor), ...]): every component is subtracted from a
    fresh copy of subtract_images(w, h)."""
    f = F(0.375)
    for w in (4101, 4100):          # centre: a window of 4100 = 2 * 2048 + 4 (three trips of the
        for h in (6, 7):            # x loop, the last partial); x = 0: 2050
            yield w, h, [(w // 2, h // 2, f), (0, 0, -f), (w - 1, h - 1, f), (w // 2 + 1, 1, f)]
    # a window is W/2 wide at x = 0 and W/2 + 1 wide at x = W - 1, never narrower:
    # exactly 1, 256, 257, 2048 and 2049 pixels
    yield 2, 3, [(0, 1, f)]
    yield 512, 3, [(0, 1, f)]
    yield 513, 3, [(512, 1, -f)]
    yield 4096, 2, [(0, 1, f)]
    yield 4097, 3, [(4096, 2, f), (2048, 1, f)]
    yield 3, 4099, [(1, 2049, f), (0, 0, f), (2, 4098, -f), (1, 1, f)]   # grid.y = window rows
    for w, h in ((9, 7), (8, 6), (9, 6), (8, 7)):
        cx, cy = w // 2, h // 2
        comps = [(0, 0, f), (w - 1, 0, f), (0, h - 1, f), (w - 1, h - 1, f)]
        comps += [(cx + dx, cy + dy, -f) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        yield w, h, comps
    for w in range(1, 7):
        for h in range(1, 7):
            yield w, h, [(x, y, f) for y in range(h) for x in range(w)]
    yield 70, 9, [(35, 4, F(0)), (3, 1, F(-2.5)), (69, 8, F(0.125))]


def subtract_nan_cases():
    """(w, h, x, y, factor, (px, py), inside): a NaN at PSF pixel (px, py),
    inside or outside the part of the PSF the window reads. For (1, 1) in
    9 x 7 the window is x 0..5, y 0..4 and reads PSF x 3..8, y 2..6."""
    yield 9, 7, 1, 1, F(0.375), (4, 3), True
    yield 9, 7, 1, 1, F(0.375), (2, 3), False
    yield 9, 7, 1, 1, F(0.375), (4, 6), False
    yield 9, 7, 8, 6, F(0.375), (0, 0), True        # window x 4..9, y 3..7 reads PSF x 0..5, y 0..4
    yield 9, 7, 8, 6, F(0.375), (5, 2), False


def subtract_failures(got, before, want, x, y, factor):
    """What is wrong with `got` as the subtraction of (x, y, factor) from
    `before`: its bits against `want` (the oracle's; NaN equals NaN), and the
    set of changed pixels, which must be exactly the window."""
    h, w = before.shape
    out = []
    g, o = got.view(np.uint32), want.view(np.uint32)
    if not np.all((g == o) | (np.isnan(got) & np.isnan(want))):
        out.append("bits differ from the oracle's")
    if factor != 0:
        x0, x1, y0, y1 = subtract_window(w, h, x, y)
        window = np.zeros((h, w), bool)
        window[y0:y1, x0:x1] = True
        changed = g != before.view(np.uint32)
        if not np.array_equal(changed, window):
            out.append("the changed pixels are not the window")
    elif not np.array_equal(g, before.view(np.uint32)):
        out.append("factor 0 changed a pixel")
    return out


def window_sizes():
    """The x extents of subtract_cases' windows: the test of the cases checks
    that 1, 256, 257, 2048, 2049, 2050 and 4100 are among them."""
    out = set()
    for w, h, comps in subtract_cases():
        for x, y, _ in comps:
            x0, x1, _, _ = subtract_window(w, h, x, y)
            out.add(x1 - x0)
    return out


# --------------------------------------------------------------- integration
MAX_IMAGES = 64
LINEAR, SQUARE, SQUARED_JOINS = 0, 1, 2
GRID_CAP = 8192 * 256
INTEGRATE_MUTANTS = ["fma first term", "zero weights not skipped", "pol_mask ignored",
                     "grid stride stops at 2 097 152"]


class IntegrateCase:
    """`images` (n_images, n); `expect` is None where the oracle decides
    (orc.integrate with these weights / n_pol / pol_factor / mode), else the
    exact result in integer arithmetic with `factor` given outright."""

    def __init__(self, name, images, n_ch, n_pol, weights, mode, pol_factor=1.0, pol_mask=None,
                 factor=None, expect=None):
        self.name, self.images = name, np.ascontiguousarray(images, F)
        self.n_ch, self.n_pol, self.mode = n_ch, n_pol, mode
        self.weights = [1.0] * n_ch if weights is None else list(weights)
        self.pol_factor, self.factor, self.expect = pol_factor, factor, expect
        self.pol_mask = (1 << n_pol) - 1 if pol_mask is None else pol_mask
        self.copy_fast_path = int(n_ch == 1 and n_pol == 1 and mode != SQUARED_JOINS)

    @property
    def n(self):
        return self.images.shape[1]


def integration_factor(n_ch, weights, pol_factor, mode):
    """The host-side factor of image_set.cc:309-462, as rdl_lib.integration."""
    wsum = float(sum(float(F(x)) for x in weights if x != 0.0))
    if mode == LINEAR:
        return F(pol_factor / wsum) if wsum > 0 else F(0)
    if mode == SQUARE:
        if n_ch == 1:
            return np.sqrt(F(pol_factor))
        return F(np.float64(np.sqrt(F(pol_factor))) / wsum)
    return F(np.sqrt(pol_factor / wsum)) if wsum > 0 else F(0)


def integrate(case, dest, mutant=None):
    """IntegratePixel (rdl_internal.h) over every pixel, into `dest`."""
    c, n = case, case.n
    n_written = min(n, GRID_CAP) if mutant == "grid stride stops at 2 097 152" else n
    img = c.images[:, :n_written]
    factor = F(c.factor) if c.factor is not None else integration_factor(c.n_ch, c.weights,
                                                                          c.pol_factor, c.mode)
    n_images, np_ = c.n_ch * c.n_pol, c.n_pol
    w = [F(c.weights[i // np_]) for i in range(n_images)]
    pol_on = [(c.pol_mask >> p) & 1 or mutant == "pol_mask ignored" for p in range(np_)]
    skip_zero = mutant != "zero weights not skipped"
    zero = np.zeros(n_written, F)

    def accumulate(acc, v, weight):          # first term v * w, then fma(v, w, acc)
        if acc is None:
            return fma32(v, weight, zero) if mutant == "fma first term" else v * F(weight)
        return fma32(v, weight, acc)

    with np.errstate(invalid="ignore", over="ignore"):
        if c.copy_fast_path:
            out = img[0].copy()
        elif c.mode == LINEAR:
            acc = None
            for i in range(n_images):
                if (w[i] != 0 or not skip_zero) and pol_on[i % np_]:
                    acc = accumulate(acc, img[i], w[i])
            out = zero if acc is None else acc * factor
        elif c.mode == SQUARE and c.n_ch == 1:
            acc = None
            for p in range(np_):
                if pol_on[p]:
                    acc = img[p] * img[p] if acc is None else fma32(img[p], img[p], acc)
            out = np.sqrt(zero if acc is None else acc) * factor
        elif c.mode == SQUARE:
            out = None
            for ch in range(c.n_ch):
                wc = w[ch * np_]
                scratch = zero
                if wc != 0 or not skip_zero:
                    if np_ == 1:
                        scratch = img[ch]
                    else:
                        acc = None
                        for p in range(np_):
                            if pol_on[p]:
                                v = img[ch * np_ + p]
                                acc = v * v if acc is None else fma32(v, v, acc)
                        scratch = zero if acc is None else np.sqrt(acc)
                out = scratch * wc if ch == 0 else fma32(scratch, wc, out)
            out = out * factor
        else:
            acc = None
            for i in range(n_images):
                if (w[i] != 0 or not skip_zero) and pol_on[i % np_]:
                    acc = accumulate(acc, img[i] * img[i], w[i])
            out = zero if acc is None else np.sqrt(acc) * factor
    dest[:n_written] = out.astype(F)


def integrate_cases(only=None):
    """only: one n of the sizes below, or "RDL_MAX_IMAGES" for the 64-image
    cases at n = 257; None for all."""
    big = GRID_CAP + 257

    def rnd(n_images, n, seed):
        return np.random.default_rng(seed).standard_normal((n_images, n)).astype(F)

    def small_ints(n_images, n, seed):
        return np.random.default_rng(seed).integers(-8, 9, (n_images, n)).astype(F)

    for n in (1, 255, 256, 257, big):      # sizes(8192) of tests/test_primitives_gpu.py
        if only not in (None, n):
            continue
        few = n == big                     # at most 4 images there: a small upload
        yield IntegrateCase(f"copy fast path n={n}", rnd(1, n, n), 1, 1, None, LINEAR)
        yield IntegrateCase(f"linear n={n}", rnd(3, n, n + 1), 3, 1, [0.5, 2.0, 4.2], LINEAR)
        yield IntegrateCase(f"linear, 2 pol n={n}", rnd(4, n, n + 2), 2, 2, [0.7, 1.3], LINEAR, 0.5)
        yield IntegrateCase(f"square, 1 channel, 2 pol n={n}", rnd(2, n, n + 3), 1, 2, None,
                            SQUARE, 0.5)
        yield IntegrateCase(f"square, 1 channel, 4 pol n={n}", rnd(4, n, n + 4), 1, 4, None, SQUARE)
        yield IntegrateCase(f"square, channels n={n}", rnd(4, n, n + 5), 4, 1, [1, 2, 3, 4], SQUARE)
        yield IntegrateCase(f"square, channels, 2 pol n={n}", rnd(4, n, n + 6), 2, 2, [1.5, 2.0],
                            SQUARE, 0.5)
        yield IntegrateCase(f"squared joins n={n}", rnd(4, n, n + 7), 2, 2, [0.7, 1.3],
                            SQUARED_JOINS, 0.5)
        yield IntegrateCase(f"squared joins, 1 image n={n}", rnd(1, n, n + 8), 1, 1, None,
                            SQUARED_JOINS)
        if few:
            continue
        # zero weights: first (the first term is not image 0), middle, everywhere; NaN under them
        for weights, name in (([0.0, 0.5, 2.0, 1.25], "first"), ([0.5, 0.0, 0.0, 1.25], "middle"),
                              ([0.0, 0.0, 0.0, 0.0], "all")):
            for mode in (LINEAR, SQUARE, SQUARED_JOINS):
                if name == "all" and mode == SQUARE:
                    continue    # the reference's 0 * (1 / 0): a NaN, whose bits are not specified
                images = rnd(4, n, n + 9)
                for ch, wt in enumerate(weights):
                    if wt == 0.0:
                        images[ch] = np.nan
                if name == "all":
                    images[:] = np.nan
                yield IntegrateCase(f"zero weight {name}, mode {mode} n={n}", images, 4, 1,
                                    weights, mode)
        # -0 everywhere: v * w = -0 and fma(-0, w, -0) = -0, times a positive factor: -0
        # (image_set.cc:432-460: AssignMultiply, not a sum started at +0)
        yield IntegrateCase(f"minus zero n={n}", np.full((3, n), -0.0, F), 3, 1, [0.5, 2.0, 4.0],
                            LINEAR, expect=np.full(n, -0.0, F))
        # a proper subset of 4 polarisations (the oracle has none): exact integers,
        # power-of-two weights and factor
        images = small_ints(8, n, n + 10)
        v = images.astype(np.int64)
        want = (v[0] * 2 + v[2] * 2 + v[4] * 4 + v[6] * 4) * 0.25
        yield IntegrateCase(f"linear, pol_mask 0101 n={n}", images, 2, 4, [2.0, 4.0], LINEAR,
                            pol_mask=0b0101, factor=0.25, expect=want.astype(F))
        images = small_ints(4, n, n + 11)
        images[0], images[3] = 3 * images[1], 4 * images[1]          # sqrt(9 + 16) |v|
        want = 5 * np.abs(images[1].astype(np.int64)) * 0.5
        yield IntegrateCase(f"square, pol_mask 1001 n={n}", images, 1, 4, None, SQUARE,
                            pol_mask=0b1001, factor=0.5, expect=want.astype(F))
    if only not in (None, "RDL_MAX_IMAGES"):
        return
    n = 257
    yield IntegrateCase("linear, 64 images", rnd(MAX_IMAGES, n, 64), 16, 4,
                        list(np.linspace(0.5, 2.0, 16)), LINEAR, 0.25)
    yield IntegrateCase("square, 64 images", rnd(MAX_IMAGES, n, 65), 32, 2,
                        list(np.linspace(0.5, 2.0, 32)), SQUARE, 0.5)
    yield IntegrateCase("squared joins, 64 images", rnd(MAX_IMAGES, n, 66), 64, 1,
                        list(np.linspace(0.5, 2.0, 64)), SQUARED_JOINS)
    images = small_ints(MAX_IMAGES, n, 67)
    images[1::2] = 1000                      # the unselected polarisation
    want = images[0::2].astype(np.int64).sum(axis=0) * 2 * 0.125
    yield IntegrateCase("linear, 64 images, pol_mask 01", images, 32, 2, [2.0] * 32, LINEAR,
                        pol_mask=0b01, factor=0.125, expect=want.astype(F))
