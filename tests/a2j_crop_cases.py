"""Box rows for the sweep of the A2J inference crop (pn_a2j_crop) and of the crop-level augmentation (pn_a2j_train_crop), shared by the recipe
that runs the reference on them (tests/golden/make_golden_a2j_crop_edges.py), the CPU tests (tests/test_a2j_crop_edges.py) and the GPU tests
(tests/test_gpu_a2j_crop_edges.py).  Arrays and numbers only.

Two sets of three small frames from the 16-value PALETTE (a wrong source index shows at 15 of 16 pixels), both with imgWidth x imgHeight =
30 x 32: "tall", 40 x 30 (H x W), is the deployed relation -- the frame is taller than imgHeight and as wide as imgWidth --, "wide", 24 x 34,
the opposite in both axes.  Frame 2 of "tall" holds one NaN and one +Inf pixel.  Per set about 300 seeded random rows, and on top of them
every class of tests/test_a2j_crop_edges.py::test_class_census built on purpose, 8 rows or more each.
"""
import numpy as np

from a2j_cases import PALETTE

SEED = 5150
SETS = {"tall": (40, 30), "wide": (24, 34)}          # frame H, W
IMG_WH = (30, 32)                                     # imgWidth, imgHeight
N_FRAMES = 3
SPECIALS = [(2, 17, 11, float("nan")), (2, 22, 16, float("inf"))]      # frame, row, column, value: set "tall" only
CROPS = [(64, 48), (50, 37)]                          # crop w, h; 50 x 37 = 1850 pixels: the last block of 256 threads is ragged
LARGE = (288, 288)
N_LARGE = 6                                           # rows per set at 288 x 288
N_RANDOM = 300
f32 = np.float32


def frames(name):
    """[3, H, W] float16"""
    H, W = SETS[name]
    rng = np.random.default_rng(SEED + len(name) + H)
    f = PALETTE[rng.integers(0, 16, (N_FRAMES, H, W))]
    if name == "tall":
        for k, y, x, v in SPECIALS:
            f[k, y, x] = v
    return f


def _up(v):
    return float(np.nextafter(f32(v), f32(np.inf)))


def _truncation_pairs(rng, n):
    """(lo, hi) float32 pairs with lo < 0 whose float32 difference truncates to another integer than their exact (float64) difference:
    near-integer and .5-like fractions whose subtraction rounds up to the integer."""
    out = []
    while len(out) < n:
        lo = f32(-rng.integers(1, 6) - rng.choice([0.1, 0.3, 0.7, 0.9, 0.45]))
        hi = f32(rng.integers(5, 14) + rng.choice([0.9, 0.7, 0.3, 0.1, 0.55]))
        if int(hi - lo) != int(float(hi) - float(lo)):
            out.append((float(lo), float(hi)))
    return out


def rows(name):
    """[n, 6] float32 (frame, x0, y0, x1, y1, conf): every row the reference itself can be run on."""
    H, W = SETS[name]
    iw, ih = IMG_WH
    rng = np.random.default_rng(SEED + 31 * len(name))
    xin, yin = float(min(W - 1, iw)), float(min(H - 1, ih))          # the largest end that crosses neither bound
    xout, yout = float(max(W - 1, iw)), float(max(H - 1, ih))        # past it an end crosses both
    out = []

    def add(x0, y0, x1, y1, conf=None, frame=None):
        out.append([rng.integers(0, N_FRAMES) if frame is None else frame, x0, y0, x1, y1, rng.uniform(0.02, 1.0) if conf is None else conf])

    def u(a, b):
        return float(rng.uniform(a, b))

    def x_in():
        x0 = u(0, xin - 8)
        return x0, u(x0 + 2, xin)

    def y_in():
        y0 = u(0, yin - 8)
        return y0, u(y0 + 2, yin)

    # ---- random boxes: 200 with a positive size, 100 with independent corners (half of them have a negative size)
    for k in range(N_RANDOM):
        if k < 200:
            x0, y0 = u(-10, W + 4), u(-10, H + 4)
            x1, y1 = x0 + u(0.2, W + 8), y0 + u(0.2, H + 8)
        else:
            x0, x1, y0, y1 = u(-10, W + 10), u(-10, W + 10), u(-10, H + 10), u(-10, H + 10)
        if k % 3 == 0:      # quarter-pixel values: integers, .25, .5, .75
            x0, y0, x1, y1 = (round(4 * v) / 4 for v in (x0, y0, x1, y1))
        add(x0, y0, x1, y1)
    for k in range(8):
        (x0, x1), (y0, y1) = x_in(), y_in()
        add(x0, y0, x1, y1)                                                  # unpadded, inside
        add(-u(0.3, 6), y0, x1, y1)                                          # each side alone
        add(x0, -u(0.3, 6), x1, y1)
        add(x0, y0, xout + u(0.2, 8), y1)
        add(x0, y0, x1, yout + u(0.2, 8))
        add(-u(0.3, 6), -u(0.3, 6), xout + u(0.2, 8), yout + u(0.2, 8))      # all four
        # between the image bound and the frame bound, in x and in y: alone, and padded through the other axis or the near side
        bx, by = u(xin + 0.05, xout), u(yin + 0.05, yout)
        add(x0, y0, bx, y1)
        add(x0, y0, x1, by)
        add(x0, -u(0.3, 6), bx, y1)
        add(-u(0.3, 6), y0, x1, by)
        add(-u(0.3, 6), y0, bx, y1)
        add(x0, -u(0.3, 6), x1, by)
        add(-u(0.3, 4), -u(0.3, 4), bx, by)
        # wholly outside: a negative slice end (padded, and unpadded with a negative size), a start past the frame
        add(-u(6, 12), y0, -u(1.2, 5), y1)
        add(x0, -u(6, 12), x1, -u(1.2, 5))
        add(x0, y0, -u(1.2, 5), y1)
        add(x0, y0, x1, -u(1.2, 5))
        add(-u(6, 12), -u(6, 12), -u(1.2, 5), -u(1.2, 5))
        add(W + u(0, 5), y0, W + u(6, 12), y1)
        add(x0, H + u(0, 5), x1, H + u(6, 12))
        add(float(W + k), float(H + k), W + k + u(2, 8), H + k + u(2, 8))
        # integer-valued edges with a negative origin: i == start and j == start occur
        add(-float(1 + k % 4), y0, float(6 + k), y1)
        add(x0, -float(1 + k % 5), x1, float(7 + k))
        add(-float(1 + k % 3), -float(2 + k % 3), float(5 + k), float(4 + 2 * k))
        add(-float(2 + k % 3), -float(1 + k % 4), xout + 1 + k, yout + 2 + k)
        # int() width or height 0 (the reference raises) and 1, padded and not
        add(-2.5, y0, -2.5 + 0.7, y1)
        add(x0, -1.5, x1, -1.5 + 0.9)
        add(-0.5, y0, -0.5 + 1.4, y1)
        add(x0, -0.25, x1, -0.25 + 1.9)
        add(x0 + 0.2, y0, x0 + 0.9, y1)
        add(x0, y0 + 0.3, x1, y0 + 0.8)
        add(np.floor(x0) + 0.2, y0, np.floor(x0) + 1.7, y1)
        add(x0, np.floor(y0) + 0.6, x1, np.floor(y0) + 1.9)
        # confidences at and around the threshold, and a low confidence in front of NaN coordinates: never read
        add(x0, y0, x1, y1, conf=f32(0.01))
        add(-u(0.3, 6), y0, x1, y1, conf=_up(0.01))
        add(x0, -u(0.3, 6), x1, y1, conf=0.0)
        add(x0, y0, xout + 3, y1, conf=float("nan"))
        add(float("nan"), y0, float("inf"), float("nan"), conf=0.005)
        add(-1.0, -1.0, -1.0, -1.0, conf=0.0, frame=k % N_FRAMES)           # the no-detection row
        add(x0, -u(0.3, 6), x1, y1, frame=N_FRAMES - 1)
    # float32 x1 - x0 / y1 - y0 truncating differently from float64
    for (a, b), (c, d) in zip(_truncation_pairs(rng, 8), _truncation_pairs(rng, 8)):
        y0, y1 = y_in()
        x0, x1 = x_in()
        add(a, y0, b, y1)
        add(x0, c, x1, d)
    # edges exactly at 0, -0.0, img, nextafter(img), size - 1 and size, as the near and as the far edge, in x and in y
    for k in range(4):
        (x0, x1), (y0, y1) = x_in(), y_in()
        for v in (0.0, -0.0, float(iw), _up(iw), float(W - 1), float(W)):
            add(v, y0, v + 3.5 + k, y1)
            add(v - 4.25 - k, y0 - (k % 2) * 9, v, y1)
        for v in (0.0, -0.0, float(ih), _up(ih), float(H - 1), float(H)):
            add(x0, v, x1, v + 3.5 + k)
            add(x0 - (k % 2) * 9, v - 4.25 - k, x1, v)
    # the specials' frame, around the NaN and the Inf pixel
    if name == "tall":
        for k in range(4):
            add(5.5 - 3 * k, 12.0 - 4 * k, 22.0 + k, 28.5 + 3 * k, frame=2)
    return np.array(out, dtype=np.float32)


def hostile_rows(name):
    """Rows above the confidence threshold that the reference cannot be run on: NaN, +-Inf and 1e12 in each coordinate position.  Expected:
    zeros, flag 1 (int(nan), int(inf), or a zero image / a slice of an absurd size)."""
    H, W = SETS[name]
    out = []
    for pos in range(4):
        for k, v in enumerate((float("nan"), float("inf"), float("-inf"), 1e12)):
            r = [(pos + k) % N_FRAMES, 3.5, 4.25, W - 6.0, H - 5.5, 0.6]
            r[1 + pos] = v
            out.append(r)
    return np.array(out, dtype=np.float32)


def all_rows(name):
    """rows(name) with hostile_rows(name) put between them, one after every 25th row -> (rows, index of each rows(name) row, of each hostile row)"""
    a, b = rows(name), hostile_rows(name)
    order, ia, ib = [], [], []
    nb = 0
    for k in range(len(a)):
        ia.append(len(order)); order.append(a[k])
        if k % 25 == 24 and nb < len(b):
            ib.append(len(order)); order.append(b[nb]); nb += 1
    assert nb == len(b)
    return np.array(order, dtype=np.float32), np.array(ia), np.array(ib)


def large_index(name):
    """The N_LARGE rows of rows(name) that also run at 288 x 288: inside, one side, all four, between the bounds, negative origin, a random one"""
    base = N_RANDOM
    return [base + 0, base + 1, base + 5, base + 12, base + 23, 7]


def bad_frame_rows(name):
    """Frame indices that name no frame, in front of good boxes, above and below the confidence threshold.  Expected: zeros, flag 1."""
    H, W = SETS[name]
    return np.array([[v, 3.5, 4.25, W - 6.0, H - 5.5, c] for v in (-1.0, float(N_FRAMES), float("nan"), 1e12, -0.5) for c in (0.6, 0.0)], dtype=np.float32)
