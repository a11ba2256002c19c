"""Inputs of the A2J training-crop fixture (tests/golden/a2j_traincrop.npz), shared by the recipe that runs the reference on them
(tests/golden/make_golden_a2j_traincrop.py) and by the tests that run the numpy restatement, the host module and the HIP kernel on them.
Arrays and numbers only.  The shapes are the smallest that still expose each rule: two frame sizes that are no multiple of anything,
a non-square crop (a w / h swap in the matrix centre or in dsize shows) and one case of each form at the trainers' 288 x 288.
"""
import numpy as np

from a2j_cases import PALETTE

SEED = 4242
CROP_W, CROP_H = 64, 48
LARGE = 288
SETS = {"a": (24, 32), "b": (40, 30)}          # frame H, W
N_FRAMES = 3
IMG_WH_B = (30, 32)                            # imgWidth / imgHeight of the box form on the 40 x 30 frames: 480 x 512 over 16
P = 15

# ITOP depth window: depth_thres is the script's 0.4.  With the centre depth float32(2.6) the upper bound c + 0.4 is exactly 3.0 and with
# float32(2.4) the lower bound c - 0.4 is exactly 2.0 (the recipe asserts both): 3.0 and 2.0 are PALETTE values, so every frame holds pixels
# exactly at hi and exactly at lo.
C_HI, C_LO = 2.6, 2.4
ITOP_MEAN, ITOP_STD = 0.1, 0.3                 # MEAN / STD of the ITOP form: one-element float32 arrays in the script, loaded from files
# frame 2 of set "a": one NaN and one +Inf pixel (frame, row, column, value), inside the boxes of the two `specials` cases only
SPECIALS = [(2, 10, 12, float("nan")), (2, 14, 20, float("inf"))]


def frames(name):
    """[3, H, W] float16: every pixel one of 16 depths at random, plus SPECIALS in set "a"."""
    H, W = SETS[name]
    rng = np.random.default_rng(SEED + ord(name))
    f = PALETTE[rng.integers(0, 16, (N_FRAMES, H, W))]
    if name == "a":
        for k, y, x, v in SPECIALS:
            f[k, y, x] = v
    return f


def masks_and_backgrounds(name):
    """The background swap of the bgaug form: ([3, H, W] uint8 foreground masks, [3, H, W] float16 backgrounds)."""
    H, W = SETS[name]
    rng = np.random.default_rng(SEED + 7 + ord(name))
    mask = (rng.random((N_FRAMES, H, W)) < 0.6).astype(np.uint8)
    return mask, PALETTE[rng.integers(0, 16, (N_FRAMES, H, W))]


# name, set, frame, lefttop (x, y), rightbottom (x, y), centre depth, draws (o1, o2, o3, o4, rotate, scale) or None (augment=False), crop (w, h)
S = (CROP_W, CROP_H)
ITOP_CASES = [
    ("inside", "a", 0, (5.5, 3.25), (25.0, 20.5), C_HI, (1, -2, 3, 0, -10, 0.5), S),
    ("clip_left", "a", 1, (-3.5, 4.0), (20.0, 19.0), C_LO, (-1, 0, 0, 0, 9, 1.49), S),
    ("clip_top", "a", 0, (4.0, -2.5), (28.0, 18.0), C_HI, (0, -3, 0, 0, 0, 1.0), S),
    ("clip_right", "a", 1, (10.0, 2.0), (33.5, 22.0), C_LO, (0, 0, 2, 0, -10, 1.0), S),
    ("clip_bottom", "a", 0, (3.0, 6.0), (30.0, 22.5), C_HI, (0, 0, 0, 3, 9, 0.5), S),
    ("offsets_m5_p4", "a", 1, (8.0, 7.0), (24.0, 18.0), C_HI, (-5, 4, -5, 4, 3, 0.8125), S),
    ("one_pixel_wide", "a", 0, (10.2, 3.0), (11.7, 20.0), C_LO, (0, 0, 0, 0, -4, 1.25), S),
    ("empty", "a", 1, (10.2, 3.0), (10.9, 20.0), C_HI, (0, 0, 0, 0, 0, 1.0), S),
    ("no_augment_hi", "a", 0, (5.5, 3.25), (25.0, 20.5), C_HI, None, S),
    ("no_augment_lo", "a", 1, (5.5, 3.25), (25.0, 20.5), C_LO, None, S),
    ("specials_plain", "a", 2, (6.0, 5.0), (26.0, 20.0), C_HI, None, S),
    ("specials_warp", "a", 2, (6.0, 5.0), (26.0, 20.0), C_HI, (0, 0, 0, 0, 9, 1.0), S),
    ("tall_frame", "b", 0, (3.0, 4.5), (27.5, 36.0), C_LO, (2, -1, -3, 4, -7, 1.1), S),
    ("from_centre", "b", 1, None, None, C_HI, (2, -1, -3, 4, 6, 0.75), S),          # the box of itop_boxes: the whole frame at these depths
    ("large_288", "a", 0, (2.0, 1.0), (30.0, 22.0), C_HI, (1, 1, -1, -1, 5, 0.9), (LARGE, LARGE)),
]
NAN_CASES = ("specials_plain", "specials_warp")
# centres (u, v, depth) of the ITOP cases; `from_centre` derives its box from this one
ITOP_CENTRE_UV = (15.0, 20.0)

# the nine boxes of a2j_cases.CROP_CASES (640 x 480 frames, img 480 x 512) brought to the 40 x 30 frames with img 30 x 32
# name, frame, (x0, y0, x1, y1), draws or None, crop
BOX_CASES = [
    ("inside", 0, (7.5, 12.5, 12.5, 20.625), (1, 2, 3, 4, -10, 0.7), S),
    ("left", 1, (-1.28125, 6.25, 3.75, 13.75), (0, 0, 0, 0, 9, 1.699), S),
    ("top", 0, (6.25, -0.953125, 11.875, 5.625), (-5, 4, -5, 4, 2, 1.0), S),
    ("right", 1, (26.25, 3.125, 31.28125, 10.625), (0, 0, 0, 0, -3, 0.9), S),
    ("bottom", 0, (12.5, 35.0, 17.5, 41.25), (0, 0, 0, 0, 5, 1.2), S),
    ("all_four", 1, (-0.65625, -1.265625, 30.96875, 40.9375), (0, 0, 0, 0, -10, 1.699), S),
    ("bottom_img_frame", 0, (9.375, 26.875, 14.375, 35.0), (0, 0, 0, 0, 9, 0.7), S),
    ("fractional", 1, (2.08, 2.99, 6.35, 10.2), (0, 0, 0, 0, 0, 1.0), S),
    ("one_pixel_high", 0, (3.0, 6.2, 8.0, 7.7), (0, 0, 0, 0, 1, 1.0), S),
    ("no_augment", 1, (7.5, 12.5, 12.5, 20.625), None, S),
    ("no_augment_padded", 0, (-0.65625, -1.265625, 30.96875, 40.9375), None, S),
    ("large_288", 1, (2.5, 3.0, 26.0, 30.5), (0, 0, 0, 0, 4, 1.2), (LARGE, LARGE)),
]


def draws_of(case_draws):
    if case_draws is None:
        return None
    o1, o2, o3, o4, rot, scale = case_draws
    return dict(offsets=(o1, o2, o3, o4), rotate=rot, scale=scale)


def itop_centres():
    """[n, 1, 3] float32 (u, v, depth)"""
    return np.array([[[ITOP_CENTRE_UV[0], ITOP_CENTRE_UV[1], c[5]]] for c in ITOP_CASES], dtype=np.float32)


def itop_keypoints():
    """[n, 15, 3] float32 (u, v, depth): joints inside and a little outside the frame, depths around the centre's"""
    rng = np.random.default_rng(SEED + 1)
    out = np.zeros((len(ITOP_CASES), P, 3), np.float32)
    for i, c in enumerate(ITOP_CASES):
        H, W = SETS[c[1]]
        out[i, :, 0] = rng.uniform(-2, W + 2, P)
        out[i, :, 1] = rng.uniform(-2, H + 2, P)
        out[i, :, 2] = rng.uniform(c[5] - 0.5, c[5] + 0.5, P)
    return out


def box_arrays():
    """(bndbox [n, 4], keypoints_2d [n, 15, 2], keypoints_3d [n, 15, 3]) float32"""
    rng = np.random.default_rng(SEED + 2)
    H, W = SETS["b"]
    bnd = np.array([c[2] for c in BOX_CASES], dtype=np.float32)
    k2 = np.stack([rng.uniform(-2, W + 2, (len(BOX_CASES), P)), rng.uniform(-2, H + 2, (len(BOX_CASES), P))], -1).astype(np.float32)
    k3 = rng.uniform(-1, 4, (len(BOX_CASES), P, 3)).astype(np.float32)
    return bnd, k2, k3


# the ITOP map-back: votes (y, x, z) in crop pixels, targets (u, v, depth) and centres whose +- xy_thres box lies partly inside 640 x 480
def map_back_inputs(n=4):
    rng = np.random.default_rng(SEED + 3)
    votes = np.stack([rng.uniform(0, 288, (n, P)), rng.uniform(0, 288, (n, P)), rng.uniform(-0.4, 0.4, (n, P))], -1).astype(np.float32)
    target = np.stack([rng.uniform(0, 320, (n, P)), rng.uniform(0, 240, (n, P)), rng.uniform(2, 3.5, (n, P))], -1).astype(np.float32)
    centres = np.array([[[150.5, 110.25, 2.75]], [[20.0, 200.0, 3.125]], [[300.0, 30.0, 140.0]], [[170.0, 125.0, 250.0]]], dtype=np.float32)[:n]
    return votes, target, centres
