"""Seeded inputs of the A2J fixture (tests/golden/a2j.npz, a2j_crops.npz), shared by the recipe that runs the reference on them
(tests/golden/make_golden_a2j.py) and by the tests that run the HIP path on them.  Arrays and numbers only.

Weights for a seed (numpy.random.default_rng, state-dict order): conv / fc weights N(0, sqrt(2 / fan_in)), the three heads'
output.weight x 0.5, conv / fc biases N(0, .05); BatchNorm gamma U(.8, 1.2) -- U(.2, .4) for every bn3, which keeps the residual
sums of 16 bottlenecks from growing --, beta N(0, .1), running mean N(0, .1), running var U(.5, 1.5).  With it the classification
logits have a standard deviation of about 0.5, so the softmax of the vote spreads over many anchors (the recipe asserts the
largest weight is < 0.05): a default-initialised net would give a one-hot softmax and the vote test would show nothing.
"""
import numpy as np
import torch

SEED = 2024
FRAME_H, FRAME_W = 640, 480          # the depth frames of the evaluation set (h_org x w_org); imgWidth / imgHeight stay 480 / 512
SMALL = (80, 96, 3)                  # crop H, W, batch: a 5 x 6 map, the smallest where every dilated tap meets real pixels; non-square
LARGE = (288, 288, 2)
SUBSAMPLE = 37                       # of the large case only every 37th head element is kept


def state_dict_for_seed(seed, keys, shapes):
    rng = np.random.default_rng(seed)
    shp = {k: tuple(int(v) for v in s) for k, s in zip(keys, shapes)}
    sd = {}
    for k in keys:
        s = shp[k]
        mod, leaf = k.rsplit(".", 1)
        is_bn = (mod + ".running_mean") in shp
        if leaf == "num_batches_tracked":
            v = np.zeros(s, np.int64)
        elif is_bn:
            if leaf == "weight":
                lo, hi = (0.2, 0.4) if mod.rsplit(".", 1)[-1] == "bn3" else (0.8, 1.2)
                v = rng.uniform(lo, hi, s)
            elif leaf == "running_var":
                v = rng.uniform(0.5, 1.5, s)
            else:
                v = rng.normal(0, 0.1, s)
        elif leaf == "weight":
            fan_in = int(np.prod(s[1:]))
            v = rng.normal(0, np.sqrt(2.0 / fan_in), s)
            if k.endswith("output.weight"):
                v = v * 0.5
        else:
            v = rng.normal(0, 0.05, s)
        sd[k] = torch.from_numpy(np.asarray(v, dtype=np.int64 if leaf == "num_batches_tracked" else np.float32))
    return sd


def net_input(seed, B, H, W):
    """Crops as the net sees them: smooth blobs in the value range of (depth - 3) / 2 plus noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    x = np.zeros((B, 1, H, W), np.float32)
    for b in range(B):
        cy, cx, s = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W, rng.uniform(0.15, 0.3) * min(H, W)
        blob = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        x[b, 0] = (-1.5 + 1.2 * blob + rng.normal(0, 0.05, (H, W))).astype(np.float32)
    return x


PALETTE = np.array([0.0, 0.5, 0.75, 1.0, 1.25, 1.5, 1.875, 2.0, 2.5, 3.0, 3.25, 4.0, 4.5, 5.0, 6.5, 7.25], np.float16)      # two values past depth_max 6: no clamp


def depth_frames(seed, F):
    """[F, 640, 480] float16: every pixel one of 16 depths at random -- a wrong source index shows at 15 of 16 pixels, and the crops compress."""
    rng = np.random.default_rng(seed)
    return PALETTE[rng.integers(0, 16, (F, FRAME_H, FRAME_W))]


# name, (x0, y0, x1, y1, conf)
CROP_CASES = [
    ("inside", (120.0, 200.0, 200.0, 330.0, 0.9)),
    ("left", (-20.5, 100.0, 60.0, 220.0, 0.8)),
    ("top", (100.0, -15.25, 190.0, 90.0, 0.7)),
    ("right", (420.0, 50.0, 500.5, 170.0, 0.95)),
    ("bottom", (200.0, 560.0, 280.0, 660.0, 0.6)),
    ("all_four", (-10.5, -20.25, 495.5, 655.0, 0.85)),
    ("bottom_512_640", (150.0, 430.0, 230.0, 560.0, 0.75)),
    ("fractional", (33.3, 47.8, 101.6, 163.2, 0.65)),
    ("one_pixel_high", (50.0, 100.2, 130.0, 101.7, 0.55)),
    ("low_conf", (100.0, 100.0, 200.0, 200.0, 0.005)),
    ("no_detection", (-1.0, -1.0, -1.0, -1.0, 0.0)),
]


def crop_rows(frame=0):
    return np.array([[frame] + list(b) for _, b in CROP_CASES], np.float32)


# the chain: frame 0 without a detection, frame 1 with two
CHAIN_ROWS = np.array([[0, -1, -1, -1, -1, 0],
                       [1, 96.5, 130.25, 230.0, 470.5, 0.91],
                       [1, 250.0, 88.0, 410.75, 520.0, 0.62]], np.float32)
INTRINSICS = {"fx": 504.1189880371094, "fy": 504.042724609375, "cx": 231.7421875, "cy": 320.62640380859375}


def map_back(votes, rows, crop_w=288, crop_h=288):
    """votes [n, 15, 3] float32 (y, x, z), rows [n, 6] float32 -> (xy [n, 15, 2], XYZ [n, 15, 3]) in float32 arithmetic: the frame
    coordinates x = x_crop (x1 - x0) / crop_w + x0 and the back-projection X = (x - cx) Z / fx."""
    f = np.float32
    votes, rows = votes.astype(f), rows.astype(f)
    x = votes[:, :, 1] * (rows[:, 3] - rows[:, 1])[:, None] / f(crop_w) + rows[:, 1][:, None]
    y = votes[:, :, 0] * (rows[:, 4] - rows[:, 2])[:, None] / f(crop_h) + rows[:, 2][:, None]
    z = votes[:, :, 2]
    X = (x - f(INTRINSICS["cx"])) * z / f(INTRINSICS["fx"])
    Y = (y - f(INTRINSICS["cy"])) * z / f(INTRINSICS["fy"])
    return np.stack([x, y], -1), np.stack([X, Y, z], -1)
