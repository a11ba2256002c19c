"""numpy restatement of pn_a2j_train_crop (csrc/a2j_traincrop.hip): item records -> crops, one numpy operation per operation of the
reference chain (dataPreprocess + transform of the A2J trainers), so that every dtype rounds where the original rounds.  Test
infrastructure in the style of tests/cv2_warp_reference.py: slow and explicit.  It takes the same pn_a2j_crop_item records as the kernel
(ctypes, popnet_amd._lib.A2JCropItem), so a CPU test can compare records -> crops with the golden of the reference itself, and a GPU
failure can be told apart: records wrong, or kernel wrong.
"""
import numpy as np

f32 = np.float32


def normalised_crop(frame, it, crop_w, crop_h, mean, std):
    """The image transform() receives: [crop_h, crop_w] float32."""
    # the image cv2.resize reads
    region = np.asarray(frame)[it.cy0:it.cy0 + it.ih, it.cx0:it.cx0 + it.iw].astype(np.float32)
    if it.padded:
        src = np.zeros((it.sh, it.sw), np.float32)
        start1, start2, end1, end2 = f32(it.start1), f32(it.start2), f32(it.end1), f32(it.end2)
        for i in range(it.sh):
            for j in range(it.sw):
                py, px = int(f32(i) - start1), int(f32(j) - start2)
                if start1 < i < end1 and start2 < j < end2 and py < it.ih and px < it.iw:
                    src[i, j] = region[py, px]
    else:
        src = region
    # cv2.resize(INTER_NEAREST): min(floor(d * (1 / (dsize / ssize))), ssize - 1) in double
    xs = np.minimum(np.floor(np.arange(crop_w) * (1.0 / (crop_w / it.sw))).astype(np.int64), it.sw - 1)
    ys = np.minimum(np.floor(np.arange(crop_h) * (1.0 / (crop_h / it.sh))).astype(np.int64), it.sh - 1)
    img = src[ys][:, xs]
    if it.window:
        with np.errstate(invalid="ignore"):
            img = img.copy()
            img[img >= f32(it.hi)] = f32(it.fill)
            img[img <= f32(it.lo)] = f32(it.fill)
            img = (img - f32(it.sub)) * f32(it.scale)
    with np.errstate(invalid="ignore"):
        return ((img - f32(mean)) / f32(std)).astype(np.float32)


def warp_inverted(src, m, dw, dh):
    """cv2.warpAffine(src, M, (dw, dh), INTER_LINEAR, constant border 0) of OpenCV 4.2's generic float32 path, given the INVERTED matrix m
    (six doubles) as warpAffine holds it: the arithmetic of tests/cv2_warp_reference.warpAffine after its inversion."""
    H, W = src.shape
    x = np.arange(dw, dtype=np.float64)
    y = np.arange(dh, dtype=np.float64)
    adelta = np.rint(m[0] * x * 1024).astype(np.int64)
    bdelta = np.rint(m[3] * x * 1024).astype(np.int64)
    X0 = np.rint((m[1] * y + m[2]) * 1024).astype(np.int64) + 16
    Y0 = np.rint((m[4] * y + m[5]) * 1024).astype(np.int64) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    sx = np.clip(X >> 5, -32768, 32767)
    sy = np.clip(Y >> 5, -32768, 32767)
    fx = (X & 31).astype(np.float32) * f32(0.03125)
    fy = (Y & 31).astype(np.float32) * f32(0.03125)
    wx, wy = (f32(1) - fx, fx), (f32(1) - fy, fy)
    out = None
    with np.errstate(invalid="ignore"):
        for k1 in range(2):
            for k2 in range(2):
                yy, xx = sy + k1, sx + k2
                inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                v = np.where(inside, src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], f32(0)).astype(np.float32)
                term = v * (wy[k1] * wx[k2])
                out = term if out is None else out + term
    out[(sx >= W) | (sx + 1 < 0) | (sy >= H) | (sy + 1 < 0)] = f32(0)
    return out.astype(np.float32)


def train_crops(frames, items, crop_w, crop_h, mean, std):
    """frames [F, H, W] (float16 / float32), items: pn_a2j_crop_item records -> (crops [n, crop_h, crop_w] float32, flags [n] int32)."""
    n = len(items)
    out, flags = np.zeros((n, crop_h, crop_w), np.float32), np.zeros((n,), np.int32)
    for i, it in enumerate(items):
        if it.sh < 1 or it.sw < 1:
            flags[i] = 1
            continue
        img = normalised_crop(frames[it.frame], it, crop_w, crop_h, mean, std)
        out[i] = warp_inverted(img, [float(v) for v in it.m], crop_w, crop_h) if it.warp else img
    return out, flags
