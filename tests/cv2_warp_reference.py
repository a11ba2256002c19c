"""numpy restatement of OpenCV 4.2 ``cv2.getRotationMatrix2D`` / ``cv2.warpAffine`` (float32, INTER_LINEAR, constant border 0) and,
built on it and on oracle.cv2_resize.resize, a pure-numpy ``augment_reference`` of the reference's random training transform

    Compose([Cvt2ndarray(), Rotate(cx, cy), RenderDepth(cx, cy, max_ratio), Crop(), Resize(S)])
    third_party_methods/lib/datasets/data_augmentation_2d3d.py:70-89, 411-448, 283-350, 94-128, 497-522

for given draws.  Test infrastructure, in the style of tests/layer_reference.py: slow, explicit, one numpy operation per operation of
the original so that every dtype rounds where the original rounds.

What is restated of OpenCV (modules/imgproc/src/imgwarp.cpp, 4.2.0, the generic C++ path -- the version oracle/cv2_resize.py names):

  getRotationMatrix2D   centre is a Point2f (float32); angle *= CV_PI / 180; alpha = cos, beta = sin in double;
                        [[alpha, beta, (1 - alpha) cx - beta cy], [-beta, alpha, beta cx + (1 - alpha) cy]]
  warpAffine            inverts the matrix in double (D = m0 m4 - m1 m3; D = D ? 1 / D : 0; A11 = m4 D; A22 = m0 D; m0 = A11; m1 *= -D;
                        m3 *= -D; m4 = A22; b1 = -m0 m2 - m1 m5; b2 = -m3 m2 - m4 m5), then fixed point with AB_BITS = 10 and
                        INTER_BITS = 5: adelta[x] = cvRound(m0 x 1024), bdelta[x] = cvRound(m3 x 1024), per row
                        X0 = cvRound((m1 y + m2) 1024) + 16, Y0 likewise; X = (X0 + adelta[x]) >> 5; source pixel (X >> 5, Y >> 5)
                        saturated to short, fractions (X & 31) / 32, (Y & 31) / 32
  remapBilinear         weights from the float table: products of the float32 entries 1 - k/32 and k/32; value
                        v0 w0 + v1 w1 + v2 w2 + v3 w3 in float32, left to right; a tap outside the source reads the border value 0
  cvRound               round half to even

Agreement with a live cv2 build is UNVERIFIED (OpenCV is not installed where this suite runs); tests/test_cv2_warp_kat.py pins the
restatement against an exact-rational derivation instead.  Newer OpenCV releases route float32 warpAffine through other SIMD code
whose rounding may differ.
"""
import copy
import math

import numpy as np

INTER_LINEAR = 1
AB_BITS, INTER_BITS = 10, 5
AB_SCALE, INTER_TAB_SIZE = 1 << AB_BITS, 1 << INTER_BITS


def getRotationMatrix2D(center, angle, scale):
    cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))      # Point2f
    angle = angle * (math.pi / 180)
    alpha, beta = math.cos(angle) * scale, math.sin(angle) * scale
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


def invert_affine(M):
    """The inversion warpAffine applies to a matrix given without WARP_INVERSE_MAP, in its operation order.  -> six Python floats."""
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def warpAffine(src, M, dsize, flags=INTER_LINEAR):
    """cv2.warpAffine(src, M, (width, height), flags=INTER_LINEAR) for a float32 H x W image, BORDER_CONSTANT 0."""
    src = np.asarray(src)
    if src.dtype != np.float32 or src.ndim != 2:
        raise TypeError("the warp restatement covers float32 single-channel images, got %s %s" % (src.dtype, src.shape))
    if flags != INTER_LINEAR:
        raise NotImplementedError("only INTER_LINEAR is restated")
    H, W = src.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    m = invert_affine(M)
    x = np.arange(dw, dtype=np.float64)
    y = np.arange(dh, dtype=np.float64)
    adelta = np.rint(m[0] * x * AB_SCALE).astype(np.int64)
    bdelta = np.rint(m[3] * x * AB_SCALE).astype(np.int64)
    rd = AB_SCALE // INTER_TAB_SIZE // 2
    X0 = np.rint((m[1] * y + m[2]) * AB_SCALE).astype(np.int64) + rd
    Y0 = np.rint((m[4] * y + m[5]) * AB_SCALE).astype(np.int64) + rd
    X = (X0[:, None] + adelta[None, :]) >> (AB_BITS - INTER_BITS)
    Y = (Y0[:, None] + bdelta[None, :]) >> (AB_BITS - INTER_BITS)
    sx = np.clip(X >> INTER_BITS, -32768, 32767)
    sy = np.clip(Y >> INTER_BITS, -32768, 32767)
    tab = np.zeros((INTER_TAB_SIZE, 2), dtype=np.float32)                     # interpolateLinear(i * (1.f / 32))
    tab[:, 1] = np.arange(INTER_TAB_SIZE, dtype=np.float32) * np.float32(1.0 / INTER_TAB_SIZE)
    tab[:, 0] = np.float32(1.0) - tab[:, 1]
    tx, ty = tab[X & (INTER_TAB_SIZE - 1)], tab[Y & (INTER_TAB_SIZE - 1)]     # [dh, dw, 2]
    out = None
    for k1 in range(2):
        for k2 in range(2):
            yy, xx = sy + k1, sx + k2
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            v = np.where(inside, src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], np.float32(0)).astype(np.float32)
            w = (ty[:, :, k1] * tx[:, :, k2]).astype(np.float32)
            term = (v * w).astype(np.float32)
            out = term if out is None else (out + term).astype(np.float32)
    wholly_outside = (sx >= W) | (sx + 1 < 0) | (sy >= H) | (sy + 1 < 0)
    out[wholly_outside] = np.float32(0)
    return out


def homographic_transform(M, x, y):
    """lib/utils/common.py:96-104"""
    ones = np.ones_like(y)
    pos = np.vstack([x, y, ones])
    trans = np.matmul(M, pos)
    return trans[0, :] / trans[2, :], trans[1, :] / trans[2, :]


def augment_reference(image, labels, params):
    """The transform chain for explicit draws.  image: the composed frame [H, W] (any float dtype); labels: list of persons, each a
    dict with '2d_joints' [15, 2], '3d_joints' [15, 3] and optionally 'bbox' [4]; params: dict with rot, a, crops = (left, right,
    top, bottom), cx, cy, input_size.  -> (image [S, S] float32 as Resize returns it (not clamped), labels, geometry) where geometry
    holds the integers the chain derived: shapes after Rotate / RenderDepth / Crop, RenderDepth's corner and recomputed a, Crop's bounds."""
    from oracle import cv2_resize
    rot, a, crops = float(params["rot"]), float(params["a"]), [float(c) for c in params["crops"]]
    cx, cy, S = params["cx"], params["cy"], int(params["input_size"])
    geo = {}
    # ---- Cvt2ndarray (+ 3d_joints as a float64 array: see tests/golden/make_golden_augment.py) ----
    image = np.asarray(image).astype(np.float32)
    label = []
    for lb in labels:
        n = copy.deepcopy(dict(lb))
        n["2d_joints"] = np.array(n["2d_joints"]).reshape([15, 2]).astype(np.float32)
        n["3d_joints"] = np.array(n["3d_joints"], dtype=np.float64).reshape([15, 3])
        if "bbox" in n:
            n["bbox"] = np.array(n["bbox"], dtype=np.float64)
        label.append(n)
    # ---- Rotate ----
    height, width = image.shape[:2]
    rot_mat = getRotationMatrix2D((cx, cy), rot, 1.0)
    image = warpAffine(image, rot_mat, (width, height), flags=INTER_LINEAR)
    rot_mat = np.vstack([rot_mat, [0, 0, 1]])
    for n in label:
        n["2d_joints"][:, 0], n["2d_joints"][:, 1] = homographic_transform(rot_mat, n["2d_joints"][:, 0], n["2d_joints"][:, 1])
    geo["rotate_shape"] = image.shape
    # ---- RenderDepth ----
    height, width = image.shape
    xmin, ymin, xmax, ymax = float(0), float(0), float(width), float(height)
    new_xmin, new_ymin = int(a * (xmin - cx) + cx), int(a * (ymin - cy) + cy)
    new_xmax, new_ymax = int(a * (xmax - cx) + cx), int(a * (ymax - cy) + cy)
    ax, ay = (new_xmin - cx) / (xmin - cx), (new_ymin - cy) / (ymin - cy)
    a = (ax + ay) / 2
    if a <= 1:
        new_image = image[new_ymin:new_ymax, new_xmin:new_xmax]
    else:
        dx, dy = int(xmin - new_xmin), int(ymin - new_ymin)
        new_image = np.zeros((new_ymax - new_ymin + 1, new_xmax - new_xmin + 1)).astype(np.float32)
        new_image[dy:dy + height, dx:dx + width] = image
    for n in label:
        n["2d_joints"][:, 0] -= new_xmin
        n["2d_joints"][:, 1] -= new_ymin
        n["3d_joints"][:, 2] *= a
        if "bbox" in n:
            n["bbox"][0:4:2] -= new_xmin
            n["bbox"][1:4:2] -= new_ymin
    new_image = new_image * np.float32(a)                                    # `new_image *= a` on a float32 array
    image = new_image
    geo.update(render_corner=(new_xmin, new_ymin, new_xmax, new_ymax), render_a=a, render_shape=image.shape)
    # ---- Crop ----
    height, width = image.shape[:2]
    c_xmin, c_ymin = int(min(crops[0] * width, width)), int(min(crops[2] * height, height))
    c_xmax, c_ymax = int(max(width - 1 - crops[1] * width, 0)), int(max(height - 1 - crops[3] * height, 0))
    image = image[c_ymin:c_ymax, c_xmin:c_xmax]
    for n in label:
        n["2d_joints"][:, 0] -= c_xmin
        n["2d_joints"][:, 1] -= c_ymin
        if "bbox" in n:
            n["bbox"][0:4:2] -= c_xmin
            n["bbox"][1:4:2] -= c_ymin
    geo.update(crop_bounds=(c_xmin, c_ymin, c_xmax, c_ymax), crop_shape=image.shape)
    # ---- Resize ----
    height, width = image.shape[:2]
    image = cv2_resize.resize(np.ascontiguousarray(image), (S, S), interpolation=cv2_resize.INTER_LINEAR)
    wr, hr = float(S) / width, float(S) / height
    for n in label:
        n["2d_joints"][:, 0] *= wr
        n["2d_joints"][:, 1] *= hr
        if "bbox" in n:
            n["bbox"][0:4:2] = n["bbox"][0:4:2].astype(float) * wr
            n["bbox"][1:4:2] = n["bbox"][1:4:2].astype(float) * hr
    return image, label, geo


def network_input(image, depth_max=6.0, mean=0.0, std=1.0):
    """The clamp of KDH3D_Keypoints.__getitem__ and pn_preprocess's normalisation (float32)."""
    image = image.copy()
    image[image < 0] = 0
    image[image > depth_max] = depth_max
    return ((image - np.float32(mean)) / np.float32(std)).astype(np.float32)
