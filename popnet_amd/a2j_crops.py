"""The host half of A2J's crop-level training augmentation: the draws, the integer geometry and the labels of
third_party_methods/A2J_experiments/ itop_train_64.py:139-185, 208-295, 465-534, train_a2j_base.py:236-317 and
train_a2j_bgaug_new.py:251-338, in numpy, one operation per operation of the original.  The image half is one launch
(csrc/a2j_traincrop.hip::pn_a2j_train_crop) that reads the pn_a2j_crop_item records built here; nothing here touches the GPU.

Promotion rules.  The reference mixes float32 arrays, float32 scalars taken out of them, Python numbers and the odd float64 matrix, and
what numpy makes of such a mix depends on its version.  This module follows the numpy the goldens are made with and the suite runs
under, 2.x (NEP 50: a Python int or float adapts to the other operand, so `float32 scalar + int` and `float32 scalar + 0.4` stay float32,
and a float32 array against such a scalar stays float32) -- the same rules csrc/a2j.hip already follows for `int(i - start)` and
`imCrop.shape[0] + start1`.  Under numpy 1.x's value-based casting `float32 scalar + int` is float64 instead, which moves hi / lo and the
clipped box by up to one float32 rounding.  So that the result does not depend on the installed numpy, every such scalar operation is
written out here with explicit np.float32 operands: hi / lo / fill / sub / scale are the reference's own expressions, c + depth_thres,
c - depth_thres, c, c, RandomScale, evaluated in float32 as numpy 2 evaluates them (tests/golden/a2j_traincrop.npz stores the numpy
version of the recipe run).  The two places that ARE float64 in the reference stay float64: the rotation matrix (warp_affine.py) and the label product
(homogeneous_labels: one np.matmul on operands of the script's shapes and strides, so that a BLAS which fuses multiply-adds rounds alike).

Departures from the scripts, on purpose: a `centre_*.txt` line containing `invalid` drops THAT FRAME (read_centres returns the kept
indices); the reference compacts the centre list only, after which frame i, label i and centre i no longer belong together.
"""
import math
from types import SimpleNamespace

import numpy as np

from . import _lib, warp_affine

f32 = np.float32
NUM_JOINTS = 15


# itop_train_64.py:29-51 -- the script's own camera (NOT profiles.ITOP, whose f = 1 / 0.0035) and augmentation ranges
A2J_ITOP = SimpleNamespace(fx=286, fy=-286, u0=160, v0=120, xy_thres=120, depth_thres=0.4, rand_crop_shift=5, rand_shift_depth=1, rand_rotate=10,
                      rand_scale=(1.0, 0.5), frame_w=320, frame_h=240)
# train_a2j_base.py:27-40 == train_a2j_bgaug_new.py:30-43
A2J_KDH3D = SimpleNamespace(img_w=480, img_h=512, mean=3, std=2, rand_crop_shift=5, rand_shift_depth=0.01, rand_rotate=10, scale_range=(700, 1700))


class A2JCropSampler:
    """One item's draws from np.random in the reference's order (dataPreprocess, augment=True): four randint(-5, 5) box offsets, the block
    normal(0, RandshiftDepth, crop_h * crop_w) that the reference draws and never uses, randint(-10, 10) degrees, and the scale --
    rand() * 1.0 + 0.5 (form "itop") or randint(700, 1700) / 1000 (form "box": base and bgaug).  exact_stream=True consumes the unused
    block, so that a run seeded with np.random.seed meets the stream of a single-worker run of the reference; False (default) skips it."""

    def __init__(self, form="itop", crop_w=288, crop_h=288, exact_stream=False):
        if form not in ("itop", "box"):
            raise _lib.PopnetError("A2JCropSampler: form is 'itop' or 'box', got %r" % (form,))
        self.form, self.crop_w, self.crop_h, self.exact_stream = form, int(crop_w), int(crop_h), bool(exact_stream)
        self.k = A2J_ITOP if form == "itop" else A2J_KDH3D

    def draw(self):
        k = self.k
        offsets = tuple(np.random.randint(-1 * k.rand_crop_shift, k.rand_crop_shift) for _ in range(4))
        if self.exact_stream:
            np.random.normal(0, k.rand_shift_depth, self.crop_h * self.crop_w)
        rotate = np.random.randint(-1 * k.rand_rotate, k.rand_rotate)
        if self.form == "itop":
            scale = np.random.rand() * k.rand_scale[0] + k.rand_scale[1]
        else:
            scale = np.random.randint(*k.scale_range)
            scale /= 1000
        return dict(offsets=tuple(int(o) for o in offsets), rotate=int(rotate), scale=float(scale))

    def draws(self, n):
        return [self.draw() for _ in range(n)]


def homogeneous_labels(label_xy, matrix):
    """The label half of the trainers' transform (itop_train_64.py:213-216): the float32 [P, 2] labels as float64 homogeneous rows, each
    through the 2 x 3 float64 `matrix`.  -> float64 [P, 2].  The product is np.matmul of the matrix with the [3, P] transposed view of a
    C-contiguous [P, 3] array, the operand layout the script hands to numpy: a BLAS build that fuses multiply-adds rounds like it."""
    rows = np.concatenate([np.asarray(label_xy[:, :2], dtype=np.float64), np.ones((label_xy.shape[0], 1))], axis=1)
    return np.matmul(matrix, rows.T).T


# ---- ITOP: centres and boxes ---------------------------------------------------------------------------------------------------
def read_centres(path):
    """center_{train,test}.txt -> (centres [n, 1, 3] float32, kept [n] frame indices, the number of frames the file speaks of).  Every
    non-blank line is one frame; a line containing the word `invalid` drops that frame: `kept` lists the frames that stay, for the frames
    and labels to be compacted with (see the module docstring)."""
    rows, kept, n = [], [], 0
    for line in open(path):
        parts = line.split()
        if not parts:
            continue
        if "invalid" not in parts:
            rows.append(parts)
            kept.append(n)
        n += 1
    return np.array(rows, dtype=np.float32).reshape(-1, 1, 3), np.array(kept, dtype=np.int64), n


def to_world(uvd, k=None):
    """(u, v, depth) -> (x, y, depth) with the constants block k (None = A2J_ITOP): x = (u - u0) depth / fx, in the array's own float32.
    [..., 3] -> a new [..., 3] array."""
    k = A2J_ITOP if k is None else k
    u, v, d = uvd[..., 0], uvd[..., 1], uvd[..., 2]
    return np.stack([(u - k.u0) * d / k.fx, (v - k.v0) * d / k.fy, d], axis=-1)


def to_pixel(xyz, k=None):
    """The inverse: u = x fx / depth + u0."""
    k = A2J_ITOP if k is None else k
    x, y, d = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    return np.stack([x * k.fx / d + k.u0, y * k.fy / d + k.v0, d], axis=-1)


def _centres(centres):
    c = np.array(centres, dtype=np.float32)
    return c.reshape(-1, 1, 3)


def itop_boxes(centres, profile=None, xy_thres=None):
    """The boxes of itop_train_64.py:139-185: the centres in world coordinates, moved by (-xy_thres, +xy_thres) for the left top corner and
    (+xy_thres, -xy_thres) for the right bottom one (world y points up: fy < 0), back in pixels; float32 throughout.
    centres [n, 1, 3] (u, v, depth) -> (lefttop_pixel, rightbottom_pixel) [n, 1, 3] float32.  profile: a constants block (None = A2J_ITOP);
    xy_thres=0 gives the zero-width box errorCompute builds."""
    k = A2J_ITOP if profile is None else profile
    t = k.xy_thres if xy_thres is None else xy_thres
    world = to_world(_centres(centres), k)
    move = np.array([-t, t, 0], dtype=np.float32)
    return to_pixel(world + move, k), to_pixel(world - move, k)


# ---- the item records --------------------------------------------------------------------------------------------------------
def _finite(what, i, *values):
    if not all(math.isfinite(float(v)) for v in values):
        raise _lib.PopnetError("a2j_crops: item %d has a non-finite %s" % (i, what))


def _slice(lo, hi, size):
    """depth[lo:hi] by Python's slice rules -> (start, length)"""
    s, e, _ = slice(int(lo), int(hi)).indices(size)
    return s, max(e - s, 0)


def _draw(draws, i, unit_scale=1):
    """-> (offsets, rotate, scale, augment)"""
    if draws is None:
        return (0, 0, 0, 0), 0, unit_scale, False
    d = draws[i]
    return tuple(int(o) for o in d["offsets"]), int(d["rotate"]), float(d["scale"]), True


def _records(n):
    return (_lib.A2JCropItem * n)()


def _set_warp(r, matrix, augment):
    r.warp = 1 if augment else 0
    r.m[:] = warp_affine.invert_affine(matrix) if augment else [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def itop_items(indices, centres, lefttop, rightbottom, keypoints, frame_hw, draws=None, crop_w=288, crop_h=288, frames=None, depth_thres=None):
    """dataPreprocess of itop_train_64.py:220-295 for the items `indices` (rows of centres / lefttop / rightbottom [N, 1, 3] float32 and of
    keypoints [N, P, 3] float32, the script's keypointsUVD) on frames of frame_hw = (H, W).  draws: one dict per item (A2JCropSampler.draw():
    offsets, rotate, scale) = augment=True; None = augment=False (no offsets, scale 1, transform not called).  frames: each item's index
    into the frame tensor the kernel will read (default 0 .. n - 1).
    -> (records: ctypes array of pn_a2j_crop_item, labels [n, P, 3] float32).
    The offsets move the box, which is clamped to [0, W - 1] x [0, H - 1] and cut with int(); no padding.  The depth window is centre depth
    +- depth_thres -> centre depth, then (v - centre depth) * scale.  Labels: column 0 = y, column 1 = x in crop pixels, and with
    augment=True both go through `matrix` IN THE ORDER THE SCRIPT WRITES THEM -- column 0 (y) multiplies the matrix's x column.  That is the
    reference's behaviour (the image is rotated about (x, y), its labels about (y, x)) and is kept."""
    H, W = int(frame_hw[0]), int(frame_hw[1])
    thres = A2J_ITOP.depth_thres if depth_thres is None else depth_thres
    centres, lefttop, rightbottom = (np.asarray(a, dtype=np.float32) for a in (centres, lefttop, rightbottom))
    keypoints = np.asarray(keypoints, dtype=np.float32)
    n, P = len(indices), keypoints.shape[1]
    rec, labels = _records(n), np.ones((n, P, 3), dtype=np.float32)
    for i, index in enumerate(indices):
        (o1, o2, o3, o4), rotate, scale, augment = _draw(draws, i)
        matrix = warp_affine.rotation_matrix((crop_w / 2, crop_h / 2), rotate, scale)
        c = centres[index][0][2]
        _finite("box or centre", i, lefttop[index, 0, 0], lefttop[index, 0, 1], rightbottom[index, 0, 0], rightbottom[index, 0, 1], c, scale)
        new_Xmin = max(lefttop[index, 0, 0] + f32(o1), 0)
        new_Ymin = max(lefttop[index, 0, 1] + f32(o2), 0)
        new_Xmax = min(rightbottom[index, 0, 0] + f32(o3), W - 1)
        new_Ymax = min(rightbottom[index, 0, 1] + f32(o4), H - 1)
        r = rec[i]
        r.frame = i if frames is None else int(frames[i])
        r.cy0, r.ih = _slice(new_Ymin, new_Ymax, H)
        r.cx0, r.iw = _slice(new_Xmin, new_Xmax, W)
        r.sh, r.sw, r.padded = r.ih, r.iw, 0
        r.window = 1
        r.hi, r.lo, r.fill, r.sub, r.scale = c + f32(thres), c - f32(thres), c, c, f32(scale)
        _set_warp(r, matrix, augment)
        with np.errstate(all="ignore"):      # a zero-width box divides by zero, as in the script
            label_xy = np.ones((P, 2), dtype=np.float32)
            label_xy[:, 1] = (keypoints[index, :, 0].copy() - f32(new_Xmin)) * f32(crop_w) / (f32(new_Xmax) - f32(new_Xmin))
            label_xy[:, 0] = (keypoints[index, :, 1].copy() - f32(new_Ymin)) * f32(crop_h) / (f32(new_Ymax) - f32(new_Ymin))
            if augment:
                label_xy = homogeneous_labels(label_xy, matrix)
            labels[i, :, 0] = label_xy[:, 0]
            labels[i, :, 1] = label_xy[:, 1]
            labels[i, :, 2] = (keypoints[index, :, 2] - c) * f32(scale)
    return rec, labels


def box_items(indices, bndbox, keypoints_2d, keypoints_3d, frame_hw, draws=None, crop_w=288, crop_h=288, img_wh=None, frames=None):
    """dataPreprocess of train_a2j_base.py:236-317 == train_a2j_bgaug_new.py:264-338 (the background swap happens before it, on the frame:
    targets.compose_bg) for the items `indices`: bndbox [N, 4] float32 (x0, y0, x1, y1), keypoints_2d [N, P, 2] and keypoints_3d [N, P, 3]
    float32.  draws / frames / the result as in itop_items.  The box offsets are DRAWN by the reference and never applied; the crop is the
    box clamped to the frame and cut with int(), pasted into the zero image int(y1 - y0) x int(x1 - x0) when the raw box leaves
    [0, img_w] x [0, img_h] (img_wh, default 480 x 512: the scripts' constants, independent of the frame's shape), whose paste loop tests
    start < i < end strictly.  Labels follow train_a2j.crop_labels' arithmetic in float32 (x into column 1, y into column 0) and, with
    augment=True, go through `matrix` as (x, y) first."""
    H, W = int(frame_hw[0]), int(frame_hw[1])
    img_w, img_h = (A2J_KDH3D.img_w, A2J_KDH3D.img_h) if img_wh is None else (int(img_wh[0]), int(img_wh[1]))
    bndbox = np.asarray(bndbox, dtype=np.float32)
    keypoints_2d, keypoints_3d = np.asarray(keypoints_2d, dtype=np.float32), np.asarray(keypoints_3d, dtype=np.float32)
    n, P = len(indices), keypoints_2d.shape[1]
    rec, labels = _records(n), np.ones((n, P, 3), dtype=np.float32)
    for i, index in enumerate(indices):
        _, rotate, scale, augment = _draw(draws, i)
        matrix = warp_affine.rotation_matrix((crop_w / 2, crop_h / 2), rotate, scale)
        b0, b1, b2, b3 = (bndbox[index][k] for k in range(4))
        _finite("box", i, b0, b1, b2, b3, scale)
        new_Xmin = max(b0, 0)
        new_Ymin = max(b1, 0)
        new_Xmax = min(b2, W - 1)
        new_Ymax = min(b3, H - 1)
        r = rec[i]
        r.frame = i if frames is None else int(frames[i])
        r.cy0, r.ih = _slice(new_Ymin, new_Ymax, H)
        r.cx0, r.iw = _slice(new_Xmin, new_Xmax, W)
        padded_h, padded_w = int(b3 - b1), int(b2 - b0)
        start1, start2, end1, end2 = 0, 0, padded_h, padded_w
        r.padded = 1 if (b0 < 0 or b1 < 0 or b2 > img_w or b3 > img_h) else 0
        if r.padded:
            if b1 < 0:
                start1 = f32(0) - b1
            if b0 < 0:
                start2 = f32(0) - b0
            if b3 > img_h:
                end1 = f32(r.ih) + f32(start1)
            if b2 > img_w:
                end2 = f32(r.iw) + f32(start2)
            r.sh, r.sw = padded_h, padded_w
            r.start1, r.start2, r.end1, r.end2 = f32(start1), f32(start2), f32(end1), f32(end2)
        else:
            r.sh, r.sw = r.ih, r.iw
        r.window = 0
        _set_warp(r, matrix, augment)
        with np.errstate(all="ignore"):      # an empty padded image divides by zero, as in the script (cv2.resize has raised by then)
            label_xy = np.ones((P, 2), dtype=np.float32)
            label_xy[:, 0] = (keypoints_2d[index, :, 0] - f32(new_Xmin) + f32(start2)) * f32(crop_w) / f32(padded_w)
            label_xy[:, 1] = (keypoints_2d[index, :, 1] - f32(new_Ymin) + f32(start1)) * f32(crop_h) / f32(padded_h)
            if augment:
                label_xy = homogeneous_labels(label_xy, matrix)
            labels[i, :, 1] = label_xy[:, 0]
            labels[i, :, 0] = label_xy[:, 1]
            labels[i, :, 2] = keypoints_3d[index, :, 2]
    return rec, labels


# ---- ITOP: votes back to the frame -------------------------------------------------------------------------------------------------
def _uvd(votes, centres, xy_thres, crop_w, crop_h):
    """The map back shared by writeTxt (:506-534) and errorCompute (:465-496): votes [n, P, 3] (y, x, z) -> [n, P, 3] float32 (u, v, depth).
    u = x (Xmax - Xmin) / crop_w + Xmin with the box clamped below by 0 and above by 2 * frame - 1, depth = z + centre depth; float32."""
    k = A2J_ITOP
    votes = np.asarray(votes, dtype=np.float32)
    centres = _centres(centres)
    if len(votes) != len(centres):
        raise _lib.PopnetError("a2j_crops: %d votes for %d centres" % (len(votes), len(centres)))
    lefttop, rightbottom = itop_boxes(centres, xy_thres=xy_thres)
    lo = np.where(0 > lefttop[:, :, :2], f32(0), lefttop[:, :, :2])                                     # Python's max(a, 0), element by element
    top = np.array([k.frame_w * 2 - 1, k.frame_h * 2 - 1], dtype=np.float32)
    hi = np.where(top < rightbottom[:, :, :2], top, rightbottom[:, :, :2])                             # min(b, top)
    size = np.array([crop_w, crop_h], dtype=np.float32)
    with np.errstate(all="ignore"):
        uv = votes[:, :, 1::-1] * (hi - lo) / size + lo
        return np.concatenate([uv, votes[:, :, 2:] + centres[:, :, 2:]], axis=-1)


def write_txt_rows(votes, centres, crop_w=288, crop_h=288):
    """writeTxt (itop_train_64.py:506-534) up to the file: votes [n, P, 3] (y, x, z in crop pixels / relative depth) -> [n, P * 3] float32
    rows (u, v, depth per joint) through the box centre +- xy_thres.  The clamps 320 * 2 - 1 / 240 * 2 - 1 stay as written."""
    uvd = _uvd(votes, centres, None, crop_w, crop_h)
    return uvd.reshape(len(uvd), -1)


def write_txt(path, rows):
    """The result file as writeTxt writes it: str() of every float32, each followed by one blank, one line per frame."""
    with open(path, "w") as f:
        for row in rows:
            for v in row:
                f.write(str(v) + ' ')
            f.write('\n')


def error_compute(votes, target, centres, as_reference=False, crop_w=288, crop_h=288):
    """errorCompute (itop_train_64.py:465-503): the mean 3D distance between the votes mapped back and target [n, P, 3] (the labels'
    '3d_joints' as the script reads them: u, v, depth), both in world coordinates (to_world).  -> np.float32.
    as_reference=True: the script's own box, built from the centre WITHOUT +- xy_thres -- zero width, so every joint maps to the centre
    pixel; its number bit for bit.  Default: writeTxt's box, which is what the script's result file holds."""
    source, target_ = np.asarray(votes, dtype=np.float32), np.array(target, dtype=np.float32)
    if source.shape != target_.shape:
        raise _lib.PopnetError("a2j_crops: votes %s against target %s" % (source.shape, target_.shape))
    uvd = _uvd(source, centres, 0 if as_reference else None, crop_w, crop_h)
    labels, outputs = to_world(target_), to_world(uvd)
    errors = np.sqrt(np.sum((labels - outputs) ** 2, axis=2))
    return np.mean(errors)
