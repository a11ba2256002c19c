"""numpy restatement of what the composed (`test_mpaug`) and single-person (`val`, `test_bgaug`) KDH3D evaluation scripts do around the
network, one frame at a time -- the counterpart of tests/ablation_reference.py for
  third_party_methods/evaluate/evaluation_rtpose_light3d_kdh3d_mpaug_ablation.py, evaluation_yolo_posenet_kdh3d_mpaug.py,
  evaluation_rtpose_light3d_kdh3d_ablation.py, evaluation_yolo_posenet_kdh3d.py.

  nocrop_reference     Compose([Cvt2ndarray, Rotate, RenderDepth, Resize]) (..._mpaug_ablation.py:118-123): the training chain of
                       tests/cv2_warp_reference.augment_reference with the Crop step absent, NOT with zero crop fractions
  compose_bg           the single-person background swap (lib/datasets/datasets_kdh3d_rtpose.py:227-234)
  batch_draws          the `random` draws of generate_test_batch (lib/datasets/datasets_kdh3d_rtpose_mpaug.py:431-476)
  gt_to_original       the 2D ground truth scaled back to the original frame (..._mpaug_ablation.py:179-185)
  net_input_arms       the three depth-ablation arms when the "raw depth" is the network input tensor (:204-207): the arithmetic of
                       tests/ablation_reference.py on `img *= std; img += mean`
  first_person / yolo_lists   the list conventions of the four scripts
"""
import copy
import random

import numpy as np

import ablation_reference as AR
import cv2_warp_reference as cw

NUM_JOINTS = 15
AUG_MODS = [[0, 3], [1, 2], [0, 1], [2, 3], [4]]


def nocrop_reference(image, labels, params):
    """image [H, W]; labels: persons with '2d_joints' [15, 2] / '3d_joints' [15, 3]; params: rot, a, cx, cy, input_size.
    -> (image [S, S] float32 as Resize returns it, not clamped; labels; geometry)."""
    from oracle import cv2_resize
    rot, a, cx, cy, S = float(params["rot"]), float(params["a"]), params["cx"], params["cy"], int(params["input_size"])
    image = np.asarray(image).astype(np.float32)                                      # Cvt2ndarray
    label = []
    for lb in labels:
        n = copy.deepcopy(dict(lb))
        n["2d_joints"] = np.array(n["2d_joints"]).reshape([15, 2]).astype(np.float32)
        n["3d_joints"] = np.array(n["3d_joints"], dtype=np.float64).reshape([15, 3])
        label.append(n)
    height, width = image.shape                                                       # Rotate
    rot_mat = cw.getRotationMatrix2D((cx, cy), rot, 1.0)
    image = cw.warpAffine(image, rot_mat, (width, height), flags=cw.INTER_LINEAR)
    rot_mat = np.vstack([rot_mat, [0, 0, 1]])
    for n in label:
        n["2d_joints"][:, 0], n["2d_joints"][:, 1] = cw.homographic_transform(rot_mat, n["2d_joints"][:, 0], n["2d_joints"][:, 1])
    xmin, ymin, xmax, ymax = float(0), float(0), float(width), float(height)          # RenderDepth
    new_xmin, new_ymin = int(a * (xmin - cx) + cx), int(a * (ymin - cy) + cy)
    new_xmax, new_ymax = int(a * (xmax - cx) + cx), int(a * (ymax - cy) + cy)
    a = ((new_xmin - cx) / (xmin - cx) + (new_ymin - cy) / (ymin - cy)) / 2
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
    image = new_image * np.float32(a)
    geo = dict(render_corner=(new_xmin, new_ymin, new_xmax, new_ymax), render_a=a, render_shape=image.shape)
    height, width = image.shape                                                       # Resize, on the whole render image
    image = cv2_resize.resize(np.ascontiguousarray(image), (S, S), interpolation=cv2_resize.INTER_LINEAR)
    wr, hr = float(S) / width, float(S) / height
    for n in label:
        n["2d_joints"][:, 0] *= wr
        n["2d_joints"][:, 1] *= hr
    return image, label, geo


def compose_bg(image, fg_mask, bg):
    """image * fg_mask + bg * (1 - fg_mask) in float64, as the loader computes it (mask 0 / 1)."""
    image, fg_mask = np.asarray(image).astype(np.float64), np.asarray(fg_mask).astype(np.float64)
    return image * fg_mask + np.asarray(bg) * (np.ones_like(fg_mask) - fg_mask)


def batch_draws(batch_size, set_sizes, n_bg, min_ratio=0.7, max_ratio=1.7, aug_mods=AUG_MODS):
    """Per item, in the order the reference consumes Python's `random`: the index, the aug_mods entry, one uniform per candidate set,
    the fallback randint when nobody joined, then Rotate's and RenderDepth's uniform.  -> list of dicts."""
    dataset_len = max(set_sizes)
    items = []
    for _ in range(batch_size):
        index = random.randint(0, dataset_len - 1)
        mod = aug_mods[random.randint(0, len(aug_mods) - 1)]
        src = []
        for ii in mod:
            if random.uniform(0, 1) > 0.8:
                continue
            src.append((ii, index % set_sizes[ii]))
        fallback = not src
        if fallback:
            ii = random.randint(0, len(set_sizes) - 1)
            src.append((ii, index % set_sizes[ii]))
        rot = random.uniform(-10, 10)
        a = random.uniform(min_ratio, max_ratio)
        items.append(dict(index=index, sources=src, fallback=fallback, bg=index % n_bg, rot=rot, a=a))
    return items


def gt_to_original(labels, w_org, h_org, input_size):
    """label['2d_joints'][:, 0] *= w_org / input_size (float32 array times a Python float), then .tolist()."""
    out = []
    for lb in labels:
        j = np.array(lb["2d_joints"], dtype=np.float32)
        j[:, 0] *= (w_org / input_size)
        j[:, 1] *= (h_org / input_size)
        out.append(j.tolist())
    return out


def net_input_arms(x_norm, z, parse, gt_2d, w_org, h_org, input_size, downsample=8, depth_mean=3.0, depth_std=2.0, intrinsics=AR.INTRINSICS):
    """The three arms of one frame whose raw depth is the un-normalised network input x_norm [S, S] float32."""
    return AR.ablation_reference(x_norm, (None, None, z), parse, gt_2d, w_org, h_org, input_size, downsample, depth_mean, depth_std, intrinsics)


def first_person(per_frame):
    """`if len(humans_2d) > 0: humans_2d = [humans_2d[0]]` (..._kdh3d_ablation.py:198-201)"""
    return [f[:1] for f in per_frame]


def yolo_lists(humans_prior, w_org, h_org, input_size, intrinsics, first=False):
    """human_pred_set_{2d,3d} of one frame from parse_prior_pose's persons [n][15][3] (x, y, depth in the network frame):
    every person (mpaug, :185-225) or the first (single-person, :189-233), the placeholder of -1s when there is none."""
    if len(humans_prior) > 0:
        pick = humans_prior[:1] if first else humans_prior
        humans_2d = [np.array(h)[:, :2] for h in pick]
        depth = [np.array(h)[:, 2] for h in pick]
    else:
        humans_2d = [np.ones([NUM_JOINTS, 2]) * (-1)]
        depth = [np.ones(NUM_JOINTS) * (-1)]
    out2, out3 = [], []
    for human, d in zip(humans_2d, depth):
        human = np.array(human)
        human[:, 0] = human[:, 0] / input_size * w_org
        human[:, 1] = human[:, 1] / input_size * h_org
        X = (human[:, 0] - intrinsics["cx"]) / intrinsics["fx"] * d
        Y = (human[:, 1] - intrinsics["cy"]) / intrinsics["fy"] * d
        out2.append(human.tolist())
        out3.append(np.stack([X, Y, d], axis=1).tolist())
    return out2, out3
