"""Pure-NumPy restatements of the reference's ITOP pieces (test infrastructure; our own code, pinned by tests/golden/itop.npz and
tests/golden/itop.json, which tests/golden/make_golden_itop.py records from the reference's own functions where they can be run):

  tables            lib/datasets/datasets_itop_rtpose.py:32-154 (intrinsics, depth constants, keypoints, kp_connections, get_joint2chn,
                    get_swap_part_indices)
  hflip             lib/datasets/data_augmentation_2d3d.py:452-493 (Hflip, is_3d=False)
  augment_chain     Compose([Cvt2ndarray, Rotate(), RenderDepth(), Hflip(swap), Crop(), Resize(S)]) of the two ITOP trainers, for explicit
                    draws; warpAffine / getRotationMatrix2D from tests/cv2_warp_reference.py, cv2.resize from oracle/cv2_resize.py
  readout           evaluate/evaluation_rtpose_light3d_itop.py:176-209 -- the per-frame glue behind paf_to_pose: one-cell depth read-out for
                    visible joints, rescale of visible joints, back-projection with the flipped Y.  The script indexes posedepth without a
                    check (IndexError past the last row / column); `clamp=True` takes the last cell instead, as the kernels do.
  ground_truth      lib/datasets/datasets_itop.py:395-538 (the same maps datasets_itop_rtpose.get_ground_truth means, which cannot run as
                    written: it reads self.joint_names, self.strideA and self.align_radius, none of which its class defines), pose_align off
  prior_targets     datasets_itop.py:299-363,417-445 (objects from the joints' box grown by 25 px, build_prior_targets)
"""
import copy

import numpy as np

import cv2_warp_reference as cw

INTRINSICS = {'f': 1 / 0.0035, 'cx': 160, 'cy': 120}
DEPTH_MEAN, DEPTH_STD, DEPTH_MAX = 3, 2, 5
ROOT_JOINT = 'torso'
JOINT2BOX_MARGIN = 25
KEYPOINTS = ['head', 'neck', 'right_shoulder', 'left_shoulder', 'right_elbow', 'left_elbow', 'right_wrist', 'left_wrist', 'torso', 'right_hip',
             'left_hip', 'right_knee', 'left_knee', 'right_ankle', 'left_ankle']


def kp_connections(k=KEYPOINTS):
    i = k.index
    return [[i('torso'), i('right_hip')], [i('right_hip'), i('right_knee')], [i('right_knee'), i('right_ankle')], [i('torso'), i('left_hip')],
            [i('left_hip'), i('left_knee')], [i('left_knee'), i('left_ankle')], [i('torso'), i('neck')], [i('neck'), i('right_shoulder')],
            [i('right_shoulder'), i('right_elbow')], [i('right_elbow'), i('right_wrist')], [i('neck'), i('left_shoulder')],
            [i('left_shoulder'), i('left_elbow')], [i('left_elbow'), i('left_wrist')], [i('neck'), i('head')]]


def get_joint2chn():
    out = np.zeros(len(KEYPOINTS)).astype(int)
    out[KEYPOINTS.index(ROOT_JOINT)] = 0
    for k, limb in enumerate(kp_connections()):
        out[limb[1]] = k + 1
    return out


def get_swap_part_indices():
    pairs = {}
    for part in ('shoulder', 'elbow', 'wrist', 'hip', 'knee', 'ankle'):
        pairs['right_' + part], pairs['left_' + part] = 'left_' + part, 'right_' + part
    return [KEYPOINTS.index(pairs.get(k, k)) for k in KEYPOINTS]


# ---- Hflip ----
def hflip(image, label, swap_indices):
    """The branch of Hflip.__call__ behind the coin (is_3d=False): -> (image, labels)."""
    image = np.flip(image, axis=1)
    width = image.shape[1]
    out = []
    for lb in label:
        n = copy.deepcopy(lb)
        n['2d_joints'][:, 0] = - n['2d_joints'][:, 0] + width
        n['2d_joints'] = n['2d_joints'][swap_indices, :]
        if 'visible_joints' in n:
            n['visible_joints'] = n['visible_joints'][swap_indices]
        if 'bbox' in n:
            xmin, xmax = -n['bbox'][2] + width, -n['bbox'][0] + width
            n['bbox'][0], n['bbox'][2] = xmin, xmax
        out.append(n)
    return image, out


def augment_chain(image, labels, rot, a, flip, crops, S, swap_indices=None):
    """The ITOP training transform for explicit draws (Rotate() and RenderDepth() about width / 2, height / 2).  labels: persons with
    '2d_joints', '3d_joints' and optionally 'visible_joints' / 'bbox'.  -> (image [S, S] float32 as Resize returns it, labels, render width)."""
    from oracle import cv2_resize
    image = np.asarray(image).astype(np.float32)
    label = []
    for lb in labels:
        n = copy.deepcopy(dict(lb))
        n['2d_joints'] = np.array(n['2d_joints']).reshape([15, 2]).astype(np.float32)
        n['3d_joints'] = np.array(n['3d_joints'], dtype=np.float64).reshape([15, 3])
        if 'visible_joints' in n:
            n['visible_joints'] = np.array(n['visible_joints'])
        if 'bbox' in n:
            n['bbox'] = np.array(n['bbox'], dtype=np.float64)
        label.append(n)
    # Rotate()
    height, width = image.shape[:2]
    cx, cy = width / 2, height / 2
    rot_mat = cw.getRotationMatrix2D((cx, cy), float(rot), 1.0)
    image = cw.warpAffine(image, rot_mat, (width, height), flags=cw.INTER_LINEAR)
    rot_mat = np.vstack([rot_mat, [0, 0, 1]])
    for n in label:
        n['2d_joints'][:, 0], n['2d_joints'][:, 1] = cw.homographic_transform(rot_mat, n['2d_joints'][:, 0], n['2d_joints'][:, 1])
    # RenderDepth()
    a = float(a)
    xmin, ymin, xmax, ymax = float(0), float(0), float(width), float(height)
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
        n['2d_joints'][:, 0] -= new_xmin
        n['2d_joints'][:, 1] -= new_ymin
        n['3d_joints'][:, 2] *= a
        if 'bbox' in n:
            n['bbox'][0:4:2] -= new_xmin
            n['bbox'][1:4:2] -= new_ymin
    image = new_image * np.float32(a)
    render_w = image.shape[1]
    # Hflip(swap)
    if flip:
        image, label = hflip(image, label, swap_indices)
    # Crop()
    height, width = image.shape[:2]
    c_xmin, c_ymin = int(min(crops[0] * width, width)), int(min(crops[2] * height, height))
    c_xmax, c_ymax = int(max(width - 1 - crops[1] * width, 0)), int(max(height - 1 - crops[3] * height, 0))
    image = image[c_ymin:c_ymax, c_xmin:c_xmax]
    for n in label:
        n['2d_joints'][:, 0] -= c_xmin
        n['2d_joints'][:, 1] -= c_ymin
        if 'bbox' in n:
            n['bbox'][0:4:2] -= c_xmin
            n['bbox'][1:4:2] -= c_ymin
    # Resize(S)
    height, width = image.shape[:2]
    image = cv2_resize.resize(np.ascontiguousarray(image), (S, S), interpolation=cv2_resize.INTER_LINEAR)
    wr, hr = float(S) / width, float(S) / height
    for n in label:
        n['2d_joints'][:, 0] *= wr
        n['2d_joints'][:, 1] *= hr
        if 'bbox' in n:
            n['bbox'][0:4:2] = n['bbox'][0:4:2].astype(float) * wr
            n['bbox'][1:4:2] = n['bbox'][1:4:2].astype(float) * hr
    return image, label, render_w


# ---- evaluation glue ----
def paf_to_human_list(joint_list, assoc):
    """lib/utils/common.py: per person the 15 (x, y) of its joints, (-1, -1) where the person lacks the joint, and the 0 / 1 visibility."""
    humans, vis = [], []
    for row in np.asarray(assoc).reshape(-1, 17):
        h, v = np.ones((15, 2)) * -1, np.zeros(15)
        for j in range(15):
            k = int(row[j])
            if k >= 0:
                h[j] = joint_list[k][:2]
                v[j] = 1
        humans.append(h.tolist())
        vis.append(v.tolist())
    return humans, vis


def readout(humans_2d, visibility, z_chw, downsample=8, input_size=224, w_org=320, h_org=240, clamp=True):
    """evaluation_rtpose_light3d_itop.py:154-209 for one frame: z_chw [15, h, w] float32 as the network emits it.  -> (humans_2d, humans_3d)
    lists of [15][2] / [15][3]."""
    joint2chn = get_joint2chn()
    posedepth = np.array(z_chw, dtype=np.float32).transpose(1, 2, 0)[None].copy()
    posedepth *= DEPTH_STD
    posedepth += DEPTH_MEAN
    posedepth = posedepth[0]
    humans_2d = [list(map(list, h)) for h in humans_2d]
    humans_depth = []
    for i, human in enumerate(humans_2d):
        human_depth = np.ones(len(KEYPOINTS)) * -1
        for j, joint in enumerate(human):
            if visibility[i][j] > 0.5:
                yy, xx = int(joint[1] / downsample), int(joint[0] / downsample)
                if clamp:
                    yy, xx = min(yy, posedepth.shape[0] - 1), min(xx, posedepth.shape[1] - 1)
                human_depth[j] = posedepth[yy, xx, joint2chn[j]]
        humans_depth.append(human_depth)
    for i, human in enumerate(humans_2d):
        human = np.array(human)
        human[np.where(visibility[i]), 0] = human[np.where(visibility[i]), 0] / input_size * w_org
        human[np.where(visibility[i]), 1] = human[np.where(visibility[i]), 1] / input_size * h_org
        humans_2d[i] = human
    humans_3d = []
    for i, human in enumerate(humans_2d):
        human_3d_x = (human[:, 0] - INTRINSICS['cx']) * humans_depth[i] / INTRINSICS['f']
        human_3d_y = -(human[:, 1] - INTRINSICS['cy']) * humans_depth[i] / INTRINSICS['f']
        humans_3d.append(np.vstack([human_3d_x, human_3d_y, humans_depth[i]]).T.tolist())
        humans_2d[i] = human.tolist()
    return humans_2d, humans_3d


def yolo_glue(humans_prior_b, input_size=224, w_org=320, h_org=240):
    """evaluation_yolo_posenet_itop.py:169-203 for one frame: humans_prior_b = parse_prior_pose's persons of the frame ([15, 3] rows x, y,
    depth).  -> (humans_2d, humans_3d) with one person: the first, or the -1 placeholder."""
    if len(humans_prior_b) > 0:
        human, depth = np.array(humans_prior_b[0][:, :2]), humans_prior_b[0][:, 2]
    else:
        human, depth = np.ones([15, 2]) * (-1), np.ones(15) * (-1)
    human[:, 0] = human[:, 0] / input_size * w_org
    human[:, 1] = human[:, 1] / input_size * h_org
    X = (human[:, 0] - INTRINSICS['cx']) / INTRINSICS['f'] * depth
    Y = (human[:, 1] - INTRINSICS['cy']) / INTRINSICS['f'] * depth
    h3 = np.vstack([X, Y, depth]).T
    h3[:, 1] *= (-1)
    return [human.tolist()], [h3.tolist()]


# ---- targets ----
def ground_truth(kp2d, kp3d, depth_resize, input_x=224, input_y=224, stride=8, z_radius=2, sigma=7.0, depth_max=DEPTH_MAX):
    """The heat / paf / z / fg maps of datasets_itop.ItopKeypoints.get_ground_truth: kp2d [P,15,2] network-input pixels, kp3d [P,15,3],
    depth_resize [h,w].  -> heat [h,w,16], paf [h,w,28], z [h,w,15] (normalised), fg [h,w,15]."""
    kp2d = np.asarray(kp2d, dtype=np.float64).reshape(-1, 15, 2)
    kp3d = np.asarray(kp3d, dtype=np.float64).reshape(-1, 15, 3)
    P = kp2d.shape[0]
    gh, gw = int(input_y / stride), int(input_x / stride)
    bad = (kp2d[:, :, 0] >= input_x) | (kp2d[:, :, 0] < 0) | (kp2d[:, :, 1] >= input_y) | (kp2d[:, :, 1] < 0)
    inb = (~bad).astype(np.float64)
    ys, xs = np.mgrid[0:gh, 0:gw].astype(np.float64)
    start = stride / 2.0 - 0.5
    heat = np.zeros((gh, gw, 16))
    for i in range(15):
        acc = np.zeros((gh, gw))
        for j in range(P):
            if inb[j, i] > 0.5:
                e = ((xs * stride + start - kp2d[j, i, 0]) ** 2 + (ys * stride + start - kp2d[j, i, 1]) ** 2) / 2.0 / sigma / sigma
                acc = acc + (e <= 4.6052) * np.exp(-e)
                acc[acc > 1.0] = 1.0
        heat[:, :, i] = acc
    heat[:, :, 15] = np.maximum(1 - heat[:, :, :15].max(axis=2), 0.0)
    paf = np.zeros((gh, gw, 28))
    for l, (k1, k2) in enumerate(kp_connections()):
        vx, vy, cnt = np.zeros((gh, gw)), np.zeros((gh, gw)), np.zeros((gh, gw))
        for j in range(P):
            if not (inb[j, k1] > 0.5 and inb[j, k2] > 0.5):
                continue
            a, b = kp2d[j, k1] / stride, kp2d[j, k2] / stride
            v = b - a
            n = np.linalg.norm(v)
            if n == 0.0:
                continue
            u = v / n
            x0, x1 = max(int(round(min(a[0], b[0]) - 1)), 0), min(int(round(max(a[0], b[0]) + 1)), gw - 1)
            y0, y1 = max(int(round(min(a[1], b[1]) - 1)), 0), min(int(round(max(a[1], b[1]) + 1)), gh - 1)
            m = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1) & (np.abs((xs - a[0]) * u[1] - (ys - a[1]) * u[0]) < 1)
            wx, wy = m * u[0], m * u[1]
            hit = (np.abs(wx) > 0) | (np.abs(wy) > 0)
            vx, vy = vx * cnt + wx, vy * cnt + wy
            cnt = cnt + hit
            div = np.where(cnt == 0, 1.0, cnt)
            vx, vy = vx / div, vy / div
        paf[:, :, 2 * l], paf[:, :, 2 * l + 1] = vx, vy
    zorg = np.repeat(np.asarray(depth_resize)[:, :, None], 15, axis=2)
    if zorg.dtype not in (np.float32, np.float64):
        zorg = zorg.astype(np.float64)
    dt = zorg.dtype.type
    z = np.ones_like(zorg) * 2 * depth_max
    fg = np.zeros((gh, gw, 15))
    for j in range(P):
        for k in range(15):
            if inb[j, k] < 0.5:
                continue
            cx, cy = kp2d[j, k] / stride
            x0, x1 = max(int(cx - z_radius), 0), min(int(cx + z_radius), gw - 1)
            y0, y1 = max(int(cy - z_radius), 0), min(int(cy + z_radius), gh - 1)
            win = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
            pz = np.where(win, dt(kp3d[j, k, 2]), dt(depth_max))
            zk = np.minimum(pz, z[:, :, k])
            new = (pz < depth_max) & (fg[:, :, k] == 0)
            zk[new] = pz[new]
            z[:, :, k] = zk
            fg[:, :, k] = np.logical_or(fg[:, :, k], new)
    z[fg == 0] = zorg[fg == 0]
    z[z < 0] = 0
    z[z > depth_max] = depth_max
    z = (z - DEPTH_MEAN) / DEPTH_STD
    return heat, paf, z, fg


def prior_targets(kp2d, kp3d, pose_weights=None, input_x=224, input_y=224, stride_prior=16, anchors=((6., 3.), (12., 6.)), noobject_scale=0.1,
                  object_scale=1.0):
    """datasets_itop.py:417-445 + build_prior_targets: kp2d [P,15,2] float32 network-input pixels, kp3d [P,15,3]; pose_weights None = 1.0
    each ('pose_weight' absent).  -> prior_map [h,w,A(5+3J)], mask_conf, mask_coord, weight_map [h,w,A] float64."""
    kp2d = np.asarray(kp2d, dtype=np.float32).reshape(-1, 15, 2)
    kp3d = np.asarray(kp3d, dtype=np.float64).reshape(-1, 15, 3)
    anchors = np.array(anchors)
    J, A = 15, anchors.shape[0]
    height, width = int(input_y / stride_prior), int(input_x / stride_prior)
    weights = [1.0] * len(kp2d) if pose_weights is None else list(pose_weights)
    objects = []
    for k2, k3 in zip(kp2d, kp3d):
        # np.min of a float32 column minus a Python int: a float32 scalar under NumPy 2's promotion (the margin is added in float32), which
        # the golden records; it then enters the float64 object row
        m = np.float32(JOINT2BOX_MARGIN)
        obj = np.array([np.min(k2[:, 0]) - m, np.min(k2[:, 1]) - m, np.max(k2[:, 0]) + m, np.max(k2[:, 1]) + m, 1.0], dtype=np.float64)
        obj = np.concatenate([obj, k2[:, 0].ravel(), k2[:, 1].ravel(), k3[:, 2].ravel()])
        obj[5 + 2 * J: 5 + 3 * J] -= DEPTH_MEAN
        obj[5 + 2 * J: 5 + 3 * J] /= DEPTH_STD
        objects.append(obj)
    gt = np.array(objects).reshape(-1, 5 + 3 * J)
    prior = np.zeros((height, width, A, 5 + 3 * J))
    mconf = np.ones((height, width, A)) * noobject_scale
    mcoord = np.zeros((height, width, A))
    wmap = np.ones((height, width, A))
    box = np.zeros((len(gt), 4))
    for i, an in enumerate(gt):
        box[i] = [(an[0] + an[2]) / 2 / stride_prior, (an[1] + an[3]) / 2 / stride_prior, (an[2] - an[0]) / stride_prior, (an[3] - an[1]) / stride_prior]
        an[5:5 + 2 * J] /= stride_prior
    # IoU of the boxes' sizes with the anchors, both centred on the origin
    iw = np.minimum(box[:, None, 2] / 2, anchors[None, :, 0] / 2) - np.maximum(-box[:, None, 2] / 2, -anchors[None, :, 0] / 2)
    ih = np.minimum(box[:, None, 3] / 2, anchors[None, :, 1] / 2) - np.maximum(-box[:, None, 3] / 2, -anchors[None, :, 1] / 2)
    iw[iw < 0] = 0
    ih[ih < 0] = 0
    inter = iw * ih
    a1 = (box[:, 2] / 2 + box[:, 2] / 2) * (box[:, 3] / 2 + box[:, 3] / 2)
    a2 = (anchors[:, 0] / 2 + anchors[:, 0] / 2) * (anchors[:, 1] / 2 + anchors[:, 1] / 2)
    best = np.argmax(inter / ((a1[:, None] + a2[None, :]) - inter), axis=1) if len(gt) else []
    for i, an in enumerate(gt):
        n = best[i]
        gi, gj = min(width - 1, max(0, int(box[i, 0]))), min(height - 1, max(0, int(box[i, 1])))
        mconf[gj, gi, n], mcoord[gj, gi, n] = object_scale, 1
        wmap[gj, gi, :] = weights[i]
        prior[gj, gi, n, 0], prior[gj, gi, n, 1] = box[i, 0] - gi, box[i, 1] - gj
        prior[gj, gi, n, 2], prior[gj, gi, n, 3] = box[i, 2] / anchors[n, 0], box[i, 3] / anchors[n, 1]
        prior[gj, gi, n, 4] = 1
        prior[gj, gi, n, 5:] = an[5:]
        prior[gj, gi, n, 5:5 + J] -= gi
        prior[gj, gi, n, 5 + J:5 + 2 * J] -= gj
        prior[gj, gi, n, 5:5 + J] /= (anchors[n, 0] / 2)
        prior[gj, gi, n, 5 + J:5 + 2 * J] /= (anchors[n, 1] / 2)
    return prior.reshape((height, width, -1)), mconf, mcoord, wmap
