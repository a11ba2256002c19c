#!/usr/bin/env python
"""Generates tests/golden/itop.npz, tests/golden/itop.json and tests/golden/itop_frame_00_02254.npy by running the REFERENCE ITSELF (imported
read-only, with the import shims of make_golden.py) where its ITOP code can be executed:

  itop.json   the tables of lib/datasets/datasets_itop_rtpose.py and lib/datasets/datasets_itop.py (both files must agree): intrinsics, depth
              constants, get_keypoints(), kp_connections(), get_joint2chn(), get_swap_part_indices(), joint2box_margin
  eval2d_*    evaluate/eval_pose_mp.py eval_human_dataset_2d on seeded prediction / ground-truth sets (with and without a visibility set)
  aug*_*      the ITOP trainers' chain Compose([Cvt2ndarray, Rotate(), RenderDepth(), Hflip(swap), Crop(), Resize(S)])
              (lib/datasets/data_augmentation_2d3d.py) on 12 x 15 and 12 x 16 frames with scripted draws: a < 1, a > 1 and a rotated item with
              crops on all four sides, each with Hflip's coin on both sides -- image, joints, visible_joints and boxes
  gt_*        datasets_itop.ItopKeypoints.get_ground_truth (heat / paf / z / fg and the four prior maps) for one person partly outside a
              64 x 64 input, 'pose_weight' absent
  rtpose_gt_error   what datasets_itop_rtpose.ItopKeypoints.get_ground_truth raises (it reads self.joint_names, which its class never sets)
  the frame   third_party_methods/00_02254.npy, the one ITOP depth frame the reference ships (240 x 320 float16 metres): data, copied as is

    python tests/golden/make_golden_itop.py            # rewrites the three files
    python tests/golden/make_golden_itop.py --check    # regenerates into a scratch dir and compares

What stands in for what this machine lacks: cv2 (no OpenCV here) is the shim of make_golden.py -- cv2.resize is oracle/cv2_resize.py, and
cv2.warpAffine / cv2.getRotationMatrix2D are tests/cv2_warp_reference.py, restatements of OpenCV 4.2's scalar paths.  `Joints3dToArray` is
inserted after Cvt2ndarray for the reason make_golden_augment.py gives (RenderDepth indexes '3d_joints' as an array, Cvt2ndarray never
converts it).  evaluation_rtpose_light3d_itop.py:176-209 and evaluation_yolo_posenet_itop.py:169-203 are script bodies under
`if __name__ == "__main__"` with hard-wired dataset paths and cannot be called; tests/itop_reference.py restates them line by line.
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden as mg  # noqa: E402

OUT = HERE
AUG_S = 10                 # no 12 x 15 / 12 x 16 item can be an exact 2x decimation to 10
# (rot, a, coin, crop left, right, top, bottom): the coin is what uniform(0, 1) returns inside Hflip (>= 0.5 flips)
AUG_CASES = [
    (0.0, 0.8, 0.25, 0.0, 0.0, 0.0, 0.0), (0.0, 0.8, 0.5, 0.0, 0.0, 0.0, 0.0),                      # a < 1: the render image is a slice
    (0.0, 1.2, 0.49, 0.0, 0.0, 0.0, 0.0), (0.0, 1.2, 0.75, 0.0, 0.0, 0.0, 0.0),                     # a > 1: the frame pasted into a zero image
    (7.5, 1.1, 0.1, 0.1, 0.15, 0.1, 0.2), (7.5, 1.1, 0.9, 0.1, 0.15, 0.1, 0.2),                     # rotated, crops on all four sides
]
AUG_FRAMES = [(12, 15), (12, 16)]


class Joints3dToArray(object):
    def __call__(self, data):
        image, label = data
        for lb in label:
            lb["3d_joints"] = np.array(lb["3d_joints"], dtype=np.float64).reshape([15, 3])
        return image, label


def aug_inputs(H, W, seed):
    """The frame and the one person of an augmentation case (deterministic; the tests rebuild them)."""
    rng = np.random.default_rng(seed)
    frame = rng.uniform(0.3, 4.8, (H, W)).astype(np.float16)
    j2 = np.stack([rng.uniform(1, W - 1, 15), rng.uniform(1, H - 1, 15)], axis=1)
    person = {"2d_joints": j2.tolist(), "3d_joints": np.concatenate([j2, rng.uniform(1.5, 3.5, (15, 1))], axis=1).tolist(),
              "visible_joints": (rng.uniform(0, 1, 15) < 0.7).astype(int).tolist(),
              "bbox": [float(j2[:, 0].min()) - 1, float(j2[:, 1].min()) - 1, float(j2[:, 0].max()) + 1, float(j2[:, 1].max()) + 1]}
    return frame, person


def eval2d_cases(seed=23, frames=12):
    """Seeded (pred, gt, visibility) sets: one or two ground-truth persons per frame, predictions jittered, some persons dropped, some
    joints missing (-1, -1), one frame without ground truth."""
    rng = np.random.default_rng(seed)
    pred, gt, vis = [], [], []
    for f in range(frames):
        n = 0 if f == 5 else (2 if f % 4 == 0 else 1)
        g, p, v = [], [], []
        for k in range(n):
            c = np.array([80.0 + 150 * k, 120.0])
            j = c + rng.uniform(-40, 40, (15, 2))
            g.append(j.tolist())
            v.append((rng.uniform(0, 1, 15) < 0.8).astype(int).tolist())
            if rng.uniform() < 0.85:
                q = j + rng.normal(0, 5.0, (15, 2))
                q[rng.uniform(0, 1, 15) < 0.15] = -1
                p.append(q.tolist())
        if f == 7:
            p.append((np.array([300.0, 30.0]) + rng.uniform(-10, 10, (15, 2))).tolist())      # a prediction that overlaps nobody
        pred.append(p)
        gt.append(g)
        vis.append(v)
    return pred, gt, vis


def golden_itop():
    import importlib
    aug = importlib.import_module("lib.datasets.data_augmentation_2d3d")
    dr = importlib.import_module("lib.datasets.datasets_itop_rtpose")
    dy = importlib.import_module("lib.datasets.datasets_itop")
    ev = importlib.import_module("evaluate.eval_pose_mp")
    out = {}

    # ---- tables ----
    tables = {}
    for name, m in (("rtpose", dr), ("yolo", dy)):
        kp = m.get_keypoints()
        tables[name] = {"intrinsics": m.intrinsics, "depth_mean": m.depth_mean, "depth_std": m.depth_std, "depth_max": m.depth_max,
                        "keypoints": kp, "limbs": m.kp_connections(kp), "joint2chn": [int(v) for v in m.get_joint2chn()],
                        "swap_indices": [int(v) for v in m.get_swap_part_indices()], "root_joint": m.root_joint}
    assert tables["rtpose"] == tables["yolo"]
    tab = dict(tables["rtpose"], joint2box_margin=dy.joint2box_margin, frame=[240, 320])
    json.dump(tab, open(os.path.join(OUT, "itop.json"), "w"), indent=1)

    # ---- eval_human_dataset_2d ----
    pred, gt, vis = eval2d_cases()
    th = 0.02 * np.sqrt(320 ** 2 + 240 ** 2)
    d, k = ev.eval_human_dataset_2d(pred, gt, num_joints=15, dist_th=th, iou_th=0.5)
    dv, kv = ev.eval_human_dataset_2d(pred, gt, num_joints=15, dist_th=th, iou_th=0.5, human_gt_set_visibility=vis)
    out.update(eval2d_seed=np.array(23), eval2d_frames=np.array(12), eval2d_th=np.array(th), eval2d_dist=np.array(d, dtype=np.float64),
               eval2d_kcp=np.array(k, dtype=np.float64), eval2d_dist_vis=np.array(dv, dtype=np.float64), eval2d_kcp_vis=np.array(kv, dtype=np.float64))

    # ---- the augmentation chain with Hflip ----
    script, drawn = [], []

    def uniform(lo, hi):
        v = script.pop(0)
        drawn.append((float(lo), float(hi), float(v)))
        return v
    aug.uniform = uniform
    swap = dr.get_swap_part_indices()
    for fi, (H, W) in enumerate(AUG_FRAMES):
        frame, person = aug_inputs(H, W, 100 + fi)
        for ci, case in enumerate(AUG_CASES):
            chain = aug.Compose([aug.Cvt2ndarray(), Joints3dToArray(), aug.Rotate(), aug.RenderDepth(), aug.Hflip(swap_indices=swap), aug.Crop(), aug.Resize(AUG_S)])
            script[:] = list(case)
            del drawn[:]
            image, label = chain((frame.astype(float), [person]))
            assert not script
            if fi == 0 and ci == 0:      # the order and the ranges of the draws: Rotate, RenderDepth, Hflip's coin, Crop's four
                out["aug_draw_ranges"] = np.array([(lo, hi) for lo, hi, _ in drawn])
            k = "aug%d_%d_" % (fi, ci)
            out.update({k + "image": np.ascontiguousarray(image), k + "kp2d": label[0]["2d_joints"], k + "kp3d": label[0]["3d_joints"],
                        k + "visible": np.asarray(label[0]["visible_joints"]), k + "bbox": np.asarray(label[0]["bbox"], dtype=np.float64)})
            assert image.dtype == np.float32 and label[0]["2d_joints"].dtype == np.float32
    out.update(aug_cases=np.array(AUG_CASES), aug_frames=np.array(AUG_FRAMES), aug_S=np.array(AUG_S))

    # ---- targets: one person partly outside a 64 x 64 input ----
    d_tmp = tempfile.mkdtemp(prefix="popnet_itop_")
    json.dump({"a": []}, open(os.path.join(d_tmp, "ann.json"), "w"))
    rng = np.random.default_rng(77)
    k2 = np.stack([rng.uniform(-12, 70, 15), rng.uniform(6, 76, 15)], axis=1).astype(np.float32)
    k3 = np.concatenate([k2.astype(np.float64), rng.uniform(1.0, 5.6, (15, 1))], axis=1)          # some joints deeper than depth_max = 5
    depth = rng.uniform(-0.2, 5.5, (8, 8)).astype(np.float32)
    ann = [{"2d_joints": k2.copy(), "3d_joints": k3.copy(), "visible_joints": np.zeros(15)}]      # visible_joints all 0: it must not gate the maps
    ds = dy.ItopKeypoints(d_tmp, os.path.join(d_tmp, "ann.json"), input_x=64, input_y=64, stride=8, z_radius=2)
    heat, paf, z, fg, _, _, prior, conf, coord, weight = ds.get_ground_truth(ann, depth)
    inb = ((k2[:, 0] >= 0) & (k2[:, 0] < 64) & (k2[:, 1] >= 0) & (k2[:, 1] < 64))
    assert 3 <= inb.sum() <= 12, inb.sum()
    out.update(gt_kp2d=k2, gt_kp3d=k3, gt_depth=depth, gt_heat=heat, gt_paf=paf, gt_z=z, gt_fg=fg, gt_prior=prior, gt_conf=conf, gt_coord=coord,
               gt_weight=weight)
    dsr = dr.ItopKeypoints(d_tmp, os.path.join(d_tmp, "ann.json"), input_x=64, input_y=64, stride=8, z_radius=2)
    try:
        dsr.get_ground_truth([{"2d_joints": k2.copy(), "3d_joints": k3.copy(), "visible_joints": np.ones(15)}], depth)
        msg = ""
    except AttributeError as e:
        msg = str(e)
    assert "joint_names" in msg, msg
    out["rtpose_gt_error"] = np.array(msg)
    shutil.rmtree(d_tmp)

    np.savez_compressed(os.path.join(OUT, "itop.npz"), **out)
    shutil.copyfile(os.path.join(mg.TPM, "00_02254.npy"), os.path.join(OUT, "itop_frame_00_02254.npy"))
    f = np.load(os.path.join(OUT, "itop_frame_00_02254.npy"))
    assert f.shape == (240, 320) and f.dtype == np.float16
    print("itop.npz: %d arrays, %d bytes; frame %d bytes" % (len(out), os.path.getsize(os.path.join(OUT, "itop.npz")),
                                                            os.path.getsize(os.path.join(OUT, "itop_frame_00_02254.npy"))))


if __name__ == "__main__":
    assert os.path.isdir(mg.REF), "the reference tree is needed to (re)generate golden vectors"
    import torch.optim                 # noqa: F401  -- before the torchvision shim is importable (see make_golden.py)
    import torch.distributed.tensor    # noqa: F401
    mg.SHIMS["cv2/__init__.py"] += "\n        from cv2_warp_reference import warpAffine, getRotationMatrix2D\n"
    mg.install_shims()
    import popnet_amd  # noqa: F401
    check = "--check" in sys.argv[1:]
    if check:
        OUT = tempfile.mkdtemp(prefix="popnet_golden_itop_check_")
    golden_itop()
    if check:
        frame = "itop_frame_00_02254.npy"      # a copied file: compared byte for byte here, the rest by make_golden's comparison
        same = open(os.path.join(OUT, frame), "rb").read() == open(os.path.join(HERE, frame), "rb").read()
        print("check %-28s %s" % (frame, "identical" if same else "differs"))
        os.remove(os.path.join(OUT, frame))
        fails = mg.check_outputs(OUT) + ([] if same else [frame])
        if fails:
            print("GOLDEN CHECK FAILED:\n  " + "\n  ".join(fails))
            sys.exit(1)
        print("golden check ok: %d files regenerate identically" % len(os.listdir(OUT)))
