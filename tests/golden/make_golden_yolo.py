#!/usr/bin/env python
"""Generates the YoloPoseNet training goldens under tests/golden/ by running the REFERENCE ITSELF (imported read-only, with the
import shims of make_golden.py) on seeded inputs.

    python tests/golden/make_golden_yolo.py [steps]          # rewrites tests/golden/yolo_train_step.npz / yolo_targets.npz
    python tests/golden/make_golden_yolo.py --check [steps]  # regenerates into a scratch dir and compares (tests/test_yolo_golden_recipe.py)

Only data leaves this script: the seeded inputs and the reference's outputs.
  yolo_targets.npz     build_prior_targets + bbox_ious (lib/datasets/datasets_kdh3d_mpaug.py:353-417,505-533 (CR)) on a stand-in `self`
                       carrying only the attributes the method reads, fed the `objects` / `pose_weights` that get_ground_truth (:556-585)
                       builds from ann['bbox'], ann['2d_joints'], ann['3d_joints'] and ann['pose_weight']
  yolo_train_step.npz  YoloPoseNet(15, input_dim=1).train() forward, yolo_loss_fgweight_poseweight, backward() and
                       SGD(lr 1, momentum 0.9, nesterov) for two steps (train_yolo_posenet_kdh3d_mpaug.py:157-192 (CR)); per parameter what
                       make_golden.py's train_step.npz keeps, and the four loss terms of both loss forms
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden as mg  # noqa: E402
from make_golden import install_shims, np_sd, sample_indices  # noqa: E402

OUT = HERE
NUM_JOINTS = 15
ANCHORS = np.array([(6., 3.), (12., 6.)])


# ---- prior targets ------------------------------------------------------------------------------------------------------------
def _persons(rng, P, size=224):
    """P persons: boxes [P,4] float64 (network-input pixels, fractional as Resize leaves them), kp2d [P,15,2] float32, kp_z [P,15]
    float64, pose_weight [P] float64."""
    from popnet_amd import synth
    if P == 0:
        return np.zeros((0, 4)), np.zeros((0, NUM_JOINTS, 2), np.float32), np.zeros((0, NUM_JOINTS)), np.zeros(0)
    joints, depths = synth.planted_persons(rng, P, size=size)
    kp2d = (joints * (224.0 / size)).astype(np.float32)
    lo, hi = kp2d.min(1).astype(np.float64), kp2d.max(1).astype(np.float64)
    pad = rng.uniform(2, 12, (P, 4))
    boxes = np.round(np.concatenate([lo - pad[:, :2], hi + pad[:, 2:]], 1) * (480.0 / 224.0)) * (224.0 / 480.0)     # integer boxes of a 480-wide frame, resized
    kpz = depths[:, None] + rng.normal(0, 0.05, (P, NUM_JOINTS))
    pw = rng.uniform(0.5, 3.0, P)
    return boxes, kp2d, kpz, pw


def target_cases():
    """-> list of (name, boxes, kp2d, kp_z, pose_weight)"""
    cases = []
    for name, P, seed in (("empty", 0, 50), ("one", 1, 51), ("eight", 8, 52)):
        cases.append((name,) + _persons(np.random.default_rng(seed), P))
    # two persons in one cell: the later one writes the cell (the conf / coord masks of both anchors, the weight map, the prior slots)
    b, k, z, w = _persons(np.random.default_rng(53), 3)
    b[1] = b[0] + np.array([1.5, 2.0, -1.0, -3.0])           # same centre cell, another size
    b[2] = b[0] + np.array([0.5, 0.5, 0.5, 0.5])             # same cell, same anchor
    cases.append(("shared_cell", b, k, z, w))
    # box centres outside the grid: int() truncation, then the clamp to [0, size - 1]
    b, k, z, w = _persons(np.random.default_rng(54), 3)
    b[0] = [-60.0, -40.0, -10.5, 30.25]
    b[1] = [200.0, 210.0, 300.5, 260.0]
    b[2] = [-31.9, 100.0, 31.5, 140.0]                        # centre x in (-1, 0): truncates to 0
    cases.append(("outside", b, k, z, w))
    # a box whose IoU ties between the two anchors: 9 x 4 cells -> 18 / 36 = 36 / 72 (the first anchor wins)
    b, k, z, w = _persons(np.random.default_rng(55), 2)
    b[0] = [40.0, 80.0, 184.0, 144.0]
    b[1] = [8.0, 8.0, 104.0, 56.0]                            # 6 x 3 cells: exactly anchor 0
    cases.append(("anchor_tie", b, k, z, w))
    return cases


def golden_targets():
    import importlib
    import types
    mod = importlib.import_module("lib.datasets.datasets_kdh3d_mpaug")
    K = mod.KDH3D_Keypoints
    stub = types.SimpleNamespace(anchors=ANCHORS.copy(), stride_prior=16, num_joints=NUM_JOINTS, input_x=224, input_y=224)
    stub.bbox_ious = types.MethodType(K.bbox_ious, stub)
    g = int(224 / 16)
    out = {}
    cases = target_cases()
    for ci, (name, boxes, kp2d, kpz, pw) in enumerate(cases):
        objects = []                                          # what get_ground_truth builds per annotation (:563-577)
        for p in range(boxes.shape[0]):
            o = np.array([boxes[p, 0], boxes[p, 1], boxes[p, 2], boxes[p, 3], 1.0])
            o = np.concatenate([o, kp2d[p, :, 0].ravel(), kp2d[p, :, 1].ravel(), kpz[p].ravel()])
            o[5 + 2 * NUM_JOINTS:5 + 3 * NUM_JOINTS] -= mod.depth_mean
            o[5 + 2 * NUM_JOINTS:5 + 3 * NUM_JOINTS] /= mod.depth_std
            objects.append(o)
        prior, conf, coord, weight = K.build_prior_targets(stub, np.array(objects).reshape(len(objects), 5 + 3 * NUM_JOINTS), list(pw), g, g)
        out.update({"c%d_boxes" % ci: boxes, "c%d_kp2d" % ci: kp2d, "c%d_kpz" % ci: kpz, "c%d_pw" % ci: pw,
                    "c%d_prior" % ci: prior.transpose((2, 0, 1)).astype(np.float32), "c%d_conf" % ci: conf.transpose((2, 0, 1)).astype(np.float32),
                    "c%d_coord" % ci: coord.transpose((2, 0, 1)).astype(np.float32), "c%d_weight" % ci: weight.transpose((2, 0, 1)).astype(np.float32)})
    out["n_cases"] = np.array(len(cases))
    out["names"] = np.array([c[0] for c in cases])
    np.savez_compressed(os.path.join(OUT, "yolo_targets.npz"), **out)
    print("yolo_targets.npz: %d cases" % len(cases))


# ---- training step --------------------------------------------------------------------------------------------------------------
def golden_train():
    import collections
    import torch
    from helpers import train_case_inputs
    from yolo_reference import yolo_case_targets
    from popnet_amd import synth
    from lib.network.yolo_posenet import YoloPoseNet
    from lib.network import losses

    logs = []

    class Recorder(collections.OrderedDict):                 # the plain form logs its terms but returns only the total: record the log
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            logs.append(self)
    losses.OrderedDict = Recorder
    names = ["loss_prior", "loss_bbox", "loss_obj", "loss_selfpose"]
    torch.manual_seed(0)
    model = YoloPoseNet(15, input_dim=1)
    model.load_state_dict(np_sd(synth.fill_state_dict(model.state_dict(), seed=0)))
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1.0, momentum=0.9, weight_decay=0.0, nesterov=True)
    img = torch.from_numpy(train_case_inputs()[0])
    prior, conf, coord, weight = [torch.from_numpy(a) for a in yolo_case_targets()]
    out = {}
    for step in range(2):
        pred = model(img)
        logs.clear()
        plain = losses.yolo_loss_fgweight(pred, prior, conf, coord, 15, 2)
        out["s%d_plain_terms" % step] = np.array([logs[-1][n] for n in names])
        out["s%d_plain_loss" % step] = np.float64(plain.item())
        total, log = losses.yolo_loss_fgweight_poseweight(pred, prior, conf, coord, weight, 15, 2)
        opt.zero_grad()
        total.backward()
        out["s%d_loss" % step] = np.float64(total.item())
        out["s%d_terms" % step] = np.array([log[n] for n in names])
        for name, p in model.named_parameters():
            if p.grad is None:
                if not name.startswith("model0.layer3"):
                    raise RuntimeError(name)
                continue                                      # built, never run
            g = p.grad.detach().numpy().ravel()
            idx = sample_indices(name, g.size)
            out["s%d_g_norm/%s" % (step, name)] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
            out["s%d_g_sum/%s" % (step, name)] = np.float64(g.astype(np.float64).sum())
            out["s%d_g_samp/%s" % (step, name)] = g[idx].copy()
        opt.step()
        for name, p in model.named_parameters():
            if name.startswith("model0.layer3"):
                continue
            v = p.detach().numpy().ravel()
            out["s%d_p_samp/%s" % (step, name)] = v[sample_indices(name, v.size)].copy()
            out["s%d_p_norm/%s" % (step, name)] = np.float64(np.sqrt((v.astype(np.float64) ** 2).sum()))
        for name, b in model.named_buffers():
            if (name.endswith("running_mean") or name.endswith("running_var")) and not name.startswith("model0.layer3"):
                out["s%d_stat/%s" % (step, name)] = b.detach().numpy().copy()
    out["out_shape"] = np.array(pred.shape)
    losses.OrderedDict = collections.OrderedDict
    np.savez_compressed(os.path.join(OUT, "yolo_train_step.npz"), **out)
    print("yolo_train_step.npz: loss", out["s0_loss"], "->", out["s1_loss"])


if __name__ == "__main__":
    assert os.path.isdir(mg.REF), "the reference tree is needed to (re)generate golden vectors"
    import torch.optim                 # noqa: F401  -- before the torchvision shim is importable (see make_golden.py)
    import torch.distributed.tensor    # noqa: F401
    install_shims()
    import popnet_amd  # noqa: F401
    args = sys.argv[1:]
    check = "--check" in args
    args = [a for a in args if a != "--check"]
    if check:
        OUT = tempfile.mkdtemp(prefix="popnet_golden_yolo_check_")
    fns = {"targets": golden_targets, "train": golden_train}
    for w in args or list(fns):
        fns[w]()
    if check:
        fails = mg.check_outputs(OUT)
        if fails:
            print("GOLDEN CHECK FAILED:\n  " + "\n  ".join(fails))
            sys.exit(1)
        print("golden check ok: %d files regenerate identically" % len(os.listdir(OUT)))
