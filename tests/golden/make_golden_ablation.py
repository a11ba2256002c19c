#!/usr/bin/env python
"""Golden vectors of the depth-ablation arms: the reference's evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py run end to end
(through make_golden.py's import shims, same checkpoint recipe as make_golden.golden_script: depth seed 77, weight seed 0, the
calibrated heat-bias shift, --w-org 480 --h-org 640 --batch-size 2) on labels made to exercise the ground-truth arms.

    python tests/golden/make_golden_ablation.py          # rewrites tests/golden/script_eval_data_ablation.json
    python tests/golden/make_golden_ablation.py --check  # regenerates into a scratch dir and compares (tests/test_ablation_reference.py)

Kept: the four ablation keys (human_pred_set_3d_read_raw_depth, _perfect_2d, _perfect_2d_read_raw_depth) + human_gt_set_2d_visible,
the four prediction keys make_golden.golden_script keeps, the labels, the seeds, and what the reference's own
evaluate/eval_pose_mp.py::eval_human_dataset_3d returns for the five argument sets its script keeps commented out (:451-544).
Only data leaves this script.
"""
import contextlib
import copy
import io
import json
import os
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

W_ORG, H_ORG, S, DOWN = 480, 640, 224, 8
ABLATION_KEYS = ("human_pred_set_3d_read_raw_depth", "human_pred_set_3d_perfect_2d", "human_pred_set_3d_perfect_2d_read_raw_depth",
                 "human_gt_set_2d_visible")
KEPT_KEYS = ("human_pred_set_2d", "human_pred_set_3d", "human_pred_set_visibility", "human_pred_set_part_conf")
# (2D set used for matching, 3D set, result key): the five blocks of the script, :451-544 in order
METRIC_BLOCKS = (("human_gt_set_2d", "human_pred_set_3d_perfect_2d", "perfect_2d"),
                 ("human_gt_set_2d_visible", "human_pred_set_3d_perfect_2d", "perfect_2d_visible"),
                 ("human_pred_set_2d", "human_pred_set_3d_read_raw_depth", "raw"),
                 ("human_gt_set_2d", "human_pred_set_3d_perfect_2d_read_raw_depth", "raw_perfect_2d"),
                 ("human_gt_set_2d_visible", "human_pred_set_3d_perfect_2d_read_raw_depth", "raw_perfect_2d_visible"))


def ablation_labels():
    """Frame 0: two GT persons, frame 1: three.  Joints inside the frame plus the edge cases of the cell / pixel index arithmetic:
    x < 0, x >= w_org, y >= h_org, x exactly w_org, fractional values one ulp below a pixel and below a cell boundary."""
    rng = np.random.default_rng(11)
    px_x, px_y = W_ORG / S, H_ORG / S                  # original-frame units per network pixel
    cell_x, cell_y = px_x * DOWN, px_y * DOWN
    out = []
    for n in (2, 3):
        people = []
        for p in range(n):
            base = rng.uniform([90, 120], [390, 520])
            j2 = base + rng.uniform(-70, 70, (15, 2)) * [0.6, 1.5]
            people.append(j2)
        out.append(people)
    a, b = out[0]
    a[0] = [-3.25, 100.5]                               # x < 0
    a[1] = [480.0, 320.0]                               # x exactly w_org
    a[2] = [481.5, 12.0]                                # x >= w_org
    a[3] = [200.0, 640.0]                               # y exactly h_org
    a[4] = [10.0, 655.75]                               # y >= h_org
    a[5] = [np.nextafter(37 * px_x, 0.0), np.nextafter(101 * px_y, 0.0)]      # one ulp below a pixel boundary
    a[6] = [37 * px_x, 101 * px_y]                      # ... and on it
    b[0] = [np.nextafter(9 * cell_x, 0.0), np.nextafter(17 * cell_y, 0.0)]    # one ulp below a cell boundary
    b[1] = [9 * cell_x, 17 * cell_y]
    b[2] = [-0.5, -0.5]                                 # int() truncates toward zero: cell / pixel 0 without the clamp
    b[3] = [479.999, 639.999]
    c, d, e = out[1]
    c[0] = [-120.0, -7.0]
    c[14] = [np.nextafter(223 * px_x, 0.0), np.nextafter(223 * px_y, 0.0)]
    d[7] = [np.nextafter(27 * cell_x, 0.0), 27 * cell_y]
    d[8] = [500.0, 700.0]
    e[3] = [0.0, 0.0]
    e[4] = [np.nextafter(1 * px_x, 0.0), np.nextafter(1 * cell_y, 0.0)]
    return [[np.asarray(p, dtype=np.float64).tolist() for p in people] for people in out]


def golden_script_ablation():
    import torch
    from popnet_amd import synth
    from lib.network.rtpose_light3d import rtpose_light3d
    work = tempfile.mkdtemp(prefix="popnet_fake_ds_ablation_")
    img_dir = os.path.join(work, "depth_maps")
    os.makedirs(img_dir)
    frames = synth.synth_depth(2, 640, 480, seed=77)
    intr = {"fx": 504.1189880371094, "fy": 504.042724609375, "cx": 231.7421875, "cy": 320.62640380859375}
    labels = {"intrinsics": intr}
    gt2 = ablation_labels()
    for i in range(2):
        np.save(os.path.join(img_dir, "f%d.npy" % i), frames[i])
        # 3D placeholders: the script only copies them; the stored labels get 3D joints derived from its own output below
        labels["f%d.npy" % i] = [{"2d_joints": j2, "3d_joints": [[0.0, 0.0, 3.0]] * 15} for j2 in gt2[i]]
    ann = os.path.join(work, "labels.json")
    json.dump(labels, open(ann, "w"))
    model = rtpose_light3d(15, 14, 2, input_dim=1).eval()
    arrays = synth.fill_state_dict(model.state_dict(), seed=0)
    model.load_state_dict(MG.np_sd(arrays))
    x = np.stack([MG.reference_preprocess(f, 6) for f in frames]).astype(np.float32)
    shift = MG.calibrated_heat_bias(model, x)
    arrays["model2_2.12.bias"][:15] += shift
    ckpt = os.path.join(work, "ckpt.pth")
    torch.save({"module." + k: torch.from_numpy(v) for k, v in arrays.items()}, ckpt)
    outdir = os.path.join(work, "out")
    argv, cwd = sys.argv, os.getcwd()
    try:
        os.chdir(os.path.join(MG.TPM, "evaluate"))
        sys.argv = ["eval", "--annotations", ann, "--image-dir", img_dir, "--w-org", str(W_ORG), "--h-org", str(H_ORG),
                    "--batch-size", "2", "--weight", ckpt, "--output-dir", outdir]
        import matplotlib
        matplotlib.use("Agg")
        with contextlib.redirect_stdout(io.StringIO()):
            try:
                runpy.run_path(os.path.join(MG.TPM, "evaluate", "evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py"), run_name="__main__")
            except Exception as e:      # the script's own metric tail may trip after eval_data.json has been written
                print("ablation: script raised after the dump: %r" % (e,), file=sys.stderr)
    finally:
        sys.argv = argv
        os.chdir(cwd)
    data = json.load(open(os.path.join(outdir, "eval_data.json")))
    assert data["human_gt_set_2d"] == gt2               # float64 survives the two JSON round trips
    keep = {k: data[k] for k in ABLATION_KEYS + KEPT_KEYS}
    # ground-truth 3D joints for the metric blocks: the raw-depth read-out at the ground-truth pixel, jittered (seeded), so that
    # PCK / error are neither 0 nor 1
    rng = np.random.default_rng(23)
    gt3 = [[(np.asarray(h, dtype=np.float64) + rng.normal(0, 0.06, (15, 3))).tolist() for h in fr]
           for fr in data["human_pred_set_3d_perfect_2d_read_raw_depth"]]
    for i in range(2):
        for p, j3 in zip(labels["f%d.npy" % i], gt3[i]):
            p["3d_joints"] = j3
    data["human_gt_set_3d"] = gt3
    from evaluate.eval_pose_mp import eval_human_dataset_3d
    metrics = {}
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        for k2, k3, name in METRIC_BLOCKS:
            d, k = eval_human_dataset_3d(copy.deepcopy(data[k2]), copy.deepcopy(data["human_gt_set_2d"]), copy.deepcopy(data[k3]),
                                         copy.deepcopy(gt3), num_joints=15, dist_th=0.1, iou_th=0.5)
            metrics["pck3d_" + name] = [float(v) for v in k]
            metrics["err3d_" + name] = [float(v) for v in d]
    keep["labels"] = labels
    keep["metrics"] = metrics
    keep["heat_bias_shift"] = shift.tolist()
    keep["depth_seed"] = 77
    keep["weight_seed"] = 0
    json.dump(keep, open(os.path.join(MG.OUT, "script_eval_data_ablation.json"), "w"))
    vis = [[int(np.sum(v)) for v in f] for f in keep["human_pred_set_visibility"]]
    print("ablation script: persons per frame", [len(f) for f in keep["human_pred_set_2d"]], "visible joints", vis,
          "GT persons", [len(f) for f in keep["human_gt_set_2d_visible"]])
    for name in ("perfect_2d", "raw", "raw_perfect_2d"):
        print("  %s: PCK3D %.3f err %.4f" % (name, np.nanmean(metrics["pck3d_" + name]), np.nanmean(metrics["err3d_" + name])))


if __name__ == "__main__":
    assert os.path.isdir(MG.REF), "the reference tree is needed to (re)generate golden vectors"
    check = "--check" in sys.argv[1:]
    if check:                       # regenerate into a scratch directory and compare with the committed file, leaf by leaf
        MG.OUT = tempfile.mkdtemp(prefix="popnet_golden_ablation_check_")
    MG.install_shims()
    golden_script_ablation()
    if check:
        fails = MG.check_outputs(MG.OUT)
        if fails:
            print("GOLDEN CHECK FAILED:\n  " + "\n  ".join(fails))
            sys.exit(1)
        print("golden check ok: %d files regenerate identically" % len(os.listdir(MG.OUT)))
