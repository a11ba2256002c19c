#!/usr/bin/env python
"""Golden vectors of the composed and single-person KDH3D evaluation sets: the reference's own loaders run on the fake tree of
tests/evalsets_cases.py (through make_golden.py's import shims) with Python's `random` seeded --
  lib/datasets/datasets_kdh3d_rtpose_mpaug.py  KDH3D_Keypoints.generate_test_batch with the evaluation scripts' chain
        Compose([Cvt2ndarray, Rotate, RenderDepth(max_ratio=1.7), Resize(32)])          two batches of three
  lib/datasets/datasets_kdh3d_rtpose.py        KDH3D_Keypoints.__getitem__ with Compose([Cvt2ndarray, Resize(32)]), bg_aug False and True

  evaluate/evaluation_rtpose_light3d_kdh3d_mpaug_ablation.py, evaluation_yolo_posenet_kdh3d_mpaug.py,
  evaluate/evaluation_rtpose_light3d_kdh3d_ablation.py, evaluation_yolo_posenet_kdh3d.py       the four SCRIPTS, end to end under runpy

    python tests/golden/make_golden_evalsets.py          # rewrites tests/golden/evalsets_inputs.npz and script_eval_data_{mpaug,mpaug_yolo,kdh3d,kdh3d_yolo}.json / .npz
    python tests/golden/make_golden_evalsets.py --check  # regenerates into a scratch dir and compares (tests/test_evalsets_golden_recipe.py)

Kept: every draw the loaders made (random.randint / random.shuffle results and the `uniform` of the dataset and augmentation modules, in
order, with their arguments), the shuffled id and background orders, the network inputs the loaders returned and the transformed labels.
Only data leaves this script.

Recipe-side stand-ins, as in make_golden_augment.py: cv2.warpAffine / getRotationMatrix2D / resize are the restatements of
tests/cv2_warp_reference.py and oracle/cv2_resize.py; '3d_joints' becomes a float64 array after Cvt2ndarray (RenderDepth's
`label['3d_joints'][:, 2] *= a` raises on the nested lists JSON gives); the dataset modules' `intrinsics` constant (the MP-3DHP camera) is
set to the fake tree's, whose frames are 40 x 36.

The scripts: each fixture keeps the script's whole eval_data.json, the metric values of the reference's own evaluate/eval_pose_mp.py on it
(the numbers the script's tail prints, at full precision), the weight recipe and, in the .npz, the network inputs the model received (for
Open-Pose+ also the three maps it returned).  Three of the four do not run as written against the reference's own library; their stand-ins
are recipe-side and named where they are installed: Joints3dToArray inside the chain the composed scripts build, paf_to_human_list handing
back the two values the Open-Pose+ scripts unpack (it returns three), the frame size of the composed Yolo-Pose+ dataset (the script never
passes --w-org / --h-org on), the annotation list (a glob of the author's disk), drawing calls that hand back their image (vis=True).
A Yolo-Pose+ frame without a detection cannot be recorded (golden_yolo_scripts).
"""
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import evalsets_cases as EC  # noqa: E402

SEED = 0
NAME = "evalsets_inputs.npz"
KINDS = {"randint": 0, "uniform": 1}


class Joints3dToArray(object):
    """Recipe-side transform (see the module docstring): '3d_joints' as a float64 [15, 3] array."""

    def __call__(self, data):
        image, label = data
        for lb in label:
            lb["3d_joints"] = np.array(lb["3d_joints"], dtype=np.float64).reshape([15, 3])
        return image, label


def golden_evalsets():
    from lib.datasets import data_augmentation_2d3d as aug
    from lib.datasets import datasets_kdh3d_rtpose as DS
    from lib.datasets import datasets_kdh3d_rtpose_mpaug as DM
    work = tempfile.mkdtemp(prefix="popnet_fake_evalsets_")
    tree = EC.write_tree(work)
    for mod in (DM, DS):
        mod.intrinsics.clear()
        mod.intrinsics.update(EC.INTRINSICS)
    log = []

    def logged(kind, fn):
        def f(a, b):
            v = fn(a, b)
            log.append((KINDS[kind], float(a), float(b), float(v)))
            return v
        return f

    real_randint, real_uniform = random.randint, random.uniform
    random.randint = logged("randint", real_randint)
    DM.uniform = aug.uniform = logged("uniform", real_uniform)
    out = {"seed": np.array(SEED), "frame": np.array([EC.H, EC.W, EC.S])}
    try:
        # ---- the composed test set ----
        random.seed(SEED)
        chain = aug.Compose([aug.Cvt2ndarray(), Joints3dToArray(), aug.Rotate(cx=EC.CX, cy=EC.CY), aug.RenderDepth(cx=EC.CX, cy=EC.CY, max_ratio=1.7),
                             aug.Resize(EC.S)])
        ds = DM.KDH3D_Keypoints(img_dir=tree["img"], ann_file_list=tree["ann_files"], preprocess=chain, w_org=EC.W, h_org=EC.H, input_x=EC.S, input_y=EC.S,
                                stride=8, z_radius=2, bg_file=tree["bg_file"], bg_dir=tree["bg"], seg_dir=tree["seg"])
        out["mpaug_ids"] = np.array([";".join(ids) for ids in ds.ids_list])
        out["mpaug_bgs"] = np.array([b["file_name"] for b in ds.bg_list])
        for k in range(2):
            start = len(log)
            images, labels = ds.generate_test_batch(3)
            out["mpaug_b%d_images" % k] = np.asarray(images)
            out["mpaug_b%d_log" % k] = np.array(log[start:], dtype=np.float64)
            out["mpaug_b%d_npers" % k] = np.array([len(l) for l in labels])
            out["mpaug_b%d_kp2d" % k] = np.concatenate([np.stack([np.asarray(p["2d_joints"]) for p in l]) for l in labels])
            out["mpaug_b%d_kp3d" % k] = np.concatenate([np.stack([np.asarray(p["3d_joints"]) for p in l]) for l in labels])
        # ---- the single-person sets ----
        for bg_aug in (0, 1):
            random.seed(SEED)
            single = DS.KDH3D_Keypoints(img_dir=tree["img"], ann_file=tree["single_ann"], preprocess=aug.Compose([aug.Cvt2ndarray(), Joints3dToArray(), aug.Resize(EC.S)]),
                                        input_x=EC.S, input_y=EC.S, stride=8, bg_aug=bool(bg_aug), bg_file=tree["bg_file"], bg_dir=tree["bg"], seg_dir=tree["seg"])
            out["single%d_images" % bg_aug] = np.stack([np.asarray(single[i][0]) for i in range(len(single))])
            if bg_aug:
                out["single_bgs"] = np.array([b["file_name"] for b in single.bg_list])
    finally:
        random.randint = real_randint
        DM.uniform = aug.uniform = real_uniform
    np.savez_compressed(os.path.join(MG.OUT, NAME), **out)
    return out
    print("evalsets: images", {k: v.shape for k, v in out.items() if k.endswith("images")}, "draws", [len(out["mpaug_b%d_log" % k]) for k in range(2)],
          "persons", [out["mpaug_b%d_npers" % k].tolist() for k in range(2)])


# ---- the two Yolo-Pose+ evaluation SCRIPTS, end to end ---------------------------------------------------------------------------------
def _metrics(data):
    """The reference's own eval_pose_mp on the lists a script wrote: what its metric tail prints, at full precision."""
    import contextlib
    import copy
    import io
    from evaluate.eval_pose_mp import eval_human_dataset_2d, eval_human_dataset_3d
    th = 0.02 * np.sqrt(EC.W ** 2 + EC.H ** 2)
    cp = copy.deepcopy
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        d2, k2 = eval_human_dataset_2d(cp(data["human_pred_set_2d"]), cp(data["human_gt_set_2d"]), num_joints=15, dist_th=th, iou_th=0.5)
        d3, k3 = eval_human_dataset_3d(cp(data["human_pred_set_2d"]), cp(data["human_gt_set_2d"]), cp(data["human_pred_set_3d"]), cp(data["human_gt_set_3d"]),
                                       num_joints=15, dist_th=0.1, iou_th=0.5)
    return {"dist_th_2d": float(th), "pck2d": [float(v) for v in k2], "err2d": [float(v) for v in d2], "pck3d": [float(v) for v in k3],
            "err3d": [float(v) for v in d3]}


def _counts(model, x, conf):
    import torch
    from lib.utils.prior_pose_align import parse_prior_pose
    with torch.no_grad():
        pm = model(torch.from_numpy(x))
    _, humans, _ = parse_prior_pose(pm, np.array([(6., 3.), (12., 6.)]), 15, EC.S, EC.S, 3, 2, conf_threshold=conf, nms_threshold=0.5)
    return [len(h) for h in humans]


def golden_yolo_scripts(loader_images):
    """evaluation_yolo_posenet_kdh3d.py (bg_aug as its default: on) and evaluation_yolo_posenet_kdh3d_mpaug.py under runpy, as
    make_golden.golden_script_yolo runs the mpreal one.  Weights: seeded, the two confidence filters shifted by a delta chosen per script on
    the single-person loader's inputs: the largest that leaves every frame a detection and some frame several (the shift is stored).
    A frame WITHOUT a detection cannot be recorded: both scripts build their -1 placeholder person and then rescale `bboxes[b][i]` of an
    empty list -- IndexError before anything is written (observed here with a larger shift).  The placeholder rows are therefore checked
    against the restated script lines only (tests/evalsets_reference.yolo_lists)."""
    import contextlib
    import glob as globmod
    import io
    import json
    import runpy
    import torch
    from popnet_amd import synth
    from lib.datasets import data_augmentation_2d3d as aug
    from lib.datasets import datasets_kdh3d, datasets_kdh3d_mpaug
    from lib.network.yolo_posenet import YoloPoseNet
    work = tempfile.mkdtemp(prefix="popnet_fake_evalsets_yolo_")
    tree = EC.write_tree(work)
    for mod in (datasets_kdh3d, datasets_kdh3d_mpaug):
        mod.intrinsics.clear()
        mod.intrinsics.update(EC.INTRINSICS)
    # the composed script never hands --w-org / --h-org to its dataset, whose frame size is the constructor's default (480 x 512)
    init = datasets_kdh3d_mpaug.KDH3D_Keypoints.__init__
    real_defaults = init.__defaults__
    assert real_defaults[1:3] == (480, 512)
    model = YoloPoseNet(15, input_dim=1).eval()
    base = synth.fill_state_dict(model.state_dict(), seed=1)
    captured = []
    real_forward, real_cvt, real_glob = YoloPoseNet.forward, aug.Cvt2ndarray.__call__, globmod.glob

    def forward(self, x):
        captured.append(x.detach().cpu().numpy().copy())
        return real_forward(self, x)

    def cvt(self, data):            # Joints3dToArray after Cvt2ndarray, inside the chain the script builds itself
        return Joints3dToArray()(real_cvt(self, data))

    def pick_delta(conf):
        best = None
        for d in np.linspace(0.0, 0.03, 601):
            arrays = {k: v.copy() for k, v in base.items()}
            arrays["model2_4.0.weight"][[4, 54]] -= np.float32(d)
            model.load_state_dict(MG.np_sd(arrays))
            c = _counts(model, loader_images, conf)
            if min(c) >= 1 and max(c) >= 2:
                best = (float(d), arrays)
        if best is None:
            raise SystemExit("no confidence shift leaves one person in a frame and several in another at conf %g" % conf)
        return best

    jobs = (("kdh3d_yolo", "evaluation_yolo_posenet_kdh3d.py", 0.1,
             ["--val-annotations", tree["single_ann"], "--val-image-dir", tree["img"], "--loader-workers", "0"]),
            ("mpaug_yolo", "evaluation_yolo_posenet_kdh3d_mpaug.py", 0.5, ["--image-dir", tree["img"], "--num-batches", "2"]))
    argv, cwd = sys.argv, os.getcwd()
    import matplotlib
    matplotlib.use("Agg")
    for name, script, conf, extra in jobs:
        delta, arrays = pick_delta(conf)
        ckpt = os.path.join(work, name + ".pth")
        torch.save({"module." + k: torch.from_numpy(v) for k, v in arrays.items()}, ckpt)
        outdir = os.path.join(work, "out_" + name)
        del captured[:]
        try:
            os.chdir(os.path.join(MG.TPM, "evaluate"))
            YoloPoseNet.forward, aug.Cvt2ndarray.__call__ = forward, cvt
            init.__defaults__ = real_defaults[:1] + (EC.W, EC.H) + real_defaults[3:]
            globmod.glob = lambda pat, *a, **k: list(tree["ann_files"]) if "labels_test_" in pat else real_glob(pat, *a, **k)
            sys.argv = ["eval", "--bg-file", tree["bg_file"], "--bg-dir", tree["bg"], "--seg-dir", tree["seg"], "--batch-size", "3", "--input-size", str(EC.S),
                        "--w-org", str(EC.W), "--h-org", str(EC.H), "--weight", ckpt, "--output-dir", outdir] + extra
            random.seed(SEED)
            with contextlib.redirect_stdout(io.StringIO()):
                try:
                    runpy.run_path(os.path.join(MG.TPM, "evaluate", script), run_name="__main__")
                except Exception as e:      # the script's own metric tail may trip after eval_data.json has been written
                    import traceback
                    print("%s: script raised: %r at %s" % (name, e, traceback.extract_tb(e.__traceback__)[-1]), file=sys.stderr)
        finally:
            YoloPoseNet.forward, aug.Cvt2ndarray.__call__, globmod.glob = real_forward, real_cvt, real_glob
            init.__defaults__ = real_defaults
            sys.argv = argv
            os.chdir(cwd)
        data = json.load(open(os.path.join(outdir, "eval_data.json")))
        keep = dict(data, metrics=_metrics(data), conf_weight_shift=delta, weight_seed=1, seed=SEED, conf_threshold=conf)
        json.dump(keep, open(os.path.join(MG.OUT, "script_eval_data_%s.json" % name), "w"))
        np.savez_compressed(os.path.join(MG.OUT, "script_eval_data_%s.npz" % name), inputs=np.concatenate(captured))
        print("%s: persons per frame" % name, [len(f) for f in data["human_pred_set_2d"]], "delta", delta)


# ---- the two Open-Pose+ evaluation SCRIPTS, end to end ---------------------------------------------------------------------------------
ABLATION_BLOCKS = (("human_gt_set_2d", "human_pred_set_3d_perfect_2d", "perfect_2d"),
                   ("human_gt_set_2d_visible", "human_pred_set_3d_perfect_2d", "perfect_2d_visible"),
                   ("human_pred_set_2d", "human_pred_set_3d_read_raw_depth", "raw"),
                   ("human_gt_set_2d", "human_pred_set_3d_perfect_2d_read_raw_depth", "raw_perfect_2d"),
                   ("human_gt_set_2d_visible", "human_pred_set_3d_perfect_2d_read_raw_depth", "raw_perfect_2d_visible"))


def _ablation_metrics(data):
    """The five blocks of the scripts' metric tail (make_golden_ablation.METRIC_BLOCKS) through the reference's eval_human_dataset_3d."""
    import contextlib
    import copy
    import io
    from evaluate.eval_pose_mp import eval_human_dataset_3d
    out = {}
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        for k2, k3, name in ABLATION_BLOCKS:
            d, k = eval_human_dataset_3d(copy.deepcopy(data[k2]), copy.deepcopy(data["human_gt_set_2d"]), copy.deepcopy(data[k3]),
                                         copy.deepcopy(data["human_gt_set_3d"]), num_joints=15, dist_th=0.1, iou_th=0.5)
            out["pck3d_" + name], out["err3d_" + name] = [float(v) for v in k], [float(v) for v in d]
    return out


def golden_rtpose_scripts(loader_images, frac=0.08):
    """evaluation_rtpose_light3d_kdh3d_ablation.py and evaluation_rtpose_light3d_kdh3d_mpaug_ablation.py under runpy.  One more recipe-side
    stand-in: lib.utils.common.paf_to_human_list hands back its first two values, the two the scripts unpack (it returns three; as written
    the scripts stop there with "too many values to unpack").  Weights: seeded, the stage-2 heat bias shifted per channel
    (make_golden.calibrated_heat_bias on the single-person loader's inputs) so that persons are found on 4 x 4 maps; the shift is stored.
    Kept next to eval_data.json: the network inputs and the three maps the reference module returned for them."""
    import contextlib
    import glob as globmod
    import io
    import json
    import runpy
    import torch
    from popnet_amd import synth
    from lib.datasets import data_augmentation_2d3d as aug
    from lib.datasets import datasets_kdh3d_rtpose, datasets_kdh3d_rtpose_mpaug
    from lib.network.rtpose_light3d import rtpose_light3d
    from lib.utils import common
    work = tempfile.mkdtemp(prefix="popnet_fake_evalsets_rtpose_")
    tree = EC.write_tree(work)
    for mod in (datasets_kdh3d_rtpose, datasets_kdh3d_rtpose_mpaug):
        mod.intrinsics.clear()
        mod.intrinsics.update(EC.INTRINSICS)
    model = rtpose_light3d(15, 14, 2, input_dim=1).eval()
    arrays = synth.fill_state_dict(model.state_dict(), seed=0)
    model.load_state_dict(MG.np_sd(arrays))
    shift = MG.calibrated_heat_bias(model, np.ascontiguousarray(loader_images, dtype=np.float32), frac=frac)
    arrays["model2_2.12.bias"][:15] += shift
    ckpt = os.path.join(work, "rtpose.pth")
    torch.save({"module." + k: torch.from_numpy(v) for k, v in arrays.items()}, ckpt)
    captured = []
    real_forward, real_cvt, real_glob, real_list = rtpose_light3d.forward, aug.Cvt2ndarray.__call__, globmod.glob, common.paf_to_human_list

    def forward(self, x):
        res = real_forward(self, x)
        captured.append((x.detach().cpu().numpy().copy(),) + tuple(t.detach().cpu().numpy().copy() for t in res[0][-3:]))
        return res

    def cvt(self, data):
        return Joints3dToArray()(real_cvt(self, data))

    jobs = (("kdh3d", "evaluation_rtpose_light3d_kdh3d_ablation.py", ["--annotations", tree["single_ann"], "--loader-workers", "0"]),
            ("mpaug", "evaluation_rtpose_light3d_kdh3d_mpaug_ablation.py", ["--num-batches", "2"]))
    argv, cwd = sys.argv, os.getcwd()
    import matplotlib
    matplotlib.use("Agg")
    for name, script, extra in jobs:
        outdir = os.path.join(work, "out_" + name)
        del captured[:]
        try:
            os.chdir(os.path.join(MG.TPM, "evaluate"))
            rtpose_light3d.forward, aug.Cvt2ndarray.__call__ = forward, cvt
            common.paf_to_human_list = lambda *a, **k: real_list(*a, **k)[:2]
            globmod.glob = lambda pat, *a, **k: list(tree["ann_files"]) if "labels_test_" in pat else real_glob(pat, *a, **k)
            sys.argv = ["eval", "--image-dir", tree["img"], "--bg-file", tree["bg_file"], "--bg-dir", tree["bg"], "--seg-dir", tree["seg"], "--batch-size", "3",
                        "--input-size", str(EC.S), "--w-org", str(EC.W), "--h-org", str(EC.H), "--weight", ckpt, "--output-dir", outdir] + extra
            random.seed(SEED)
            with contextlib.redirect_stdout(io.StringIO()):
                try:
                    runpy.run_path(os.path.join(MG.TPM, "evaluate", script), run_name="__main__")
                except Exception as e:      # the script's own metric tail may trip after eval_data.json has been written
                    import traceback
                    print("%s: script raised: %r at %s" % (name, e, traceback.extract_tb(e.__traceback__)[-1]), file=sys.stderr)
        finally:
            rtpose_light3d.forward, aug.Cvt2ndarray.__call__, globmod.glob, common.paf_to_human_list = real_forward, real_cvt, real_glob, real_list
            sys.argv = argv
            os.chdir(cwd)
        data = json.load(open(os.path.join(outdir, "eval_data.json")))
        metrics = dict(_metrics(data), **_ablation_metrics(data))
        keep = dict(data, metrics=metrics, heat_bias_shift=shift.tolist(), weight_seed=0, seed=SEED)
        json.dump(keep, open(os.path.join(MG.OUT, "script_eval_data_%s.json" % name), "w"))
        np.savez_compressed(os.path.join(MG.OUT, "script_eval_data_%s.npz" % name), inputs=np.concatenate([c[0] for c in captured]),
                            paf=np.concatenate([c[1] for c in captured]), heat=np.concatenate([c[2] for c in captured]),
                            z=np.concatenate([c[3] for c in captured]))
        print("%s: persons per frame" % name, [len(f) for f in data["human_pred_set_2d"]], "visible joints",
              [[int(np.sum(v)) for v in f] for f in data["visibility_pred_set"]])


if __name__ == "__main__":
    assert os.path.isdir(MG.REF), "the reference tree is needed to (re)generate golden vectors"
    check = "--check" in sys.argv[1:]
    if check:
        MG.OUT = tempfile.mkdtemp(prefix="popnet_golden_evalsets_check_")
    MG.SHIMS["cv2/__init__.py"] += "\n        from cv2_warp_reference import warpAffine, getRotationMatrix2D\n"
    # the composed Yolo script hard-codes vis=True: its drawing calls (cvtColor, rectangle, circle, imshow, waitKey, ...) hand back their image
    MG.SHIMS["cv2/__init__.py"] += """
        def __getattr__(k):
            if k.startswith('__'): raise AttributeError(k)
            return lambda *a, **kw: (a[0] if a else None)
"""
    MG.install_shims()
    loaders = golden_evalsets()
    golden_yolo_scripts(loaders["single1_images"])
    golden_rtpose_scripts(loaders["single0_images"])
    if check:
        fails = MG.check_outputs(MG.OUT)
        if fails:
            print("GOLDEN CHECK FAILED:\n  " + "\n  ".join(fails))
            sys.exit(1)
        print("golden check ok: %d files regenerate identically" % len(os.listdir(MG.OUT)))
