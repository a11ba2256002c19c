#!/usr/bin/env python
"""Generates tests/golden/augment.npz by running the REFERENCE ITSELF (imported read-only, with the import shims of make_golden.py):
its own Rotate, RenderDepth, Crop and Resize classes (lib/datasets/data_augmentation_2d3d.py) inside the full training chain

    Compose([Cvt2ndarray(), Rotate(cx, cy), RenderDepth(cx, cy, max_ratio=1.7), Crop(), Resize(224)])

through KDH3D_Keypoints.__getitem__ of both trainers' datasets (lib/datasets/datasets_kdh3d_rtpose_mpaug.py for the four target maps,
lib/datasets/datasets_kdh3d_mpaug.py for the prior maps) on a small fake MP-3DHP tree.

    python tests/golden/make_golden_augment.py            # rewrites tests/golden/augment.npz
    python tests/golden/make_golden_augment.py --check    # regenerates into a scratch dir and compares (tests/test_augment_golden_recipe.py)

Only data leaves this script: per item the six draws, the integers the chain derived (image shapes after every stage), the
transformed labels, the image and the target maps.  The frames are NOT stored: `write_fake_tree` rebuilds them from its seed, and
the fixture names the files every item composed, so a test replays an item from the tree it writes itself.

Two things stand in for what the reference needs and this suite lacks:
  * cv2: the shim routes cv2.resize to oracle/cv2_resize.py and cv2.warpAffine / cv2.getRotationMatrix2D to tests/cv2_warp_reference.py
    (restatements of OpenCV 4.2's scalar paths; agreement with a live cv2 build is unverified, see those files).
  * `Joints3dToArray`, inserted after Cvt2ndarray.  RenderDepth does `label['3d_joints'][:, 2] *= a`, and Cvt2ndarray converts
    '2d_joints', 'visible_joints' and 'bbox' to arrays but never '3d_joints'.  On annotations straight from JSON (nested lists) that
    line raises "TypeError: list indices must be integers or slices, not tuple" -- confirmed here (`reference_raises_on_json_lists`).
    The evident intent is z times a; the transform turns '3d_joints' into a float64 array so that the line does what it says.
    (The YoloPoseNet dataset's get_ground_truth indexes ann['3d_joints'][:, 2] too, so it needs the array even without RenderDepth.)

`uniform` of the augmentation module is wrapped: it logs every value it returns, and for the scripted items it hands out fixed
values to force the boundary cases (rot 0 and +-10, a at 0.7 and 1.7, a just above 1 with new_xmin truncating to 0 while new_ymin
does not, a just above 1 with both truncating to 0, all crops 0 and all crops 0.1).
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden as mg  # noqa: E402

OUT = HERE
H, W, S = 320, 240, 224                    # small frames keep the recipe fast; the path is size-agnostic
CX, CY = 100.25, 140.5                     # an off-centre principal point (the MP-3DHP one is off-centre too), left of and above the middle
MAX_RATIO = 1.7

# (name, dataset index, scripted draws or None = seeded random): rot, a, crop left, right, top, bottom
CASES = [
    ("random0", 0, None),
    ("random1", 1, None),
    ("rot0_a0.7_crop0", 0, (0.0, 0.7, 0.0, 0.0, 0.0, 0.0)),
    ("rot10_a1.7_crop0.1", 1, (10.0, 1.7, 0.1, 0.1, 0.1, 0.1)),
    # a just above 1: the corner a (0 - c) + c is (-(a - 1) cx, -(a - 1) cy).  With a - 1 = 0.0085 the x corner is -0.85 -> 0 and the
    # y corner -1.19 -> -1: ax = 1, ay > 1, so the zero-image branch runs with dx = 0, dy = 1
    ("rot-10_mixed", 0, (-10.0, 1.0085, 0.03, 0.07, 0.0, 0.1)),
    # a - 1 = 0.0065: both corners truncate to 0 (-0.65, -0.91), a recomputes to exactly 1 and the `a <= 1` slice runs with
    # new_ymax = int(321.17) = 321 beyond the 320 rows: numpy clamps the slice end
    ("both_truncate", 1, (3.5, 1.0065, 0.1, 0.0, 0.05, 0.02)),
]


class Joints3dToArray(object):
    """Recipe-side transform (see the module docstring): '3d_joints' as a float64 [15, 3] array."""

    def __call__(self, data):
        image, label = data
        for lb in label:
            lb["3d_joints"] = np.array(lb["3d_joints"], dtype=np.float64).reshape([15, 3])
        return image, label


class Tap(object):
    """Runs a transform of the reference and notes the shape of the image it returns and the labels."""

    def __init__(self, fn, log):
        self.fn, self.log = fn, log

    def __call__(self, data):
        image, label = self.fn(data)
        self.log.append((type(self.fn).__name__, tuple(image.shape), label))
        return image, label


def write_fake_tree(d, seed=177):
    """A tiny MP-3DHP training tree under `d` (five annotation sets of two frames, two backgrounds), every person with '2d_joints',
    '3d_joints', 'bbox' and 'pose_weight'.  Deterministic in `seed`: the tests rebuild the same files.  -> the annotation file list."""
    from popnet_amd import synth
    for sub in ("img", "seg", "bg"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    rng = np.random.default_rng(seed)
    ann_files = []
    for ii in range(5):
        ann = {"intrinsics": {"fx": 252.0594940185547, "fy": 252.0213623046875, "cx": CX, "cy": CY}}
        for f in range(2):
            name = "s%d_%d.npy" % (ii, f)
            joints, depths = synth.planted_persons(rng, 1, size=224)
            j2 = joints[0] * [W / 224.0, H / 224.0]
            x0, x1 = int(j2[:, 0].min()) - 10, int(j2[:, 0].max()) + 10
            y0, y1 = int(j2[:, 1].min()) - 10, int(j2[:, 1].max()) + 10
            ann[name] = [{"2d_joints": j2.tolist(), "3d_joints": np.concatenate([j2, np.full((15, 1), depths[0])], 1).tolist(),
                          "bbox": [float(x0), float(y0), float(x1), float(y1)], "pose_weight": float(rng.uniform(0.5, 3.0))}]
            depth = np.clip(rng.normal(depths[0], 0.1, (H, W)), 0.3, 5.9)
            mask = np.zeros((H, W))
            mask[max(y0, 0):y1, max(x0, 0):x1] = 1.0
            np.save(os.path.join(d, "img", name), depth.astype(np.float16))
            np.save(os.path.join(d, "seg", name), mask.astype(np.uint8))
        path = os.path.join(d, "ann%d.json" % ii)
        json.dump(ann, open(path, "w"))
        ann_files.append(path)
    bgs = {}
    for f in range(2):
        name = "bg%d.npy" % f
        np.save(os.path.join(d, "bg", name), np.clip(rng.normal(4.5, 0.3, (H, W)), 0, 6).astype(np.float16))
        bgs[str(f)] = {"file_name": name}
    json.dump(bgs, open(os.path.join(d, "bg.json"), "w"))
    return ann_files


def reference_raises_on_json_lists(aug):
    """The observation behind Joints3dToArray: the reference's chain without it, on JSON-style labels."""
    chain = aug.Compose([aug.Cvt2ndarray(), aug.RenderDepth(cx=CX, cy=CY, max_ratio=MAX_RATIO)])
    lab = [{"2d_joints": np.zeros((15, 2)).tolist(), "3d_joints": np.ones((15, 3)).tolist()}]
    try:
        chain((np.ones((H, W)), lab))
    except TypeError as e:
        return str(e)
    return ""


def golden_augment():
    import importlib
    import random
    aug = importlib.import_module("lib.datasets.data_augmentation_2d3d")
    mods = {"rtpose": importlib.import_module("lib.datasets.datasets_kdh3d_rtpose_mpaug"), "yolo": importlib.import_module("lib.datasets.datasets_kdh3d_mpaug")}
    d = tempfile.mkdtemp(prefix="popnet_augment_")
    ann_files = write_fake_tree(d)

    drawn, script = [], []
    plain_uniform = aug.uniform

    def uniform(lo, hi):
        v = script.pop(0) if script else plain_uniform(lo, hi)
        drawn.append(float(v))
        return v
    aug.uniform = uniform                                      # the name Rotate / RenderDepth / Crop call
    msg = reference_raises_on_json_lists(aug)
    assert "list indices must be integers or slices" in msg, msg
    del drawn[:]

    log = []
    chain = aug.Compose([Tap(t, log) for t in (aug.Cvt2ndarray(), Joints3dToArray(), aug.Rotate(cx=CX, cy=CY),
                                               aug.RenderDepth(cx=CX, cy=CY, max_ratio=MAX_RATIO), aug.Crop(), aug.Resize(S))])
    out = {"names": np.array([c[0] for c in CASES]), "n_items": np.array(len(CASES)), "frame": np.array([H, W, S]), "centre": np.array([CX, CY]),
           "tree_seed": np.array(177), "json_list_error": np.array(msg)}
    sets = {}
    for net, mod in mods.items():
        random.seed(5)
        sets[net] = mod.KDH3D_Keypoints(os.path.join(d, "img"), ann_files, preprocess=chain, w_org=W, h_org=H, input_x=S, input_y=S, stride=8, z_radius=2,
                                        bg_file=os.path.join(d, "bg.json"), bg_dir=os.path.join(d, "bg"), seg_dir=os.path.join(d, "seg"))
    out["ids"] = np.array([[nm for nm in ids] for ids in sets["rtpose"].ids_list])          # the shuffled id lists (random.seed(5))
    out["bgs"] = np.array([b["file_name"] for b in sets["rtpose"].bg_list])
    assert sets["yolo"].ids_list == sets["rtpose"].ids_list and sets["yolo"].bg_list == sets["rtpose"].bg_list
    random.seed(9)
    for ci, (name, idx, draws) in enumerate(CASES):
        ds, mod = sets["rtpose"], mods["rtpose"]
        state = random.getstate()
        # replay the item's source draws to record WHICH sources it composes (as make_golden.golden_targets does)
        mod_id = random.randint(0, len(mod.aug_mods) - 1)
        picks = []
        for ii in mod.aug_mods[mod_id]:
            if mod.uniform(0, 1) > 0.8:
                continue
            picks.append(ii)
        if not picks:
            picks.append(random.randint(0, len(ds.ids_list) - 1))
        per_net = {}
        for net in ("rtpose", "yolo"):                         # the same generator state for both datasets: the same item
            random.setstate(state)
            script[:] = list(draws) if draws else []
            del drawn[:], log[:]
            item = sets[net][idx]
            assert not script and len(drawn) == 6, (name, drawn)
            per_net[net] = (item, list(drawn), list(log))
        (it_r, draws_r, log_r), (it_y, draws_y, log_y) = per_net["rtpose"], per_net["yolo"]
        assert draws_r == draws_y and np.array_equal(it_r[0].numpy(), it_y[0].numpy())
        labels = log_r[-1][2]
        k = "it%d_" % ci
        out.update({k + "index": np.array(idx), k + "picks": np.array(picks), k + "draws": np.array(draws_r),
                    k + "scripted": np.array(draws is not None),
                    k + "shapes": np.array([s for n, s, _ in log_r if n in ("Rotate", "RenderDepth", "Crop", "Resize")]),
                    k + "kp2d": np.stack([lb["2d_joints"] for lb in labels]), k + "kp3d": np.stack([lb["3d_joints"] for lb in labels]),
                    k + "bbox": np.stack([lb["bbox"] for lb in labels]), k + "pose_weight": np.array([lb["pose_weight"] for lb in labels]),
                    k + "image": it_r[0].numpy(), k + "heat": it_r[1].numpy(), k + "paf": it_r[2].numpy(), k + "z": it_r[3].numpy(), k + "fg": it_r[4].numpy(),
                    k + "prior": it_y[7].numpy(), k + "conf": it_y[8].numpy(), k + "coord": it_y[9].numpy(), k + "weight": it_y[10].numpy()})
        assert out[k + "kp2d"].dtype == np.float32 and out[k + "kp3d"].dtype == np.float64 and out[k + "bbox"].dtype == np.float64
        # the yolo dataset's labels went through the same chain
        assert all(np.array_equal(a["2d_joints"], b["2d_joints"]) and np.array_equal(a["bbox"], b["bbox"]) for a, b in zip(labels, log_y[-1][2]))
        if draws is None:                                      # where the generator stands after the seeded items, which come first: a
            state = random.getstate()                          # seeded MPAugSampler.batch(augment=True) must arrive at the same place
            out["next_after_random_items"] = np.array(random.random())
            random.setstate(state)
    np.savez_compressed(os.path.join(OUT, "augment.npz"), **out)
    print("augment.npz: %d items, %d bytes" % (len(CASES), os.path.getsize(os.path.join(OUT, "augment.npz"))))
    for ci, c in enumerate(CASES):
        print("  %-22s shapes %s persons %d" % (c[0], out["it%d_shapes" % ci].tolist(), out["it%d_kp2d" % ci].shape[0]))


if __name__ == "__main__":
    assert os.path.isdir(mg.REF), "the reference tree is needed to (re)generate golden vectors"
    import torch.optim                 # noqa: F401  -- before the torchvision shim is importable (see make_golden.py)
    import torch.distributed.tensor    # noqa: F401
    mg.SHIMS["cv2/__init__.py"] += "\n        from cv2_warp_reference import warpAffine, getRotationMatrix2D\n"
    mg.install_shims()
    import popnet_amd  # noqa: F401
    check = "--check" in sys.argv[1:]
    if check:
        OUT = tempfile.mkdtemp(prefix="popnet_golden_augment_check_")
    golden_augment()
    if check:
        fails = mg.check_outputs(OUT)
        if fails:
            print("GOLDEN CHECK FAILED:\n  " + "\n  ".join(fails))
            sys.exit(1)
        print("golden check ok: %d files regenerate identically" % len(os.listdir(OUT)))
