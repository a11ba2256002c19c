"""The fake KDH3D tree of the evaluation-set tests (tests/test_evalsets_reference.py, tests/test_gpu_evalsets.py): small enough that every
case runs in a moment, shaped so that the code can still go wrong.

  frames 40 x 36 (H x W), network input 32 -> 4 x 4 maps: neither axis is a 2x decimation, x shrinks by another ratio than y
  five annotation sets of 2 or 3 frames (every AUG_MODS entry is reachable), three backgrounds
  persons whose joints are negative, exactly on the far edge (x = W, y = H) and beyond the frame
  single-person set: frame 0 has one foreground pixel above 2 * depth_max next to a near one
Everything is drawn from one seeded generator; nothing is stored.
"""
import json
import os

import numpy as np

H, W, S = 40, 36, 32
CX, CY = 17.25, 20.5
INTRINSICS = {"fx": 38.0, "fy": 37.5, "cx": CX, "cy": CY}
DMAX, MEAN, STD = 6.0, 3.0, 2.0
SET_SIZES = (3, 2, 3, 2, 3)
N_BG = 3
SEED = 20
FAR = (7, 9)            # (y, x) of the single-person set's pixel above 2 * depth_max; (7, 10) next to it is near
# Python `random` seed (found by search, pinned by test_draw_seed_covers_every_branch) whose two batches of three items cover:
# an item with one source, one with two, one where nobody joined (the fallback randint), RenderDepth with a < 1 and with a > 1.
# Two is the most: every aug_mods entry of the reference names at most two sets (datasets_kdh3d_rtpose_mpaug.py:51, targets.AUG_MODS), so
# a frame with three or more sources cannot be drawn -- test_tree_holds_its_edge_cases asserts that bound.
DRAW_SEED = 2


def _person(rng, edge):
    base = rng.uniform([8, 10], [W - 8, H - 10])
    j2 = base + rng.uniform(-7, 7, (15, 2))
    if edge == 0:
        j2[0], j2[1], j2[2] = (-2.5, 11.0), (float(W), 20.0), (W + 3.5, 4.0)        # negative, exactly on the far edge, beyond
        j2[3], j2[4] = (12.0, float(H)), (5.0, H + 2.25)
    elif edge == 1:
        j2[5], j2[6] = (0.0, 0.0), (W - 1.0, H - 1.0)
    z = rng.uniform(1.5, 4.0)
    j3 = np.stack([(j2[:, 0] - CX) * z / INTRINSICS["fx"], (j2[:, 1] - CY) * z / INTRINSICS["fy"], np.full(15, z) + rng.normal(0, 0.05, 15)], 1)
    x0, y0, x1, y1 = j2[:, 0].min(), j2[:, 1].min(), j2[:, 0].max(), j2[:, 1].max()
    return {"2d_joints": j2.tolist(), "3d_joints": j3.tolist(), "bbox": [x0, y0, x1, y1], "pose_weight": 1.0}


def build():
    """-> dict: ids [set][frame], frames / masks {id: array}, annos [set] {id: persons}, bg_names, bgs {name: array}, single (the
    single-person set: ids, annos) -- float16 frames in metres, uint8 masks."""
    rng = np.random.default_rng(SEED)
    frames, masks, annos, ids = {}, {}, [], []
    for ii, n in enumerate(SET_SIZES):
        ann, names = {"intrinsics": INTRINSICS}, []
        for f in range(n):
            name = "s%d_f%d.npy" % (ii, f)
            depth = rng.uniform(1.0, 5.5, (H, W))
            depth[rng.random((H, W)) < 0.02] = 13.5                                   # speckle beyond 2 * depth_max, in and out of the masks
            m = np.zeros((H, W), np.uint8)
            y0, x0 = int(rng.integers(2, 14)), int(rng.integers(2, 12))
            m[y0:y0 + int(rng.integers(12, 22)), x0:x0 + int(rng.integers(8, 18))] = 1
            frames[name], masks[name] = depth.astype(np.float16), m
            ann[name] = [_person(rng, (ii + f) % 3) for _ in range(1 + (ii + f) % 2)]
            names.append(name)
        annos.append(ann)
        ids.append(names)
    bg_names = ["bg%d.npy" % i for i in range(N_BG)]
    bgs = {n: rng.uniform(3.0, 7.5, (H, W)).astype(np.float16) for n in bg_names}    # partly above depth_max: the clamp works
    # the single-person set: the frames of set 0 and 2, first person only in the labels' order
    single_ids = ids[0] + ids[2]
    single = {"intrinsics": INTRINSICS}
    for name in single_ids:
        single[name] = (annos[0] if name in annos[0] else annos[2])[name]
    f0 = frames[single_ids[0]].copy()
    m0 = masks[single_ids[0]].copy()
    f0[FAR], f0[FAR[0], FAR[1] + 1] = 12.5, 1.25
    m0[FAR[0] - 1:FAR[0] + 2, FAR[1] - 1:FAR[1] + 3] = 1
    frames[single_ids[0]], masks[single_ids[0]] = f0, m0
    return dict(ids=ids, frames=frames, masks=masks, annos=annos, bg_names=bg_names, bgs=bgs, single_ids=single_ids, single=single)


def write_tree(d, data=None):
    """Writes the tree under d the way the loaders read it.  -> dict of paths: img, seg, bg, bg_file, ann_files, single_ann."""
    data = build() if data is None else data
    d = str(d)
    for sub in ("img", "seg", "bg"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    for name, a in data["frames"].items():
        np.save(os.path.join(d, "img", name), a)
        np.save(os.path.join(d, "seg", name), data["masks"][name])
    for name, a in data["bgs"].items():
        np.save(os.path.join(d, "bg", name), a)
    json.dump({str(i): {"file_name": n} for i, n in enumerate(data["bg_names"])}, open(os.path.join(d, "bg.json"), "w"))
    ann_files = []
    for ii, ann in enumerate(data["annos"]):
        ann_files.append(os.path.join(d, "labels_%d.json" % ii))
        json.dump(ann, open(ann_files[-1], "w"))
    json.dump(data["single"], open(os.path.join(d, "labels_single.json"), "w"))
    return dict(img=os.path.join(d, "img"), seg=os.path.join(d, "seg"), bg=os.path.join(d, "bg"), bg_file=os.path.join(d, "bg.json"),
                ann_files=ann_files, single_ann=os.path.join(d, "labels_single.json"))


def composed_item(data, item):
    """The z-buffer composition of one drawn item (evalsets_reference.batch_draws) through the oracle, and its persons in source order."""
    from oracle import targets as ot
    depths, ms, persons = [], [], []
    for ii, f in item["sources"]:
        name = data["ids"][ii][f]
        depths.append(data["frames"][name])
        ms.append(data["masks"][name])
        persons += data["annos"][ii][name]
    image, _ = ot.compose_depth(np.stack(depths), np.stack(ms), data["bgs"][data["bg_names"][item["bg"]]])
    return image, persons


# ---- the reference loaders' own outputs on this tree (tests/golden/make_golden_evalsets.py) -------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evalsets_inputs.npz")


def golden():
    return np.load(GOLDEN)


def shuffled(data, seed):
    """The tree as the loaders see it after `random.seed(seed)` and their constructor's shuffles (every id list in file order, then the
    background list; the single-person loader shuffles only its backgrounds).  -> (data with the composed set's orders, the single-person
    loader's background order); Python's `random` is left where the constructor of the composed set leaves it."""
    import random
    random.seed(seed)
    bgs = list(data["bg_names"])
    random.shuffle(bgs)
    random.seed(seed)
    ids = [list(i) for i in data["ids"]]
    for i in ids:
        random.shuffle(i)
    bg_names = list(data["bg_names"])
    random.shuffle(bg_names)
    return dict(data, ids=ids, bg_names=bg_names), bgs
