"""Shared by the augmentation tests: the golden of the reference's random training transform (tests/golden/augment.npz) and the
replay of its items.  The fixture stores no frames: tests/golden/make_golden_augment.py's `write_fake_tree` rebuilds the fake
MP-3DHP tree from its seed, and the fixture names the files every item composed."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_augment as mga  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "augment.npz"))
H, W, S = (int(v) for v in G["frame"])
CX, CY = (float(v) for v in G["centre"])
N = int(G["n_items"])


def write_tree(d):
    """-> annotation file list of the tree written under d (the golden's own tree)."""
    return mga.write_fake_tree(str(d), seed=int(G["tree_seed"]))


def item_sources(d, ci):
    """What item ci composed: (fg_depths [n,H,W] f16, fg_masks [n,H,W] u8, bg [H,W] f16, persons: list of annotation dicts)."""
    d = str(d)
    idx = int(G["it%d_index" % ci])
    depths, masks, persons = [], [], []
    for ii in G["it%d_picks" % ci]:
        name = str(G["ids"][int(ii)][idx % G["ids"].shape[1]])
        depths.append(np.load(os.path.join(d, "img", name)))
        masks.append(np.load(os.path.join(d, "seg", name)))
        persons += json.load(open(os.path.join(d, "ann%d.json" % int(ii))))[name]
    bg = np.load(os.path.join(d, "bg", str(G["bgs"][idx % len(G["bgs"])])))
    return np.stack(depths), np.stack(masks), bg, persons


def item_params(ci):
    dr = G["it%d_draws" % ci]
    return dict(rot=float(dr[0]), a=float(dr[1]), crops=tuple(float(v) for v in dr[2:6]), cx=CX, cy=CY, input_size=S)


def composed(d, ci):
    """The frame the item's transform chain receives (float64, as the reference's compositor leaves it) and its persons."""
    from oracle import targets as ot
    depths, masks, bg, persons = item_sources(d, ci)
    image, _ = ot.compose_depth(depths, masks, bg)
    return image, persons


def ulp_distance_f32(a, b):
    """Element-wise distance in float32 steps (same-sign finite values)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)
