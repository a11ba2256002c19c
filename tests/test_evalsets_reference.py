"""CPU: the host half of the composed and single-person KDH3D evaluation sets against tests/evalsets_reference.py -- the chain without
Crop (targets.augmentation(crops=None), draw_augmentation(crop=False)), the test-set sampler (MPAugSampler.test_batch), the ground truth
scaled back to the original frame, the scripts' list conventions (dataset.kdh3d_pose_lists, dataset.yolo_kdh3d_lists) -- and the fake
tree of tests/evalsets_cases.py itself: a tree that lost one of its edge cases fails here.

Everything compared here is integer geometry, float32 label arithmetic restated operation for operation, or a selection of rows: ==."""
import random

import numpy as np
import pytest

import evalsets_cases as EC
import evalsets_reference as ER
from oracle import targets as ot
from popnet_amd import _lib, dataset, profiles, targets

GEOM = dict(H=EC.H, W=EC.W, cx=EC.CX, cy=EC.CY, input_size=EC.S)


@pytest.fixture(scope="module")
def data():
    return EC.build()


@pytest.fixture(scope="module")
def drawn():
    """The restatement's two batches of three items under DRAW_SEED, and Python's next random number after them."""
    random.seed(EC.DRAW_SEED)
    items = ER.batch_draws(3, EC.SET_SIZES, EC.N_BG) + ER.batch_draws(3, EC.SET_SIZES, EC.N_BG)
    return items, random.random()


def test_draw_seed_covers_every_branch(drawn):
    items, _ = drawn
    joined = [len(i["sources"]) for i in items if not i["fallback"]]
    geo = [targets.augmentation(i["rot"], i["a"], None, **GEOM) for i in items]
    assert 1 in joined and 2 in joined and any(i["fallback"] for i in items)
    assert any(g["render_a"] < 1 for g in geo) and any(g["render_a"] > 1 for g in geo)
    assert all((g["src_w"], g["src_h"]) != (2 * EC.S, 2 * EC.S) for g in geo)
    assert {ii for i in items for ii, _ in i["sources"]} >= {0, 1, 2}


def test_sampler_reproduces_the_restated_draws(drawn):
    items, after = drawn
    sm = targets.MPAugSampler(EC.SET_SIZES, EC.N_BG)
    random.seed(EC.DRAW_SEED)
    got = [sm.test_batch(3, max(EC.SET_SIZES), crop=False, **GEOM) for _ in range(2)]
    assert random.random() == after                                              # not one draw more or fewer
    for k, (idx, src, n_src, bg, aug) in enumerate(got):
        want = items[3 * k:3 * k + 3]
        assert idx.tolist() == [w["index"] for w in want] and bg.tolist() == [w["bg"] for w in want]
        assert n_src.tolist() == [len(w["sources"]) for w in want] and n_src.dtype == np.int32
        for b, w in enumerate(want):
            assert [tuple(r) for r in src[b, :n_src[b]].tolist()] == w["sources"] and (src[b, n_src[b]:] == -1).all()
            assert (aug.items[b]["rot"], aug.items[b]["a"], aug.items[b]["crops"]) == (w["rot"], w["a"], None)


def test_crop_false_skips_exactly_the_four_crop_draws():
    random.seed(9)
    it = targets.draw_augmentation(crop=False, **GEOM)
    nxt = random.random()
    random.seed(9)
    assert (it["rot"], it["a"]) == (random.uniform(-10, 10), random.uniform(0.7, 1.7)) and nxt == random.random()
    random.seed(9)
    full = targets.draw_augmentation(**GEOM)                                     # the default still draws six
    random.seed(9)
    six = [random.uniform(-10, 10), random.uniform(0.7, 1.7)] + [random.uniform(0, 0.1) for _ in range(4)]
    assert [full["rot"], full["a"]] + list(full["crops"]) == six
    # Hflip's coin keeps its place between RenderDepth's draw and where Crop's would be
    random.seed(9)
    fl = targets.draw_augmentation(crop=False, hflip=True, swap_indices=profiles.ITOP.swap_indices, **GEOM)
    random.seed(9)
    random.uniform(-10, 10), random.uniform(0.7, 1.7)
    assert fl["hflip"] == (random.uniform(0, 1) >= 0.5) and fl["crops"] is None


def test_no_crop_geometry_and_labels_equal_the_restatement(data, drawn):
    items, _ = drawn
    for it in items:
        image, persons = EC.composed_item(data, it)
        _, want, geo = ER.nocrop_reference(image, persons, dict(rot=it["rot"], a=it["a"], cx=EC.CX, cy=EC.CY, input_size=EC.S))
        g = targets.augmentation(it["rot"], it["a"], None, **GEOM)
        assert g["render_corner"] == geo["render_corner"] and g["render_a"] == geo["render_a"]
        assert (g["src_h"], g["src_w"]) == geo["render_shape"] == (g["render_h"], g["render_w"])
        assert (g["crop_x0"], g["crop_y0"], g["crop_x1"], g["crop_y1"]) == (0, 0, g["render_w"], g["render_h"])
        k2 = np.array([[p["2d_joints"] for p in persons]], dtype=np.float32)
        k3 = np.array([[p["3d_joints"] for p in persons]], dtype=np.float64)
        kp, kz, _ = targets.AugmentationBatch([g]).transform_labels(k2, k3)
        assert np.array_equal(kp[0], np.stack([w["2d_joints"] for w in want]))
        assert np.array_equal(kz[0], np.stack([w["3d_joints"][:, 2] for w in want]))
        # ... and the ground truth the scripts collect from them
        gt2, gt3 = targets.composed_ground_truth(kp, k3, kz, [len(persons)], EC.W, EC.H, EC.S)
        assert gt2[0] == ER.gt_to_original(want, EC.W, EC.H, EC.S)
        assert gt3[0] == [w["3d_joints"].tolist() for w in want]


def test_no_crop_is_not_crop_with_zero_fractions():
    """Crop's xmax = w - 1 - 0 and the exclusive slice drop the last row and column; without Crop they stay."""
    a = targets.augmentation(3.0, 1.2, None, **GEOM)
    z = targets.augmentation(3.0, 1.2, (0.0, 0.0, 0.0, 0.0), **GEOM)
    assert (a["src_w"], a["src_h"]) == (z["src_w"] + 1, z["src_h"] + 1) == (a["render_w"], a["render_h"])
    assert a["inv_mat"] == z["inv_mat"] and a["render_corner"] == z["render_corner"]


def test_tree_holds_its_edge_cases(data):
    j = np.array([p["2d_joints"] for ann in data["annos"] for k, v in ann.items() if k != "intrinsics" for p in v])
    x, y = j[..., 0], j[..., 1]
    assert (x < 0).any() and (x == EC.W).any() and (x > EC.W).any() and (y == EC.H).any() and (y > EC.H).any()
    assert (x == 0).any() and (x == EC.W - 1).any()
    assert [len(i) for i in data["ids"]] == list(EC.SET_SIZES) and len(data["bg_names"]) == EC.N_BG
    assert max(max(m) for m in targets.AUG_MODS) < len(EC.SET_SIZES)              # every aug_mods entry is reachable
    assert max(len(m) for m in targets.AUG_MODS) == 2 == max(len(m) for m in ER.AUG_MODS)      # ... and none composes more than two sources
    name = data["single_ids"][0]
    f, m = data["frames"][name].astype(np.float32), data["masks"][name]
    assert f[EC.FAR] > 2 * EC.DMAX and f[EC.FAR[0], EC.FAR[1] + 1] < 2.0 and m[EC.FAR] == 1 and m[EC.FAR[0], EC.FAR[1] + 1] == 1
    assert any((b.astype(np.float32) > EC.DMAX).any() for b in data["bgs"].values())
    assert all(len(data["single"][n]) >= 1 for n in data["single_ids"])


def test_background_swap_is_a_select_and_keeps_what_the_z_buffer_cuts(data):
    for i, name in enumerate(data["single_ids"]):
        f, m, bg = data["frames"][name], data["masks"][name], data["bgs"][data["bg_names"][i % EC.N_BG]]
        want = ER.compose_bg(f, m, bg)
        assert np.array_equal(want, np.where(m > 0, f, bg).astype(np.float64))
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)   # float16 inputs: float32 holds the result exactly
    name = data["single_ids"][0]
    f, m, bg = data["frames"][name], data["masks"][name], data["bgs"][data["bg_names"][0]]
    zbuf, _ = ot.compose_depth(f[None], m[None], bg)
    swap = ER.compose_bg(f, m, bg)
    assert swap[EC.FAR] == 12.5 and zbuf[EC.FAR] == 2 * EC.DMAX
    diff = swap != zbuf
    assert diff[EC.FAR] and not diff[m == 0].any()


def _pose_lists():
    rng = np.random.default_rng(5)
    counts = (2, 0, 1)
    mk = lambda n, shape: rng.normal(size=(n,) + shape).tolist()      # noqa: E731
    full = {"human_pred_set_2d": [mk(n, (15, 2)) for n in counts], "human_pred_set_3d": [mk(n, (15, 3)) for n in counts],
            "human_pred_set_visibility": [rng.integers(0, 2, (n, 15)).tolist() for n in counts],
            "human_pred_set_part_conf": [mk(n, (15,)) for n in counts]}
    abl = {"human_pred_set_3d_read_raw_depth": [mk(n, (15, 3)) for n in counts], "human_pred_set_3d_perfect_2d": [mk(3, (15, 3)) for _ in counts],
           "human_pred_set_3d_perfect_2d_read_raw_depth": [mk(3, (15, 3)) for _ in counts], "human_gt_set_2d_visible": [mk(3, (15, 2)) for _ in counts]}
    return full, abl


def test_pose_list_conventions():
    full, abl = _pose_lists()
    out = dataset.kdh3d_pose_lists(full)
    assert set(out) == {"human_pred_set_2d", "human_pred_set_3d", "visibility_pred_set"}
    assert out["visibility_pred_set"] == full["human_pred_set_visibility"] and out["human_pred_set_2d"] == full["human_pred_set_2d"]
    both = dict(full, **abl)
    out = dataset.kdh3d_pose_lists(both, first_person=True)
    assert set(out) == {"human_pred_set_2d", "human_pred_set_3d", "visibility_pred_set"} | set(abl)
    for k_out, k_in in (("human_pred_set_2d",) * 2, ("human_pred_set_3d",) * 2, ("visibility_pred_set", "human_pred_set_visibility"),
                        ("human_pred_set_3d_read_raw_depth",) * 2):
        assert out[k_out] == ER.first_person(both[k_in])
        assert [len(f) for f in out[k_out]] == [1, 0, 1]                          # an empty frame stays empty: no placeholder in this net's scripts
    for k in ("human_pred_set_3d_perfect_2d", "human_pred_set_3d_perfect_2d_read_raw_depth", "human_gt_set_2d_visible"):
        assert out[k] == abl[k]                                                   # these follow the ground-truth persons
    assert dataset.kdh3d_pose_lists(both)["human_pred_set_3d_read_raw_depth"] == abl["human_pred_set_3d_read_raw_depth"]


def test_yolo_list_conventions():
    rng = np.random.default_rng(6)
    recs = np.zeros((3,), _lib.YOLO_FRAME_DTYPE)
    recs["joints_2d"] = rng.normal(size=recs["joints_2d"].shape)
    recs["joints_3d"] = rng.normal(size=recs["joints_3d"].shape)
    recs["n_det"] = (3, 0, 1)
    prof = profiles.get(None)
    hold2, hold3 = ER.yolo_lists([], prof.w_org, prof.h_org, 224, prof.intrinsics)
    every = dataset.yolo_kdh3d_lists(recs)
    first = dataset.yolo_kdh3d_lists(recs, first_person=True)
    assert set(every) == set(first) == {"human_pred_set_2d", "human_pred_set_3d"}
    assert [len(f) for f in every["human_pred_set_2d"]] == [3, 1, 1] and [len(f) for f in first["human_pred_set_3d"]] == [1, 1, 1]
    for out in (every, first):
        assert out["human_pred_set_2d"][1] == hold2 and out["human_pred_set_3d"][1] == hold3
        assert out["human_pred_set_2d"][2] == recs[2]["joints_2d"][:1].tolist()
    assert every["human_pred_set_3d"][0] == recs[0]["joints_3d"][:3].tolist() and first["human_pred_set_3d"][0] == recs[0]["joints_3d"][:1].tolist()
    # the placeholder at another input size and frame size: the restated script lines again
    small = dataset.yolo_kdh3d_lists(recs[1:2], input_size=EC.S, profile=prof)
    assert small["human_pred_set_2d"][0] == ER.yolo_lists([], prof.w_org, prof.h_org, EC.S, prof.intrinsics)[0]
    recs["status"][0] = 1
    with pytest.raises(_lib.PopnetError, match="overflow"):
        dataset.yolo_kdh3d_lists(recs)
    assert dataset.yolo_kdh3d_lists(recs, first_person=True)["human_pred_set_2d"][0] == first["human_pred_set_2d"][0]


def test_yolo_restatement_rescales_and_back_projects_like_the_script():
    """One person by hand: x / input_size * w_org, (x - cx) / fx * Z."""
    k = {"fx": 2.0, "fy": 4.0, "cx": 1.0, "cy": 3.0}
    h = np.zeros((15, 3))
    h[0] = (8.0, 16.0, 2.0)
    j2, j3 = ER.yolo_lists([h, h + 1], 64, 32, 32, k, first=True)
    assert len(j2) == 1 and j2[0][0] == [16.0, 16.0] and j3[0][0] == [(16.0 - 1.0) / 2.0 * 2.0, (16.0 - 3.0) / 4.0 * 2.0, 2.0]
    assert len(ER.yolo_lists([h, h + 1], 64, 32, 32, k)[0]) == 2


# ---------------------------------------------------------------------------------------------
# the restatement against the reference loaders' own outputs (tests/golden/evalsets_inputs.npz)
# ---------------------------------------------------------------------------------------------
def _logged_random(monkeypatch):
    log = []

    def wrap(kind, fn):
        def f(a, b):
            v = fn(a, b)
            log.append((kind, float(a), float(b), float(v)))
            return v
        return f
    monkeypatch.setattr(random, "randint", wrap(0, random.randint))
    monkeypatch.setattr(random, "uniform", wrap(1, random.uniform))
    return log


def test_restatement_reproduces_the_reference_loader_of_the_composed_set(data, monkeypatch):
    """Under the golden's seed: the shuffled orders, every draw in order with its arguments, the network inputs bit for bit and the
    transformed labels -- for the restatement, and the draws for the product's sampler."""
    from oracle import cv2_resize  # noqa: F401
    import cv2_warp_reference as cw
    G = EC.golden()
    seed = int(G["seed"])
    assert [int(v) for v in G["frame"]] == [EC.H, EC.W, EC.S]
    sh, _ = EC.shuffled(data, seed)
    state = random.getstate()
    assert [";".join(i) for i in sh["ids"]] == G["mpaug_ids"].tolist() and sh["bg_names"] == G["mpaug_bgs"].tolist()
    log = _logged_random(monkeypatch)
    batches = [ER.batch_draws(3, EC.SET_SIZES, EC.N_BG) for _ in range(2)]
    want_log = np.concatenate([G["mpaug_b0_log"], G["mpaug_b1_log"]])
    assert np.array_equal(np.array(log, dtype=np.float64), want_log)
    log.clear()
    random.setstate(state)
    sm = targets.MPAugSampler(EC.SET_SIZES, EC.N_BG)
    for _ in range(2):
        sm.test_batch(3, max(EC.SET_SIZES), crop=False, **GEOM)
    assert np.array_equal(np.array(log, dtype=np.float64), want_log)                 # the product draws the same values in the same order
    seen = set()
    for k, items in enumerate(batches):
        row = 0
        for b, it in enumerate(items):
            image, persons = EC.composed_item(sh, it)
            img, lab, geo = ER.nocrop_reference(image, persons, dict(rot=it["rot"], a=it["a"], cx=EC.CX, cy=EC.CY, input_size=EC.S))
            assert np.array_equal(cw.network_input(img, EC.DMAX, EC.MEAN, EC.STD), G["mpaug_b%d_images" % k][b]), (k, b)
            n = int(G["mpaug_b%d_npers" % k][b])
            assert n == len(lab)
            assert np.array_equal(np.stack([l["2d_joints"] for l in lab]), G["mpaug_b%d_kp2d" % k][row:row + n])
            assert np.array_equal(np.stack([l["3d_joints"] for l in lab]), G["mpaug_b%d_kp3d" % k][row:row + n])
            row += n
            seen |= {("fallback", it["fallback"]), ("sources", len(it["sources"])), ("a<=1", geo["render_a"] <= 1)}
    # the golden really holds each case: one source, two, nobody joined, RenderDepth shrinking and growing
    assert seen >= {("fallback", True), ("fallback", False), ("sources", 1), ("sources", 2), ("a<=1", True), ("a<=1", False)}


@pytest.mark.parametrize("bg_aug", [0, 1])
def test_restatement_reproduces_the_reference_loader_of_the_single_person_sets(data, bg_aug):
    from oracle import cv2_resize
    import cv2_warp_reference as cw
    G = EC.golden()
    _, bgs = EC.shuffled(data, int(G["seed"]))
    assert bgs == G["single_bgs"].tolist()
    want = G["single%d_images" % bg_aug]
    assert want.shape == (6, 1, EC.S, EC.S)
    for i, name in enumerate(data["single_ids"]):
        f = data["frames"][name].astype(np.float64)
        if bg_aug:
            f = ER.compose_bg(f, data["masks"][name], data["bgs"][bgs[i % EC.N_BG]])
        img = cv2_resize.resize(f.astype(np.float32), (EC.S, EC.S), interpolation=cv2_resize.INTER_LINEAR)
        assert np.array_equal(cw.network_input(img, EC.DMAX, EC.MEAN, EC.STD), want[i, 0]), i
    if bg_aug:      # the pixel above 2 * depth_max reached the network input: the swap without a cap differs from the z-buffer composition there
        name = data["single_ids"][0]
        capped = np.minimum(ER.compose_bg(data["frames"][name], data["masks"][name], data["bgs"][bgs[0]]), 2 * EC.DMAX)
        img = cv2_resize.resize(capped.astype(np.float32), (EC.S, EC.S), interpolation=cv2_resize.INTER_LINEAR)
        assert not np.array_equal(cw.network_input(img, EC.DMAX, EC.MEAN, EC.STD), want[0, 0])
