"""CPU: the four fixtures tests/golden/make_golden_evalsets.py recorded by running the REFERENCE's evaluation scripts end to end on the fake
tree of tests/evalsets_cases.py -- script_eval_data_{mpaug,mpaug_yolo,kdh3d,kdh3d_yolo}.json (eval_data.json, the metric values of the
reference's own eval_pose_mp on it, the weight recipe) and .npz (the network inputs; for Open-Pose+ also the three maps the reference
module returned).

  * the oracle's forward and parse on the recorded inputs, with the restated script lines of tests/evalsets_reference.py and
    tests/ablation_reference.py, reproduce every list -- at the bars tests/test_ablation_reference.py and tests/test_oracle_golden.py apply
    to the same quantities of the mpreal fixtures (assignment and visibility ==, the raw-depth arms ==, Open-Pose+ 2D 1e-9, what reads the
    pose-depth map 1e-5; Yolo-Pose+ 2D 2e-3 px, 3D 1e-4 m);
  * popnet_amd.metrics equals the recorded metric values at 1e-12;
  * the fixtures really hold their cases: an empty frame and a frame with several persons (Open-Pose+), the first-person cut, several
    detections in a frame (Yolo-Pose+), the scripts' key sets, inputs equal to the loaders' golden.
A frame with THREE or more sources is not among the cases: every aug_mods entry of the reference names at most two sets
(datasets_kdh3d_rtpose_mpaug.py:51), so generate_test_batch never composes more than two.  A Yolo-Pose+ frame WITHOUT a detection is not
either: both reference scripts raise on it (make_golden_evalsets.golden_yolo_scripts); the placeholder rows are pinned to the restated
lines in tests/test_evalsets_reference.py."""
import json
import os

import numpy as np
import pytest
import torch

import ablation_reference as AR
import evalsets_cases as EC
import evalsets_reference as ER
from helpers import state_dict_from_keys
from oracle import nets, parse_paf, parse_yolo
from popnet_amd import metrics as M
from popnet_amd import targets
from popnet_amd.config import YOLO_ANCHORS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARMS = ("human_pred_set_3d_read_raw_depth", "human_pred_set_3d_perfect_2d", "human_pred_set_3d_perfect_2d_read_raw_depth")
POSE_KEYS = {"human_pred_set_2d", "human_pred_set_3d", "visibility_pred_set", "human_gt_set_2d", "human_gt_set_3d", "human_gt_set_2d_visible"} | set(ARMS)
YOLO_KEYS = {"human_pred_set_2d", "human_pred_set_3d", "human_gt_set_2d", "human_gt_set_3d"}
RECIPE = {"metrics", "weight_seed", "seed"}


def fixture(name):
    return json.load(open(os.path.join(GOLDEN, "script_eval_data_%s.json" % name))), np.load(os.path.join(GOLDEN, "script_eval_data_%s.npz" % name))


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.abs(a - b) <= tol) | (np.isnan(a) & np.isnan(b))))


def rtpose_sd(golden, fix):
    sd = state_dict_from_keys(golden.keys["rtpose_light3d"], seed=fix["weight_seed"])
    sd["model2_2.12.bias"][:15] += torch.tensor(fix["heat_bias_shift"])
    return sd


def yolo_sd(golden, fix):
    sd = state_dict_from_keys(golden.keys["yolo_posenet"], seed=fix["weight_seed"])
    sd["model2_4.0.weight"][[4, 54]] -= np.float32(fix["conf_weight_shift"])
    return sd


def expected_ground_truth(name, seed):
    """human_gt_set_{2d,3d} as the script collects them, from the restatement: the labels as stored (single-person sets) or the transformed
    labels of the restated generate_test_batch scaled back to the original frame (composed set)."""
    data = EC.build()
    if name.startswith("kdh3d"):
        return ([[p["2d_joints"] for p in data["single"][n]] for n in data["single_ids"]], [[p["3d_joints"] for p in data["single"][n]] for n in data["single_ids"]])
    sh, _ = EC.shuffled(data, seed)
    g2, g3 = [], []
    for it in ER.batch_draws(3, EC.SET_SIZES, EC.N_BG) + ER.batch_draws(3, EC.SET_SIZES, EC.N_BG):
        image, persons = EC.composed_item(sh, it)
        _, lab, _ = ER.nocrop_reference(image, persons, dict(rot=it["rot"], a=it["a"], cx=EC.CX, cy=EC.CY, input_size=EC.S))
        g2.append(ER.gt_to_original(lab, EC.W, EC.H, EC.S))
        g3.append([l["3d_joints"].tolist() for l in lab])
    return g2, g3


@pytest.mark.parametrize("name", ["mpaug", "kdh3d", "mpaug_yolo", "kdh3d_yolo"])
def test_fixture_inputs_and_ground_truth_are_the_loaders(name):
    fix, arr = fixture(name)
    G = EC.golden()
    want = {"mpaug": np.concatenate([G["mpaug_b0_images"], G["mpaug_b1_images"]])[:, None], "mpaug_yolo": np.concatenate([G["mpaug_b0_images"], G["mpaug_b1_images"]])[:, None],
            "kdh3d": G["single0_images"], "kdh3d_yolo": G["single1_images"]}[name]
    assert arr["inputs"].dtype == np.float32 and np.array_equal(arr["inputs"], want)
    assert set(fix) - RECIPE - {"heat_bias_shift", "conf_weight_shift", "conf_threshold"} == (YOLO_KEYS if name.endswith("yolo") else POSE_KEYS)
    g2, g3 = expected_ground_truth(name, fix["seed"])
    assert fix["human_gt_set_2d"] == g2 and fix["human_gt_set_3d"] == g3
    if not name.endswith("yolo"):
        assert fix["human_gt_set_2d_visible"] == g2
    j = np.array([jt for f in g2 for p in f for jt in p])
    assert (j[:, 0] < 0).any() and (j[:, 0] > EC.W).any() and (j[:, 1] > EC.H).any()      # joints off the frame on both sides
    if name.startswith("kdh3d"):
        assert (j[:, 0] == EC.W).any() and (j[:, 1] == EC.H).any()                            # ... and exactly on the far edge


@pytest.mark.parametrize("name", ["mpaug", "kdh3d"])
def test_oracle_and_restatement_reproduce_the_open_pose_scripts(golden, name):
    fix, arr = fixture(name)
    first = name == "kdh3d"
    x = arr["inputs"]
    paf, heat, z = (a.numpy() for a in nets.rtpose_light3d_forward(torch.from_numpy(x), rtpose_sd(golden, fix)))
    for got, key in ((paf, "paf"), (heat, "heat"), (z, "z")):
        assert got.shape == arr[key].shape == (6, got.shape[1], EC.S // 8, EC.S // 8) and np.allclose(got, arr[key], atol=1e-5), key
    counts = []
    for b in range(6):
        rec = parse_paf.frame_to_records(heat[b].transpose(1, 2, 0).copy(), paf[b].transpose(1, 2, 0).copy(), z[b].transpose(1, 2, 0).copy(), w_org=EC.W, h_org=EC.H,
                                         input_size=EC.S, intrinsics=EC.INTRINSICS)
        pj = np.asarray(rec["assoc"]).reshape(-1, 17)[:, :15]
        counts.append(len(pj))
        arms = ER.net_input_arms(x[b, 0], z[b], (np.asarray(rec["joint_list"]).reshape(-1, 5) if len(rec["joint_list"]) else np.zeros((0, 5)), pj),
                                 fix["human_gt_set_2d"][b], EC.W, EC.H, EC.S, intrinsics=EC.INTRINSICS)
        cut = (lambda v: v[:1]) if first else (lambda v: v)
        assert cut(rec["visibility"]) == fix["visibility_pred_set"][b]                         # same assignment, same first person
        n = len(fix["human_pred_set_2d"][b])
        assert n == len(cut(rec["humans_2d"]))
        if n:
            assert np.allclose(np.array(cut(rec["humans_2d"])), np.array(fix["human_pred_set_2d"][b]), atol=1e-9)
            assert np.allclose(np.array(cut(rec["humans_3d"])), np.array(fix["human_pred_set_3d"][b]), atol=1e-5)
        assert np.array_equal(cut(arms[ARMS[0]]), np.array(fix[ARMS[0]][b]).reshape(-1, 15, 3))
        assert np.array_equal(arms[ARMS[2]], np.array(fix[ARMS[2]][b]))
        assert np.allclose(arms[ARMS[1]], np.array(fix[ARMS[1]][b]), atol=1e-5)
        assert len(fix[ARMS[1]][b]) == len(fix["human_gt_set_2d"][b])                          # the perfect-2D arms follow the ground truth, uncut
    got_counts = [len(f) for f in fix["human_pred_set_2d"]]
    assert got_counts == ([min(c, 1) for c in counts] if first else counts)
    assert 0 in got_counts and max(got_counts) >= 1                                            # an empty frame stays an empty list
    if not first:
        assert max(got_counts) >= 2
    missing = [v for f in fix["visibility_pred_set"] for p in f for v in p]
    assert 0 in missing and 1 in missing                                                       # persons with missing joints: the -1 rows


@pytest.mark.parametrize("name", ["mpaug_yolo", "kdh3d_yolo"])
def test_oracle_and_restatement_reproduce_the_yolo_scripts(golden, name):
    fix, arr = fixture(name)
    first = name == "kdh3d_yolo"
    assert fix["conf_threshold"] == (0.1 if first else 0.5)
    out = nets.yolo_posenet_forward(torch.from_numpy(arr["inputs"]), yolo_sd(golden, fix)).numpy()
    bb, hh, _ = parse_yolo.parse_prior_pose(out, YOLO_ANCHORS, 15, EC.S, EC.S, 3, 2, fix["conf_threshold"], 0.5)
    counts = [len(h) for h in hh]
    assert min(counts) >= 1                                                                    # (the reference scripts raise on an empty frame)
    for b in range(6):
        w2, w3 = ER.yolo_lists(hh[b], EC.W, EC.H, EC.S, EC.INTRINSICS, first=first)
        g2, g3 = np.array(fix["human_pred_set_2d"][b]), np.array(fix["human_pred_set_3d"][b])
        assert g2.shape == np.array(w2).shape and g3.shape == np.array(w3).shape
        assert np.allclose(np.array(w2), g2, atol=2e-3) and np.allclose(np.array(w3), g3, atol=1e-4)
    assert [len(f) for f in fix["human_pred_set_2d"]] == ([1] * 6 if first else counts)
    if not first:
        assert max(counts) >= 2                                                                # every person of a frame is kept
    else:
        assert max(counts) >= 2                                                                # the first-person cut dropped somebody


@pytest.mark.parametrize("name", ["mpaug", "kdh3d", "mpaug_yolo", "kdh3d_yolo"])
def test_metrics_equal_the_reference(name):
    fix, _ = fixture(name)
    want = fix["metrics"]
    th = 0.02 * np.sqrt(EC.W ** 2 + EC.H ** 2)
    assert want["dist_th_2d"] == th
    with np.errstate(all="ignore"):
        d2, k2 = M.eval_human_dataset_2d(fix["human_pred_set_2d"], fix["human_gt_set_2d"], num_joints=15, dist_th=th, iou_th=0.5)
        d3, k3 = M.eval_human_dataset_3d(fix["human_pred_set_2d"], fix["human_gt_set_2d"], fix["human_pred_set_3d"], fix["human_gt_set_3d"], num_joints=15,
                                         dist_th=0.1, iou_th=0.5)
        got = {"pck2d": k2, "err2d": d2, "pck3d": k3, "err3d": d3}
        if not name.endswith("yolo"):
            got.update(M.evaluate_ablation_blocks(fix, fix["human_gt_set_2d"], fix["human_gt_set_3d"], verbose=False))
    assert set(got) == set(want) - {"dist_th_2d"}
    for k, v in got.items():
        assert close(v, want[k]), k
    # not tables of nan: the untrained Yolo-Pose+ net's persons match no ground-truth person (error columns nan, PCK 0); the Open-Pose+
    # fixtures have matched persons and finite errors
    assert np.isfinite(np.asarray(want["pck2d"], dtype=np.float64)).all()
    if not name.endswith("yolo"):
        assert np.isfinite(np.asarray(want["err2d"], dtype=np.float64)).any()


def test_composed_ground_truth_helper_equals_the_fixture():
    """targets.composed_ground_truth on the loader golden's transformed labels: the lists the composed scripts wrote."""
    fix, _ = fixture("mpaug")
    G = EC.golden()
    g2, g3 = [], []
    for k in range(2):
        n = G["mpaug_b%d_npers" % k]
        kp, k3 = G["mpaug_b%d_kp2d" % k], G["mpaug_b%d_kp3d" % k]
        row = 0
        for b in range(3):
            a2, a3 = targets.composed_ground_truth(kp[None, row:row + n[b]], k3[None, row:row + n[b]], k3[None, row:row + n[b], :, 2], [int(n[b])], EC.W, EC.H, EC.S)
            g2 += a2
            g3 += a3
            row += int(n[b])
    assert g2 == fix["human_gt_set_2d"] and g3 == fix["human_gt_set_3d"]
