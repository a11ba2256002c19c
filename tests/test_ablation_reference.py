"""CPU: tests/ablation_reference.py (the numpy restatement the HIP ablation entries are checked against) must reproduce
tests/golden/script_eval_data_ablation.json, which tests/golden/make_golden_ablation.py produced by running the REFERENCE's
evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py on labels with edge-case joints; popnet_amd.metrics' five ablation blocks
must equal what the reference's own eval_human_dataset_3d returned for them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ablation_reference as AR
from helpers import state_dict_from_keys
from oracle import nets, parse_paf, preproc
from popnet_amd import metrics as M
from popnet_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "script_eval_data_ablation.json")))
ARMS = ("human_pred_set_3d_read_raw_depth", "human_pred_set_3d_perfect_2d", "human_pred_set_3d_perfect_2d_read_raw_depth")


def fixture_gt_2d():
    lab = FIX["labels"]
    return [[p["2d_joints"] for p in lab[k]] for k in lab if k != "intrinsics"]


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.abs(a - b) <= tol) | (np.isnan(a) & np.isnan(b))))


@pytest.fixture(scope="module")
def oracle_run(golden):
    """The oracle's pre-process, forward and parse of the fixture's two frames, and the restatement's arms on them."""
    sd = state_dict_from_keys(golden.keys["rtpose_light3d"], seed=FIX["weight_seed"])
    sd["model2_2.12.bias"][:15] += torch.tensor(FIX["heat_bias_shift"])
    frames = synth.synth_depth(2, 640, 480, seed=FIX["depth_seed"])
    x = preproc.preprocess_batch(frames)
    paf, heat, z = (a.numpy() for a in nets.rtpose_light3d_forward(torch.from_numpy(x), sd))
    gt = fixture_gt_2d()
    out = []
    for b in range(2):
        rec = parse_paf.frame_to_records(heat[b].transpose(1, 2, 0).copy(), paf[b].transpose(1, 2, 0).copy(), z[b].transpose(1, 2, 0).copy())
        pj = np.asarray(rec["assoc"]).reshape(-1, 17)[:, :15]
        arms = AR.ablation_reference(x[b].reshape(224, 224), (paf[b], heat[b], z[b]), (np.asarray(rec["joint_list"]), pj), gt[b])
        out.append((rec, arms))
    return out


def test_fixture_covers_the_edge_cases():
    gt = fixture_gt_2d()
    assert [len(g) for g in gt] == [2, 3] and gt == FIX["human_gt_set_2d_visible"]
    assert [len(f) for f in FIX["human_pred_set_2d"]] == [2, 5]
    vis = [np.sum(v) for f in FIX["human_pred_set_visibility"] for v in f]
    assert min(vis) >= 3 and max(vis) <= 6                       # every person has missing joints: the -1 rows
    a = np.array([j for f in gt for p in f for j in p])
    assert (a[:, 0] < 0).any() and (a[:, 0] == 480.0).any() and (a[:, 0] > 480).any() and (a[:, 1] >= 640).any()
    assert set(FIX) >= set(ARMS) | {"human_gt_set_2d_visible", "human_pred_set_2d", "human_pred_set_3d", "human_pred_set_visibility",
                                    "human_pred_set_part_conf", "labels", "metrics", "depth_seed", "weight_seed"}
    for f in range(2):
        for key in ARMS[1:]:
            assert np.array(FIX[key][f]).shape == (len(gt[f]), 15, 3)      # the perfect_* arms follow the GT persons
        assert np.array(FIX[ARMS[0]][f]).shape == (len(FIX["human_pred_set_2d"][f]), 15, 3)


def test_restatement_reproduces_the_reference_script(oracle_run):
    for b, (rec, arms) in enumerate(oracle_run):
        assert rec["visibility"] == FIX["human_pred_set_visibility"][b]                       # same assignment
        assert np.allclose(np.array(rec["humans_2d"]).reshape(-1, 15, 2), np.array(FIX["human_pred_set_2d"][b]).reshape(-1, 15, 2), atol=1e-9)
        # raw depth at the ground-truth pixel: nothing of the network in it, bit-equal
        assert np.array_equal(arms[ARMS[2]], np.array(FIX[ARMS[2]][b]))
        # raw depth at the predicted joints: integer pixels, bit-equal given the same assignment
        assert np.array_equal(arms[ARMS[0]], np.array(FIX[ARMS[0]][b]).reshape(-1, 15, 3))
        missing = np.array(FIX["human_pred_set_visibility"][b]) == 0
        assert missing.any() and np.all(arms[ARMS[0]][missing][:, 2] == -1.0)
        # the pose-depth map at the ground-truth cell: the oracle's forward against the reference module's, the tolerance
        # tests/test_oracle_golden.py applies to human_pred_set_3d of the script fixture
        assert np.allclose(arms[ARMS[1]], np.array(FIX[ARMS[1]][b]), atol=1e-5)


def test_metric_blocks_equal_the_reference(tmp_path):
    lab = FIX["labels"]
    g2 = fixture_gt_2d()
    g3 = [[p["3d_joints"] for p in lab[k]] for k in lab if k != "intrinsics"]
    res = {k: FIX[k] for k in ARMS + ("human_gt_set_2d_visible", "human_pred_set_2d", "human_pred_set_3d", "human_pred_set_part_conf")}
    out = M.evaluate_ablation_blocks(res, g2, g3, verbose=False)
    assert len(out) == 10 and set(out) == set(FIX["metrics"])
    for k, want in FIX["metrics"].items():
        assert close(out[k], want), k
    # through the file interface; without the argument nothing is added
    gt_file, res_file = str(tmp_path / "labels.json"), str(tmp_path / "eval_data.json")
    json.dump(lab, open(gt_file, "w"))
    json.dump(res, open(res_file, "w"))
    plain = M.evaluate_mp_human_3d(gt_file, res_file, verbose=False)
    full = M.evaluate_mp_human_3d(gt_file, res_file, verbose=False, ablation=True)
    assert set(full) - set(plain) == set(FIX["metrics"]) and not any(k.endswith(("perfect_2d", "raw", "visible")) for k in plain)
    for k, want in FIX["metrics"].items():
        assert close(full[k], want), k
    for k in plain:
        assert close(plain[k], full[k]), k


def test_ablation_needs_its_keys(tmp_path):
    with pytest.raises(KeyError, match="--ablation"):
        M.evaluate_ablation_blocks({"human_pred_set_2d": [], "human_pred_set_3d": []}, [], [], verbose=False)


@pytest.mark.skipif(not os.path.isdir("/root/reference/third_party_methods"), reason="needs the reference tree")
def test_recipe_regenerates_the_fixture_identically():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_ablation.py"), "--check"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "golden check ok: 1 files regenerate identically" in r.stdout
