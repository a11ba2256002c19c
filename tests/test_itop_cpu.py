"""The ITOP dataset profile without a GPU: the profile's tables against the lists recorded from the reference (tests/golden/itop.json), the
host half of Hflip and the random draws, the 2D metric, the two scripts' command lines, and tests/itop_reference.py (the CPU
restatements the GPU tests compare the kernels with) against what the reference's own functions returned (tests/golden/itop.npz)."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import itop_reference as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
G = np.load(os.path.join(GOLD, "itop.npz"))
T = json.load(open(os.path.join(GOLD, "itop.json")))
sys.path.insert(0, GOLD)


def _aug_inputs(fi):
    from make_golden_itop import aug_inputs
    H, W = (int(v) for v in G["aug_frames"][fi])
    return aug_inputs(H, W, 100 + fi)


def test_profile_tables_equal_the_reference_lists():
    from popnet_amd import config
    from popnet_amd.profiles import ITOP, MP3DHP, get
    assert ITOP.keypoints == T["keypoints"] and ITOP.limbs == T["limbs"] and ITOP.joint2chn == T["joint2chn"]
    assert ITOP.get_swap_part_indices() == T["swap_indices"] and ITOP.z_chn == T["joint2chn"] and ITOP.root_joint == T["root_joint"]
    assert [ITOP.h_org, ITOP.w_org] == T["frame"]
    k = ITOP.intrinsics
    assert k["fx"] == T["intrinsics"]["f"] and k["fy"] == -T["intrinsics"]["f"] and (k["cx"], k["cy"]) == (T["intrinsics"]["cx"], T["intrinsics"]["cy"])
    assert (ITOP.depth_mean, ITOP.depth_std, ITOP.depth_max) == (T["depth_mean"], T["depth_std"], T["depth_max"]) == (3, 2, 5)
    assert ITOP.single_person and ITOP.z_readout == 1
    assert ITOP.aug == dict(cx=None, cy=None, min_ratio=0.7, max_ratio=1.2, max_crop=0.1, hflip=True) and ITOP.aug_centre(240, 320) == (160.0, 120.0)
    # the restatement the GPU tests use carries the same tables
    assert ir.KEYPOINTS == T["keypoints"] and ir.kp_connections() == T["limbs"] and ir.get_joint2chn().tolist() == T["joint2chn"]
    assert ir.get_swap_part_indices() == T["swap_indices"] and ir.JOINT2BOX_MARGIN == T["joint2box_margin"]
    # MP3DHP: today's constants, bit for bit
    assert MP3DHP.intrinsics == config.INTRINSICS and (MP3DHP.depth_mean, MP3DHP.depth_std, MP3DHP.depth_max) == (config.DEPTH_MEAN, config.DEPTH_STD, config.DEPTH_MAX)
    assert MP3DHP.keypoints == config.KEYPOINTS and MP3DHP.limbs == config.LIMBS == ITOP.limbs and (MP3DHP.w_org, MP3DHP.h_org) == (480, 640)
    assert MP3DHP.z_readout == 0 and MP3DHP.z_chn == list(range(15)) and not MP3DHP.single_person and MP3DHP.aug["max_ratio"] == 1.7 and not MP3DHP.aug["hflip"]
    assert get(None) is MP3DHP and get("itop") is ITOP and get(ITOP) is ITOP


def test_parse_cfg_carries_the_profile_and_defaults_to_todays_rule():
    from popnet_amd import _lib
    from popnet_amd.profiles import ITOP
    from popnet_amd.utils.paf_to_pose import make_parse_cfg
    cfg = _lib.ParseCfg()
    _lib.lib().pn_parse_cfg_default(C.byref(cfg))
    assert cfg.z_readout == _lib.PN_Z_READOUT_HEAT_WEIGHTED == 0 and list(cfg.z_chn) == list(range(15))
    assert _lib.lib().pn_sizeof_parse_cfg() == C.sizeof(_lib.ParseCfg)
    d = make_parse_cfg()
    assert (d.w_org, d.h_org, d.fx, d.fy, d.cx, d.cy, d.depth_mean, d.depth_std, d.z_readout) == (cfg.w_org, cfg.h_org, cfg.fx, cfg.fy, cfg.cx, cfg.cy, 3.0, 2.0, 0)
    c = make_parse_cfg(profile=ITOP)
    assert (c.w_org, c.h_org, c.cx, c.cy, c.depth_mean, c.depth_std) == (320, 240, 160.0, 120.0, 3.0, 2.0)
    assert c.fx == 1 / 0.0035 and c.fy == -(1 / 0.0035) and c.z_readout == _lib.PN_Z_READOUT_CELL and list(c.z_chn) == T["joint2chn"]
    assert make_parse_cfg(profile=ITOP, w_org=64).w_org == 64
    from popnet_amd import targets
    t = targets.target_cfg(64, profile=ITOP)
    assert (t.depth_max, t.depth_mean, t.depth_std) == (5.0, 3.0, 2.0) and targets.target_cfg(64).depth_max == 6.0
    assert targets.yolo_target_cfg(64, profile=ITOP).depth_mean == 3.0


def test_draws_without_hflip_are_todays_and_the_coin_sits_between_renderdepth_and_crop():
    from popnet_amd import targets
    from popnet_amd.profiles import ITOP
    geom = dict(H=240, W=320, cx=160.0, cy=120.0, max_ratio=1.2)
    random.seed(11)
    rot, a = random.uniform(-10, 10), random.uniform(0.7, 1.2)
    crops = tuple(random.uniform(0, 0.1) for _ in range(4))
    today = random.getstate()
    random.seed(11)
    it = targets.draw_augmentation(**geom)
    assert random.getstate() == today and (it["rot"], it["a"], it["crops"]) == (rot, a, crops) and it["hflip"] is False
    random.seed(11)
    it = targets.draw_augmentation(hflip=False, swap_indices=ITOP.swap_indices, **geom)
    assert random.getstate() == today and it["hflip"] is False
    # with hflip: rot, a, the coin, then the four crops
    flips = set()
    for seed in range(8):
        random.seed(seed)
        rot, a, coin = random.uniform(-10, 10), random.uniform(0.7, 1.2), random.uniform(0, 1)
        crops = tuple(random.uniform(0, 0.1) for _ in range(4))
        after = random.getstate()
        random.seed(seed)
        it = targets.draw_augmentation(hflip=True, swap_indices=ITOP.swap_indices, **geom)
        assert random.getstate() == after and (it["rot"], it["a"], it["crops"]) == (rot, a, crops) and it["hflip"] == (coin >= 0.5)
        flips.add(it["hflip"])
    assert flips == {True, False}
    assert np.array_equal(G["aug_draw_ranges"], [(-10, 10), (0.7, 1.2), (0, 1), (0, 0.1), (0, 0.1), (0, 0.1), (0, 0.1)])      # the reference's own order
    with pytest.raises(Exception, match="swap_indices"):
        targets.augmentation(0.0, 1.0, (0, 0, 0, 0), 12, 15, 7.5, 6.0, 10, hflip=True)


@pytest.mark.parametrize("fi", [0, 1])
def test_restated_chain_and_host_labels_equal_the_reference_chain(fi):
    """tests/itop_reference.augment_chain (image and labels) and AugmentationBatch.transform_labels (labels) against the reference's own
    Compose([Cvt2ndarray, Rotate(), RenderDepth(), Hflip, Crop(), Resize]) output, flag set and clear."""
    from popnet_amd import targets
    H, W = (int(v) for v in G["aug_frames"][fi])
    S = int(G["aug_S"])
    frame, person = _aug_inputs(fi)
    swap = T["swap_indices"]
    items = []
    for ci, (rot, a, coin, *crops) in enumerate(G["aug_cases"]):
        k = "aug%d_%d_" % (fi, ci)
        img, lab, rw = ir.augment_chain(frame, [person], rot, a, coin >= 0.5, crops, S, swap)
        assert np.array_equal(img, G[k + "image"]), (fi, ci)
        assert np.array_equal(lab[0]["2d_joints"], G[k + "kp2d"]) and np.array_equal(lab[0]["3d_joints"], G[k + "kp3d"])
        assert np.array_equal(lab[0]["visible_joints"], G[k + "visible"]) and np.array_equal(lab[0]["bbox"], G[k + "bbox"])
        items.append(targets.augmentation(rot, a, crops, H, W, W / 2, H / 2, S, hflip=coin >= 0.5, swap_indices=swap))
        assert items[-1]["render_w"] == rw
    n = len(items)
    k2 = np.broadcast_to(np.asarray(person["2d_joints"], dtype=np.float32), (n, 1, 15, 2))
    k3 = np.broadcast_to(np.asarray(person["3d_joints"], dtype=np.float64), (n, 1, 15, 3))
    bb = np.broadcast_to(np.asarray(person["bbox"], dtype=np.float64), (n, 1, 4))
    vs = np.broadcast_to(np.asarray(person["visible_joints"]), (n, 1, 15))
    aug = targets.AugmentationBatch(items)
    kp, kz, bx, vis = aug.transform_labels(k2, k3, bb, vs)
    for ci in range(n):
        k = "aug%d_%d_" % (fi, ci)
        assert np.array_equal(kp[ci, 0], G[k + "kp2d"]) and kp.dtype == np.float32, ci
        assert np.array_equal(kz[ci, 0], G[k + "kp3d"][:, 2]) and np.array_equal(bx[ci, 0], G[k + "bbox"]) and np.array_equal(vis[ci, 0], G[k + "visible"]), ci
        assert aug.records[ci].hflip == int(G["aug_cases"][ci][2] >= 0.5)
    # a flipped item differs from its unflipped twin, and the three-result form is unchanged
    assert not np.array_equal(kp[0], kp[1]) and len(aug.transform_labels(k2, k3, bb)) == 3


def test_restated_targets_equal_the_reference_loader():
    heat, paf, z, fg = ir.ground_truth(G["gt_kp2d"][None], G["gt_kp3d"][None], G["gt_depth"], 64, 64, 8, 2)
    assert np.array_equal(heat, G["gt_heat"]) and np.array_equal(paf, G["gt_paf"]) and np.array_equal(fg, G["gt_fg"])
    assert np.array_equal(z, G["gt_z"]) and z.dtype == G["gt_z"].dtype and z.max() <= (5 - 3) / 2
    assert 0 < fg.sum() < fg.size and (G["gt_kp3d"][:, 2] > 5).any()
    prior, conf, coord, weight = ir.prior_targets(G["gt_kp2d"][None], G["gt_kp3d"][None], None, 64, 64)
    for a, b in ((prior, "gt_prior"), (conf, "gt_conf"), (coord, "gt_coord"), (weight, "gt_weight")):
        assert np.array_equal(a, G[b]), b
    assert "joint_names" in str(G["rtpose_gt_error"])


def test_eval_human_dataset_2d_equals_the_reference_function():
    from make_golden_itop import eval2d_cases
    from popnet_amd import metrics
    from popnet_amd.profiles import ITOP
    pred, gt, vis = eval2d_cases(int(G["eval2d_seed"]), int(G["eval2d_frames"]))
    th = ITOP.dist_th_2d()
    assert th == float(G["eval2d_th"])
    d, k = metrics.eval_human_dataset_2d(pred, gt, num_joints=15, dist_th=th, iou_th=0.5)
    assert np.array_equal(np.array(d), G["eval2d_dist"]) and np.array_equal(np.array(k), G["eval2d_kcp"])
    d, k = metrics.eval_human_dataset_2d(pred, gt, num_joints=15, dist_th=th, iou_th=0.5, human_gt_set_visibility=vis)
    assert np.array_equal(np.array(d), G["eval2d_dist_vis"]) and np.array_equal(np.array(k), G["eval2d_kcp_vis"])
    assert 0 < np.mean(G["eval2d_kcp"]) < 1


def test_yolo_placeholder_and_list_keys():
    from popnet_amd import _lib, dataset
    from popnet_amd.profiles import ITOP
    j2, j3 = dataset.yolo_placeholder_person(ITOP)
    w2, w3 = ir.yolo_glue([])
    assert np.array_equal(j2, np.array(w2[0])) and np.array_equal(j3, np.array(w3[0]))
    recs = np.zeros(2, dtype=_lib.YOLO_FRAME_DTYPE)
    recs[1]["n_det"] = 2
    recs[1]["joints_2d"][0], recs[1]["joints_3d"][0] = 7.0, 9.0
    out = dataset.yolo_records_to_lists(recs, profile=ITOP)
    assert sorted(out) == ["human_pred_set_2d", "human_pred_set_3d"] and out["human_pred_set_2d"][0] == w2 and out["human_pred_set_3d"][0] == w3
    assert len(out["human_pred_set_2d"][1]) == 1 and np.array(out["human_pred_set_3d"][1]).shape == (1, 15, 3) and out["human_pred_set_3d"][1][0][0] == [9.0] * 3
    recs[1]["status"] = 1                  # more than 64 survivors: truncated first-come, the first person stands; the MP-3DHP lists refuse it
    assert dataset.yolo_records_to_lists(recs, profile=ITOP) == out
    with pytest.raises(_lib.PopnetError, match="overflow"):
        dataset.yolo_records_to_lists(recs)
    recs[1]["status"] = 2
    with pytest.raises(_lib.PopnetError, match="overflow"):
        dataset.yolo_records_to_lists(recs, profile=ITOP)
    recs[1]["status"] = 0
    assert sorted(dataset.yolo_records_to_lists(recs)) == ["human_pred_set_2d", "human_pred_set_3d", "human_pred_set_part_conf"]
    precs = np.zeros(1, dtype=_lib.POSE_FRAME_DTYPE)
    assert sorted(dataset.pose_records_to_lists(precs, profile=ITOP)) == ["human_pred_set_2d", "human_pred_set_3d", "visibility_pred_set"]
    assert "human_pred_set_part_conf" in dataset.pose_records_to_lists(precs)


def test_committed_itop_frame():
    f = np.load(os.path.join(GOLD, "itop_frame_00_02254.npy"))
    assert f.shape == (240, 320) and f.dtype == np.float16 and 0 < float(f.max()) < 10


@pytest.mark.parametrize("script", ["evaluate_itop.py", "train_itop.py"])
def test_scripts_parse_their_arguments_and_fail_cleanly_without_a_gpu(script, tmp_path):
    path = os.path.join(ROOT, "scripts", script)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")      # the GPU box too: no device for the child
    r = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "--net" in r.stdout
    r = subprocess.run([sys.executable, path, "--net", "a2j"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 2 and "invalid choice" in r.stderr
    if script == "evaluate_itop.py":
        argv = ["--net", "rtpose", "--annotations", "a.json", "--image-dir", "d", "--weight", "w.pth", "--output-dir", str(tmp_path)]
    else:
        argv = ["--net", "yolo", "--train-annotations", "a.json", "--train-image-dir", "d", "--output-dir", str(tmp_path)]
    r = subprocess.run([sys.executable, path] + argv, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 1 and "needs a GPU" in r.stderr and "Traceback" not in r.stderr
