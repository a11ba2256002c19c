"""GPU: the ITOP dataset profile -- Hflip inside the one-launch augmentation (T1), the one-cell depth read-out of the pose-parse kernels
(T2), the single-person target batches (T3) and both engines end to end on the ITOP frame the reference ships (T4) -- against
tests/itop_reference.py, which tests/test_itop_cpu.py pins to the reference's own outputs.

Bars.  T1: bit for bit (the kernel rounds where OpenCV 4.2's scalar float32 paths round).  T2: bit for bit, the contract of
parse_device.h.  T3: the bars of tests/test_gpu_targets.py -- z, fg, paf, image and prior maps exact, Gaussian heat maps within one
float32 ulp at 1.0 (HEAT_TOL, the device's double exp).  T4: the comparison of tests/test_gpu_parity.py's
test_end_to_end_vs_reference_eval_script / test_yolo_end_to_end_vs_reference_eval_script, taken from there: persons and visibility
exact, 2D within 1e-9 (Open-Pose+) / 5e-2 px (Yolo-Pose+), 3D within 1e-3 m.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import cv2_warp_reference as cw
import itop_reference as ir
import parse_cases as PC
import parse_options_reference as POR
from helpers import YOLO_ANCHORS, state_dict_from_keys
from oracle import parse_paf as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
G = np.load(os.path.join(GOLD, "itop.npz"))
T = json.load(open(os.path.join(GOLD, "itop.json")))
sys.path.insert(0, GOLD)
HEAT_TOL = 1.2e-7            # tests/test_gpu_targets.py


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


# ---- T1: Hflip in the augmentation launch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fi", [0, 1], ids=["12x15", "12x16"])
def test_hflip_launch_equals_the_cpu_chain(gpu, fi):
    """One batch per frame width (odd, even): a < 1 (slice), a > 1 (paste into the zero image) and a rotated item with crops on all four
    sides, each with the flag set and clear.  Image == warpAffine restatement -> np.flip(axis=1) of the render image -> crop -> resize,
    bit for bit; flag-clear items == the call through today's path (no hflip argument); labels == the restated Hflip."""
    from make_golden_itop import aug_inputs
    from popnet_amd import targets
    H, W = (int(v) for v in G["aug_frames"][fi])
    S = int(G["aug_S"])
    frame, person = aug_inputs(H, W, 100 + fi)
    swap = T["swap_indices"]
    cases = [(float(c[0]), float(c[1]), bool(c[2] >= 0.5), tuple(float(v) for v in c[3:])) for c in G["aug_cases"]]
    assert [c[2] for c in cases] == [False, True] * 3 and cases[0][1] < 1 < cases[2][1] and cases[4][0] != 0 and min(cases[4][3]) > 0
    items = [targets.augmentation(rot, a, crops, H, W, W / 2, H / 2, S, hflip=flip, swap_indices=swap) for rot, a, flip, crops in cases]
    assert all((it["src_w"], it["src_h"]) != (2 * S, 2 * S) for it in items)
    n = len(items)
    frames = _dev(np.repeat(frame.astype(np.float32)[None], n, axis=0), gpu)
    aug = targets.AugmentationBatch(items)
    out = targets.augment_resize(frames, aug, S, 5.0, 3.0, 2.0).cpu().numpy()
    raw = targets.augment_resize(frames, aug, S, profile="ITOP").cpu().numpy()
    worst = 0.0
    for ci, (rot, a, flip, crops) in enumerate(cases):
        img, lab, _ = ir.augment_chain(frame, [person], rot, a, flip, crops, S, swap)
        assert np.array_equal(img, G["aug%d_%d_image" % (fi, ci)])
        want = cw.network_input(img, 5.0, 3.0, 2.0)
        worst = max(worst, float(np.abs(out[ci, 0] - want).max()))
        assert np.array_equal(out[ci, 0], want), (fi, ci, np.abs(out[ci, 0] - want).max())
        assert np.array_equal(raw[ci, 0], cw.network_input(img, 5.0, 0.0, 1.0)), (fi, ci)
    print("T1 %dx%d: %d items, max |kernel - cpu chain| = %g" % (H, W, n, worst))
    # the flipped twin differs (the frames are not symmetric), so the flag reaches the kernel
    assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[4], out[5])
    # flag clear == today's path, bit for bit: the same items built without the new arguments, in a batch of their own
    plain = [targets.augmentation(rot, a, crops, H, W, W / 2, H / 2, S) for rot, a, flip, crops in cases if not flip]
    old = targets.augment_resize(frames[:len(plain)], targets.AugmentationBatch(plain), S, 5.0, 3.0, 2.0).cpu().numpy()
    assert np.array_equal(old, out[0::2])
    # labels, visible_joints and boxes == the restated Hflip inside the chain
    k2 = np.broadcast_to(np.asarray(person["2d_joints"], dtype=np.float32), (n, 1, 15, 2))
    k3 = np.broadcast_to(np.asarray(person["3d_joints"], dtype=np.float64), (n, 1, 15, 3))
    bb = np.broadcast_to(np.asarray(person["bbox"], dtype=np.float64), (n, 1, 4))
    vs = np.broadcast_to(np.asarray(person["visible_joints"]), (n, 1, 15))
    kp, kz, bx, vis = aug.transform_labels(k2, k3, bb, vs)
    for ci, (rot, a, flip, crops) in enumerate(cases):
        _, lab, _ = ir.augment_chain(frame, [person], rot, a, flip, crops, S, swap)
        assert np.array_equal(kp[ci, 0], lab[0]["2d_joints"]) and np.array_equal(kz[ci, 0], lab[0]["3d_joints"][:, 2])
        assert np.array_equal(bx[ci, 0], lab[0]["bbox"]) and np.array_equal(vis[ci, 0], lab[0]["visible_joints"])


def test_hflip_flag_outside_0_1_is_refused(gpu):
    from popnet_amd import _lib, targets
    it = targets.augmentation(0.0, 0.8, (0, 0, 0, 0), 12, 15, 7.5, 6.0, 10)
    aug = targets.AugmentationBatch([it])
    aug.records[0].hflip = 2
    with pytest.raises(_lib.PopnetError, match="inconsistent geometry"):
        targets.augment_resize(torch.ones((1, 12, 15), device=gpu), aug, 10)


# ---- T2: the cell read-out ---------------------------------------------------------------------------------------------------------
H_MAP, W_MAP = 6, 9
# peaks in row 0 (joint 8), in the last column (9, 11), in column 0 (10, 12) and in the last row (person B)
PERSON_A = {8: (4, 0), 9: (8, 1), 11: (8, 4), 10: (0, 1), 12: (0, 4)}
PERSON_B = {1: (4, 5), 2: (1, 5), 0: (7, 5)}


def _readout_maps():
    heat, paf, _ = PC.build_maps(H_MAP, W_MAP, persons=[PERSON_A, PERSON_B], seed=3, noise=0.5)
    c, y, x = np.meshgrid(np.arange(15), np.arange(H_MAP), np.arange(W_MAP), indexing="ij")
    z = (100 * c + 10 * y + x).astype(np.float32)            # z[c, y, x]: a wrong channel or cell shows in the value
    return heat, paf, z


def _readout_reference(heat, paf, z, f):
    joint_list, assoc, _ = POR.paf_to_pose(heat.copy(), paf.copy(), f, 10)
    humans, vis, _ = O.paf_to_human_list(joint_list, assoc)
    h2, h3 = ir.readout(humans, vis, z, downsample=f, input_size=224, w_org=320, h_org=240, clamp=True)
    return joint_list, assoc, np.array(vis), np.array(h2, dtype=np.float64).reshape(-1, 15, 2), np.array(h3, dtype=np.float64).reshape(-1, 15, 3)


@pytest.mark.parametrize("family", ["default", "downsample4", "unbounded"])
def test_cell_readout_equals_the_restated_itop_glue(gpu, family):
    """6 x 9 maps (h != w), two persons with peaks on all four borders; per kernel family -- the kernels built for (x8, ten points), the
    generic ones (downsample 4) and the unbounded second pass, which the existing tests call directly on maps as small as 3 x 3 -- depths,
    2D and 3D joints == evaluation_rtpose_light3d_itop.py:176-209 restated, bit for bit, fy = -f included.  The z map sits in the middle of
    a NaN-filled buffer: a read outside it would show."""
    from popnet_amd import _lib
    from popnet_amd.profiles import ITOP
    from popnet_amd.utils import paf_to_pose as P2P
    f = 4 if family == "downsample4" else 8
    heat, paf, z = _readout_maps()
    joint_list, assoc, vis, want2, want3 = _readout_reference(heat, paf, z, f)
    assert len(assoc) == 2 and sorted(vis.sum(axis=1).tolist()) == [3, 5]
    cfg = P2P.make_parse_cfg(profile=ITOP)
    cfg.downsample = f
    assert cfg.z_readout == _lib.PN_Z_READOUT_CELL and cfg.fy == -cfg.fx
    th, tp = (_dev(a.transpose(2, 0, 1)[None], gpu) for a in (heat, paf))
    guard = torch.full((3, 15, H_MAP, W_MAP), float("nan"), device=gpu)
    guard[1] = _dev(z, gpu)
    tz = guard[1:2]
    if family == "unbounded":
        r = P2P.parse_paf_unbounded(th[0], tp[0], tz[0], cfg)
        jl, pj, j2, j3 = r["joint_list"], r["person_joint"], r["joints_2d"], r["joints_3d"]
    else:
        fr = P2P.parse_paf_batch(th, tp, tz, cfg)[0]
        assert int(fr["status"]) == 0
        n = int(fr["n_persons"])
        jl, pj, j2, j3 = P2P.frame_joint_list(fr), fr["person_joint"][:n], fr["joints_2d"][:n], fr["joints_3d"][:n]
    assert np.array_equal(jl, joint_list) and np.array_equal(pj, assoc[:, :15].astype(np.int32))
    assert np.array_equal(j2, want2) and np.array_equal(j3, want3), (np.abs(j2 - want2).max(), np.abs(j3 - want3).max())
    print("T2 %s: 2 persons, %d visible joints, max |2D| diff %g, max |3D| diff %g" % (family, int(vis.sum()), np.abs(j2 - want2).max(), np.abs(j3 - want3).max()))
    # what was compared: the expected depth of every visible joint is the one cell of channel joint2chn[j] (2 z + 3 of 100 c + 10 y + x),
    # cells of all four borders among them; invisible joints stay at -1; Y carries the flipped sign
    chn = ir.get_joint2chn()
    cells = set()
    for p in range(2):
        for j in range(15):
            if not vis[p, j]:
                assert j3[p, j, 2] == -1.0 and tuple(j2[p, j]) == (-1.0, -1.0)
                continue
            x, y = joint_list[int(assoc[p, j]), :2]
            cx, cy = min(int(x / f), W_MAP - 1), min(int(y / f), H_MAP - 1)
            assert j3[p, j, 2] == float(np.float32(np.float32(100 * chn[j] + 10 * cy + cx) * np.float32(2) + np.float32(3))), (p, j)
            assert j3[p, j, 1] == -(j2[p, j, 1] - 120) * j3[p, j, 2] / (1 / 0.0035)
            cells.add((cx, cy))
    assert {0, W_MAP - 1} <= {c[0] for c in cells} and {0, H_MAP - 1} <= {c[1] for c in cells}
    # the heat-weighted default on the same maps reads channel j and another value: the rule is what changed the result
    d = P2P.make_parse_cfg(w_org=320, h_org=240)
    d.downsample = f
    fr0 = P2P.parse_paf_batch(th, tp, tz, d)[0]
    assert int(fr0["n_persons"]) == 2 and not np.array_equal(fr0["joints_3d"][:2, :, 2], j3[:, :, 2])


def test_cell_readout_rejects_a_channel_outside_the_map(gpu):
    from popnet_amd import _lib
    from popnet_amd.utils import paf_to_pose as P2P
    heat, paf, z = _readout_maps()
    cfg = P2P.make_parse_cfg(profile="ITOP")
    cfg.z_chn[3] = 15
    args = tuple(_dev(a.transpose(2, 0, 1)[None], gpu) for a in (heat, paf)) + (_dev(z[None], gpu),)
    with pytest.raises(_lib.PopnetError, match="z_chn"):
        P2P.parse_paf_batch(*args, cfg)
    cfg = P2P.make_parse_cfg(profile="ITOP")
    cfg.z_readout = 7
    with pytest.raises(_lib.PopnetError, match="z_readout"):
        P2P.parse_paf_unbounded(args[0][0], args[1][0], args[2][0], cfg)


# ---- T3: targets -------------------------------------------------------------------------------------------------------------------
def test_itop_targets_equal_the_restated_loader(gpu):
    """One person partly outside a 64 x 64 input (8 x 8 maps), depth_max = 5, visible_joints ignored: rasterize_targets and prior_targets
    with the ITOP profile against the restated datasets_itop get_ground_truth (pinned to the reference's own maps on the CPU)."""
    from popnet_amd import targets
    from popnet_amd.profiles import ITOP
    k2, k3, depth = G["gt_kp2d"], G["gt_kp3d"], G["gt_depth"]
    one = torch.ones((1,), dtype=torch.int32, device=gpu)
    out = targets.rasterize_targets(_dev(k2[None, None], gpu), _dev(k3[None, None, :, 2], gpu), one, _dev(depth[None], gpu), input_size=64, profile=ITOP)
    heat, paf, z, fg = (o[0].permute(1, 2, 0).cpu().numpy() for o in out)
    oh, op, oz, of = ir.ground_truth(k2[None], k3[None], depth, 64, 64, 8, 2)
    assert np.array_equal(fg, of.astype(np.float32)) and 0 < fg.sum() < fg.size
    assert np.array_equal(z, oz.astype(np.float32)) and oz.dtype == np.float32 and z.max() == 1.0      # (5 - 3) / 2: the 5 m clamp, not 6 m
    assert np.array_equal(paf, op.astype(np.float32))
    print("T3: max |heat - restated| = %g" % np.abs(heat - oh.astype(np.float32)).max())
    assert np.abs(heat - oh.astype(np.float32)).max() <= HEAT_TOL
    # the default profile clamps at 6 m: another z map for the joints deeper than 5 m
    z6 = targets.rasterize_targets(_dev(k2[None, None], gpu), _dev(k3[None, None, :, 2], gpu), one, _dev(depth[None], gpu), input_size=64)[2]
    assert float(z6.max()) > 1.0
    # prior targets, 'pose_weight' absent (1.0), the box from the joints
    box = targets.joints_box(k2[None, None])
    prior = targets.prior_targets(_dev(box, gpu), _dev(k2[None, None], gpu), _dev(k3[None, None, :, 2], gpu), torch.ones((1, 1), dtype=torch.float64, device=gpu),
                                  one, input_size=64, profile=ITOP)
    want = ir.prior_targets(k2[None], k3[None], None, 64, 64)
    for got, ref, name in zip(prior, want, ("prior", "conf", "coord", "weight")):
        assert np.array_equal(got[0].permute(1, 2, 0).cpu().numpy(), ref.astype(np.float32)), name
    assert want[2].sum() == 1


def test_itop_batch_runs_the_frame_through_both_transforms(gpu):
    """itop_batch / itop_batch_yolo on the committed ITOP frame: the evaluation transform == oracle pre-processing + restated targets; the
    random transform with Hflip == the CPU chain + restated targets (same bars)."""
    from oracle import cv2_resize, preproc as opre
    from popnet_amd import targets
    frame = np.load(os.path.join(GOLD, "itop_frame_00_02254.npy"))
    rng = np.random.default_rng(12)
    k2 = np.stack([rng.uniform(20, 300, 15), rng.uniform(10, 230, 15)], axis=1).astype(np.float32)
    k3 = np.concatenate([k2.astype(np.float64), rng.uniform(1.5, 3.5, (15, 1))], axis=1)
    fr = _dev(frame[None], gpu)
    x, heat, paf, z, fg = targets.itop_batch(fr, k2[None], k3[None])
    want_x = opre.preprocess_batch(frame[None], depth_max=5)
    assert np.array_equal(x.cpu().numpy(), want_x)
    # (the targets see the clamped, un-normalised image: rebuilt here as the loader does, from the resized frame)
    img = cw.network_input(cv2_resize.resize(frame.astype(np.float32), (224, 224), interpolation=cv2_resize.INTER_LINEAR), 5.0, 0.0, 1.0)
    kp = k2.copy()
    kp[:, 0] *= 224.0 / 320
    kp[:, 1] *= 224.0 / 240
    oh, op, oz, of = ir.ground_truth(kp[None], k3[None], cv2_resize.resize(img, (28, 28), interpolation=cv2_resize.INTER_LINEAR))
    t = lambda a: a[0].permute(1, 2, 0).cpu().numpy()      # noqa: E731
    assert np.array_equal(t(fg), of.astype(np.float32)) and np.array_equal(t(z), oz.astype(np.float32)) and np.array_equal(t(paf), op.astype(np.float32))
    assert np.abs(t(heat) - oh.astype(np.float32)).max() <= HEAT_TOL
    # the random transform, coin up
    swap = T["swap_indices"]
    it = targets.augmentation(-6.0, 0.9, (0.02, 0.05, 0.03, 0.08), 240, 320, 160.0, 120.0, 224, hflip=True, swap_indices=swap)
    aug = targets.AugmentationBatch([it])
    xa, ha, pa, za, fa = targets.itop_batch(fr, k2[None], k3[None], aug=aug)
    cimg, lab, _ = ir.augment_chain(frame, [{"2d_joints": k2, "3d_joints": k3}], -6.0, 0.9, True, (0.02, 0.05, 0.03, 0.08), 224, swap)
    assert np.array_equal(xa[0, 0].cpu().numpy(), cw.network_input(cimg, 5.0, 3.0, 2.0))
    cl = cw.network_input(cimg, 5.0, 0.0, 1.0)
    oh, op, oz, of = ir.ground_truth(lab[0]["2d_joints"][None], lab[0]["3d_joints"][None], cv2_resize.resize(cl, (28, 28), interpolation=cv2_resize.INTER_LINEAR))
    assert np.array_equal(t(fa), of.astype(np.float32)) and np.array_equal(t(za), oz.astype(np.float32)) and np.array_equal(t(pa), op.astype(np.float32))
    assert np.abs(t(ha) - oh.astype(np.float32)).max() <= HEAT_TOL
    xy, prior, conf, coord, weight = targets.itop_batch_yolo(fr, k2[None], k3[None], aug=aug)
    assert torch.equal(xy, xa)
    want = ir.prior_targets(lab[0]["2d_joints"][None], lab[0]["3d_joints"][None], None)
    for got, ref, name in zip((prior, conf, coord, weight), want, ("prior", "conf", "coord", "weight")):
        assert np.array_equal(t(got), ref.astype(np.float32)), name


# ---- T4: end to end on the ITOP frame ----------------------------------------------------------------------------------------------
RTPOSE_SEED, YOLO_SEED = 0, 1            # chosen on the CPU: with these the oracle alone finds persons on the ITOP frame (asserted below)


@pytest.fixture(scope="module")
def itop_frame():
    return np.load(os.path.join(GOLD, "itop_frame_00_02254.npy"))


def test_pose_engine_itop_end_to_end_vs_oracle(gpu, golden, itop_frame):
    from oracle import nets, preproc as opre
    from popnet_amd.pipeline import PoseEngine
    from popnet_amd.profiles import ITOP
    sd = state_dict_from_keys(golden.keys["rtpose_light3d"], seed=RTPOSE_SEED)
    sd["model2_2.12.bias"][:15] += torch.tensor(golden.script["heat_bias_shift"])
    # the CPU oracle forward and parse, then the restated ITOP glue
    x = opre.preprocess_batch(itop_frame[None], depth_max=5)
    paf, heat, z = nets.rtpose_light3d_forward(torch.from_numpy(x), sd)
    hh, hp, hz = (a[0].numpy().transpose(1, 2, 0) for a in (heat, paf, z))
    joint_list, assoc = O.paf_to_pose(hh.copy(), hp.copy())
    humans, vis, _ = O.paf_to_human_list(joint_list, assoc)
    assert len(humans) >= 1 and int(np.array(vis).sum()) >= 1, "the oracle must find a person with a visible joint for this seed"
    want2, want3 = ir.readout(humans, vis, hz.transpose(2, 0, 1))
    eng = PoseEngine(precision="fp32", state_dict=sd, device=gpu, max_batch=2, profile=ITOP)
    assert (eng.cfg.w_org, eng.cfg.h_org, eng.cfg.z_readout) == (320, 240, 1)
    dev_frame = torch.from_numpy(itop_frame[None]).to(gpu)
    fr = eng.predict_host(dev_frame)[0]
    assert np.array_equal(eng.x[:1].cpu().numpy(), x)
    n = int(fr["n_persons"])
    assert n == len(humans) and int(fr["status"]) == 0
    assert (fr["person_joint"][:n] >= 0).astype(int).tolist() == vis
    d2, d3 = np.abs(fr["joints_2d"][:n] - np.array(want2)).max(), np.abs(fr["joints_3d"][:n] - np.array(want3)).max()
    print("T4 rtpose: %d persons, %d visible joints, max 2D diff %g px, max 3D diff %g m" % (n, int(np.array(vis).sum()), d2, d3))
    assert np.allclose(fr["joints_2d"][:n], np.array(want2), atol=1e-9)
    assert d3 < 1e-3
    lists = eng.predict_lists(dev_frame)
    assert sorted(lists) == ["human_pred_set_2d", "human_pred_set_3d", "visibility_pred_set"] and lists["visibility_pred_set"][0] == vis
    assert lists["human_pred_set_3d"][0] == np.asarray(fr["joints_3d"][:n]).tolist()


@pytest.mark.parametrize("case", ["detection", "placeholder"])
def test_yolo_engine_itop_end_to_end_vs_oracle(gpu, golden, itop_frame, case):
    from oracle import nets, parse_yolo as OY, preproc as opre
    from popnet_amd import dataset
    from popnet_amd.pipeline import YoloEngine
    from popnet_amd.profiles import ITOP
    sd = state_dict_from_keys(golden.keys["yolo_posenet"], seed=YOLO_SEED)
    # the recorded confidence calibration; the placeholder case pushes every confidence below the script's 0.1
    sd["model2_4.0.weight"][[4, 54]] -= np.float32(golden.script_yolo["conf_weight_shift"] + (1.0 if case == "placeholder" else 0.0))
    x = opre.preprocess_batch(itop_frame[None], depth_max=5)
    out = nets.yolo_posenet_forward(torch.from_numpy(x), sd).numpy()
    _, rh, _ = OY.parse_prior_pose(out.copy(), YOLO_ANCHORS, 15, 224, 224, 3, 2, 0.1, 0.5)
    assert (len(rh[0]) >= 1) == (case == "detection"), "seed / shift chosen on the CPU: %d detections" % len(rh[0])
    want2, want3 = ir.yolo_glue(rh[0])
    eng = YoloEngine(precision="fp32", state_dict=sd, device=gpu, max_batch=2, conf_threshold=0.1, profile=ITOP)
    recs = eng.predict_host(torch.from_numpy(itop_frame[None]).to(gpu))
    assert int(recs[0]["n_det"]) == len(rh[0]) and int(recs[0]["status"]) == 0
    lists = dataset.yolo_records_to_lists(recs, profile=ITOP)
    assert sorted(lists) == ["human_pred_set_2d", "human_pred_set_3d"] and len(lists["human_pred_set_2d"][0]) == 1
    d2 = np.abs(np.array(lists["human_pred_set_2d"][0]) - np.array(want2)).max()
    d3 = np.abs(np.array(lists["human_pred_set_3d"][0]) - np.array(want3)).max()
    print("T4 yolo %s: %d detections, max 2D diff %g px, max 3D diff %g m" % (case, len(rh[0]), d2, d3))
    assert d2 < 5e-2 and d3 < 1e-3
    if case == "placeholder":
        assert d2 == 0 and d3 == 0 and want3[0][0][2] == -1.0
    else:
        assert np.array(want3)[0, :, 2].max() > 0      # a decoded pose, not the placeholder; Y carries the flipped sign
        j2, j3 = np.array(lists["human_pred_set_2d"][0][0]), np.array(lists["human_pred_set_3d"][0][0])
        assert np.array_equal(np.sign(j3[:, 1]), -np.sign((j2[:, 1] - 120) * j3[:, 2]))


# ---- the two scripts on a tiny ITOP tree -------------------------------------------------------------------------------------------
def _write_itop_tree(d, frame, n=4, seed=21):
    """annotations/ITOP_side_{train,test}_labels.json + <id>.npy frames: the committed frame with seeded noise, one person per id, every
    other one without 'pose_weight'."""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(d, "annotations"))
    os.makedirs(os.path.join(d, "depth"))
    ann = {}
    for i in range(n):
        name = "00_%05d" % i
        np.save(os.path.join(d, "depth", name + ".npy"), (frame.astype(np.float32) + rng.normal(0, 0.01, frame.shape)).astype(np.float16))
        j2 = np.stack([rng.uniform(60, 260, 15), rng.uniform(30, 210, 15)], axis=1)
        z = rng.uniform(2.0, 3.0, 15)
        person = {"2d_joints": j2.tolist(), "visible_joints": (rng.uniform(0, 1, 15) < 0.8).astype(int).tolist(),
                  "3d_joints": np.stack([(j2[:, 0] - 160) * z * 0.0035, -(j2[:, 1] - 120) * z * 0.0035, z], axis=1).tolist()}
        if i % 2:
            person["pose_weight"] = 1.5
        ann[name] = [person]
    for split in ("train", "test"):
        json.dump(ann, open(os.path.join(d, "annotations", "ITOP_side_%s_labels.json" % split), "w"))
    return os.path.join(d, "annotations"), os.path.join(d, "depth")


@pytest.mark.parametrize("net,n_keys", [("rtpose", 234), ("yolo", 223)])
def test_train_itop_then_evaluate_itop(gpu, itop_frame, tmp_path, net, n_keys):
    """scripts/train_itop.py (one epoch with the random transform, a validation loss, best_pose.pth in the reference's key format) and
    scripts/evaluate_itop.py on that checkpoint (eval_data.json with the reference script's keys, one entry per frame).  Each script is a
    child process under its own time limit; the first failure ends the test."""
    import subprocess
    ann_dir, img_dir = _write_itop_tree(str(tmp_path / "itop"), itop_frame)
    out = str(tmp_path / "model")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_itop.py"), "--net", net, "--train-annotations", os.path.join(ann_dir, "ITOP_side_train_labels.json"),
           "--train-image-dir", img_dir, "--val-annotations", os.path.join(ann_dir, "ITOP_side_test_labels.json"), "--val-image-dir", img_dir,
           "--output-dir", out, "--batch-size", "2", "--epochs", "1", "--lr", "0.05", "--print-freq", "1", "--seed", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(l.split("Loss")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("Epoch: [")]
    vals = [float(l.split("val loss")[1].split()[0]) for l in r.stdout.splitlines() if "val loss" in l]
    assert len(losses) == 2 and len(vals) == 1 and all(np.isfinite(v) for v in losses + vals), r.stdout
    sd = torch.load(os.path.join(out, "best_pose.pth"), map_location="cpu")
    assert len(sd) == n_keys and all(k.startswith("module.") for k in sd)
    res = str(tmp_path / "eval")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "evaluate_itop.py"), "--net", net, "--annotations", os.path.join(ann_dir, "ITOP_side_test_labels.json"),
           "--image-dir", img_dir, "--weight", os.path.join(out, "best_pose.pth"), "--output-dir", res, "--batch-size", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    data = json.load(open(os.path.join(res, "eval_data.json")))
    keys = ["human_gt_set_2d", "human_gt_set_3d", "human_pred_set_2d", "human_pred_set_3d"] + (["visibility_pred_set"] if net == "rtpose" else [])
    assert sorted(data) == sorted(keys) and all(len(data[k]) == 4 for k in keys)
    if net == "yolo":
        assert all(np.array(p).shape == (1, 15, 2) for p in data["human_pred_set_2d"])      # one person per frame, detection or placeholder
    assert "evaluation result of 2D poses" in r.stdout and "evaluation result of 3D poses" in r.stdout and "2D threshold: 8.000000" in r.stdout
    assert os.path.exists(os.path.join(res, "eval_res2d.json")) and os.path.exists(os.path.join(res, "eval_res3d.json"))
