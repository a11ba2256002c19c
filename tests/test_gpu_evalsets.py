"""GPU: what the composed (`test_mpaug`) and single-person (`val`, `test_bgaug`) KDH3D evaluation sets add -- the chain without Crop through
pn_augment_resize, the background swap pn_compose_bg, the depth-ablation arms reading the network input tensor (PN_DEPTH_NET),
PoseEngine / YoloEngine.predict_inputs, the loaders and the two scripts -- against tests/evalsets_reference.py and
tests/ablation_reference.py on the fake tree of tests/evalsets_cases.py (40 x 36 frames, network input 32).

Bars: the ones the same launches already have.  The composed network input bit for bit (tests/test_gpu_augment.py); the swap bit for bit (a
select); the arms == in float64 (tests/test_gpu_ablation.py: one float32 value un-normalised with two roundings, back-projected in
float64 -- a read-out has nothing to tolerate); predict_inputs bit for bit against the calls it is made of; the loaders bit for bit against
what the reference's own loaders returned on the same tree (tests/golden/evalsets_inputs.npz).  The scripts run as child processes and are
compared with the loader, the engine and the restated script lines in this process: == for Open-Pose+, and for Yolo-Pose+ the bars of
tests/test_gpu_itop.py for the same quantities (2D within 5e-2 px, 3D within 1e-3 m of the float64 restatement; the records are float32).
Last, the two scripts against what the REFERENCE's four scripts wrote on the same tree, seed and weights
(tests/golden/script_eval_data_{mpaug,mpaug_yolo,kdh3d,kdh3d_yolo}.json): eval_data.json and the metric tables."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import ablation_reference as AR
import cv2_warp_reference as cw
import evalsets_cases as EC
import evalsets_reference as ER
import parse_cases as PC
import popnet_amd  # noqa: F401
from popnet_amd import _lib, synth
from popnet_amd.utils.paf_to_pose import make_parse_cfg, parse_paf_unbounded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = dict(H=EC.H, W=EC.W, cx=EC.CX, cy=EC.CY, input_size=EC.S)
ARMS = ("human_pred_set_3d_read_raw_depth", "human_pred_set_3d_perfect_2d", "human_pred_set_3d_perfect_2d_read_raw_depth")
J, P = _lib.PN_NUM_JOINTS, _lib.PN_MAX_PERSONS


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _ctx(gpu):
    return _lib.Context.for_device(gpu.index), _lib.lib(), _lib.current_stream_ptr(gpu)


def _intr(cfg):
    return {"fx": cfg.fx, "fy": cfg.fy, "cx": cfg.cx, "cy": cfg.cy}


@pytest.fixture(scope="module")
def data():
    return EC.build()


@pytest.fixture(scope="module")
def tree(tmp_path_factory, data):
    return EC.write_tree(tmp_path_factory.mktemp("evalsets_tree"), data)


# ---------------------------------------------------------------------------------------------
# the composed test set: draws -> compose_depth -> augment_resize(crops=None)
# ---------------------------------------------------------------------------------------------
def test_composed_network_input_equals_the_restatement(gpu, data, tree):
    """MPAugTrainSet.test_batch under the seed draws what the restatement draws, and its two batches go through the two launches to the
    restatement's network input, bit for bit; the labels to the ground truth the scripts collect."""
    from popnet_amd import targets
    ts = targets.MPAugTrainSet(tree["img"], tree["ann_files"], tree["bg_file"], tree["bg"], tree["seg"], device=gpu, shuffle=False)
    assert len(ts) == max(EC.SET_SIZES)
    random.seed(EC.DRAW_SEED)
    want_items = ER.batch_draws(3, EC.SET_SIZES, EC.N_BG) + ER.batch_draws(3, EC.SET_SIZES, EC.N_BG)
    random.seed(EC.DRAW_SEED)
    seen_a = set()
    for k in range(2):
        fd, fm, n_src, bg, k2, k3, npers, aug = ts.test_batch(3, input_size=EC.S)
        assert fd.dtype == torch.float16 and tuple(fd.shape) == (3, 2, EC.H, EC.W) and isinstance(k2, np.ndarray)
        image = targets.compose_depth(fd, fm, n_src, bg)
        x = targets.augment_resize(image, aug, EC.S, EC.DMAX, EC.MEAN, EC.STD).cpu().numpy()
        kp, kz, _ = aug.transform_labels(k2, k3)
        gt2, gt3 = targets.composed_ground_truth(kp, k3, kz, npers, EC.W, EC.H, EC.S)
        for b in range(3):
            it = want_items[3 * k + b]
            assert (aug.items[b]["rot"], aug.items[b]["a"], aug.items[b]["crops"]) == (it["rot"], it["a"], None)
            composed, persons = EC.composed_item(data, it)
            assert np.array_equal(image[b].cpu().numpy(), composed.astype(np.float32))
            img, lab, _ = ER.nocrop_reference(composed, persons, dict(rot=it["rot"], a=it["a"], cx=EC.CX, cy=EC.CY, input_size=EC.S))
            want = cw.network_input(img, EC.DMAX, EC.MEAN, EC.STD)
            assert np.array_equal(x[b, 0], want), (k, b, np.abs(x[b, 0] - want).max())
            assert gt2[b] == ER.gt_to_original(lab, EC.W, EC.H, EC.S) and gt3[b] == [l["3d_joints"].tolist() for l in lab]
            seen_a.add(aug.items[b]["render_a"] <= 1)
    assert seen_a == {True, False}


def test_no_crop_differs_from_zero_crop_by_one_row_and_column(gpu):
    """The switch does something: Crop with zero fractions resizes a source one row and one column smaller, and both are the restatement's."""
    from popnet_amd import targets
    rng = np.random.default_rng(12)
    frames = rng.uniform(-0.5, 6.5, (2, EC.H, EC.W)).astype(np.float32)
    for rot, a in ((3.0, 1.2), (-7.0, 0.8)):
        none = targets.augmentation(rot, a, None, **GEOM)
        zero = targets.augmentation(rot, a, (0.0, 0.0, 0.0, 0.0), **GEOM)
        assert (none["src_w"], none["src_h"]) == (zero["src_w"] + 1, zero["src_h"] + 1)
        out = targets.augment_resize(_dev(frames, gpu), targets.AugmentationBatch([none, zero]), EC.S, EC.DMAX, EC.MEAN, EC.STD).cpu().numpy()
        par = dict(rot=rot, a=a, cx=EC.CX, cy=EC.CY, input_size=EC.S)
        assert np.array_equal(out[0, 0], cw.network_input(ER.nocrop_reference(frames[0], [], par)[0], EC.DMAX, EC.MEAN, EC.STD))
        assert np.array_equal(out[1, 0], cw.network_input(cw.augment_reference(frames[1], [], dict(par, crops=(0, 0, 0, 0)))[0], EC.DMAX, EC.MEAN, EC.STD))
        same = targets.augment_resize(_dev(frames[:1], gpu), targets.AugmentationBatch([zero]), EC.S, EC.DMAX, EC.MEAN, EC.STD).cpu().numpy()
        assert np.count_nonzero(same[0] != out[0]) > EC.S * EC.S // 2               # the same frame through the two chains


# ---------------------------------------------------------------------------------------------
# pn_compose_bg
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("B", [1, 3])
def test_compose_bg_equals_the_restatement_bit_for_bit(gpu, data, dtype, B):
    from popnet_amd import targets
    names = data["single_ids"][:B]
    rng = np.random.default_rng(B)
    fg = np.stack([data["frames"][n] for n in names]).astype(dtype)
    bg = np.stack([data["bgs"][data["bg_names"][i % EC.N_BG]] for i in range(B)]).astype(dtype)
    if dtype == np.float32:                                                         # values float16 cannot hold
        fg, bg = fg + rng.uniform(0, 1e-3, fg.shape).astype(dtype), bg + rng.uniform(0, 1e-3, bg.shape).astype(dtype)
        fg[0][EC.FAR] = 12.5
    mask = np.stack([data["masks"][n] for n in names])
    mask[0, 20, 5] = 255                                                            # any value above 0 selects the foreground
    out = targets.compose_bg(_dev(fg, gpu), _dev(mask, gpu), _dev(bg, gpu))
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, EC.H, EC.W)
    want = np.stack([ER.compose_bg(fg[b], (mask[b] > 0), bg[b]) for b in range(B)])
    assert np.array_equal(out.cpu().numpy().astype(np.float64), want)
    # the pixel above 2 * depth_max survives here; the z-buffer composition with that one source cuts it to the cap
    zb = targets.compose_depth(_dev(fg[:, None], gpu), _dev((mask[:, None] > 0).astype(np.uint8), gpu), torch.ones((B,), dtype=torch.int32, device=gpu),
                               _dev(bg, gpu)).cpu().numpy()
    o = out.cpu().numpy()
    assert o[0][EC.FAR] == 12.5 and zb[0][EC.FAR] == np.float32(2 * EC.DMAX)
    assert np.array_equal(o[mask == 0], zb[mask == 0]) and (o != zb).any()


def test_compose_bg_refuses_bad_arguments_before_any_launch(gpu):
    from popnet_amd import targets
    ctx, L, st = _ctx(gpu)
    fg = torch.ones((1, 4, 4), device=gpu)
    m = torch.ones((1, 4, 4), dtype=torch.uint8, device=gpu)
    out = torch.full((1, 4, 4), -7.0, device=gpu)
    assert L.pn_compose_bg(ctx.handle, _vp(fg), _vp(m), _vp(fg), _lib.PN_DEPTH_NET, 1, 4, 4, _vp(out), st) == -1      # not a frame dtype
    assert L.pn_compose_bg(ctx.handle, None, _vp(m), _vp(fg), _lib.PN_DEPTH_F32, 1, 4, 4, _vp(out), st) == -1
    assert L.pn_compose_bg(ctx.handle, _vp(fg), _vp(m), _vp(fg), _lib.PN_DEPTH_F32, 65536, 4, 4, _vp(out), st) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    with pytest.raises(_lib.PopnetError, match="float16 or float32"):
        targets.compose_bg(fg, m, fg.half())
    with pytest.raises(_lib.PopnetError, match="shape"):
        targets.compose_bg(fg, m[:, :2], fg)


# ---------------------------------------------------------------------------------------------
# PN_DEPTH_NET: the arms on the network input tensor
# ---------------------------------------------------------------------------------------------
S, B, MEAN, STD = 16, 3, 2.9, 1.7                  # a normalisation whose `* std + mean` is not exact
W_ORG, H_ORG = 12, 20


@pytest.fixture(scope="module")
def hand(gpu):
    """A hand-built network input, records, maps and ground truth -- the records and ground truth of tests/test_gpu_ablation.py's `hand`."""
    rng = np.random.default_rng(43)
    x = rng.normal(0.0, 1.2, (B, 1, S, S)).astype(np.float32)
    cfg = make_parse_cfg(input_size=S, w_org=W_ORG, h_org=H_ORG, depth_mean=MEAN, depth_std=STD)
    z = rng.normal(0.0, 1.0, (B, 15, S // 8, S // 8)).astype(np.float32)
    recs = np.zeros((B,), _lib.POSE_FRAME_DTYPE)
    npk = 40
    for b in range(B):
        r = recs[b]
        r["n_peaks"] = npk
        xy = rng.integers(0, S, (npk, 2)).astype(np.float32)
        xy[0], xy[1] = (0, 0), (S - 1, S - 1)                                 # the frame's corners
        r["peak_x"][:npk], r["peak_y"][:npk] = xy[:, 0], xy[:, 1]
        r["person_joint"][:] = rng.integers(0, npk, (P, J))                   # rows past n_persons hold ids too: they must not be read out
    recs[0]["n_persons"] = 0
    recs[1]["n_persons"] = P
    recs[1]["person_joint"][0] = -1
    recs[1]["person_joint"][1, :2] = (0, 1)
    recs[1]["person_joint"][2:][rng.random((P - 2, J)) < 0.3] = -1
    recs[2]["n_persons"] = 3
    recs[2]["person_joint"][1, ::2] = -1
    for b in range(B):
        r = recs[b]
        ids = r["person_joint"]
        vis = ids >= 0
        px, py = r["peak_x"][np.maximum(ids, 0)].astype(np.float64), r["peak_y"][np.maximum(ids, 0)].astype(np.float64)
        r["joints_2d"][..., 0] = np.where(vis, px / S * W_ORG, -1.0)
        r["joints_2d"][..., 1] = np.where(vis, py / S * H_ORG, -1.0)
    G = 3
    W, H = W_ORG, H_ORG
    # ground truth at 0, S - 1 (in network pixels), negative, on and past the far edge, one ulp below a pixel / cell boundary
    edge = [[-2.5, -0.25], [float(W), float(H)], [W + 1.5, H + 7.0], [0, 0], [W - 1, H - 1], [W, 3], [np.nextafter(W / 2, 0), np.nextafter(H / 2, 0)],
            [W / 2, H / 2], [np.nextafter(5 * W / S, 0), np.nextafter(11 * H / S, 0)], [5 * W / S, 11 * H / S], [-1e9, 1e9], [W - 1e-9, H - 1e-9],
            [(S - 1) * W / S, (S - 1) * H / S], [0.999 * W / S, 0.999 * H / S], [W / 2 + 0.01, H / 2 - 0.01]]
    gt = [[], [edge, rng.uniform([-2, -2], [W + 2, H + 2], (J, 2)).tolist(), rng.integers(0, W + 1, (J, 2)).tolist()],
          [rng.uniform([0, 0], [W, H], (J, 2)).tolist()]]
    gt_arr = np.full((B, G, J, 2), 123.0)
    for b, g in enumerate(gt):
        for i, h in enumerate(g):
            gt_arr[b, i] = np.asarray(h, dtype=np.float64)
    return dict(x=x, cfg=cfg, z=z, recs=recs, gt=gt, G=G, d_x=_dev(x, gpu), d_z=_dev(z, gpu), d_recs=_dev(recs.view(np.uint8).reshape(B, -1), gpu),
                d_gt=_dev(gt_arr, gpu), d_cnt=_dev(np.array([len(g) for g in gt], np.int32), gpu))


def test_hand_built_input_shows_a_fused_unnormalisation(hand):
    x = hand["x"].astype(np.float64)
    fused = (x * np.float64(np.float32(STD)) + np.float64(np.float32(MEAN))).astype(np.float32)
    assert np.count_nonzero(AR.unnormalise(hand["x"], MEAN, STD) != fused) > 20


def test_depth_probe_on_the_tensor_equals_indexing_it(hand, gpu):
    ctx, L, st = _ctx(gpu)
    x = hand["d_x"]
    want = AR.unnormalise(hand["x"][:, 0], MEAN, STD)
    yy, xx = np.mgrid[0:S, 0:S]
    pts = np.concatenate([np.stack([np.full(S * S, b), yy.ravel(), xx.ravel()], 1) for b in (2, 1, 0)]).astype(np.int32)      # 768 points: three blocks
    out = torch.full((len(pts),), float("nan"), device=gpu)
    # depth_max plays no part for this kind: a value far below the pixels must not clamp them
    ctx.check(L.pn_depth_probe(ctx.handle, _vp(x), _lib.PN_DEPTH_NET, B, S, S, S, 0.001, MEAN, STD, _vp(_dev(pts, gpu)), len(pts), _vp(out), st), "pn_depth_probe")
    assert np.array_equal(out.cpu().numpy().reshape(3, S, S), want[::-1])
    out = torch.full((2,), 7.0, device=gpu)
    for bad in ((0, S, 0), (0, 0, S), (0, -1, 0), (B, 0, 0), (-1, 0, 0)):
        pts = torch.tensor([[0, 0, 0], list(bad)], dtype=torch.int32, device=gpu)
        rc = L.pn_depth_probe(ctx.handle, _vp(x), _lib.PN_DEPTH_NET, B, S, S, S, 6.0, MEAN, STD, _vp(pts), 2, _vp(out), st)
        assert rc == -1 and "outside" in ctx.last_error(), bad
    assert out.cpu().tolist() == [7.0, 7.0]


def test_pred_raw_on_the_tensor_equals_the_restatement(hand, gpu):
    ctx, L, st = _ctx(gpu)
    cfg = hand["cfg"]
    out = torch.full((B, P, J, 3), float("nan"), device=gpu, dtype=torch.float64)
    ctx.check(L.pn_ablation_pred_raw(ctx.handle, _vp(hand["d_x"]), _lib.PN_DEPTH_NET, B, S, S, 6.0, C.byref(cfg), _vp(hand["d_recs"]), _vp(out), st),
              "pn_ablation_pred_raw")
    got = out.cpu().numpy()
    corners = 0
    for b in range(B):
        r = hand["recs"][b]
        n = int(r["n_persons"])
        img = AR.unnormalise(hand["x"][b, 0], MEAN, STD)
        want = AR.pred_raw(img, np.stack([r["peak_x"], r["peak_y"]], 1), r["person_joint"][:n], W_ORG, H_ORG, S, _intr(cfg))
        assert np.array_equal(got[b, :n], want), b
        assert np.all(got[b, n:] == 0.0)
        assert np.all(got[b, :n][r["person_joint"][:n] < 0][:, 2] == -1.0)
        corners += int(np.isin(r["person_joint"][:n], (0, 1)).sum())
    assert corners >= 2                                                              # pixels (0, 0) and (S - 1, S - 1) were read


def test_perfect_2d_on_the_tensor_equals_the_restatement(hand, gpu):
    ctx, L, st = _ctx(gpu)
    cfg, G = hand["cfg"], hand["G"]
    om = torch.full((B, G, J, 3), float("nan"), device=gpu, dtype=torch.float64)
    orw = torch.full((B, G, J, 3), float("nan"), device=gpu, dtype=torch.float64)
    ctx.check(L.pn_ablation_perfect_2d(ctx.handle, _vp(hand["d_x"]), _lib.PN_DEPTH_NET, B, S, S, 6.0, _vp(hand["d_z"]), S // 8, S // 8, C.byref(cfg),
                                       _vp(hand["d_gt"]), _vp(hand["d_cnt"]), G, _vp(om), _vp(orw), st), "pn_ablation_perfect_2d")
    gm, gr = om.cpu().numpy(), orw.cpu().numpy()
    for b in range(B):
        g = hand["gt"][b]
        img = AR.unnormalise(hand["x"][b, 0], MEAN, STD)
        wm, wr = AR.perfect_2d(img, hand["z"][b], g, W_ORG, H_ORG, S, 8, MEAN, STD, _intr(cfg))
        assert np.array_equal(gm[b, :len(g)], wm) and np.array_equal(gr[b, :len(g)], wr), b
        assert np.all(gm[b, len(g):] == 0.0) and np.all(gr[b, len(g):] == 0.0)


def test_tensor_kind_refusals_leave_the_outputs_untouched(hand, gpu):
    """H != S or W != S, a null buffer and an unknown kind: PN_ERR_INVALID from all three entries before any launch.  A 2S x 2S "tensor" is the
    size mismatch, not the 2x decimation of the frame kinds."""
    ctx, L, st = _ctx(gpu)
    cfg = hand["cfg"]
    x = hand["d_x"]
    big = torch.zeros((1, 1, 2 * S, 2 * S), device=gpu)
    out = torch.full((B, P, J, 3), 5.0, device=gpu, dtype=torch.float64)
    om, orw = (torch.full((B, hand["G"], J, 3), 5.0, device=gpu, dtype=torch.float64) for _ in range(2))
    pts, po = torch.zeros((1, 3), dtype=torch.int32, device=gpu), torch.full((1,), 5.0, device=gpu)
    NET = _lib.PN_DEPTH_NET
    cases = [(_vp(x), NET, S + 1, S), (_vp(x), NET, S, S - 1), (_vp(big), NET, 2 * S, 2 * S), (None, NET, S, S), (_vp(x), 3, S, S), (_vp(x), -1, S, S)]
    for buf, kind, Hh, Ww in cases:
        nb = 1 if Hh == 2 * S else B
        rcs = [L.pn_ablation_pred_raw(ctx.handle, buf, kind, nb, Hh, Ww, 6.0, C.byref(cfg), _vp(hand["d_recs"]), _vp(out), st),
               L.pn_ablation_perfect_2d(ctx.handle, buf, kind, nb, Hh, Ww, 6.0, _vp(hand["d_z"]), S // 8, S // 8, C.byref(cfg), _vp(hand["d_gt"]),
                                        _vp(hand["d_cnt"]), hand["G"], _vp(om), _vp(orw), st),
               L.pn_depth_probe(ctx.handle, buf, kind, nb, Hh, Ww, S, 6.0, MEAN, STD, _vp(pts), 1, _vp(po), st)]
        assert rcs == [-1, -1, -1], (kind, Hh, Ww, rcs)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((om == 5.0).all()) and bool((orw == 5.0).all()) and po.item() == 5.0
    # the other entries that take a depth dtype do not take this one
    o = torch.empty((1, 1, S, S), device=gpu)
    assert L.pn_preprocess(ctx.handle, _vp(x), NET, 1, S, S, _vp(o), S, 6.0, MEAN, STD, st) == -1


# ---------------------------------------------------------------------------------------------
# predict_inputs and the engine's arms on the network input
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def depth4(gpu):
    return torch.from_numpy(synth.synth_depth(4, 640, 480, seed=13)).to(gpu)


@pytest.fixture(scope="module")
def bf16_engine(gpu):
    from popnet_amd.pipeline import PoseEngine
    return PoseEngine(precision="bf16", device=gpu, max_batch=4)


def _input_of(eng, depth):
    n = eng.preprocess(depth)
    return eng.x[:n].clone()


def test_predict_inputs_fp32_equals_preprocess_forward_parse(gpu, depth4):
    from popnet_amd.pipeline import PoseEngine, records_to_numpy
    eng = PoseEngine(precision="fp32", device=gpu, max_batch=4)
    n = eng.preprocess(depth4[:3])
    x = eng.x[:3].clone()
    eng.forward(n)
    eng.parse(n)
    want = eng.frames[:3].clone()
    maps = [t[:3].clone() for t in (eng.paf, eng.heat, eng.z)]
    assert int(records_to_numpy(want)["n_persons"].sum()) > 0
    for t in (eng.x, eng.paf, eng.heat, eng.z, eng.frames):
        t.zero_()
    got = eng.predict_inputs(x)
    assert torch.equal(got, want) and all(torch.equal(a[:3], b) for a, b in zip((eng.paf, eng.heat, eng.z), maps))
    own = torch.zeros_like(want)
    assert eng.predict_inputs(x[:2], frames=own).data_ptr() == own.data_ptr() and torch.equal(own[:2], want[:2])
    for bad in (x[:, 0], x.double(), x[:, :, :100], torch.zeros((5, 1, 224, 224), device=gpu)):
        with pytest.raises(_lib.PopnetError):
            eng.predict_inputs(bad)
    with pytest.raises(_lib.PopnetError, match="CUDA/ROCm"):
        eng.predict_inputs(x.cpu())


def test_predict_inputs_bf16_equals_forward_after_a_copy(gpu, bf16_engine, depth4):
    """The frames-in precisions have a fused stem for raw frames; on a network input they run the plain forward on self.x."""
    eng = bf16_engine
    x = _input_of(eng, depth4)
    eng.x.zero_()
    eng.x[:4].copy_(x)
    eng.forward(4)
    eng.parse(4)
    want = eng.frames[:4].clone()
    maps = [t[:4].clone() for t in (eng.paf, eng.heat, eng.z)]
    for t in (eng.x, eng.paf, eng.heat, eng.z, eng.frames):
        t.zero_()
    got = eng.predict_inputs(x)
    assert torch.equal(got, want) and all(torch.equal(a[:4], b) for a, b in zip((eng.paf, eng.heat, eng.z), maps))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_yolo_predict_inputs_equals_its_parts(gpu, depth4, precision):
    from popnet_amd.pipeline import YoloEngine
    eng = YoloEngine(precision=precision, device=gpu, max_batch=4)
    n = eng.preprocess(depth4[:3])
    x = eng.x[:3].clone()
    eng.forward(n)
    eng.parse(n)
    want, out = eng.frames[:3].clone(), eng.out[:3].clone()
    assert int(want.cpu().numpy().view(_lib.YOLO_FRAME_DTYPE)["n_det"].sum()) > 0
    for t in (eng.x, eng.out, eng.frames):
        t.zero_()
    assert torch.equal(eng.predict_inputs(x), want) and torch.equal(eng.out[:3], out)


def test_engine_arms_on_the_network_input_equal_the_restatement_and_the_frames_path(gpu, bf16_engine, depth4):
    """Every arm == the restatement on the engine's own z, records and input tensor; and, the tensor being pn_preprocess of these frames,
    == the arms that re-derive the pixel from the raw frames."""
    from popnet_amd.pipeline import records_to_numpy
    eng = bf16_engine
    x = _input_of(eng, depth4)
    rng = np.random.default_rng(3)
    gt = [rng.uniform([-20, -20], [500, 660], (n, J, 2)).tolist() for n in (2, 0, 1, 3)]
    gt[0][0][0], gt[0][0][1], gt[0][0][2] = [0.0, 0.0], [479.999, 639.999], [480.0, 640.0]
    recs_dev = eng.predict_inputs(x)
    raw, pm, pr = eng.ablation_arms(x, recs_dev, gt)
    via_frames = eng.ablation_arms(depth4, recs_dev, gt)
    assert all(torch.equal(a, b) for a, b in zip((raw, pm, pr), via_frames))
    recs, raw, pm, pr = records_to_numpy(recs_dev).copy(), raw.cpu().numpy(), pm.cpu().numpy(), pr.cpu().numpy()
    z, xh = eng.z[:4].cpu().numpy(), x[:, 0].cpu().numpy()
    assert int(recs["n_persons"].sum()) > 0 and not recs["status"].any()
    for b in range(4):
        r = recs[b]
        n, g = int(r["n_persons"]), len(gt[b])
        want = ER.net_input_arms(xh[b], z[b], (np.stack([r["peak_x"], r["peak_y"]], 1), r["person_joint"][:n]), gt[b], 480, 640, 224,
                                 intrinsics=_intr(eng.cfg))
        assert np.array_equal(raw[b, :n], want[ARMS[0]]) and np.all(raw[b, n:] == 0.0)
        assert np.array_equal(pm[b, :g], want[ARMS[1]]) and np.array_equal(pr[b, :g], want[ARMS[2]])
    pts = np.array([[0, 0, 0], [3, 223, 223], [1, 100, 7]])
    assert np.array_equal(eng.depth_probe(x, pts), AR.unnormalise(xh, 3.0, 2.0)[pts[:, 0], pts[:, 1], pts[:, 2]])
    with pytest.raises(_lib.PopnetError, match="network input"):
        eng.ablation_arms(x[:, :, :200], recs_dev, gt)


def test_overflowing_frame_takes_the_second_pass_on_the_network_input(gpu, bf16_engine, depth4):
    """tests/test_gpu_ablation.py's overflow case with the tensor in place of the frames: the raw arm of the re-parsed frame comes from
    pn_depth_probe on the tensor."""
    from popnet_amd.pipeline import records_to_numpy
    eng = bf16_engine
    x = _input_of(eng, depth4[:1])
    c = PC.case("peaks33")
    for name in ("heat", "paf", "z"):
        getattr(eng, name)[0].copy_(torch.from_numpy(np.ascontiguousarray(getattr(c, name).transpose(2, 0, 1))))
    eng.parse(1)
    recs = eng.frames[:1]
    gt = [np.random.default_rng(4).uniform(0, 480, (2, J, 2)).tolist()]
    raw, pm, pr = eng.ablation_arms(x, recs, gt)
    host = records_to_numpy(recs)
    assert int(host[0]["status"]) == _lib.PN_FRAME_OVERFLOW_PEAKS
    lists = eng.ablation_lists(x, gt, host, raw, pm, pr)
    ub = parse_paf_unbounded(eng.heat[0], eng.paf[0], eng.z[0], eng.cfg)
    assert (ub["person_joint"] >= 0).any() and len(ub["joint_list"]) > int(host[0]["n_peaks"])
    want = AR.pred_raw(AR.unnormalise(x[0, 0].cpu().numpy(), 3.0, 2.0), ub["joint_list"], ub["person_joint"], 480, 640, 224, _intr(eng.cfg))
    assert lists[ARMS[0]][0] == want.tolist() and len(lists[ARMS[1]][0]) == 2


# ---------------------------------------------------------------------------------------------
# end to end: the loaders, the engines and the two scripts on the fake tree (fp32 parity mode, network input 32)
# ---------------------------------------------------------------------------------------------
SEED = 5
ENG = dict(precision="fp32", max_batch=3, input_size=EC.S, w_org=EC.W, h_org=EC.H, intrinsics=EC.INTRINSICS)
POSE_KEYS = {"human_pred_set_2d", "human_pred_set_3d", "visibility_pred_set", "human_gt_set_2d", "human_gt_set_3d"}
YOLO_KEYS = {"human_pred_set_2d", "human_pred_set_3d", "human_gt_set_2d", "human_gt_set_3d"}
ABL_KEYS = set(ARMS) | {"human_gt_set_2d_visible"}


@pytest.fixture(scope="module")
def checkpoints(gpu, tmp_path_factory):
    """Synthetic calibrated weights of both nets as the checkpoints the scripts load ('module.'-prefixed, like the reference's).  Weight
    seed 1: on this tree the Open-Pose+ net finds nobody in some frames and two persons in others (asserted below)."""
    from popnet_amd.pipeline import PoseEngine, YoloEngine
    d = tmp_path_factory.mktemp("evalsets_ckpt")
    out = {}
    for net, cls in (("rtpose", PoseEngine), ("yolo", YoloEngine)):
        eng = cls(weight_seed=1, device=gpu, **ENG)
        sd = {k: v.detach().cpu().clone() for k, v in eng.model.state_dict().items()}
        torch.save({"module." + k: v for k, v in sd.items()}, str(d / (net + ".pth")))
        out[net] = (str(d / (net + ".pth")), sd)
    return out


def _engine(net, sd, gpu, first_person):
    from popnet_amd.pipeline import PoseEngine, YoloEngine
    if net == "rtpose":
        return PoseEngine(state_dict=sd, device=gpu, **ENG)
    return YoloEngine(state_dict=sd, device=gpu, conf_threshold=0.1 if first_person else 0.5, nms_threshold=0.5, **ENG)


def _expected_lists(eng, net, x, g2, first_person):
    """The script's per-frame lists of one batch from the engine's own records and maps: the restatement's arms and list conventions."""
    from popnet_amd import dataset
    from popnet_amd.pipeline import records_to_numpy
    nb = x.shape[0]
    if net == "yolo":
        recs = eng.predict_inputs(x).cpu().numpy().view(_lib.YOLO_FRAME_DTYPE).reshape(-1)
        got = dataset.yolo_kdh3d_lists(recs, first_person=first_person, input_size=EC.S, w_org=EC.W, h_org=EC.H, intrinsics=EC.INTRINSICS)
        for b in range(nb):
            n = int(recs[b]["n_det"])
            w2, w3 = ER.yolo_lists(recs[b]["human"][:n].astype(np.float64), EC.W, EC.H, EC.S, EC.INTRINSICS, first=first_person)
            g2d, g3d = np.array(got["human_pred_set_2d"][b]), np.array(got["human_pred_set_3d"][b])
            assert g2d.shape == np.array(w2).shape and g3d.shape == np.array(w3).shape            # person count, first-person / placeholder choice
            assert np.abs(g2d - np.array(w2)).max() < 5e-2 and np.abs(g3d - np.array(w3)).max() < 1e-3
        return got, [int(r["n_det"]) for r in recs]
    recs = records_to_numpy(eng.predict_inputs(x)).copy()
    assert not recs["status"].any()
    full = dataset.pose_records_to_lists(recs)
    z, xh = eng.z[:nb].cpu().numpy(), x[:, 0].cpu().numpy()
    cut = ER.first_person if first_person else (lambda v: v)
    out = {"human_pred_set_2d": cut(full["human_pred_set_2d"]), "human_pred_set_3d": cut(full["human_pred_set_3d"]),
           "visibility_pred_set": cut(full["human_pred_set_visibility"]), ARMS[0]: [], ARMS[1]: [], ARMS[2]: [], "human_gt_set_2d_visible": []}
    for b in range(nb):
        r = recs[b]
        n = int(r["n_persons"])
        arms = ER.net_input_arms(xh[b], z[b], (np.stack([r["peak_x"], r["peak_y"]], 1), r["person_joint"][:n]), g2[b], EC.W, EC.H, EC.S,
                                 intrinsics=EC.INTRINSICS)
        out[ARMS[0]].append(arms[ARMS[0]].tolist()[:1] if first_person else arms[ARMS[0]].tolist())
        out[ARMS[1]].append(arms[ARMS[1]].tolist())
        out[ARMS[2]].append(arms[ARMS[2]].tolist())
        out["human_gt_set_2d_visible"].append([np.array(h).tolist() for h in g2[b]])
    return out, [int(r["n_persons"]) for r in recs]


def _run_script(script, argv, out_dir, limit=240):
    """A fresh child process under its own time limit."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + argv + ["--output-dir", out_dir], capture_output=True, text=True,
                       cwd=ROOT, timeout=limit)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout, json.load(open(os.path.join(out_dir, "eval_data.json")))


@pytest.mark.parametrize("net", ["rtpose", "yolo"])
def test_evaluate_mpaug_script_equals_the_pieces(gpu, tree, checkpoints, tmp_path, net):
    """scripts/evaluate_mpaug.py, two batches of three under --seed, against the loader, the engine and the restatement in this process."""
    from popnet_amd import targets
    ckpt, sd = checkpoints[net]
    argv = ["--net", net, "--annotations"] + tree["ann_files"] + ["--image-dir", tree["img"], "--bg-file", tree["bg_file"], "--bg-dir", tree["bg"],
            "--seg-dir", tree["seg"], "--weight", ckpt, "--batch-size", "3", "--num-batches", "2", "--input-size", str(EC.S), "--w-org", str(EC.W),
            "--h-org", str(EC.H), "--seed", str(SEED)] + (["--ablation"] if net == "rtpose" else [])
    stdout, data = _run_script("evaluate_mpaug.py", argv, str(tmp_path / "out"))
    assert set(data) == (POSE_KEYS | ABL_KEYS if net == "rtpose" else YOLO_KEYS) and all(len(v) == 6 for v in data.values())
    assert "evaluating in 2D..." in stdout and "evaluating in 3D..." in stdout and ("given perfect 2d" in stdout.lower()) == (net == "rtpose")
    eng = _engine(net, sd, gpu, False)
    random.seed(SEED)
    ts = targets.MPAugTrainSet(tree["img"], tree["ann_files"], tree["bg_file"], tree["bg"], tree["seg"], device=gpu)
    counts = []
    for k in range(2):
        fd, fm, n_src, bg, k2, k3, npers, aug = ts.test_batch(3, input_size=EC.S)
        assert all(it["crops"] is None for it in aug.items)
        x = targets.augment_resize(targets.compose_depth(fd, fm, n_src, bg), aug, EC.S, EC.DMAX, EC.MEAN, EC.STD)
        kp, kz, _ = aug.transform_labels(k2, k3)
        g2, g3 = targets.composed_ground_truth(kp, k3, kz, npers, EC.W, EC.H, EC.S)
        want, n = _expected_lists(eng, net, x, g2, False)
        counts += n
        want["human_gt_set_2d"], want["human_gt_set_3d"] = g2, g3
        for key, v in want.items():
            assert data[key][3 * k:3 * k + 3] == v, (key, k)
    assert [len(f) for f in data["human_pred_set_2d"]] == ([c for c in counts] if net == "rtpose" else [max(c, 1) for c in counts])
    if net == "rtpose":
        assert 0 in counts and max(counts) >= 2                                  # an empty frame and a frame with several persons
    # the seed above drew this process's frames; another seed draws other frames
    other =_run_script("evaluate_mpaug.py", argv[:-1 - (net == "rtpose")] + [str(SEED + 1), "--no-metrics"], str(tmp_path / "other"))[1]
    assert other["human_gt_set_2d"] != data["human_gt_set_2d"]


@pytest.mark.parametrize("net,bg_aug", [("rtpose", 1), ("rtpose", 0), ("yolo", 1)])
def test_evaluate_kdh3d_script_equals_the_pieces(gpu, data, tree, checkpoints, tmp_path, net, bg_aug):
    """scripts/evaluate_kdh3d.py on the single-person set (six frames, batches of three): the first-person rule, the placeholder of the Yolo
    net, the swapped background."""
    from popnet_amd import targets
    ckpt, sd = checkpoints[net]
    argv = ["--net", net, "--annotations", tree["single_ann"], "--image-dir", tree["img"], "--weight", ckpt, "--batch-size", "3", "--input-size", str(EC.S),
            "--w-org", str(EC.W), "--h-org", str(EC.H), "--seed", str(SEED), "--bg-aug", str(bg_aug)]
    if bg_aug:
        argv += ["--bg-file", tree["bg_file"], "--bg-dir", tree["bg"], "--seg-dir", tree["seg"]]
    if net == "rtpose":
        argv.append("--ablation")
    stdout, got = _run_script("evaluate_kdh3d.py", argv, str(tmp_path / "out"))
    assert set(got) == (POSE_KEYS | ABL_KEYS if net == "rtpose" else YOLO_KEYS) and all(len(v) == 6 for v in got.values())
    eng = _engine(net, sd, gpu, True)
    random.seed(SEED)
    ds = targets.KDH3DSingleSet(tree["img"], tree["single_ann"], bg_aug=bool(bg_aug), bg_file=tree["bg_file"], bg_dir=tree["bg"], seg_dir=tree["seg"], device=gpu)
    counts = []
    for k in range(2):
        chunk = list(range(3 * k, 3 * k + 3))
        frames = ds.frames(chunk).cpu().numpy()
        for b, i in enumerate(chunk):                                               # the loader against the restatement: bg index % n_bg of the shuffled list
            name = data["single_ids"][i]
            f = data["frames"][name]
            want = ER.compose_bg(f, data["masks"][name], data["bgs"][ds.bg[i % EC.N_BG]["file_name"]]) if bg_aug else f.astype(np.float64)
            assert np.array_equal(frames[b].astype(np.float64), want)
        x = ds.inputs(chunk, EC.S)
        g2, g3 = ds.ground_truth(chunk)
        want, n = _expected_lists(eng, net, x, g2, True)
        counts += n
        want["human_gt_set_2d"], want["human_gt_set_3d"] = g2, g3
        for key, v in want.items():
            assert got[key][3 * k:3 * k + 3] == v, (key, k)
    assert [len(f) for f in got["human_pred_set_2d"]] == ([min(c, 1) for c in counts] if net == "rtpose" else [1] * 6)
    if net == "rtpose" and bg_aug:
        assert 0 in counts and max(counts) >= 2                                  # the first-person rule cut somebody, an empty frame stayed empty
        assert len(got[ARMS[1]][0]) == len(got["human_gt_set_2d"][0])            # the perfect-2D arms follow the ground truth, uncut
    # --drop-last with a batch size that leaves a tail
    short = _run_script("evaluate_kdh3d.py", [a if a != "3" else "4" for a in argv] + ["--drop-last", "--no-metrics"], str(tmp_path / "short"))[1]
    assert all(len(v) == 4 for v in short.values())


def test_yolo_placeholder_rows_end_to_end(gpu, tree, checkpoints):
    """A confidence threshold nobody passes: every frame gets the scripts' placeholder person."""
    from popnet_amd import dataset, targets
    from popnet_amd.pipeline import YoloEngine
    eng = YoloEngine(state_dict=checkpoints["yolo"][1], device=gpu, conf_threshold=0.9999, **ENG)
    ds = targets.KDH3DSingleSet(tree["img"], tree["single_ann"], device=gpu)
    recs = eng.predict_inputs(ds.inputs([0, 1, 2], EC.S)).cpu().numpy().view(_lib.YOLO_FRAME_DTYPE).reshape(-1)
    assert recs["n_det"].tolist() == [0, 0, 0]
    want = ER.yolo_lists([], EC.W, EC.H, EC.S, EC.INTRINSICS)
    for first in (False, True):
        out = dataset.yolo_kdh3d_lists(recs, first_person=first, input_size=EC.S, w_org=EC.W, h_org=EC.H, intrinsics=EC.INTRINSICS)
        assert out["human_pred_set_2d"] == [want[0]] * 3 and out["human_pred_set_3d"] == [want[1]] * 3


# ---------------------------------------------------------------------------------------------
# the loaders against the reference loaders' own outputs (tests/golden/evalsets_inputs.npz)
# ---------------------------------------------------------------------------------------------
def test_composed_set_reproduces_the_reference_loader(gpu, tree):
    """random.seed + MPAugTrainSet (which shuffles like the reference's constructor) + test_batch + the two launches: the network inputs
    generate_test_batch returned, bit for bit, and its transformed labels."""
    from popnet_amd import targets
    G = EC.golden()
    random.seed(int(G["seed"]))
    ts = targets.MPAugTrainSet(tree["img"], tree["ann_files"], tree["bg_file"], tree["bg"], tree["seg"], device=gpu)
    assert [";".join(i) for i in ts.ids] == G["mpaug_ids"].tolist() and [b["file_name"] for b in ts.bg] == G["mpaug_bgs"].tolist()
    for k in range(2):
        fd, fm, n_src, bg, k2, k3, npers, aug = ts.test_batch(3, input_size=EC.S)
        x = targets.augment_resize(targets.compose_depth(fd, fm, n_src, bg), aug, EC.S, EC.DMAX, EC.MEAN, EC.STD).cpu().numpy()
        assert np.array_equal(x[:, 0], G["mpaug_b%d_images" % k]), (k, np.abs(x[:, 0] - G["mpaug_b%d_images" % k]).max())
        kp, kz, _ = aug.transform_labels(k2, k3)
        n = npers.cpu().numpy()
        assert n.tolist() == G["mpaug_b%d_npers" % k].tolist()
        assert np.array_equal(np.concatenate([kp[b, :n[b]] for b in range(3)]), G["mpaug_b%d_kp2d" % k])
        assert np.array_equal(np.concatenate([kz[b, :n[b]] for b in range(3)]), G["mpaug_b%d_kp3d" % k][:, :, 2])
        assert np.array_equal(np.concatenate([k3[b, :n[b], :, :2] for b in range(3)]), G["mpaug_b%d_kp3d" % k][:, :, :2])      # X, Y as labelled


@pytest.mark.parametrize("bg_aug", [0, 1])
def test_single_person_sets_reproduce_the_reference_loader(gpu, tree, bg_aug):
    from popnet_amd import targets
    G = EC.golden()
    random.seed(int(G["seed"]))
    ds = targets.KDH3DSingleSet(tree["img"], tree["single_ann"], bg_aug=bool(bg_aug), bg_file=tree["bg_file"], bg_dir=tree["bg"], seg_dir=tree["seg"], device=gpu)
    if bg_aug:
        assert [b["file_name"] for b in ds.bg] == G["single_bgs"].tolist()
    x = torch.cat([ds.inputs([0, 1, 2, 3], EC.S), ds.inputs([4, 5], EC.S)]).cpu().numpy()
    assert np.array_equal(x, G["single%d_images" % bg_aug])
    assert not np.array_equal(G["single0_images"], G["single1_images"])


# ---------------------------------------------------------------------------------------------
# the two scripts against the REFERENCE's four scripts (tests/golden/script_eval_data_{mpaug,mpaug_yolo,kdh3d,kdh3d_yolo}.json)
# ---------------------------------------------------------------------------------------------
REF_SCRIPTS = {"mpaug": ("evaluate_mpaug.py", "rtpose"), "mpaug_yolo": ("evaluate_mpaug.py", "yolo"),
               "kdh3d": ("evaluate_kdh3d.py", "rtpose"), "kdh3d_yolo": ("evaluate_kdh3d.py", "yolo")}


def _script_module(script):
    import importlib.util
    spec = importlib.util.spec_from_file_location(script[:-3], os.path.join(ROOT, "scripts", script))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference_checkpoint(golden, fix, net, path, conf_shift=None):
    """The checkpoint the reference script ran on, from the fixture's recipe (seeded weights + the stored shift)."""
    from helpers import state_dict_from_keys
    if net == "rtpose":
        sd = state_dict_from_keys(golden.keys["rtpose_light3d"], seed=fix["weight_seed"])
        sd["model2_2.12.bias"][:15] += torch.tensor(fix["heat_bias_shift"])
    else:
        sd = state_dict_from_keys(golden.keys["yolo_posenet"], seed=fix["weight_seed"])
        sd["model2_4.0.weight"][[4, 54]] -= np.float32(fix["conf_weight_shift"] if conf_shift is None else conf_shift)
    torch.save({"module." + k: v for k, v in sd.items()}, str(path))
    return str(path)


@pytest.mark.parametrize("name", sorted(REF_SCRIPTS))
def test_scripts_reproduce_the_reference_scripts(gpu, golden, tree, tmp_path, capsys, name):
    """Same tree, same seed, same weights as the reference script's run: the same frames (the loaders' golden), so eval_data.json must hold
    the same persons -- counts, visibilities, the first-person choice ==; the ground truth ==; the raw-depth arm at the ground-truth pixel
    ==; the bars of tests/test_gpu_ablation.py (Open-Pose+: 2D and the raw arm at the predicted joints 1e-9, what reads the pose-depth map
    1e-3 m) and tests/test_gpu_itop.py (Yolo-Pose+: 2D 5e-2 px, 3D 1e-3 m) for the rest; the metric tables within what those bars allow."""
    script, net = REF_SCRIPTS[name]
    fix = json.load(open(os.path.join(ROOT, "tests", "golden", "script_eval_data_%s.json" % name)))
    mod = _script_module(script)
    common = ["--net", net, "--image-dir", tree["img"], "--batch-size", "3", "--input-size", str(EC.S), "--w-org", str(EC.W), "--h-org", str(EC.H),
              "--seed", str(fix["seed"])] + (["--ablation"] if net == "rtpose" else [])
    bg = ["--bg-file", tree["bg_file"], "--bg-dir", tree["bg"], "--seg-dir", tree["seg"]]
    if script == "evaluate_mpaug.py":
        common += ["--annotations"] + tree["ann_files"] + bg + ["--num-batches", "2"]
    else:       # the reference's Open-Pose+ script never swaps the background, its Yolo-Pose+ script does by default
        common += ["--annotations", tree["single_ann"], "--bg-aug", "1" if net == "yolo" else "0"] + (bg if net == "yolo" else [])
    out = mod.main(common + ["--weight", _reference_checkpoint(golden, fix, net, tmp_path / "ref.pth"), "--output-dir", str(tmp_path / "out")])
    capsys.readouterr()
    data = json.load(open(tmp_path / "out" / "eval_data.json"))
    recipe = {"metrics", "weight_seed", "seed", "heat_bias_shift", "conf_weight_shift", "conf_threshold"}
    assert set(data) == set(fix) - recipe
    assert data["human_gt_set_2d"] == fix["human_gt_set_2d"] and data["human_gt_set_3d"] == fix["human_gt_set_3d"]
    assert [len(f) for f in data["human_pred_set_2d"]] == [len(f) for f in fix["human_pred_set_2d"]]
    tol2 = 1e-9 if net == "rtpose" else 5e-2
    for b in range(6):
        g2, w2 = np.array(data["human_pred_set_2d"][b]), np.array(fix["human_pred_set_2d"][b])
        g3, w3 = np.array(data["human_pred_set_3d"][b]), np.array(fix["human_pred_set_3d"][b])
        assert g2.shape == w2.shape and g3.shape == w3.shape
        if g2.size:
            print("%s frame %d: 2D max diff %.3g, 3D max diff %.3g" % (name, b, np.abs(g2 - w2).max(), np.abs(g3 - w3).max()))
            assert np.abs(g2 - w2).max() <= tol2 and np.abs(g3 - w3).max() < 1e-3
        if net == "rtpose":
            assert data["visibility_pred_set"][b] == fix["visibility_pred_set"][b]
            assert data["human_gt_set_2d_visible"][b] == fix["human_gt_set_2d_visible"][b]
            got, want = ({k: np.array(src[k][b]).reshape(-1, 15, 3) for k in ARMS} for src in (data, fix))
            assert all(got[k].shape == want[k].shape for k in ARMS)
            assert np.array_equal(got[ARMS[2]], want[ARMS[2]])
            assert got[ARMS[0]].size == 0 or np.abs(got[ARMS[0]] - want[ARMS[0]]).max() <= 1e-9
            assert np.abs(got[ARMS[1]] - want[ARMS[1]]).max() < 1e-3
    # The metric tables.  What depends only on 2D and on raw depth is held to the bars above; a mean of 3D joint distances that reads the
    # pose-depth map (Open-Pose+) or the prior pose (Yolo-Pose+) inherits 1e-3 m in depth, at most sqrt(3) * 1e-3 m per joint (|x - cx| / fx
    # and |y - cy| / fy stay below 1 on this frame): 2e-3, as in tests/test_gpu_ablation.py; the PCK counts must still agree.
    assert set(out) == set(fix["metrics"])
    for k, want in fix["metrics"].items():
        got, want = np.asarray(out[k], dtype=np.float64), np.asarray(want, dtype=np.float64)
        exact = net == "rtpose" and (k.endswith("2d") and not k.startswith(("pck3d", "err3d")) or "raw" in k)
        tol = 0.0 if k.startswith("pck") or k == "dist_th_2d" else (1e-9 if exact else (5e-2 if k == "err2d" else 2e-3))
        assert got.shape == want.shape and np.all((np.abs(got - want) <= tol) | (np.isnan(got) & np.isnan(want))), (k, got, want)
    if net == "yolo":
        # A frame without a detection.  The reference scripts build their -1 placeholder person and then raise on the empty box list, so no
        # fixture holds such a frame; a confidence shift nobody passes shows the rows the drop-ins write: the restated placeholder, per frame.
        ck = _reference_checkpoint(golden, fix, net, tmp_path / "empty.pth", conf_shift=0.02)
        mod.main(common + ["--weight", ck, "--output-dir", str(tmp_path / "empty"), "--no-metrics"])
        capsys.readouterr()
        empty = json.load(open(tmp_path / "empty" / "eval_data.json"))
        hold2, hold3 = ER.yolo_lists([], EC.W, EC.H, EC.S, EC.INTRINSICS)
        assert empty["human_pred_set_2d"] == [hold2] * 6 and empty["human_pred_set_3d"] == [hold3] * 6
