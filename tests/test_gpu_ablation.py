"""GPU: the depth-ablation arms (pn_ablation_pred_raw, pn_ablation_perfect_2d, pn_depth_probe; csrc/ablation.hip) against
tests/ablation_reference.py, the numpy restatement of evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py:197-299 that
tests/test_ablation_reference.py pins to the reference script's own output.

Kernel checks run on hand-built frames, records and ground truth and compare float64 with ==: the arms are read-outs (one
float32 pixel or map cell, un-normalised in float32, back-projected in float64), so there is nothing to tolerate.  The
end-to-end checks run the fp32 parity engine on the reference script's fixture; only the arm that reads the network's
pose-depth map inherits the forward's 1e-3 m."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import ablation_reference as AR
import parse_cases as PC
import popnet_amd  # noqa: F401
from helpers import state_dict_from_keys
from oracle import preproc
from popnet_amd import _lib, synth
from popnet_amd.utils.paf_to_pose import make_parse_cfg, parse_paf_unbounded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "script_eval_data_ablation.json")))
ARMS = ("human_pred_set_3d_read_raw_depth", "human_pred_set_3d_perfect_2d", "human_pred_set_3d_perfect_2d_read_raw_depth")
TEN_KEYS = set(ARMS) | {"human_pred_set_2d", "human_pred_set_3d", "human_pred_set_visibility", "human_pred_set_part_conf", "human_gt_set_2d",
                        "human_gt_set_2d_visible", "human_gt_set_3d"}
S, B, DMAX, MEAN, STD = 16, 3, 6.0, 3.0, 2.0                 # MEAN, STD: the reference's normalisation
J, P = _lib.PN_NUM_JOINTS, _lib.PN_MAX_PERSONS
# (frame dtype, H, W, depth_mean, depth_std): 20x12 shrinks to 16x16 in y and grows in x, 10x7 grows in both; the original-frame size of the
# rescale is the frame's.  float16 values times the eighths that are 20x12's weights are exact products, so only the float32 frames can show
# a contracted multiply-add in the mix; they also get a normalisation whose `* std + mean` is not exact (2 and 3 make it so).
SHAPES = {"f16_20x12": (np.float16, 20, 12, MEAN, STD), "f32_10x7": (np.float32, 10, 7, 2.9, 1.7)}


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _dt(frames):
    return _lib.PN_DEPTH_F16 if frames.dtype == torch.float16 else _lib.PN_DEPTH_F32


def _ctx(gpu):
    return _lib.Context.for_device(gpu.index), _lib.lib(), _lib.current_stream_ptr(gpu)


def _intr(cfg):
    return {"fx": cfg.fx, "fy": cfg.fy, "cx": cfg.cx, "cy": cfg.cy}


def _bilinear(frame, size, fma, mean=MEAN, std=STD):
    """The float32 bilinear mix of pn_preprocess (OpenCV's float path: horizontal pass, then vertical, products summed left to right),
    with every a * b + c contracted to one rounding when fma: what the kernel would give if the compiler fused it."""
    H, W = frame.shape
    f = frame.astype(np.float32)
    f32 = lambda a: np.asarray(a).astype(np.float32)

    def axis(N):
        c = f32((np.arange(size) + 0.5) * (1.0 / (size / N)) - 0.5)
        s = np.floor(c).astype(np.int64)
        return s, f32(c - f32(s))

    def mix(v0, w0, v1, w1):
        if fma:
            return f32(v1.astype(np.float64) * w1.astype(np.float64) + f32(v0 * w0).astype(np.float64))
        return f32(f32(v0 * w0) + f32(v1 * w1))

    sx, fx = axis(W)
    sy, fy = axis(H)
    fx[sx < 0] = 0
    fx[sx >= W - 1] = 0
    sx = np.clip(sx, 0, W - 1)
    x1 = np.minimum(sx + 1, W - 1)
    y0, y1 = np.clip(sy, 0, H - 1), np.clip(sy + 1, 0, H - 1)
    one = np.float32(1)
    a0, a1 = np.broadcast_to(f32(one - fx), (size, size)), np.broadcast_to(fx, (size, size))
    h0 = mix(f[y0][:, sx], a0, f[y0][:, x1], a1)
    h1 = mix(f[y1][:, sx], a0, f[y1][:, x1], a1)
    b0, b1 = np.broadcast_to(f32(one - fy)[:, None], (size, size)), np.broadcast_to(fy[:, None], (size, size))
    v = np.clip(mix(h0, b0, h1, b1), np.float32(0), np.float32(DMAX))
    return f32(f32(v - np.float32(mean)) / np.float32(std))


@pytest.fixture(scope="module", params=sorted(SHAPES))
def hand(request, gpu):
    """Hand-built frames, records, maps and ground truth of one shape, uploaded once, with the restatement's inputs next to them."""
    dtype, H, W, mean, std = SHAPES[request.param]
    rng = np.random.default_rng(41 if dtype == np.float16 else 42)
    frames = (rng.normal(2.0, 3.0, (B, H, W))).astype(dtype)             # negative values and values above depth_max = 6 among them
    frames[0, 0, 0], frames[0, -1, -1], frames[2, 0, -1] = -4.0, 9.5, 6.0
    x_norm = np.stack([preproc.preprocess_frame(f, input_size=S, depth_mean=mean, depth_std=std)[0] for f in frames])          # the oracle's pixels
    cfg = make_parse_cfg(input_size=S, w_org=W, h_org=H, depth_mean=mean, depth_std=std)
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
    recs[1]["n_persons"] = P                                                  # a full record
    recs[1]["person_joint"][0] = -1                                           # a person with every joint missing
    recs[1]["person_joint"][1, :2] = (0, 1)
    recs[1]["person_joint"][2:][rng.random((P - 2, J)) < 0.3] = -1
    recs[2]["n_persons"] = 3
    recs[2]["status"] = _lib.PN_FRAME_OVERFLOW_PEAKS                          # an overflowing record: its persons are computed all the same
    recs[2]["person_joint"][1, ::2] = -1
    for b in range(B):                                                        # joints_2d as group_readout_kernel leaves it
        r = recs[b]
        ids = r["person_joint"]
        vis = ids >= 0
        x, y = r["peak_x"][np.maximum(ids, 0)].astype(np.float64), r["peak_y"][np.maximum(ids, 0)].astype(np.float64)
        r["joints_2d"][..., 0] = np.where(vis, x / S * W, -1.0)
        r["joints_2d"][..., 1] = np.where(vis, y / S * H, -1.0)

    # ground truth: count 0, count Gmax, one person; negative, on and past the frame's edge, one ulp below a pixel / cell boundary, integers
    G = 3
    edge = [[-2.5, -0.25], [float(W), float(H)], [W + 1.5, H + 7.0], [0, 0], [W - 1, H - 1], [W, 3], [np.nextafter(W / 2, 0), np.nextafter(H / 2, 0)],
            [W / 2, H / 2], [np.nextafter(5 * W / S, 0), np.nextafter(11 * H / S, 0)], [5 * W / S, 11 * H / S], [-1e9, 1e9], [W - 1e-9, H - 1e-9],
            [3, 7], [0.999 * W / S, 0.999 * H / S], [W / 2 + 0.01, H / 2 - 0.01]]
    gt = [[], [edge, rng.uniform([-2, -2], [W + 2, H + 2], (J, 2)).tolist(), rng.integers(0, W + 1, (J, 2)).tolist()],
          [rng.uniform([0, 0], [W, H], (J, 2)).tolist()]]
    gt_arr = np.full((B, G, J, 2), 123.0)                                     # rows past a frame's count hold values too
    for b, g in enumerate(gt):
        for i, h in enumerate(g):
            gt_arr[b, i] = np.asarray(h, dtype=np.float64)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return dict(name=request.param, H=H, W=W, mean=mean, std=std, frames=frames, x_norm=x_norm, cfg=cfg, z=z, recs=recs, gt=gt, G=G,
                d_frames=to(frames), d_z=to(z), d_recs=to(recs.view(np.uint8).reshape(B, -1)), d_gt=to(gt_arr),
                d_cnt=to(np.array([len(g) for g in gt], np.int32)))


def test_hand_built_frames_are_fma_sensitive(hand):
    """The restated mix equals the oracle's pixels, and contracting its multiply-adds changes some: frames on which a fused kernel shows."""
    plain = np.stack([_bilinear(f, S, False, hand["mean"], hand["std"]) for f in hand["frames"]])
    fused = np.stack([_bilinear(f, S, True, hand["mean"], hand["std"]) for f in hand["frames"]])
    assert np.array_equal(plain, hand["x_norm"])
    if hand["frames"].dtype == np.float32:
        assert np.count_nonzero(plain != fused) > 20
        x = hand["x_norm"].astype(np.float64)                                          # ... and so does the un-normalisation
        two = AR.unnormalise(hand["x_norm"], hand["mean"], hand["std"])
        assert np.count_nonzero(two != (x * np.float64(np.float32(hand["std"])) + np.float64(np.float32(hand["mean"]))).astype(np.float32)) > 20
    raw = hand["frames"].astype(np.float32)
    assert (raw < 0).any() and (raw > DMAX).any()


def test_depth_probe_equals_preprocess_output_bit_for_bit(hand, gpu):
    ctx, L, st = _ctx(gpu)
    fr = hand["d_frames"]
    MEAN, STD = hand["mean"], hand["std"]
    x = torch.empty((B, 1, S, S), device=gpu, dtype=torch.float32)
    ctx.check(L.pn_preprocess(ctx.handle, _vp(fr), _dt(fr), B, hand["H"], hand["W"], _vp(x), S, DMAX, MEAN, STD, st), "pn_preprocess")
    want = AR.unnormalise(x.cpu().numpy()[:, 0], MEAN, STD)
    assert np.array_equal(want, AR.unnormalise(hand["x_norm"], MEAN, STD))           # (and pn_preprocess equals the oracle here)
    yy, xx = np.mgrid[0:S, 0:S]
    # every pixel of every frame in one call (3 x 256 points: three blocks), last frame first
    pts = np.concatenate([np.stack([np.full(S * S, b), yy.ravel(), xx.ravel()], 1) for b in (2, 1, 0)]).astype(np.int32)
    out = torch.full((len(pts),), float("nan"), device=gpu)
    ctx.check(L.pn_depth_probe(ctx.handle, _vp(fr), _dt(fr), B, hand["H"], hand["W"], S, DMAX, MEAN, STD, _vp(torch.from_numpy(pts).to(gpu)), len(pts),
                               _vp(out), st), "pn_depth_probe")
    assert np.array_equal(out.cpu().numpy().reshape(3, S, S), want[::-1])
    out = torch.full((2,), 7.0, device=gpu)
    for bad in ((0, S, 0), (0, 0, S), (0, -1, 0), (0, 0, -1), (B, 0, 0), (-1, 0, 0)):
        pts = torch.tensor([[0, 0, 0], list(bad)], dtype=torch.int32, device=gpu)
        rc = L.pn_depth_probe(ctx.handle, _vp(fr), _dt(fr), B, hand["H"], hand["W"], S, DMAX, MEAN, STD, _vp(pts), 2, _vp(out), st)
        assert rc == -1 and "outside" in ctx.last_error(), bad                         # PN_ERR_INVALID, not a clamp
    assert out.cpu().tolist() == [7.0, 7.0]                                            # and nothing was launched
    assert L.pn_depth_probe(ctx.handle, _vp(fr), _dt(fr), B, hand["H"], hand["W"], S, DMAX, MEAN, STD, None, 0, None, st) == 0


def test_pred_raw_equals_restatement(hand, gpu):
    ctx, L, st = _ctx(gpu)
    fr, cfg = hand["d_frames"], hand["cfg"]
    out = torch.full((B, P, J, 3), float("nan"), device=gpu, dtype=torch.float64)
    ctx.check(L.pn_ablation_pred_raw(ctx.handle, _vp(fr), _dt(fr), B, hand["H"], hand["W"], DMAX, C.byref(cfg), _vp(hand["d_recs"]), _vp(out), st),
              "pn_ablation_pred_raw")
    got = out.cpu().numpy()
    seen_missing = seen_corner = 0
    for b in range(B):
        r = hand["recs"][b]
        n = int(r["n_persons"])
        img = AR.unnormalise(hand["x_norm"][b], hand["mean"], hand["std"])
        want = AR.pred_raw(img, np.stack([r["peak_x"], r["peak_y"]], 1), r["person_joint"][:n], hand["W"], hand["H"], S, _intr(cfg))
        assert np.array_equal(got[b, :n], want), (hand["name"], b)
        assert np.all(got[b, n:] == 0.0)                                               # zero-filled, whatever the rows hold
        miss = r["person_joint"][:n] < 0
        seen_missing += int(miss.sum())
        assert np.all(got[b, :n][miss][:, 2] == -1.0)
        seen_corner += int(np.isin(r["person_joint"][:n], (0, 1)).sum())
    assert seen_missing > J and seen_corner >= 2
    assert np.array_equal(got[1, 0], AR.back_project(np.full((J, 2), -1.0), np.full(J, -1.0), _intr(cfg)))      # every joint missing


def test_perfect_2d_equals_restatement(hand, gpu):
    ctx, L, st = _ctx(gpu)
    fr, cfg, G = hand["d_frames"], hand["cfg"], hand["G"]
    om = torch.full((B, G, J, 3), float("nan"), device=gpu, dtype=torch.float64)
    orw = torch.full((B, G, J, 3), float("nan"), device=gpu, dtype=torch.float64)
    args = (ctx.handle, _vp(fr), _dt(fr), B, hand["H"], hand["W"], DMAX, _vp(hand["d_z"]), S // 8, S // 8, C.byref(cfg), _vp(hand["d_gt"]),
            _vp(hand["d_cnt"]))
    ctx.check(L.pn_ablation_perfect_2d(*args, G, _vp(om), _vp(orw), st), "pn_ablation_perfect_2d")
    gm, gr = om.cpu().numpy(), orw.cpu().numpy()
    for b in range(B):
        g = hand["gt"][b]
        img = AR.unnormalise(hand["x_norm"][b], hand["mean"], hand["std"])
        wm, wr = AR.perfect_2d(img, hand["z"][b], g, hand["W"], hand["H"], S, 8, hand["mean"], hand["std"], _intr(cfg))
        assert np.array_equal(gm[b, :len(g)], wm) and np.array_equal(gr[b, :len(g)], wr), (hand["name"], b)
        assert np.all(gm[b, len(g):] == 0.0) and np.all(gr[b, len(g):] == 0.0)
    # more ground-truth persons than one block holds rows for (20 x 15 > 256), counts 20 / 0 / 7
    G2, counts = 20, (20, 0, 7)
    rng = np.random.default_rng(7)
    gt2 = rng.uniform([-3, -3], [hand["W"] + 3, hand["H"] + 3], (B, G2, J, 2))
    om2, or2 = (torch.full((B, G2, J, 3), float("nan"), device=gpu, dtype=torch.float64) for _ in range(2))
    d_gt2, d_cnt2 = torch.from_numpy(gt2).to(gpu), torch.tensor(counts, dtype=torch.int32, device=gpu)
    ctx.check(L.pn_ablation_perfect_2d(*args[:11], _vp(d_gt2), _vp(d_cnt2), G2, _vp(om2), _vp(or2), st), "pn_ablation_perfect_2d")
    gm2, gr2 = om2.cpu().numpy(), or2.cpu().numpy()
    for b, n in enumerate(counts):
        img = AR.unnormalise(hand["x_norm"][b], hand["mean"], hand["std"])
        wm, wr = AR.perfect_2d(img, hand["z"][b], gt2[b, :n].tolist(), hand["W"], hand["H"], S, 8, hand["mean"], hand["std"], _intr(cfg))
        assert np.array_equal(gm2[b, :n], wm) and np.array_equal(gr2[b, :n], wr)
        assert np.all(gm2[b, n:] == 0.0) and np.all(gr2[b, n:] == 0.0)
    # Gmax = 0 and B = 0: nothing to do, nothing written
    before = om.clone()
    assert L.pn_ablation_perfect_2d(*args, 0, _vp(om), _vp(orw), st) == 0
    args0 = args[:3] + (0,) + args[4:]
    assert L.pn_ablation_perfect_2d(*args0, G, _vp(om), _vp(orw), st) == 0
    assert torch.equal(om, before)
    # a map that is not input_size / downsample on a side
    bad = args[:8] + (S // 8 + 1,) + args[9:]
    assert L.pn_ablation_perfect_2d(*bad, G, _vp(om), _vp(orw), st) == -1


def test_exact_2x_decimation_is_refused_by_all_three_entries(gpu):
    """32x32 -> 16: cv2.resize(INTER_LINEAR) runs INTER_AREA there; pn_preprocess refuses it and so must every pixel read."""
    ctx, L, st = _ctx(gpu)
    fr = torch.ones((1, 32, 32), device=gpu, dtype=torch.float32)
    cfg = make_parse_cfg(input_size=S, w_org=32, h_org=32)
    x = torch.empty((1, 1, S, S), device=gpu)
    want = L.pn_preprocess(ctx.handle, _vp(fr), _lib.PN_DEPTH_F32, 1, 32, 32, _vp(x), S, DMAX, MEAN, STD, st)
    assert want == -4
    recs = torch.zeros((1, _lib.POSE_FRAME_DTYPE.itemsize), dtype=torch.uint8, device=gpu)
    out = torch.full((1, P, J, 3), 5.0, device=gpu, dtype=torch.float64)
    z = torch.zeros((1, 15, 2, 2), device=gpu)
    gt, cnt = torch.zeros((1, 1, J, 2), device=gpu, dtype=torch.float64), torch.ones((1,), dtype=torch.int32, device=gpu)
    pts, po = torch.zeros((1, 3), dtype=torch.int32, device=gpu), torch.full((1,), 5.0, device=gpu)
    rcs = [L.pn_ablation_pred_raw(ctx.handle, _vp(fr), _lib.PN_DEPTH_F32, 1, 32, 32, DMAX, C.byref(cfg), _vp(recs), _vp(out), st),
           L.pn_ablation_perfect_2d(ctx.handle, _vp(fr), _lib.PN_DEPTH_F32, 1, 32, 32, DMAX, _vp(z), 2, 2, C.byref(cfg), _vp(gt), _vp(cnt), 1,
                                    _vp(out), _vp(out), st),
           L.pn_depth_probe(ctx.handle, _vp(fr), _lib.PN_DEPTH_F32, 1, 32, 32, S, DMAX, MEAN, STD, _vp(pts), 1, _vp(po), st)]
    assert rcs == [want] * 3 and "exact 2x decimation" in ctx.last_error()
    assert bool((out == 5.0).all()) and po.item() == 5.0


# ---------------------------------------------------------------------------------------------
# end to end: the engine and the script on the reference script's fixture (fp32 parity mode)
# ---------------------------------------------------------------------------------------------
def _fixture_gt():
    lab = FIX["labels"]
    return [[p["2d_joints"] for p in lab[k]] for k in lab if k != "intrinsics"]


def _fixture_sd(golden):
    sd = state_dict_from_keys(golden.keys["rtpose_light3d"], seed=FIX["weight_seed"])
    sd["model2_2.12.bias"][:15] += torch.tensor(FIX["heat_bias_shift"])
    return sd


def _check_against_fixture(data):
    """Assignment and visibility exact; the raw arm at the ground-truth pixel ==; the raw arm at the predicted joints within 1e-9 (its 2D
    factor is the float64 rescale both sides compute, its depth one float32 pixel); the map arm within the project's 1e-3 m."""
    assert data["human_gt_set_2d_visible"] == FIX["human_gt_set_2d_visible"]
    for b in range(2):
        assert data["human_pred_set_visibility"][b] == FIX["human_pred_set_visibility"][b]
        got = {k: np.array(data[k][b]) for k in ARMS}
        want = {k: np.array(FIX[k][b]) for k in ARMS}
        for k in ARMS:
            assert got[k].shape == want[k].shape, k
        assert np.array_equal(got[ARMS[2]], want[ARMS[2]])
        print("frame %d: read_raw_depth max diff %.3g, perfect_2d max diff %.3g" % (b, np.abs(got[ARMS[0]] - want[ARMS[0]]).max(),
                                                                                    np.abs(got[ARMS[1]] - want[ARMS[1]]).max()))
        assert np.abs(got[ARMS[0]] - want[ARMS[0]]).max() <= 1e-9
        assert np.abs(got[ARMS[1]] - want[ARMS[1]]).max() < 1e-3


def test_engine_fp32_reproduces_the_reference_script(gpu, golden):
    from popnet_amd.pipeline import PoseEngine, records_to_numpy
    eng = PoseEngine(precision="fp32", state_dict=_fixture_sd(golden), device=gpu, max_batch=2, intrinsics=FIX["labels"]["intrinsics"])
    depth = torch.from_numpy(synth.synth_depth(2, 640, 480, seed=FIX["depth_seed"])).to(gpu)
    gt = _fixture_gt()
    recs, raw, pm, pr = eng.predict_ablation(depth, gt)
    assert raw.shape == (2, P, J, 3) and pm.shape == pr.shape == (2, 3, J, 3) and raw.dtype == pm.dtype == torch.float64
    lists = eng.ablation_lists(depth, gt, records_to_numpy(recs), raw, pm, pr)
    _check_against_fixture(lists)
    # the streaming sweep does not carry the arms
    from popnet_amd import dataset
    with pytest.raises(_lib.PopnetError, match="streaming"):
        dataset.run_sweep_streaming(None, [], ablation=True)


def test_evaluate_mpreal_script_with_ablation(gpu, golden, tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("evaluate_mpreal", os.path.join(ROOT, "scripts", "evaluate_mpreal.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.save({"module." + k: v for k, v in _fixture_sd(golden).items()}, tmp_path / "ckpt.pth")
    img_dir = tmp_path / "depth_maps"
    img_dir.mkdir()
    frames = synth.synth_depth(2, 640, 480, seed=FIX["depth_seed"])
    for i in range(2):
        np.save(img_dir / ("f%d.npy" % i), frames[i])
    json.dump(FIX["labels"], open(tmp_path / "labels.json", "w"))
    base = ["--annotations", str(tmp_path / "labels.json"), "--image-dir", str(img_dir), "--w-org", "480", "--h-org", "640", "--batch-size", "2",
            "--weight", str(tmp_path / "ckpt.pth"), "--output-dir", str(tmp_path / "out")]
    with pytest.raises(SystemExit):                                                     # argparse error: the Yolo script has no such keys
        mod.main(base + ["--net", "yolo", "--ablation"])
    capsys.readouterr()
    out = mod.main(base + ["--ablation", "--pipeline", "1"])
    assert "sequential sweep" in capsys.readouterr().out
    data = json.load(open(tmp_path / "out" / "eval_data.json"))
    assert set(data) == TEN_KEYS
    _check_against_fixture(data)
    # The five blocks.  Three of them score a raw-depth arm, which the checks above hold to 1e-9 of the reference's: equal.  The two that
    # score the pose-depth map arm inherit the forward's 1e-3 m in depth, i.e. at most sqrt(3) * 1e-3 m per joint in 3D (|x - cx| / fx and
    # |y - cy| / fy stay below 1 on this frame size), hence in a mean of joint distances: 2e-3 m; their PCK counts must still agree.
    for k, want in FIX["metrics"].items():
        got, want = np.asarray(out[k], dtype=np.float64), np.asarray(want, dtype=np.float64)
        tol = 2e-3 if (k.startswith("err3d_perfect_2d")) else 1e-9
        assert got.shape == want.shape and np.all((np.abs(got - want) <= tol) | (np.isnan(got) & np.isnan(want))), k
    assert len(out["pck3d"]) == 15 and len(out["ap2d"]) == 16                           # the four usual blocks are still there


# ---------------------------------------------------------------------------------------------
# engine consistency in throughput mode, and the overflow second pass
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bf16_engine(gpu):
    from popnet_amd.pipeline import PoseEngine
    return PoseEngine(precision="bf16", device=gpu, max_batch=4)


def _engine_x(eng, depth):
    """The normalised S x S input of `depth` as the engine's own pn_preprocess writes it (bf16 forwards never do)."""
    n = eng.preprocess(depth)
    return eng.x[:n, 0].cpu().numpy()


def test_bf16_engine_arms_equal_restatement_on_its_own_maps(gpu, bf16_engine):
    """Whatever bf16 does to the maps, the read-out stays exact: every arm == the restatement on the engine's own z, records and frames."""
    from popnet_amd.pipeline import records_to_numpy
    eng = bf16_engine
    depth = torch.from_numpy(synth.synth_depth(4, 640, 480, seed=13)).to(gpu)
    rng = np.random.default_rng(3)
    gt = [rng.uniform([-20, -20], [500, 660], (n, J, 2)).tolist() for n in (2, 0, 1, 3)]
    recs, raw, pm, pr = eng.predict_ablation(depth, gt)
    recs, raw, pm, pr = records_to_numpy(recs).copy(), raw.cpu().numpy(), pm.cpu().numpy(), pr.cpu().numpy()
    z = eng.z[:4].cpu().numpy()
    x = _engine_x(eng, depth)
    assert int(recs["n_persons"].sum()) > 0 and not recs["status"].any()
    for b in range(4):
        r = recs[b]
        n, g = int(r["n_persons"]), len(gt[b])
        want = AR.ablation_reference(x[b], (None, None, z[b]), (np.stack([r["peak_x"], r["peak_y"]], 1), r["person_joint"][:n]), gt[b],
                                     intrinsics=_intr(eng.cfg))
        assert np.array_equal(raw[b, :n], want[ARMS[0]]) and np.all(raw[b, n:] == 0.0)
        assert np.array_equal(pm[b, :g], want[ARMS[1]]) and np.array_equal(pr[b, :g], want[ARMS[2]])
        assert np.all(pm[b, g:] == 0.0) and np.all(pr[b, g:] == 0.0)


def test_overflowing_frame_takes_the_second_pass(gpu, bf16_engine):
    """A frame whose record overflows (33 peaks in one joint map) is parsed again without capacities; its raw arm comes from
    pn_depth_probe + the float64 back-projection and must equal the restatement on the unbounded parse."""
    from popnet_amd.pipeline import records_to_numpy
    eng = bf16_engine
    c = PC.case("peaks33")
    assert c.shape == (28, 28)
    for name in ("heat", "paf", "z"):
        getattr(eng, name)[0].copy_(torch.from_numpy(np.ascontiguousarray(getattr(c, name).transpose(2, 0, 1))))
    eng.parse(1)
    recs = eng.frames[:1]
    depth = torch.from_numpy(synth.synth_depth(1, 640, 480, seed=14)).to(gpu)
    gt = [np.random.default_rng(4).uniform(0, 480, (2, J, 2)).tolist()]
    raw, pm, pr = eng.ablation_arms(depth, recs, gt)
    host = records_to_numpy(recs)
    assert int(host[0]["status"]) == _lib.PN_FRAME_OVERFLOW_PEAKS
    lists = eng.ablation_lists(depth, gt, host, raw, pm, pr)
    ub = parse_paf_unbounded(eng.heat[0], eng.paf[0], eng.z[0], eng.cfg)
    assert len(ub["person_joint"]) > 0 and (ub["person_joint"] >= 0).any() and len(ub["joint_list"]) > int(host[0]["n_peaks"])
    img = AR.unnormalise(_engine_x(eng, depth)[0], 3.0, 2.0)
    want = AR.pred_raw(img, ub["joint_list"], ub["person_joint"], 480, 640, 224, _intr(eng.cfg))
    assert lists[ARMS[0]][0] == want.tolist()
    assert lists["human_pred_set_3d"][0] == ub["joints_3d"].tolist() and len(lists[ARMS[1]][0]) == 2
    # without the second pass the frame is refused, never truncated
    from popnet_amd import dataset
    with pytest.raises(_lib.PopnetError, match="overflow"):
        dataset.pose_records_to_lists(host, ablation={"pred_raw": raw.cpu().numpy(), "perfect_map": pm.cpu().numpy(), "perfect_raw": pr.cpu().numpy(),
                                                      "gt_2d": gt})
