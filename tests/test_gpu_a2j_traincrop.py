"""A2J's crop-level training augmentation on the GPU: pn_a2j_train_crop against the reference's own crops
(tests/golden/a2j_traincrop.npz: dataPreprocess + transform of itop_train_64.py, train_a2j_base.py and train_a2j_bgaug_new.py, made by
tests/golden/make_golden_a2j_traincrop.py), its refusals, A2JEngine.train_crops + votes against the module, and the three scripts on a fake
dataset tree.  The item records come from popnet_amd.a2j_crops, which tests/test_a2j_traincrop_reference.py pins on the CPU."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2j_cases as AC  # noqa: E402
import a2j_traincrop_cases as TC  # noqa: E402
from popnet_amd import _lib, a2j_crops as AJ  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PN_ERR_INVALID = -1


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "a2j_traincrop.npz"))


_ENGINES = {}


@pytest.fixture(scope="module")
def engine(gpu):
    """One A2JEngine per crop size (its crops need no compiled net); mean / std are set per call."""
    def get(cw, ch, mean, std):
        from popnet_amd.pipeline import A2JEngine
        if (cw, ch) not in _ENGINES:
            _ENGINES[(cw, ch)] = A2JEngine(precision="fp32", device=gpu, max_batch=2, crop=(ch, cw))
        eng = _ENGINES[(cw, ch)]
        eng.cfg.mean, eng.cfg.std = mean, std
        return eng
    yield get
    _ENGINES.clear()


def itop_group(g, idx):
    """The records of several ITOP cases as one array: one launch.  Each case's record is built as the CPU test builds it."""
    rec = (_lib.A2JCropItem * len(idx))()
    for k, i in enumerate(idx):
        name, fset, fi, lt, rb, c, draws, (cw, ch) = TC.ITOP_CASES[i]
        rec[k] = AJ.itop_items([i], TC.itop_centres(), g["itop_lefttop"], g["itop_rightbottom"], TC.itop_keypoints(), TC.SETS[fset],
                               draws=None if draws is None else [TC.draws_of(draws)], crop_w=cw, crop_h=ch, frames=[fi])[0][0]
    return rec


def box_group(idx):
    bnd, k2, k3 = TC.box_arrays()
    rec = (_lib.A2JCropItem * len(idx))()
    for k, i in enumerate(idx):
        name, fi, box, draws, (cw, ch) = TC.BOX_CASES[i]
        rec[k] = AJ.box_items([i], bnd, k2, k3, TC.SETS["b"], draws=None if draws is None else [TC.draws_of(draws)], crop_w=cw, crop_h=ch,
                              img_wh=TC.IMG_WH_B, frames=[fi])[0][0]
    return rec


def golden_rows(g, form, cases, idx):
    large = [k for k, c in enumerate(cases) if c[-1][0] == TC.LARGE]
    small = [k for k in range(len(cases)) if k not in large]
    return np.stack([g[form + "_crops_large"][large.index(i)] if i in large else g[form + "_crops"][small.index(i)] for i in idx])


def same_bits(got, want, names):
    """int32 equality; where the golden is NaN the result must be NaN (the payload is not compared).  -> NaN count per row"""
    counts = []
    for a, b, name in zip(got, want, names):
        nan = np.isnan(b)
        assert np.isnan(a[nan]).all(), "%s: a NaN of the reference is a number here" % name
        ai, bi = a.view(np.int32), b.view(np.int32)
        assert np.array_equal(ai[~nan], bi[~nan]), "%s: %d pixels differ" % (name, int((ai[~nan] != bi[~nan]).sum()))
        counts.append(int(np.isnan(a).sum()))
    return counts


ITOP_GROUPS = {}
for _i, _c in enumerate(TC.ITOP_CASES):
    ITOP_GROUPS.setdefault((_c[1], _c[7]), []).append(_i)
BOX_GROUPS = {}
for _i, _c in enumerate(TC.BOX_CASES):
    BOX_GROUPS.setdefault(_c[4], []).append(_i)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_itop_crops_equal_the_reference_bit_for_bit(gpu, g, engine, dtype):
    seen = []
    for (fset, (cw, ch)), idx in ITOP_GROUPS.items():
        frames = torch.from_numpy(TC.frames(fset)).to(gpu).to(dtype)
        crops, flags = engine(cw, ch, TC.ITOP_MEAN, TC.ITOP_STD).train_crops(frames, itop_group(g, idx))
        torch.cuda.synchronize()
        names = [TC.ITOP_CASES[i][0] for i in idx]
        nans = same_bits(crops.cpu().numpy()[:, 0], golden_rows(g, "itop", TC.ITOP_CASES, idx), names)
        assert nans == [int(g["itop_nan_count"][i]) for i in idx]
        assert flags.cpu().tolist() == [int(g["itop_flags"][i]) for i in idx]
        assert all(not crops[k].any() for k, i in enumerate(idx) if g["itop_flags"][i])
        seen += idx
    assert sorted(seen) == list(range(len(TC.ITOP_CASES)))                                   # no case is left out
    assert int(g["itop_nan_count"].sum()) > 0 and int(g["itop_flags"].sum()) == 1


@pytest.mark.parametrize("swap", [False, True], ids=["base", "bgaug"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_box_crops_equal_the_reference_bit_for_bit(gpu, g, engine, dtype, swap):
    from popnet_amd import targets
    fg = torch.from_numpy(TC.frames("b")).to(gpu).to(dtype)
    if swap:      # the background swap of train_a2j_bgaug_new.py, through the existing pn_compose_bg path
        mask, bg = TC.masks_and_backgrounds("b")
        frames = targets.compose_bg(fg, torch.from_numpy(mask).to(gpu), torch.from_numpy(bg).to(gpu).to(dtype))
    else:
        frames = fg
    tag, seen = ("bg" if swap else "box"), []
    for (cw, ch), idx in BOX_GROUPS.items():
        if swap and cw == TC.LARGE:      # stored for the base form only
            continue
        crops, flags = engine(cw, ch, 3.0, 2.0).train_crops(frames, box_group(idx))
        torch.cuda.synchronize()
        nans = same_bits(crops.cpu().numpy()[:, 0], golden_rows(g, tag, TC.BOX_CASES, idx), [TC.BOX_CASES[i][0] for i in idx])
        assert not any(nans) and flags.cpu().tolist() == [int(g[tag + "_flags"][i]) for i in idx]
        seen += idx
    assert sorted(seen) == [i for i, c in enumerate(TC.BOX_CASES) if not (swap and c[4][0] == TC.LARGE)]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _call(gpu, items, n, cfg, frames, out, F=None):
    L, ctx = _lib.lib(), _lib.Context.for_device(0)
    items_dev = torch.empty((max(len(items), 1) * C.sizeof(_lib.A2JCropItem),), device=gpu, dtype=torch.uint8)
    flags = torch.zeros((max(len(items), 1),), device=gpu, dtype=torch.int32)
    rc = L.pn_a2j_train_crop(ctx.handle, C.c_void_p(frames.data_ptr()), _lib.PN_DEPTH_F16, frames.shape[0] if F is None else F, frames.shape[1], frames.shape[2],
                             C.cast(items, C.c_void_p), C.c_void_p(items_dev.data_ptr()), n, C.byref(cfg), C.c_void_p(out.data_ptr()),
                             C.c_void_p(flags.data_ptr()), _lib.current_stream_ptr(gpu))
    torch.cuda.synchronize()
    return rc, ctx.last_error()


def _good_item(g):
    return itop_group(g, [0])


def _edit(field, value):
    def f(it, cfg):
        if field.startswith("m["):
            it.m[int(field[2])] = value
        else:
            setattr(it, field, value)
    return f


def _cfg_edit(field, value):
    return lambda it, cfg: setattr(cfg, field, value)


REFUSALS = [
    ("region_past_the_frame", _edit("ih", 30)),
    ("column_start_negative", _edit("cx0", -1)),
    ("unpadded_size_mismatch", _edit("sw", 7)),
    ("frame_index", _edit("frame", 3)),
    ("padded_flag", _edit("padded", 2)),
    ("matrix_nan", _edit("m[2]", float("nan"))),
    ("matrix_inf", _edit("m[0]", float("inf"))),
    ("matrix_scale_past_64", _edit("m[0]", 64.5)),
    ("matrix_shift_past_2_19", _edit("m[5]", -524289.0)),
    ("window_hi_inf", _edit("hi", float("inf"))),
    ("window_scale_nan", _edit("scale", float("nan"))),
    ("crop_over_4096", _cfg_edit("crop_w", 4097)),
    ("std_zero", _cfg_edit("std", 0.0)),
]


@pytest.mark.parametrize("name,edit", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_launch(gpu, g, engine, name, edit):
    eng = engine(TC.CROP_W, TC.CROP_H, TC.ITOP_MEAN, TC.ITOP_STD)
    frames = torch.from_numpy(TC.frames("a")).to(gpu)
    items = _good_item(g)
    cfg = type(eng.cfg).from_buffer_copy(eng.cfg)
    out = torch.full((1, 1, TC.CROP_H, TC.CROP_W), -77.0, device=gpu)
    rc, _ = _call(gpu, items, 1, cfg, frames, out)
    assert rc == _lib.PN_OK and not bool((out == -77.0).any())                               # the unedited item runs
    edit(items[0], cfg)
    out.fill_(-77.0)
    rc, msg = _call(gpu, items, 1, cfg, frames, out)
    assert rc == PN_ERR_INVALID and "pn_a2j_train_crop" in msg, (rc, msg)
    if not name.startswith(("crop_", "std_")):
        assert "item 0" in msg, msg
    assert bool((out == -77.0).all())


def test_more_than_65535_crops_are_refused_and_none_is_ok(gpu, g, engine):
    eng = engine(TC.CROP_W, TC.CROP_H, TC.ITOP_MEAN, TC.ITOP_STD)
    frames = torch.from_numpy(TC.frames("a")).to(gpu)
    out = torch.full((1, 1, TC.CROP_H, TC.CROP_W), -77.0, device=gpu)
    rc, msg = _call(gpu, _good_item(g), 65536, eng.cfg, frames, out)                          # refused on the count alone: no record is read
    assert rc == PN_ERR_INVALID and "65535" in msg and bool((out == -77.0).all())
    rc, _ = _call(gpu, _good_item(g), 0, eng.cfg, frames, out)
    assert rc == _lib.PN_OK and bool((out == -77.0).all())
    crops, flags = eng.train_crops(frames, (_lib.A2JCropItem * 0)())
    assert tuple(crops.shape) == (0, 1, TC.CROP_H, TC.CROP_W) and tuple(flags.shape) == (0,)


# ---- the engine ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def a2j_fx():
    ga = np.load(os.path.join(GOLDEN, "a2j.npz"))
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(ga["shapes"], ga["ndim"])]
    return ga, AC.state_dict_for_seed(int(ga["seed"]), [str(k) for k in ga["keys"]], shapes)


def test_engine_train_crops_and_votes_equal_post_process_of_the_module(gpu, g, a2j_fx):
    """80 x 96 crops, B = 3 through max_batch = 2 (two chunks): the engine's votes against post_process on the module's heads for the same
    crops, within the tolerance tests/test_gpu_a2j.py uses for that comparison (s_joints_tol of a2j.npz: 4 x the reference's own fp32 error)."""
    from popnet_amd.network.a2j import post_process
    from popnet_amd.pipeline import A2JEngine
    ga, sd = a2j_fx
    H, W, B = AC.SMALL
    eng = A2JEngine(precision="fp32", state_dict=sd, device=gpu, max_batch=2, crop=(H, W))
    idx = [0, 1, 5]
    draws = [TC.draws_of(TC.ITOP_CASES[i][6]) for i in idx]
    rec, labels = AJ.itop_items(idx, TC.itop_centres(), g["itop_lefttop"], g["itop_rightbottom"], TC.itop_keypoints(), TC.SETS["a"], draws=draws,
                                crop_w=W, crop_h=H, frames=[TC.ITOP_CASES[i][2] for i in idx])
    crops, flags = eng.train_crops(torch.from_numpy(TC.frames("a")).to(gpu), rec)
    assert tuple(crops.shape) == (B, 1, H, W) and not flags.cpu().numpy().any() and labels.shape == (B, 15, 3)
    assert float(crops.std()) > 0.1 and bool(torch.isfinite(crops).all())
    votes = eng.votes(crops)
    want = post_process(shape=[H // 16, W // 16], stride=16, P_h=None, P_w=None)(eng.model(crops))
    torch.cuda.synchronize()
    err, tol = float((votes - want).abs().max()), float(ga["s_joints_tol"])
    print("\nA2J TRAINCROP engine votes vs post_process(module): max error %.3g, tolerance %.3g" % (err, tol))
    assert tuple(votes.shape) == (B, 15, 3) and err <= tol, (err, tol)
    assert float(votes[..., :2].std()) > 0


# ---- the scripts, on a fake dataset tree -----------------------------------------------------------------------------------------------
N_FAKE, FAKE_CROP = 6, 96


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fake_itop(root, split, invalid=None):
    """6 frames of 48 x 64 in the ITOP layout: <img_dir>/<id>.npy, the labels json, center_<split>.txt (line `invalid`: that frame drops out)."""
    rng = np.random.default_rng(11 + len(split))
    img_dir = root / ("itop_%s_depth" % split)
    img_dir.mkdir()
    labels, lines = {}, []
    for i in range(N_FAKE):
        np.save(img_dir / ("%s_%d.npy" % (split, i)), AC.PALETTE[rng.integers(4, 12, (48, 64))])
        uvd = np.c_[rng.uniform(5, 60, 15), rng.uniform(5, 44, 15), rng.uniform(2.2, 2.9, 15)]
        labels["%s_%d" % (split, i)] = [{"2d_joints": uvd[:, :2].tolist(), "3d_joints": uvd.tolist(), "visible_joints": [1] * 15}]
        lines.append("invalid invalid invalid" if i == invalid else "%.3f %.3f %.4f" % (rng.uniform(25, 40), rng.uniform(18, 30), rng.uniform(2.4, 2.7)))
    json.dump(labels, open(root / ("itop_%s_labels.json" % split), "w"))
    (root / ("center_%s.txt" % split)).write_text("\n".join(lines) + "\n")
    return ["--%s-annotations" % split, str(root / ("itop_%s_labels.json" % split)), "--%s-image-dir" % split, str(img_dir),
            "--%s-centres" % split, str(root / ("center_%s.txt" % split))]


@pytest.fixture(scope="module")
def itop_run(gpu, tmp_path_factory):
    """scripts/train_a2j_itop.py once: 6 frames (one train centre invalid), crop 96, batch 2, 2 steps, 1 epoch."""
    root = tmp_path_factory.mktemp("itop")
    np.save(root / "mean.npy", np.array([0.1], np.float32))
    np.save(root / "std.npy", np.array([0.3], np.float32))
    common = ["--mean-file", str(root / "mean.npy"), "--std-file", str(root / "std.npy"), "--output-dir", str(root / "out")]
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = _script("train_a2j_itop").main(_fake_itop(root, "train", invalid=2) + _fake_itop(root, "test") + common + [
            "--batch-size", "2", "--max-steps", "2", "--epochs", "1", "--crop", str(FAKE_CROP), "--seed", "3", "--print-freq", "1"])
    return root, common, out, buf.getvalue()


def _check_checkpoint(path):
    from popnet_amd.network.a2j import A2J_model
    assert os.path.basename(path) == "net_0_wetD_0.0001_depFact_0.5_RegFact_3_rndShft_5.pth"
    sd = torch.load(path, map_location="cpu")
    assert len(sd) == 410
    A2J_model(15).load_state_dict(sd)


def test_train_a2j_itop_script(itop_run):
    root, _, out, text = itop_run
    assert len(out["losses"]) == 2 and np.isfinite(out["losses"]).all()
    assert text.count("Cls_loss") == 2
    _check_checkpoint(out["checkpoint"])
    ts = out["test_set"]
    assert len(ts) == N_FAKE and out["votes"].shape == (N_FAKE, 15, 3) and np.isfinite(out["votes"]).all()
    err = AJ.error_compute(out["votes"], ts.keypoints, ts.centres, crop_w=FAKE_CROP, crop_h=FAKE_CROP)
    assert ("epoch:  0 Test error: %s\n" % err) in text, text[-400:]
    assert np.isfinite(err) and out["errors"] == [err]


def test_itop_set_drops_the_frame_of_an_invalid_centre(itop_run, gpu):
    from popnet_amd import targets
    root = itop_run[0]
    s = targets.ItopA2JSet(str(root / "itop_train_depth"), str(root / "itop_train_labels.json"), str(root / "center_train.txt"), device=gpu)
    assert s.ids == ["train_%d" % i for i in (0, 1, 3, 4, 5)] and s.centres.shape == (5, 1, 3) and s.keypoints.shape == (5, 15, 3)
    frames, items, labels = s.batch([1, 2], draws=None, crop=FAKE_CROP)
    assert tuple(frames.shape) == (2, 48, 64) and len(items) == 2 and labels.shape == (2, 15, 3)
    assert torch.equal(frames[1].cpu(), torch.from_numpy(np.load(root / "itop_train_depth" / "train_3.npy")))


def test_evaluate_a2j_itop_script(itop_run, capsys):
    root, common, out, _ = itop_run
    res = _script("evaluate_a2j_itop").main(["--annotations", str(root / "itop_test_labels.json"), "--image-dir", str(root / "itop_test_depth"),
                                             "--centres", str(root / "center_test.txt"), "--weight", out["checkpoint"], "--batch-size", "4",
                                             "--crop", str(FAKE_CROP), "--result-file", "result.txt"] + common)
    text = capsys.readouterr().out
    rows = [line.split() for line in open(res["result_file"]).read().splitlines()]
    assert len(rows) == N_FAKE and all(len(r) == 45 for r in rows)
    ts = res["test_set"]
    want = AJ.write_txt_rows(res["votes"], ts.centres, crop_w=FAKE_CROP, crop_h=FAKE_CROP)
    assert np.array_equal(np.array(rows, dtype=np.float32), want) and np.isfinite(want).all()
    err = AJ.error_compute(res["votes"], ts.keypoints, ts.centres, crop_w=FAKE_CROP, crop_h=FAKE_CROP)
    assert ("Error: %s\n" % err) in text and res["error"] == err
    # the same weights and the same un-augmented crops as the trainer's own test pass
    assert np.abs(res["votes"] - out["votes"]).max() < 1e-3


def _fake_kdh3d(root):
    """6 frames of 64 x 48 in the KDH3D layout: <img_dir>/<id>, seg_maps/<id>, bg_maps/*, labels_bg.json, one labels json per split."""
    rng = np.random.default_rng(23)
    for d in ("depth_maps", "seg_maps", "bg_maps"):
        (root / d).mkdir()
    boxes = [(5.5, 8.0, 40.0, 60.0), (-3.25, 4.0, 30.0, 50.5), (10.0, 2.0, 44.0, 58.0)]
    for split in ("train", "test"):
        labels = {"intrinsics": dict(AC.INTRINSICS)}
        for i in range(N_FAKE):
            name = "%s_%d.npy" % (split, i)
            np.save(root / "depth_maps" / name, AC.PALETTE[rng.integers(4, 12, (64, 48))])
            np.save(root / "seg_maps" / name, (rng.random((64, 48)) < 0.5).astype(np.uint8))
            j2 = np.c_[rng.uniform(5, 44, 15), rng.uniform(5, 60, 15)]
            labels[name] = [{"bbox": list(boxes[i % 3]), "2d_joints": j2.tolist(), "3d_joints": np.c_[j2 / 100, rng.uniform(2, 3, 15)].tolist()}]
        json.dump(labels, open(root / ("labels_%s.json" % split), "w"))
    for i in range(4):
        np.save(root / "bg_maps" / ("b%d.npy" % i), AC.PALETTE[rng.integers(8, 16, (64, 48))])
    json.dump({str(i): {"file_name": "b%d.npy" % i} for i in range(4)}, open(root / "labels_bg.json", "w"))


@pytest.mark.parametrize("bg_aug", [0, 1], ids=["base", "bgaug"])
def test_train_a2j_kdh3d_script(gpu, tmp_path, capsys, bg_aug):
    _fake_kdh3d(tmp_path)
    argv = ["--train-annotations", str(tmp_path / "labels_train.json"), "--test-annotations", str(tmp_path / "labels_test.json"),
            "--image-dir", str(tmp_path / "depth_maps"), "--output-dir", str(tmp_path / "out"), "--batch-size", "2", "--max-steps", "2",
            "--epochs", "1", "--crop", str(FAKE_CROP), "--seed", "5", "--print-freq", "1"]
    if bg_aug:
        argv += ["--bg-aug", "1", "--bg-file", str(tmp_path / "labels_bg.json"), "--bg-dir", str(tmp_path / "bg_maps"), "--seg-dir", str(tmp_path / "seg_maps")]
    mod = _script("train_a2j_kdh3d")
    out = mod.main(argv)
    text = capsys.readouterr().out
    assert len(out["losses"]) == 2 and np.isfinite(out["losses"]).all() and text.count("Cls_loss") == 2
    _check_checkpoint(out["checkpoint"])
    ts = out["test_set"]
    assert out["votes"].shape == (N_FAKE, 15, 3) and np.isfinite(out["votes"]).all()
    acc = mod.accuracies(out["votes"], ts.bndbox, ts.keypoints_2d, ts.keypoints_3d, AC.INTRINSICS, FAKE_CROP, (480, 512))
    assert ("Accuracy 2d: %s\n" % acc[0]) in text and ("Accuracy: %s\n" % acc[1]) in text and out["accuracies"] == [acc]
    frames = ts.frames([0])
    stored = torch.from_numpy(np.load(tmp_path / "depth_maps" / "test_0.npy")).to(gpu).float()
    assert bool((frames[0] != stored).any()) == bool(bg_aug)                                  # the background swap ran, or did not
