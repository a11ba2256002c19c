"""GPU: the random training transform (pn_augment_resize, popnet_amd.targets.mpaug_batch(..., aug) / mpaug_batch_yolo(..., aug), the
trainers' --augment option) against the pure-numpy restatement (tests/cv2_warp_reference.augment_reference) and against the
reference's own outputs (tests/golden/augment.npz).

Bars.  The image: bit for bit -- the kernel rounds every intermediate where OpenCV 4.2's scalar float32 paths round (IEEE +, -, *, /
only, no fused multiply-add).  Through mpaug_batch, the bars tests/test_gpu_targets.py already uses for the unaugmented path: image,
paf, z, fg and prior maps exact, Gaussian heat maps within one float32 ulp at 1.0 (the device's double exp).
"""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_helpers as ah
import cv2_warp_reference as cw
from augment_helpers import G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAT_TOL = 1.2e-7
BIG = dict(H=640, W=480, cx=231.7421875, cy=320.62640380859375)
SMALL = dict(H=ah.H, W=ah.W, cx=ah.CX, cy=ah.CY)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    d = tmp_path_factory.mktemp("augment_tree")
    return d, ah.write_tree(d)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _reference_image(frame, it, depth_max=6.0, mean=0.0, std=1.0):
    img, _, _ = cw.augment_reference(frame, [], dict(rot=it["rot"], a=it["a"], crops=it["crops"], cx=it["cx"], cy=it["cy"], input_size=it["input_size"]))
    return cw.network_input(img, depth_max, mean, std)


def test_kernel_equals_the_restatement_on_the_golden_items(gpu, tree):
    from popnet_amd import targets
    frames = np.stack([ah.composed(tree[0], ci)[0].astype(np.float32) for ci in range(ah.N)])
    items = []
    for ci in range(ah.N):
        p = ah.item_params(ci)
        items.append(targets.augmentation(p["rot"], p["a"], p["crops"], ah.H, ah.W, p["cx"], p["cy"], p["input_size"]))
    out = targets.augment_resize(_dev(frames, gpu), targets.AugmentationBatch(items), ah.S, 6.0, 3.0, 2.0).cpu().numpy()
    for ci in range(ah.N):
        assert np.array_equal(out[ci], G["it%d_image" % ci]), (ci, np.abs(out[ci] - G["it%d_image" % ci]).max())
        assert np.array_equal(out[ci, 0], _reference_image(frames[ci], items[ci], 6.0, 3.0, 2.0)), ci


@pytest.mark.parametrize("geom,batches", [(BIG, (1, 2, 5, 24, 32)), (SMALL, (32, 17, 8, 4, 3))], ids=["640x480", "small"])
def test_kernel_equals_the_restatement_on_a_seeded_sweep(gpu, geom, batches):
    """64 random parameter sets per frame size, in batches of 1 to 32 items, each item with its own geometry; mean 0 / std 1 is the
    un-normalised clamped image mpaug_batch needs.  Frames reach below 0 and above depth_max, so the clamp works on both sides."""
    from popnet_amd import targets
    assert sum(batches) >= 64
    rng = np.random.default_rng(geom["H"])
    random.seed(geom["W"])
    branches = set()
    for B in batches:
        frames = rng.uniform(-0.5, 6.5, (B, geom["H"], geom["W"])).astype(np.float32)
        items = [targets.draw_augmentation(**geom) for _ in range(B)]
        branches |= {it["render_a"] <= 1 for it in items}
        out = targets.augment_resize(_dev(frames, gpu), targets.AugmentationBatch(items)).cpu().numpy()
        assert out.shape == (B, 1, 224, 224) and out.min() >= 0.0 and out.max() <= 6.0
        for b in range(B):
            want = _reference_image(frames[b], items[b])
            assert np.array_equal(out[b, 0], want), (B, b, items[b]["rot"], items[b]["a"], items[b]["crops"], np.abs(out[b, 0] - want).max())
    assert branches == {True, False}


def test_items_of_a_batch_do_not_depend_on_their_neighbours(gpu):
    from popnet_amd import targets
    rng = np.random.default_rng(3)
    random.seed(3)
    B = 16
    frames = _dev(rng.uniform(0.2, 6.0, (B, SMALL["H"], SMALL["W"])).astype(np.float32), gpu)
    items = [targets.draw_augmentation(**SMALL) for _ in range(B)]
    out = targets.augment_resize(frames, targets.AugmentationBatch(items))
    perm = rng.permutation(B)
    out_p = targets.augment_resize(frames[torch.from_numpy(perm).to(gpu)], targets.AugmentationBatch([items[i] for i in perm]))
    assert torch.equal(out_p, out[torch.from_numpy(perm).to(gpu)])
    single = targets.augment_resize(frames[5:6], targets.AugmentationBatch([items[5]]))
    assert torch.equal(single[0], out[5])


def test_a_crop_one_pixel_wide_runs_like_the_restatement(gpu):
    """Crop may leave a single column or row; cv2.resize replicates it, and so do the restatement and the kernel."""
    from popnet_amd import targets
    rng = np.random.default_rng(8)
    frames = rng.uniform(0.2, 6.0, (2, 8, 8)).astype(np.float32)
    items = [targets.augmentation(0.0, 1.0, (0.3, 0.4, 0.0, 0.0), 8, 8, 4.0, 4.0), targets.augmentation(5.0, 1.0, (0.0, 0.1, 0.3, 0.4), 8, 8, 4.0, 4.0)]
    assert items[0]["src_w"] == 1 and items[1]["src_h"] == 1
    out = targets.augment_resize(_dev(frames, gpu), targets.AugmentationBatch(items)).cpu().numpy()
    for b in range(2):
        assert np.array_equal(out[b, 0], _reference_image(frames[b], items[b])), b


def _golden_batch(gpu, d):
    """All golden items as one batch, padded to the widest item: the arguments of mpaug_batch / mpaug_batch_yolo and the items' transforms."""
    from popnet_amd import targets
    src = [ah.item_sources(d, ci) for ci in range(ah.N)]
    Smax, Pmax = max(s[0].shape[0] for s in src), max(len(s[3]) for s in src)
    fd = np.zeros((ah.N, Smax, ah.H, ah.W), dtype=np.float16)
    fm = np.zeros((ah.N, Smax, ah.H, ah.W), dtype=np.uint8)
    k2 = np.zeros((ah.N, Pmax, 15, 2), dtype=np.float32)
    k3 = np.zeros((ah.N, Pmax, 15, 3), dtype=np.float64)
    bb, pw = np.zeros((ah.N, Pmax, 4)), np.zeros((ah.N, Pmax))
    items = []
    for ci, (depths, masks, _, persons) in enumerate(src):
        fd[ci, :len(depths)], fm[ci, :len(masks)] = depths, masks
        for p, ps in enumerate(persons):
            k2[ci, p], k3[ci, p], bb[ci, p], pw[ci, p] = ps["2d_joints"], ps["3d_joints"], ps["bbox"], ps["pose_weight"]
        q = ah.item_params(ci)
        items.append(targets.augmentation(q["rot"], q["a"], q["crops"], ah.H, ah.W, q["cx"], q["cy"], q["input_size"]))
    n_src = torch.tensor([s[0].shape[0] for s in src], dtype=torch.int32, device=gpu)
    npers = torch.tensor([len(s[3]) for s in src], dtype=torch.int32, device=gpu)
    bg = np.stack([s[2] for s in src])
    return (_dev(fd, gpu), _dev(fm, gpu), n_src, _dev(bg, gpu)), (k2, k3, npers), (bb, _dev(pw, gpu)), targets.AugmentationBatch(items)


def test_mpaug_batch_with_aug_equals_the_reference_dataset_items(gpu, tree):
    from popnet_amd import targets
    frames, (k2, k3, npers), (bb, pw), aug = _golden_batch(gpu, tree[0])
    x, heat, paf, z, fg = targets.mpaug_batch(*frames, k2, k3, npers, aug=aug)
    xd = targets.mpaug_batch(*frames, _dev(k2, gpu), _dev(k3, gpu), npers, aug=aug)          # labels handed over on the device: copied back, same maps
    xy, prior, conf, coord, weight = targets.mpaug_batch_yolo(*frames, k2, k3, npers, bb, pw, aug=aug)
    assert torch.equal(x, xy) and all(torch.equal(a, b) for a, b in zip((x, heat, paf, z, fg), xd))
    for ci in range(ah.N):
        k = "it%d_" % ci
        assert np.array_equal(x[ci].cpu().numpy(), G[k + "image"]), ci
        assert np.array_equal(fg[ci].cpu().numpy(), G[k + "fg"]), ci
        assert np.array_equal(z[ci].cpu().numpy(), G[k + "z"]), ci
        assert np.array_equal(paf[ci].cpu().numpy(), G[k + "paf"]), ci
        assert np.abs(heat[ci].cpu().numpy() - G[k + "heat"]).max() <= HEAT_TOL, ci
        for name, t in (("prior", prior), ("conf", conf), ("coord", coord), ("weight", weight)):
            assert np.array_equal(t[ci].cpu().numpy(), G[k + name]), (ci, name)


def test_aug_none_is_the_call_without_the_argument(gpu, tree):
    from popnet_amd import targets
    frames, (k2, k3, npers), (bb, pw), _ = _golden_batch(gpu, tree[0])
    k2, k3 = _dev(k2, gpu), _dev(k3, gpu)
    bb = _dev(bb * (224.0 / ah.W), gpu)
    for a, b in zip(targets.mpaug_batch(*frames, k2, k3, npers), targets.mpaug_batch(*frames, k2, k3, npers, aug=None)):
        assert torch.equal(a, b)
    for a, b in zip(targets.mpaug_batch_yolo(*frames, k2, k3, npers, bb, pw), targets.mpaug_batch_yolo(*frames, k2, k3, npers, bb, pw, aug=None)):
        assert torch.equal(a, b)


def test_train_set_batch_with_augment_feeds_mpaug_batch(gpu, tree):
    """MPAugTrainSet.batch(augment=True): cx, cy from the annotation file's intrinsics, the draws interleaved with the source draws, the
    labels on the host, the AugmentationBatch last; the default call returns what it returned before."""
    from popnet_amd import targets
    d, ann_files = tree
    d = str(d)
    ts = targets.MPAugTrainSet(os.path.join(d, "img"), ann_files, os.path.join(d, "bg.json"), os.path.join(d, "bg"), os.path.join(d, "seg"), device=gpu, shuffle=False)
    random.seed(4)
    plain = ts.batch([0, 1])
    assert len(plain) == 7 and all(isinstance(t, torch.Tensor) and t.is_cuda for t in plain)
    random.seed(4)
    *parts, aug = ts.batch([0, 1], with_boxes=True, augment=True, max_aug_ratio=1.2)
    assert isinstance(aug, targets.AugmentationBatch) and len(aug) == 2 and len(parts) == 9
    assert all(it["cx"] == ah.CX and it["cy"] == ah.CY and 0.7 <= it["a"] <= 1.2 for it in aug.items)
    assert isinstance(parts[4], np.ndarray) and isinstance(parts[5], np.ndarray) and isinstance(parts[7], np.ndarray)
    out = targets.mpaug_batch_yolo(*parts, aug=aug)
    assert out[0].shape == (2, 1, 224, 224) and all(bool(torch.isfinite(t).all()) for t in out)


def test_exact_2x_decimation_is_refused_by_the_c_call_naming_the_item(gpu):
    """448 x 448 -> 224: cv2.resize(INTER_LINEAR) runs INTER_AREA there, which is not built.  The status comes back from the C call before
    anything is launched; the output buffer is left alone."""
    from popnet_amd import _lib, targets
    ok = targets.augmentation(2.0, 0.9, (0.01, 0.02, 0.03, 0.04), 449, 449, 224.0, 224.0)
    bad = targets.augmentation(0.0, 1.0, (0.0, 0.0, 0.0, 0.0), 449, 449, 224.0, 224.0)
    assert (bad["src_w"], bad["src_h"]) == (448, 448)
    aug = targets.AugmentationBatch([ok, bad])
    frames = torch.ones((2, 449, 449), dtype=torch.float32, device=gpu)
    with pytest.raises(_lib.PopnetError, match=r"item 1.*exact 2x decimation"):
        targets.augment_resize(frames, aug)
    out = torch.full((2, 1, 224, 224), -7.0, dtype=torch.float32, device=gpu)
    items = torch.zeros(C.sizeof(aug.records), dtype=torch.uint8, device=gpu)
    ctx = _lib.Context.for_device(gpu.index or 0)
    rc = _lib.lib().pn_augment_resize(ctx.handle, C.c_void_p(frames.data_ptr()), C.cast(aug.records, C.c_void_p), C.c_void_p(items.data_ptr()), 2, 449, 449,
                                      C.c_void_p(out.data_ptr()), 224, 6.0, 0.0, 1.0, _lib.current_stream_ptr(gpu))
    assert rc == -4 and "item 1" in ctx.last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((items == 0).all())      # nothing launched, nothing uploaded
    # another output size is not a 2x decimation: the same batch runs
    assert targets.augment_resize(frames, targets.AugmentationBatch([dict(ok, input_size=112), dict(bad, input_size=112)]), 112).shape == (2, 1, 112, 112)
    with pytest.raises(_lib.PopnetError, match="CUDA/ROCm tensor"):
        targets.augment_resize(torch.ones(2, 449, 449), aug)


def _run_trainer(script, d, ann_files, out_dir, extra, limit=420):
    """One run of a trainer in a fresh child process under its own time limit.  -> (stdout, first-step loss)"""
    cmd = [sys.executable, os.path.join(ROOT, "scripts", script), "--train-annotations"] + ann_files + ["--val-annotations"] + ann_files + [
        "--image-dir", os.path.join(d, "img"), "--bg-file", os.path.join(d, "bg.json"), "--bg-dir", os.path.join(d, "bg"), "--seg-dir", os.path.join(d, "seg"),
        "--output-dir", out_dir, "--batch-size", "2", "--lr", "0.05", "--print-freq", "1", "--seed", "3"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=limit)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    first = [l for l in r.stdout.splitlines() if l.startswith("Epoch: [0][0/")]
    assert len(first) == 1, r.stdout
    return r.stdout, float(first[0].split("Loss")[1].split()[0])


@pytest.mark.parametrize("script,n_keys", [("train_mpaug.py", 234), ("train_yolo_mpaug.py", 223)])
def test_trainers_run_with_augment(gpu, tree, tmp_path, script, n_keys):
    """--augment 1: two epochs on the fake tree, finite losses, a loadable best_pose.pth; the same seed gives the same first-step loss;
    --augment 0 with that seed gives another one, so the option reaches the batch.  Each run is a child process with its own time
    limit, and the first failure ends the test."""
    d, ann_files = str(tree[0]), tree[1]
    out, first = _run_trainer(script, d, ann_files, str(tmp_path / "a"), ["--augment", "1", "--epochs", "2"])
    losses = [float(l.split("Loss")[1].split()[0]) for l in out.splitlines() if l.startswith("Epoch: [")]
    vals = [float(l.split("val loss")[1].split()[0]) for l in out.splitlines() if "val loss" in l]
    assert len(losses) == 2 and len(vals) == 2 and all(np.isfinite(v) for v in losses + vals), out
    sd = torch.load(str(tmp_path / "a" / "best_pose.pth"), map_location="cpu")
    assert len(sd) == n_keys and all(k.startswith("module.") for k in sd) and all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    if script == "train_mpaug.py":
        from popnet_amd.network.rtpose_light3d import rtpose_light3d
        rtpose_light3d(15, 14, 2, input_dim=1).load_state_dict(sd)
    else:
        from popnet_amd.network.yolo_posenet import YoloPoseNet
        YoloPoseNet(15, input_dim=1).load_state_dict(sd)
    _, again = _run_trainer(script, d, ann_files, str(tmp_path / "b"), ["--augment", "1", "--epochs", "1"])
    assert again == first
    _, plain = _run_trainer(script, d, ann_files, str(tmp_path / "c"), ["--augment", "0", "--epochs", "1"])
    assert plain != first
