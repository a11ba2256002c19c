#!/usr/bin/env python
"""Generates the A2J goldens under tests/golden/ by running the REFERENCE ITSELF (third_party_methods/A2J_experiments, imported
read-only) on the seeded inputs of tests/a2j_cases.py, on the CPU.

    python tests/golden/make_golden_a2j.py            # rewrites tests/golden/a2j.npz and a2j_crops.npz
    python tests/golden/make_golden_a2j.py --check    # regenerates into a scratch dir and compares (tests/test_a2j_golden_recipe.py)

Only data leaves this script: the state-dict key names and shapes, the reference's outputs and tolerances derived from them.
  a2j.npz        keys / shapes of A2J_model(15).state_dict(); per case ("s" = 80 x 96, B = 3; "l" = 288 x 288, B = 2) the three heads and
                 the voted joints of the reference run in .double() (the large case: joints, and every 37th head element), and per
                 tensor tol = 4 x max|fp32 run - fp64 run| (another summation order is the same class of error as the reference's own
                 fp32 rounding, hence the margin of 4); the chain: box rows -> crops -> net -> vote -> frame coordinates.  Of the chain
                 the crops, the heads and the votes are the reference's own (dataPreprocess, A2J_model, post_process); the frame
                 coordinates and X / Y are NOT produced by the reference's code: its map-back is inline in main()
                 (a2j_test_pred_box_new.py:373-394), which cannot be called, so tests/a2j_cases.py::map_back restates its float32
                 arithmetic, v (x1 - x0) / crop + x0 and (x - cx) z / fx, in numpy -- a restatement by this project, independent of the
                 kernel but not of its author.
  a2j_crops.npz  dataPreprocess (a2j_test_pred_box_new.py:268-313) on a 640 x 480 frame for the boxes of a2j_cases.CROP_CASES.
The reference's constructors fetch ImageNet weights: resnet.resnet50 is replaced by the plain constructor BEFORE A2J_model is built,
so nothing is downloaded.  dataPreprocess lives in a script that cannot be imported (it reads a dataset at import): the function is
cut out of the file's syntax tree and executed with the globals it reads.  cv2 is not installed: cv2.resize is the restated
INTER_NEAREST rule of oracle/cv2_resize.py.
"""
import ast
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import a2j_cases as AC  # noqa: E402

REF = "/root/reference"
A2J_DIR = os.path.join(REF, "third_party_methods", "A2J_experiments")


def reference_modules():
    import torch
    np.float = float
    np.int = int
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    sys.path.insert(0, os.path.join(REF, "third_party_methods"))
    from A2J_experiments import resnet
    resnet.resnet50 = lambda pretrained=False, **kw: resnet.ResNet(resnet.Bottleneck, [3, 4, 6, 3])      # never model_zoo.load_url
    from A2J_experiments import anchor, model
    return model, anchor


def reference_data_preprocess():
    """dataPreprocess, executed with the globals it reads."""
    from oracle import cv2_resize
    src = open(os.path.join(A2J_DIR, "a2j_test_pred_box_new.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "dataPreprocess"][0]
    import torch
    cv2 = types.SimpleNamespace(INTER_NEAREST=cv2_resize.INTER_NEAREST,
                                resize=lambda img, dsize, interpolation: cv2_resize.resize(np.asarray(img, np.float32), dsize, interpolation=interpolation))
    g = {"np": np, "os": os, "cv2": cv2, "torch": torch, "cropHeight": 288, "cropWidth": 288, "imgWidth": 480, "imgHeight": 512, "MEAN": 3, "STD": 2,
         "test_image_ids": []}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "dataPreprocess", "exec"), g)
    return g


def run_crops(frames, rows):
    """rows [n, 6] -> [n, 288, 288] float32 through the reference's dataPreprocess."""
    g = reference_data_preprocess()
    d = tempfile.mkdtemp(prefix="a2j_frames_")
    for f in range(frames.shape[0]):
        np.save(os.path.join(d, "%d.npy" % f), frames[f])
    g["test_image_ids"][:] = ["%d.npy" % int(r[0]) for r in rows]
    bnd = np.asarray(rows[:, 1:], dtype=np.float32)
    try:
        out = [g["dataPreprocess"](i, d, bnd, "TEST")[0].numpy()[0] for i in range(len(rows))]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return np.stack(out).astype(np.float32)


def generate():
    import torch
    model, anchor = reference_modules()
    torch.manual_seed(0)
    net = model.A2J_model(num_classes=15).eval()
    keys = list(net.state_dict().keys())
    shapes = [tuple(v.shape) for v in net.state_dict().values()]
    assert len(keys) == 410, len(keys)
    net.load_state_dict(AC.state_dict_for_seed(AC.SEED, keys, shapes))
    net64 = model.A2J_model(num_classes=15).eval()
    net64.load_state_dict(net.state_dict())
    net64 = net64.double()
    shp = np.zeros((len(keys), 4), np.int64)
    for i, s in enumerate(shapes):
        shp[i, :len(s)] = s
    out = {"seed": np.int64(AC.SEED), "keys": np.array(keys), "shapes": shp, "ndim": np.array([len(s) for s in shapes], np.int64),
           "n_params": np.int64(sum(int(np.prod(s)) for k, s in zip(keys, shapes) if not k.endswith("num_batches_tracked")))}

    def run(x):
        """-> (fp64 heads + joints, fp32 heads + joints) of the reference"""
        H, W = x.shape[2:]
        res = []
        for m, t in ((net64, torch.from_numpy(x).double()), (net, torch.from_numpy(x))):
            pp = anchor.post_process(shape=[H // 16, W // 16], stride=16, P_h=None, P_w=None)
            pp.all_anchors = pp.all_anchors.to(t.dtype)
            with torch.no_grad():
                heads = m(t)
                joints = pp(heads, voting=False)
            res.append([h.numpy() for h in heads] + [joints.numpy()])
        return res

    out.update(ref_generate_anchors=anchor.generate_anchors(), ref_shift_5x6=anchor.shift([5, 6], 16, anchor.generate_anchors()),
               ref_shift_18x18=anchor.shift([18, 18], 16, anchor.generate_anchors()))
    max_w = 0.0
    for tag, (H, W, B) in (("s", AC.SMALL), ("l", AC.LARGE)):
        x = AC.net_input(AC.SEED + H, B, H, W)
        r64, r32 = run(x)
        w = torch.softmax(torch.from_numpy(r64[0]), 1)
        max_w = max(max_w, float(w.max()))
        out["%s_logit_std" % tag] = np.float64(r64[0].std())
        out["%s_max_softmax" % tag] = np.float64(w.max())
        for name, a64, a32 in zip(("cls", "reg", "dep", "joints"), r64, r32):
            out["%s_%s_tol" % (tag, name)] = np.float64(4 * np.abs(a32.astype(np.float64) - a64).max())
            keep = a64 if (tag == "s" or name == "joints") else a64.reshape(-1)[::AC.SUBSAMPLE]
            out["%s_%s" % (tag, name)] = keep.astype(np.float64)
        if tag == "s":
            out["s_joints_f32"] = r32[3].astype(np.float32)
    assert max_w < 0.05, "largest softmax weight %g: the vote would not sum over many anchors" % max_w

    # chain: rows -> crops -> net -> vote -> frame coordinates (the script's float32 arithmetic, a2j_cases.map_back)
    frames = AC.depth_frames(AC.SEED + 1, 2)
    crops = run_crops(frames, AC.CHAIN_ROWS)
    r64, r32 = run(crops[:, None])
    xy, xyz = AC.map_back(r64[3].astype(np.float32), AC.CHAIN_ROWS)
    out.update(chain_votes=r64[3].astype(np.float64), chain_xy=xy, chain_xyz=xyz, chain_conf=AC.CHAIN_ROWS[:, 5].copy(), chain_frame=AC.CHAIN_ROWS[:, 0].astype(np.int32),
               chain_tol=np.float64(4 * np.abs(r32[3].astype(np.float64) - r64[3]).max()))

    cframe = AC.depth_frames(AC.SEED + 2, 1)
    crops_out = {"names": np.array([n for n, _ in AC.CROP_CASES]), "rows": AC.crop_rows(0), "crops": run_crops(cframe, AC.crop_rows(0))}
    return out, crops_out


def _same(a, b):
    if sorted(a.keys()) != sorted(b.keys()):
        return "keys differ: %s" % sorted(set(a.keys()) ^ set(b.keys()))
    for k in a.keys():
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            return "%s: %s %s vs %s %s" % (k, x.shape, x.dtype, y.shape, y.dtype)
        if k.endswith("_tol"):      # 4 x the reference's own fp32 rounding error: the same class under another split of its sums
            if not (0.5 * y <= x <= 2 * y):
                return "%s: %g vs %g" % (k, x, y)
        elif x.dtype.kind == "f" and not k.endswith("crops") and k not in ("rows", "chain_conf"):
            # the reference's CPU convolutions may split their sums by thread count: equal within a tenth of the stored tolerance
            if not np.allclose(x, y, rtol=0, atol=1e-9 + 1e-6 * np.abs(y).max()):
                return "%s differs by %g" % (k, np.abs(x - y).max())
        elif not np.array_equal(x, y):
            return "%s differs" % k
    return None


if __name__ == "__main__":
    heads, crops = generate()
    if "--check" in sys.argv:
        for name, got in (("a2j.npz", heads), ("a2j_crops.npz", crops)):
            why = _same(got, dict(np.load(os.path.join(HERE, name))))
            if why:
                print("golden check FAILED: %s: %s" % (name, why))
                sys.exit(1)
        print("golden check ok: 2 files regenerate")
    else:
        np.savez_compressed(os.path.join(HERE, "a2j.npz"), **heads)
        np.savez_compressed(os.path.join(HERE, "a2j_crops.npz"), **crops)
        for name in ("a2j.npz", "a2j_crops.npz"):
            print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")
        print({k: float(v) for k, v in heads.items() if np.asarray(v).ndim == 0})
