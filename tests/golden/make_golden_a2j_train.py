#!/usr/bin/env python
"""Generates tests/golden/a2j_train.npz by running the REFERENCE ITSELF (third_party_methods/A2J_experiments, imported read-only) for one
training step on the seeded inputs of tests/a2j_cases.py, on the CPU, in fp64 and in fp32.

    python tests/golden/make_golden_a2j_train.py            # rewrites tests/golden/a2j_train.npz
    python tests/golden/make_golden_a2j_train.py --check    # regenerates and compares (tests/test_a2j_train_reference.py)

Only data leaves this script.  The case: a2j_cases.SMALL (80 x 96, B = 3, a 5 x 6 map), state_dict_for_seed(SEED), net.train(); the body of
train_a2j_mpaug_new.py:463-501 -- heads = net(img); Cls, Reg = A2J_loss(heads, label); (Cls + 3 Reg).backward() -- with spatialFactor 0.5.
The labels are the fp64 run's own vote plus the offset table of offsets(): every magnitude from 0.05 to 20 with both signs, z scaled by
0.7, so both branches of the smooth L1 and both signs of every |.| occur in every term (asserted below).
Stored, all fp64 unless named: the labels; the two loss terms; the gradients of the three heads (the reference's [B, K, P] layout); every
parameter tensor's gradient norm; every 4099th element of the gradient in state-dict order (tensors without a gradient -- fc.* -- left out);
the BatchNorm running statistics after the step of bn1, layer4.2.bn2 and the three heads' bn4; and for each of these `*_tol` = 4 x |the
reference's fp32 run - its fp64 run| (the rule of make_golden_a2j.py).
crop_labels cases: the label half of dataPreprocess (train_a2j_mpaug_new.py:271-355) for one person per case, boxes inside the frame and past
each of its four edges.  The function is cut out of the script's syntax tree (the script reads a dataset at import) and executed with the
globals it reads, `preprocess` the identity, cv2.resize the restated INTER_NEAREST rule of oracle/cv2_resize.py.
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import a2j_cases as AC  # noqa: E402
from make_golden_a2j import A2J_DIR, reference_modules  # noqa: E402

SPATIAL_FACTOR, REG_LOSS_FACTOR = 0.5, 3
SAMPLE_EVERY = 4099
STAT_LAYERS = ("Backbone.model.bn1", "Backbone.model.layer4.2.bn2", "classificationModel.bn4", "regressionModel.bn4", "DepthRegressionModel.bn4")
MAGNITUDES = np.array([0.05, 0.3, 0.8, 1.5, 4.0, 9.0, 20.0])


def offsets(B, P):
    """[B, P, 3]: magnitudes cycling through MAGNITUDES along (b, p, c), the sign alternating with a period of its own; z x 0.7"""
    i = np.arange(B * P * 3).reshape(B, P, 3)
    off = MAGNITUDES[i % len(MAGNITUDES)] * np.where((i // 2) % 2 == 0, 1.0, -1.0)
    off[:, :, 2] *= 0.7
    return off


# name, (x0, y0, x1, y1) in the 480 x 512 frame
LABEL_CASES = [
    ("inside", (120.0, 200.0, 200.0, 330.0)),
    ("left", (-20.5, 100.0, 60.0, 220.0)),
    ("top", (100.0, -15.25, 190.0, 90.0)),
    ("right", (420.0, 50.0, 500.5, 170.0)),
    ("bottom", (200.0, 430.0, 280.0, 560.0)),
    ("all_four", (-10.5, -20.25, 495.5, 540.0)),
]


def label_case_joints(i, box):
    rng = np.random.default_rng(AC.SEED + 100 + i)
    x0, y0, x1, y1 = box
    j2 = np.stack([rng.uniform(x0, x1, 15), rng.uniform(y0, y1, 15)], 1)
    j3 = np.stack([rng.normal(0, 1, 15), rng.normal(0, 1, 15), rng.uniform(1.0, 5.0, 15)], 1)
    return j2, j3


def reference_labels():
    """the reference's dataPreprocess on one person per case -> [n, 15, 3] float32 (y, x, z)"""
    import torch
    from oracle import cv2_resize
    src = open(os.path.join(A2J_DIR, "train_a2j_mpaug_new.py")).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "dataPreprocess"][0]
    cv2 = types.SimpleNamespace(INTER_NEAREST=cv2_resize.INTER_NEAREST,
                                resize=lambda img, dsize, interpolation: cv2_resize.resize(np.asarray(img, np.float32), dsize, interpolation=interpolation))
    g = {"np": np, "cv2": cv2, "torch": torch, "cropHeight": 288, "cropWidth": 288, "imgWidth": 480, "imgHeight": 512, "MEAN": 3, "STD": 2,
         "keypointsNumber": 15, "preprocess": lambda t: t}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "dataPreprocess", "exec"), g)
    image = np.full((512, 480), 3.0)
    out = []
    for i, (_, box) in enumerate(LABEL_CASES):
        j2, j3 = label_case_joints(i, box)
        ann = {"bbox": list(box), "2d_joints": j2.tolist(), "3d_joints": j3.tolist()}
        _, label, _ = g["dataPreprocess"](image, [ann], "TRAIN")
        out.append(label.numpy().astype(np.float32))
    return np.stack(out)


def generate():
    import torch
    model, anchor = reference_modules()
    torch.manual_seed(0)
    H, W, B = AC.SMALL
    h, w = H // 16, W // 16
    probe = model.A2J_model(num_classes=15)
    keys = list(probe.state_dict().keys())
    shapes = [tuple(v.shape) for v in probe.state_dict().values()]
    sd = AC.state_dict_for_seed(AC.SEED, keys, shapes)
    x = torch.from_numpy(AC.net_input(AC.SEED + H, B, H, W))

    def step(dtype, labels):
        net = model.A2J_model(num_classes=15)
        net.load_state_dict(sd)
        net = net.to(dtype).train()
        crit = anchor.A2J_loss(shape=[h, w], thres=[16.0, 32.0], stride=16, spatialFactor=SPATIAL_FACTOR, img_shape=[W, H], P_h=None, P_w=None)
        crit.all_anchors = crit.all_anchors.to(dtype)
        heads = net(x.to(dtype))
        if labels is None:          # the fp64 run's own vote (post_process's arithmetic on the train-mode heads) plus the offset table
            with torch.no_grad():
                wgt = torch.softmax(heads[0], 1)
                yx = (wgt.unsqueeze(3) * (crit.all_anchors[None, :, None, :] + heads[1])).sum(1)
                z = (wgt * heads[2]).sum(1)
                labels = torch.cat([yx, z.unsqueeze(2)], 2) + torch.from_numpy(offsets(B, 15))
        for t in heads:
            t.retain_grad()
        cls_loss, reg_loss = crit(heads, labels.to(dtype))
        (1 * cls_loss + reg_loss * REG_LOSS_FACTOR).backward()
        named = dict(net.named_parameters())
        grads = [(k, named[k].grad.detach().double()) for k in keys if k in named and named[k].grad is not None]
        nograd = [k for k in keys if k in named and named[k].grad is None]
        flat = torch.cat([g.reshape(-1) for _, g in grads])
        after = net.state_dict()
        r = {"terms": np.array([float(cls_loss), float(reg_loss)]),
             "dcls": heads[0].grad.double().numpy(), "dreg": heads[1].grad.double().numpy(), "ddep": heads[2].grad.double().numpy(),
             "grad_norms": np.array([float(g.norm()) for _, g in grads]), "grad_samples": flat[::SAMPLE_EVERY].numpy()}
        for name in STAT_LAYERS:
            r["stat_mean." + name] = after[name + ".running_mean"].double().numpy()
            r["stat_var." + name] = after[name + ".running_var"].double().numpy()
        return r, labels, [k for k, _ in grads], nograd, (heads, crit.all_anchors)

    r64, labels, gkeys, nograd, (heads64, anchors) = step(torch.float64, None)
    r32 = step(torch.float32, labels)[0]
    assert nograd == ["Backbone.model.fc.weight", "Backbone.model.fc.bias"], nograd
    # the labels exercise both branches of the smooth L1 and both signs on each of the three terms
    with torch.no_grad():
        wgt = torch.softmax(heads64[0], 1)
        d_a = labels[:, :, :2] - (wgt.unsqueeze(3) * anchors[None, :, None, :]).sum(1)
        d_r = labels[:, :, :2] - (wgt.unsqueeze(3) * (anchors[None, :, None, :] + heads64[1])).sum(1)
        d_z = labels[:, :, 2] - (wgt * heads64[2]).sum(1)
    for d in (d_a, d_r):
        assert bool((d.abs() <= 1).any() and (d.abs() > 1).any() and (d > 0).any() and (d < 0).any())
    assert bool((d_z > 0).any() and (d_z < 0).any())
    assert all(float(n) > 0 for n in r64["grad_norms"][[i for i, k in enumerate(gkeys) if not (k.endswith(".bias") and ".conv" in k)]]), "a zero gradient tensor"

    out = {"seed": np.int64(AC.SEED), "labels": labels.numpy().astype(np.float64), "grad_keys": np.array(gkeys), "sample_every": np.int64(SAMPLE_EVERY),
           "spatial_factor": np.float64(SPATIAL_FACTOR), "reg_loss_factor": np.float64(REG_LOSS_FACTOR)}
    for k, v in r64.items():
        out[k] = v.astype(np.float64)
        d = np.abs(r32[k].astype(np.float64) - v)
        out[k + "_tol"] = 4 * d if k in ("terms", "grad_norms") else np.float64(4 * d.max())
    out["label_case_names"] = np.array([n for n, _ in LABEL_CASES])
    out["label_case_boxes"] = np.array([b for _, b in LABEL_CASES], np.float64)
    out["label_case_labels"] = reference_labels()
    return out


def _same(a, b):
    if sorted(a.keys()) != sorted(b.keys()):
        return "keys differ: %s" % sorted(set(a.keys()) ^ set(b.keys()))
    for k in a.keys():
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            return "%s: %s %s vs %s %s" % (k, x.shape, x.dtype, y.shape, y.dtype)
        if k.endswith("_tol"):      # 4 x the reference's own fp32 rounding error: the same class under another split of its sums
            continue
        if x.dtype.kind == "f" and not k.startswith("label_case"):
            # the reference's CPU convolutions may split their sums by thread count: equal well within the stored tolerance
            tol = np.asarray(b[k + "_tol"]) if k + "_tol" in b else 0.0
            if not bool((np.abs(x - y) <= 1e-12 + 0.1 * tol + 1e-9 * np.abs(y).max()).all()):
                return "%s differs by %g" % (k, np.abs(x - y).max())
        elif not np.array_equal(x, y):
            return "%s differs" % k
    return None


if __name__ == "__main__":
    got = generate()
    path = os.path.join(HERE, "a2j_train.npz")
    if "--check" in sys.argv:
        why = _same(got, dict(np.load(path)))
        if why:
            print("golden check FAILED: a2j_train.npz: %s" % why)
            sys.exit(1)
        print("golden check ok: a2j_train.npz regenerates")
    else:
        np.savez_compressed(path, **got)
        print("a2j_train.npz", os.path.getsize(path), "bytes")
        print("Cls %.4f Reg %.4f" % tuple(got["terms"]), {k: (float(np.max(v))) for k, v in got.items() if k.endswith("_tol")})
