#!/usr/bin/env python
"""Generates tests/golden/a2j_traincrop.npz by running the REFERENCE ITSELF on the inputs of tests/a2j_traincrop_cases.py, on the CPU.

    python tests/golden/make_golden_a2j_traincrop.py            # rewrites tests/golden/a2j_traincrop.npz
    python tests/golden/make_golden_a2j_traincrop.py --check    # regenerates and compares (tests/test_a2j_traincrop_golden_recipe.py)

What runs is the reference's own code, cut out of the syntax tree of scripts that cannot be imported (they read a dataset at import)
and executed with the globals it reads (third_party_methods/A2J_experiments/):
  itop_train_64.py          dataPreprocess, transform, pixel2world, world2pixel, errorCompute, writeTxt, and the module-level statements that
                            build train_lefttop_pixel / train_rightbottom_pixel from center_train (:139, :164-173)
  train_a2j_base.py         dataPreprocess, transform
  train_a2j_bgaug_new.py    dataPreprocess, transform (the background swap included: depth, mask and background are files it loads)
cv2 is not installed: cv2.resize is oracle.cv2_resize.resize (the INTER_NEAREST rule), cv2.getRotationMatrix2D and cv2.warpAffine are the
restatements of tests/cv2_warp_reference.py; the shim asserts that the image reaching warpAffine is float32.  np.random is replaced by a
scripted source that hands out each case's draws and logs the calls; the log is stored (the sampler's draw order is tested against it).
Only data leaves this script: crops, labels, flags, boxes, the map-back results, the call log and numpy's version -- whose promotion rules
decide where the reference's mixed float32 / Python-number expressions round (see popnet_amd/a2j_crops.py).
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
import a2j_traincrop_cases as TC  # noqa: E402
import cv2_warp_reference as WR  # noqa: E402

REF = "/root/reference"
A2J_DIR = os.path.join(REF, "third_party_methods", "A2J_experiments")
NAME = "a2j_traincrop.npz"


class EmptyImage(Exception):
    """cv2.resize raises on an empty image."""


class Scripted:
    """np.random of the reference, scripted: hands out the queued values and logs every call."""

    def __init__(self):
        self.queue, self.log = [], []

    def _next(self, kind):
        k, v = self.queue.pop(0)
        assert k == kind, "the reference called %s where %s was scripted" % (kind, k)
        return v

    def randint(self, lo, hi):
        self.log.append("randint(%d, %d)" % (lo, hi))
        return self._next("randint")

    def normal(self, mu, sigma, n):
        self.log.append("normal(%g, %g, %d)" % (mu, sigma, n))
        return np.zeros(n)

    def rand(self):
        self.log.append("rand()")
        return self._next("rand")


class NumpyWith:
    """numpy with np.random scripted and the aliases the reference's numpy still had"""

    def __init__(self, rnd):
        self.random, self.float, self.int = rnd, float, int

    def __getattr__(self, name):
        return getattr(np, name)


def cut(path, functions=(), assigns=()):
    """The named functions, and the module-level assignments to the named variables, of a reference script as one module node."""
    body = []
    for n in ast.parse(open(path).read()).body:
        if isinstance(n, ast.FunctionDef) and n.name in functions:
            body.append(n)
        elif isinstance(n, ast.Assign) and assigns:
            names = {t.id if isinstance(t, ast.Name) else getattr(getattr(t, "value", None), "id", None) for t in n.targets}
            if names & set(assigns):
                body.append(n)
    return body


def cv2_shim():
    from oracle import cv2_resize

    def resize(img, dsize, interpolation):
        if np.asarray(img).size == 0:
            raise EmptyImage()
        return cv2_resize.resize(np.asarray(img, np.float32), dsize, interpolation=interpolation)

    def warpAffine(img, matrix, dsize):
        assert np.asarray(img).dtype == np.float32, "the image reaching warpAffine is %s" % np.asarray(img).dtype
        return WR.warpAffine(img, matrix, dsize)

    return types.SimpleNamespace(INTER_NEAREST=cv2_resize.INTER_NEAREST, resize=resize, warpAffine=warpAffine, getRotationMatrix2D=WR.getRotationMatrix2D)


def script(rnd, form, draws):
    if draws is None:
        return
    o1, o2, o3, o4, rot, scale = draws
    rnd.queue += [("randint", int(o)) for o in (o1, o2, o3, o4)] + [("randint", int(rot))]
    if form == "itop":
        r = scale - 0.5
        assert r * 1.0 + 0.5 == scale, scale
        rnd.queue.append(("rand", r))
    else:
        k = int(round(scale * 1000))
        assert k / 1000 == scale, scale
        rnd.queue.append(("randint", k))


def run_itop():
    import torch
    rnd = Scripted()
    consts = dict(fx=286, fy=-286, u0=160, v0=120, keypointsNumber=15, RandCropShift=5, RandshiftDepth=1, RandRotate=10, RandScale=(1.0, 0.5),
                  xy_thres=120, depth_thres=0.4)
    path = os.path.join(A2J_DIR, "itop_train_64.py")
    fns = cut(path, functions=("dataPreprocess", "transform", "pixel2world", "world2pixel", "errorCompute", "writeTxt"))
    box_stmts = cut(path, assigns=("centre_train_world", "centerlefttop_train", "centerrightbottom_train", "train_lefttop_pixel", "train_rightbottom_pixel"))
    assert len(fns) == 6 and len(box_stmts) == 9, (len(fns), len(box_stmts))
    out = {}
    centres = TC.itop_centres()
    kp = TC.itop_keypoints()
    frames = {k: TC.frames(k) for k in TC.SETS}
    mean, std = np.array([TC.ITOP_MEAN], np.float32), np.array([TC.ITOP_STD], np.float32)
    assert np.float32(TC.C_HI) + np.float32(0.4) == np.float32(3.0) and np.float32(TC.C_LO) - np.float32(0.4) == np.float32(2.0)
    for f, y, x, v in TC.SPECIALS:
        got = frames["a"][f, y, x]
        assert (np.isnan(got) and np.isnan(v)) or got == v
    small, large, labels, flags, nans = [], [], [], [], []
    lts, rbs = np.zeros((len(TC.ITOP_CASES), 1, 3), np.float32), np.zeros((len(TC.ITOP_CASES), 1, 3), np.float32)
    g = None
    for i, (name, fset, fi, lt, rb, c, draws, (cw, ch)) in enumerate(TC.ITOP_CASES):
        g = dict(consts, np=NumpyWith(rnd), cv2=cv2_shim(), torch=torch, os=os, cropWidth=cw, cropHeight=ch)
        exec(compile(ast.Module(body=fns, type_ignores=[]), "itop_train_64", "exec"), g)
        g["center_train"] = centres
        exec(compile(ast.Module(body=box_stmts, type_ignores=[]), "itop_train_64_boxes", "exec"), g)
        lt_all, rb_all = g["train_lefttop_pixel"].copy(), g["train_rightbottom_pixel"].copy()
        assert lt_all.dtype == np.float32
        out["itop_boxes_lefttop"], out["itop_boxes_rightbottom"] = lt_all.copy(), rb_all.copy()
        if lt is not None:
            lt_all[i, 0, :2], rb_all[i, 0, :2] = lt, rb
        lts[i], rbs[i] = lt_all[i], rb_all[i]
        script(rnd, "itop", draws)
        img = frames[fset][fi].astype(float)
        H, W = img.shape
        if name in ("no_augment_hi", "no_augment_lo"):      # a pixel exactly at the bound lies in the box
            bound = 3.0 if name.endswith("hi") else 2.0
            assert (img[int(lt[1]):int(rb[1]), int(lt[0]):int(rb[0])] == bound).any()
        try:
            with np.errstate(all="ignore"):
                data, label = g["dataPreprocess"](i, img, kp, centres, mean, std, lt_all, rb_all, 120, 0.4, draws is not None)
            crop, label, flag = data.numpy()[0], label.numpy(), 0
            assert crop.dtype == np.float32 and crop.shape == (ch, cw)
        except EmptyImage:
            crop, label, flag = np.zeros((ch, cw), np.float32), np.zeros((15, 3), np.float32), 1
        assert not rnd.queue
        (large if cw == TC.LARGE else small).append(crop)
        labels.append(label)
        flags.append(flag)
        nans.append(int(np.isnan(crop).sum()))
        assert (nans[-1] > 0) == (name in TC.NAN_CASES), (name, nans[-1])
    out.update(itop_names=np.array([c[0] for c in TC.ITOP_CASES]), itop_crops=np.stack(small), itop_crops_large=np.stack(large), itop_labels=np.stack(labels),
               itop_flags=np.array(flags, np.int32), itop_nan_count=np.array(nans, np.int64), itop_lefttop=lts, itop_rightbottom=rbs,
               itop_draw_log=np.array(rnd.log[:7]))
    assert flags == [1 if c[0] == "empty" else 0 for c in TC.ITOP_CASES]
    # the map-back: writeTxt's file and errorCompute's number
    votes, target, mcentres = TC.map_back_inputs()
    d = tempfile.mkdtemp(prefix="a2j_txt_")
    try:
        g.update(cropWidth=TC.LARGE, cropHeight=TC.LARGE, save_dir=d, result_file="result.txt", np=np)
        exec(compile(ast.Module(body=fns, type_ignores=[]), "itop_train_64", "exec"), g)
        with np.errstate(all="ignore"):
            g["writeTxt"](votes.copy(), mcentres.copy())
            err_ref = g["errorCompute"](votes.copy(), target.copy(), mcentres.copy())
        text = open(os.path.join(d, "result.txt")).read()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    rows = np.array([[float(v) for v in line.split()] for line in text.splitlines()], dtype=np.float32)
    assert rows.shape == (len(votes), 45)
    # the error through writeTxt's box: errorCompute's own tail (:498-503) on the rows the reference wrote
    labels_w = g["pixel2world"](target.copy(), 286, -286, 160, 120)
    outputs_w = g["pixel2world"](rows.reshape(len(votes), 15, 3).copy(), 286, -286, 160, 120)
    err = np.mean(np.sqrt(np.sum((labels_w - outputs_w) ** 2, axis=2)))
    out.update(txt_rows=rows, txt_text=np.array(text), err_reference=np.float32(err_ref), err_default=np.float32(err))
    assert np.asarray(err_ref).dtype == np.float32 and np.isfinite(err_ref) and np.isfinite(err)
    return out


def run_box(fname, tag, swap):
    import torch
    rnd = Scripted()
    fns = cut(os.path.join(A2J_DIR, fname), functions=("dataPreprocess", "transform"))
    assert len(fns) == 2
    bnd, k2, k3 = TC.box_arrays()
    frames = TC.frames("b")
    mask, bg = TC.masks_and_backgrounds("b")
    d = tempfile.mkdtemp(prefix="a2j_box_")
    small, large, labels, flags = [], [], [], []
    try:
        for sub in ("depth", "seg", "bg"):
            os.mkdir(os.path.join(d, sub))
        ids = []
        for i, case in enumerate(TC.BOX_CASES):
            ids.append("%d.npy" % i)
            np.save(os.path.join(d, "depth", ids[-1]), frames[case[1]])
            np.save(os.path.join(d, "seg", ids[-1]), mask[case[1]])
            np.save(os.path.join(d, "bg", ids[-1]), bg[case[1]])
        for i, (name, fi, box, draws, (cw, ch)) in enumerate(TC.BOX_CASES):
            g = dict(np=NumpyWith(rnd), cv2=cv2_shim(), torch=torch, os=os, cropWidth=cw, cropHeight=ch, imgWidth=TC.IMG_WH_B[0], imgHeight=TC.IMG_WH_B[1],
                     MEAN=3, STD=2, keypointsNumber=15, RandCropShift=5, RandshiftDepth=0.01, RandRotate=10, train_image_ids=ids, test_image_ids=[],
                     maskDir=os.path.join(d, "seg"), bgDir=os.path.join(d, "bg"), bg_list=[{"file_name": n} for n in ids], BgImgFrames=len(ids))
            exec(compile(ast.Module(body=fns, type_ignores=[]), fname, "exec"), g)
            script(rnd, "box", draws)
            try:
                with np.errstate(all="ignore"):
                    data, label = g["dataPreprocess"](i, os.path.join(d, "depth"), k2, k3, bnd, "TRAIN", draws is not None)
                crop, label, flag = data.numpy()[0], label.numpy(), 0
                assert crop.dtype == np.float32 and crop.shape == (ch, cw)
            except EmptyImage:
                crop, label, flag = np.zeros((ch, cw), np.float32), np.zeros((15, 3), np.float32), 1
            assert not rnd.queue and not np.isnan(crop).any()
            if cw == TC.LARGE:
                if not swap:
                    large.append(crop)
            else:
                small.append(crop)
            labels.append(label)
            flags.append(flag)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out = {tag + "_crops": np.stack(small), tag + "_labels": np.stack(labels), tag + "_flags": np.array(flags, np.int32)}
    if not swap:
        out.update(box_names=np.array([c[0] for c in TC.BOX_CASES]), box_crops_large=np.stack(large), box_draw_log=np.array(rnd.log[:7]))
    return out


def generate():
    np.float = float
    np.int = int
    out = {"numpy_version": np.array(np.__version__)}
    out.update(run_itop())
    out.update(run_box("train_a2j_base.py", "box", False))
    out.update(run_box("train_a2j_bgaug_new.py", "bg", True))
    assert np.array_equal(out["box_labels"], out["bg_labels"]) and not np.array_equal(out["box_crops"], out["bg_crops"])
    return out


def _same(a, b):
    if sorted(a.keys()) != sorted(b.keys()):
        return "keys differ: %s" % sorted(set(a.keys()) ^ set(b.keys()))
    for k in a.keys():
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            return "%s: %s %s vs %s %s" % (k, x.shape, x.dtype, y.shape, y.dtype)
        if not np.array_equal(x, y, equal_nan=x.dtype.kind == "f"):
            return "%s differs" % k
    return None


if __name__ == "__main__":
    got = generate()
    path = os.path.join(HERE, NAME)
    if "--check" in sys.argv:
        why = _same(got, dict(np.load(path)))
        if why:
            print("golden check FAILED: %s: %s" % (NAME, why))
            sys.exit(1)
        assert os.path.getsize(path) < 1 << 20
        print("golden check ok: %s regenerates" % NAME)
    else:
        np.savez_compressed(path, **got)
        size = os.path.getsize(path)
        print(NAME, size, "bytes; numpy", np.__version__)
        assert size < 1 << 20, "%s is %d bytes, over 1 MiB" % (NAME, size)
