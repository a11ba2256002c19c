#!/usr/bin/env python
"""Generates tests/golden/a2j_crop_edges.npz by running the REFERENCE ITSELF -- dataPreprocess of
third_party_methods/A2J_experiments/a2j_test_pred_box_new.py:268-313, cut out of the script's syntax tree and executed with the globals it
reads, as tests/golden/make_golden_a2j.py does -- on every row of tests/a2j_crop_cases.py::rows, on the CPU.

    python tests/golden/make_golden_a2j_crop_edges.py            # rewrites tests/golden/a2j_crop_edges.npz
    python tests/golden/make_golden_a2j_crop_edges.py --check    # regenerates and compares (tests/test_a2j_crop_edges_golden_recipe.py)

Only data leaves this script: per frame set and crop size (64 x 48 and 50 x 37: every row; 288 x 288: the rows of large_index) one SHA-256
digest per crop (tests/a2j_crop_reference.py::digest, every NaN made one NaN first) and one flag per row, 1 where the reference raised --
the digest is then that of a zero crop.  The rows of hostile_rows (NaN, infinities, 1e12) are not run: on some of them the reference
allocates or loops without end; what they must give is the project's rule, not a recorded output.  cv2 is not installed: cv2.resize is the
restated INTER_NEAREST rule of oracle/cv2_resize.py, which raises on an empty image as cv2 does (there by a division by zero).
"""
import importlib.util
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import a2j_crop_cases as CC  # noqa: E402
import a2j_crop_reference as CR  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_a2j", os.path.join(HERE, "make_golden_a2j.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)
NAME = "a2j_crop_edges.npz"


def key(name, crop_wh):
    return "%s_%dx%d" % (name, crop_wh[0], crop_wh[1])


def run(frames, rows, crop_wh):
    """-> (digests [n, 32] uint8, flags [n] uint8) of the reference's dataPreprocess"""
    np.float = float
    g = MG.reference_data_preprocess()
    g.update(cropWidth=crop_wh[0], cropHeight=crop_wh[1], imgWidth=CC.IMG_WH[0], imgHeight=CC.IMG_WH[1])
    d = tempfile.mkdtemp(prefix="a2j_frames_")
    for f in range(frames.shape[0]):
        np.save(os.path.join(d, "%d.npy" % f), frames[f])
    g["test_image_ids"][:] = ["%d.npy" % int(r[0]) for r in rows]
    bnd = np.asarray(rows[:, 1:], dtype=np.float32)
    digests, flags = np.zeros((len(rows), 32), np.uint8), np.zeros((len(rows),), np.uint8)
    zero = np.zeros((crop_wh[1], crop_wh[0]), np.float32)
    try:
        for i in range(len(rows)):
            try:
                with np.errstate(invalid="ignore"):
                    crop = g["dataPreprocess"](i, d, bnd, "TEST")[0].numpy()[0]
            except Exception:
                crop, flags[i] = zero, 1
            assert crop.shape == zero.shape and crop.dtype == np.float32
            digests[i] = CR.digest(crop)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return digests, flags


def generate():
    out = {"numpy_version": np.array(np.__version__)}
    for name in CC.SETS:
        frames, rows = CC.frames(name), CC.rows(name)
        out["%s_rows" % name] = rows
        for crop_wh in CC.CROPS:
            out[key(name, crop_wh) + "_sha256"], out[key(name, crop_wh) + "_flags"] = run(frames, rows, crop_wh)
        out[key(name, CC.LARGE) + "_sha256"], out[key(name, CC.LARGE) + "_flags"] = run(frames, rows[CC.large_index(name)], CC.LARGE)
    return out


if __name__ == "__main__":
    got = generate()
    path = os.path.join(HERE, NAME)
    if "--check" in sys.argv:
        want = dict(np.load(path))
        bad = [k for k in sorted(set(got) | set(want)) if k != "numpy_version" and not (k in got and k in want and np.array_equal(got[k].view(np.uint8) if got[k].dtype.kind == "f" else got[k], want[k].view(np.uint8) if want[k].dtype.kind == "f" else want[k]))]
        if bad:
            print("golden check FAILED: %s: %s differ" % (NAME, bad))
            sys.exit(1)
        print("golden check ok: %s regenerates" % NAME)
    else:
        np.savez_compressed(path, **got)
        print(NAME, os.path.getsize(path), "bytes;", {k: int(v.sum()) for k, v in got.items() if k.endswith("_flags")})
