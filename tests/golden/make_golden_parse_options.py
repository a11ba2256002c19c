#!/usr/bin/env python
"""Golden vectors of the pose parse outside its default arguments: the reference's own NMS and paf_to_pose
(third_party_methods/lib/utils/paf_to_pose.py:75-153, :354-377), imported through make_golden.py's shims (cv2.resize goes to
oracle/cv2_resize.py) and run with the installed scipy, and numpy's BLAS pinned to a core type without fused multiply-add (see below), on the maps of the hand-built cases in tests/parse_cases.py.

    python tests/golden/make_golden_parse_options.py          # rewrites tests/golden/parse_options.npz
    python tests/golden/make_golden_parse_options.py --check  # regenerates into a scratch dir and compares (tests/test_parse_options_golden_recipe.py)

Stored per (case, option set) -- the lists live in tests/parse_options_reference.py:
  nms/<case>/f<f>_r<refine>_g<gauss>/peaks [N, 4] float64 (x, y, score, id), /counts [J] int32
  parse/<case>/f<f>_n<n>/joint_list [N, 5], /assoc [P, J + 2], /conn [M, 6] (limb, src_id, dst_id, score, i, j) float64
plus gauss_weights (the 13 distinct weights of scipy's sigma-3 kernel), scipy_version, blas_coretype and the case / option lists.  Only data leaves this script.
"""
import os
import sys
import tempfile
from types import SimpleNamespace

# The one BLAS call of the path is intermed_paf.dot(limb_dir) (paf_to_pose.py:221).  numpy's OpenBLAS picks its kernels by the CPU it runs on, and
# they do not agree in the last bit: on every core type tried (Katmai, Nehalem, Sandybridge, Haswell, Zen) the product is x * dx + y * dy with both
# products rounded -- oracle/parse_paf.py's form -- while the AVX-512 kernel (SkylakeX) fuses one multiply-add per row, in an order that depends on
# the row's position in a block of four.  A fixture must not depend on the CPU of the machine that wrote it, so the core type is pinned, before
# numpy loads, to one whose instruction set has no fused multiply-add at all.
os.environ["OPENBLAS_CORETYPE"] = "Nehalem"

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402


def ref_cfg(f, n):
    return SimpleNamespace(MODEL=SimpleNamespace(DOWNSAMPLE=f, NUM_KEYPOINTS=15),
                           TEST=SimpleNamespace(THRESH_HEATMAP=0.1, THRESH_PAF=0.05, NUM_INTERMED_PTS_BETWEEN_KEYPOINTS=n))


def golden_parse_options():
    import scipy
    from scipy.ndimage import _filters
    import cv2
    import lib.utils.paf_to_pose as ref
    import parse_cases as PC
    import parse_options_reference as PR

    out = {}
    w = _filters._gaussian_kernel1d(3.0, 0, 12)[::-1]       # gaussian_filter1d hands correlate1d the reversed kernel
    assert len(w) == 25 and all(w[k] == w[24 - k] for k in range(13))
    out["gauss_weights"] = np.asarray(w[:13], dtype=np.float64)
    out["scipy_version"] = np.array(scipy.__version__)
    out["blas_coretype"] = np.array(os.environ["OPENBLAS_CORETYPE"])

    # ---- NMS: every option set on every case; NMS(heat, config=cfg) with nothing else is the (1, True, False) entry ----
    def run_nms(c, f, refine, gauss):
        cfg = ref_cfg(f, 10)
        if (f, refine, gauss) == (1, True, False):
            per_type = ref.NMS(c.heat.copy(), config=cfg)
        else:
            per_type = ref.NMS(c.heat.copy(), upsampFactor=float(f), bool_refine_center=refine, bool_gaussian_filt=gauss, config=cfg)
        peaks, counts = PR.flat_peaks(per_type)
        key = "nms/%s/%s" % (c.name, PR.nms_key(f, refine, gauss))
        out[key + "/peaks"], out[key + "/counts"] = peaks, counts
        return len(peaks)

    for name in PR.NMS_CASES:
        c = PC.case(name)
        n = [run_nms(c, *opt) for opt in PR.NMS_OPTIONS]
        print("nms   %-14s %dx%d peaks %d" % (name, c.h, c.w, n[0]))
    run_nms(PC.case(PR.NMS_BIG[0]), *PR.NMS_BIG[1])

    # ---- the whole parse; find_connected_joints is wrapped to keep its return value, cv2.resize of the PAF tensor is computed once per factor ----
    keep = {}
    real_fcj, real_resize = ref.find_connected_joints, cv2.resize

    def fcj(*a, **k):
        keep["conn"] = real_fcj(*a, **k)
        return keep["conn"]

    def resize(img, *a, **k):
        if img.ndim != 3:
            return real_resize(img, *a, **k)
        key = (keep["case"], k["fx"])
        if key not in keep:
            keep[key] = real_resize(img, *a, **k)
        return keep[key]

    ref.find_connected_joints, ref.cv2 = fcj, SimpleNamespace(resize=resize, INTER_CUBIC=cv2.INTER_CUBIC)
    try:
        for name in PR.PARSE_CASES:
            c = PC.case(name)
            keep["case"] = name
            for f, n in PR.PARSE_OPTIONS:
                jl, assoc = ref.paf_to_pose(c.heat.copy(), c.paf.copy(), ref_cfg(f, n))
                key = "parse/%s/%s" % (name, PR.parse_key(f, n))
                out[key + "/joint_list"] = np.asarray(jl, dtype=np.float64).reshape(-1, 5)
                out[key + "/assoc"] = np.asarray(assoc, dtype=np.float64).reshape(-1, 17)
                out[key + "/conn"] = PR.flat_connections(keep["conn"])
                print("parse %-14s f %2d n %2d peaks %3d connections %3d persons %2d" % (name, f, n, len(out[key + "/joint_list"]), len(out[key + "/conn"]),
                                                                                       len(out[key + "/assoc"])))
            for k in [k for k in keep if isinstance(k, tuple)]:
                del keep[k]
    finally:
        ref.find_connected_joints, ref.cv2 = real_fcj, cv2
    out["nms_cases"], out["parse_cases"] = np.array(PR.NMS_CASES), np.array(PR.PARSE_CASES)
    out["nms_options"] = np.array([(f, int(r), int(g)) for f, r, g in PR.NMS_OPTIONS], dtype=np.int32)
    out["parse_options"] = np.array(PR.PARSE_OPTIONS, dtype=np.int32)
    np.savez_compressed(os.path.join(MG.OUT, "parse_options.npz"), **out)


if __name__ == "__main__":
    assert os.path.isdir(MG.REF), "the reference tree is needed to (re)generate golden vectors"
    check = "--check" in sys.argv[1:]
    if check:
        MG.OUT = tempfile.mkdtemp(prefix="popnet_golden_parse_options_check_")
    MG.install_shims()
    golden_parse_options()
    if check:
        fails = MG.check_outputs(MG.OUT)
        if fails:
            print("GOLDEN CHECK FAILED:\n  " + "\n  ".join(fails))
            sys.exit(1)
        print("golden check ok: %d files regenerate identically" % len(os.listdir(MG.OUT)))
