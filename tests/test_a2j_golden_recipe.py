"""The committed recipe of the A2J goldens reproduces them: tests/golden/make_golden_a2j.py imports the reference (read-only, its
weight download patched out) and regenerates a2j.npz and a2j_crops.npz; `--check` compares with the committed files.  The reference
tree exists only where the goldens are made, so the regeneration skips elsewhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import a2j_cases as AC  # noqa: E402

REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "third_party_methods", "A2J_experiments")), reason="needs the reference tree")
def test_a2j_goldens_regenerate():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_a2j.py"), "--check"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "golden check ok: 2 files regenerate" in r.stdout


def test_a2j_golden_files_are_small_and_complete():
    for name in ("a2j.npz", "a2j_crops.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < 1 << 20
    g = np.load(os.path.join(ROOT, "tests", "golden", "a2j.npz"))
    assert int(g["seed"]) == AC.SEED and len(g["keys"]) == 410
    H, W, B = AC.SMALL
    K = (H // 16) * (W // 16) * 16
    assert g["s_cls"].shape == (B, K, 15) and g["s_reg"].shape == (B, K, 15, 2) and g["s_joints"].shape == (B, 15, 3)
    assert g["l_joints"].shape == (AC.LARGE[2], 15, 3)
    assert float(g["s_max_softmax"]) < 0.05 and float(g["l_max_softmax"]) < 0.05      # the vote sums over many anchors
    for k in g.files:
        if k.endswith("_tol"):
            assert 0 < float(g[k]) < 1e-2, (k, float(g[k]))
    c = np.load(os.path.join(ROOT, "tests", "golden", "a2j_crops.npz"))
    assert [str(n) for n in c["names"]] == [n for n, _ in AC.CROP_CASES] and c["crops"].shape == (len(AC.CROP_CASES), 288, 288)
    assert not c["crops"][-1].any() and not c["crops"][-2].any()                       # conf <= 0.01: all-zero crops
