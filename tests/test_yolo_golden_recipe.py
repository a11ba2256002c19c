"""The committed recipe of the YoloPoseNet training goldens reproduces them: tests/golden/make_golden_yolo.py imports the reference
(read-only) and regenerates yolo_train_step.npz and yolo_targets.npz; `--check` writes into a scratch directory and compares with the
committed files bit for bit.  The reference tree exists only where the goldens are made, so the test skips elsewhere."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden import REF  # noqa: E402


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "third_party_methods")), reason="needs the reference tree")
def test_yolo_goldens_regenerate_identically():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_yolo.py"), "--check"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "golden check ok: 2 files regenerate identically" in r.stdout


def test_yolo_golden_files_are_small_and_complete():
    import numpy as np
    for name in ("yolo_train_step.npz", "yolo_targets.npz"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < 1 << 20
    t = np.load(os.path.join(ROOT, "tests", "golden", "yolo_targets.npz"))
    assert sorted(str(n) for n in t["names"]) == sorted(["empty", "one", "eight", "shared_cell", "outside", "anchor_tie"])
    g = np.load(os.path.join(ROOT, "tests", "golden", "yolo_train_step.npz"))
    assert g["s0_terms"].shape == g["s0_plain_terms"].shape == (4,) and not any(k.split("/", 1)[-1].startswith("model0.layer3") for k in g.files)
