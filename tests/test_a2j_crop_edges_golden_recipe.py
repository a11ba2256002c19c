"""The committed recipe of the A2J crop-sweep golden reproduces it: tests/golden/make_golden_a2j_crop_edges.py cuts dataPreprocess out of the
reference's script (read-only), runs it on every row of tests/a2j_crop_cases.py and regenerates a2j_crop_edges.npz; `--check` compares with
the committed file.  The reference tree exists only where the goldens are made, so the regeneration skips elsewhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "third_party_methods", "A2J_experiments")), reason="needs the reference tree")
def test_a2j_crop_edges_golden_regenerates():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_a2j_crop_edges.py"), "--check"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "golden check ok: a2j_crop_edges.npz regenerates" in r.stdout


def test_a2j_crop_edges_golden_is_small_and_holds_digests_only():
    path = os.path.join(ROOT, "tests", "golden", "a2j_crop_edges.npz")
    assert os.path.getsize(path) < 128 << 10
    g = np.load(path)
    for k in g.files:
        if k.endswith("_sha256"):
            assert g[k].dtype == np.uint8 and g[k].shape[1] == 32 and len(g[k]) == len(g[k[:-7] + "_flags"])
