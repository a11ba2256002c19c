"""The committed recipe of the A2J training-crop golden reproduces it: tests/golden/make_golden_a2j_traincrop.py cuts dataPreprocess,
transform, errorCompute and writeTxt out of the reference's scripts (read-only) and regenerates a2j_traincrop.npz; `--check` compares with
the committed file.  The reference tree exists only where the goldens are made, so the regeneration skips elsewhere."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "third_party_methods", "A2J_experiments")), reason="needs the reference tree")
def test_a2j_traincrop_golden_regenerates():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_a2j_traincrop.py"), "--check"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "golden check ok: a2j_traincrop.npz regenerates" in r.stdout


def test_a2j_traincrop_golden_is_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "a2j_traincrop.npz")) < 1 << 20
