"""The committed recipe of tests/golden/augment.npz reproduces it.

tests/golden/make_golden_augment.py imports the reference (read-only) and runs its own Rotate / RenderDepth / Crop / Resize classes
through both trainers' KDH3D_Keypoints.__getitem__; `--check` writes into a scratch directory and compares with the committed file,
array by array, bit for bit.  The reference tree exists only in the build container, so the test skips on the GPU box."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.isdir("/root/reference/third_party_methods"), reason="needs the reference tree")
def test_recipe_regenerates_the_augmentation_golden_identically():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_augment.py"), "--check"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "golden check ok: 1 files regenerate identically" in r.stdout
