"""The committed recipe of tests/golden/evalsets_inputs.npz and script_eval_data_{mpaug,mpaug_yolo,kdh3d,kdh3d_yolo}.json / .npz reproduces them.

tests/golden/make_golden_evalsets.py imports the reference (read-only) and runs its loaders -- generate_test_batch of the composed test
set, __getitem__ of the single-person sets -- and its four evaluation scripts on the fake tree of tests/evalsets_cases.py; `--check` writes into a scratch directory and
compares with the committed files, array by array and leaf by leaf, bit for bit.  The reference tree exists only in the build container, so the test skips
on the GPU box."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.isdir("/root/reference/third_party_methods"), reason="needs the reference tree")
def test_recipe_regenerates_the_evaluation_set_golden_identically():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_evalsets.py"), "--check"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "golden check ok: 9 files regenerate identically" in r.stdout
