"""The committed recipe of tests/golden/parse_options.npz reproduces it: tests/golden/make_golden_parse_options.py imports the reference
(read-only checkout) through make_golden.py's shims, regenerates the fixture into a scratch directory with `--check` and compares it with the
committed file array by array, bit for bit.  The reference tree exists only where the goldens are made, so the test skips elsewhere."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.isdir("/root/reference/third_party_methods"), reason="needs the reference tree")
def test_recipe_regenerates_the_parse_options_golden_identically():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_parse_options.py"), "--check"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "golden check ok: 1 files regenerate identically" in r.stdout
