"""bb64s_strip_kernel keeps every register in the register file: no VGPR spill, no scratch memory.

Its tile loop holds two fully unrolled conv1 bodies (the first tile of a column segment, the carried tiles) and one conv2 body; a
register the compiler spills would be reloaded from scratch inside that loop behind an s_waitcnt vmcnt(0).  As
tests/test_bb64_resources.py does for bb64_kernel, the translation unit is compiled device-only to assembly with the flags of
popnet_amd/build.py (hipcc cross-compiles without a GPU) and two metadata fields of the kernel are read -- nothing else of the
assembly is looked at."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_module():
    spec = importlib.util.spec_from_file_location("_popnet_build_flags", os.path.join(ROOT, "popnet_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def strip_metadata(tmp_path_factory):
    b = _build_module()
    if not os.path.exists(b.HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("bb64s") / "bb64s_inst.s")
    cmd = [b.HIPCC] + b.FLAGS + ["--cuda-device-only", "-S", os.path.join(b.CSRC, "bb64s_inst.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kernels = {}
    name = None
    for line in open(out):
        m = re.match(r"\s*(?:- )?\.(name|vgpr_spill_count|private_segment_fixed_size):\s*(\S+)", line)
        if not m:
            continue
        if m.group(1) == "name":
            name = m.group(2)
        elif name is not None and "bb64s_strip_kernel" in name:
            kernels.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return kernels


def test_the_strip_kernel_is_the_only_kernel_of_its_translation_unit(strip_metadata):
    assert len(strip_metadata) == 1, sorted(strip_metadata)
    for name, fields in strip_metadata.items():
        assert set(fields) == {"vgpr_spill_count", "private_segment_fixed_size"}, (name, fields)


def test_the_strip_kernel_spills_no_vgpr_and_uses_no_scratch(strip_metadata):
    for name, fields in strip_metadata.items():
        assert fields["vgpr_spill_count"] == 0, (name, fields)
        assert fields["private_segment_fixed_size"] == 0, (name, fields)
