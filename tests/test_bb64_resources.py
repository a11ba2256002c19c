"""bb64_kernel keeps every register in the register file: no scratch memory in either instantiation.

A compute wave of the fused BasicBlock kernel is meant to issue MFMA and ds_read only; a register the compiler spills is
reloaded from scratch inside the per-tile loop behind an s_waitcnt vmcnt(0).  The translation unit is compiled device-only
to assembly with the flags of popnet_amd/build.py (hipcc cross-compiles without a GPU) and the two metadata fields of each
kernel are read -- nothing else of the assembly is looked at."""
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
def bb64_metadata(tmp_path_factory):
    b = _build_module()
    if not os.path.exists(b.HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("bb64") / "bb64_inst.s")
    cmd = [b.HIPCC] + b.FLAGS + ["--cuda-device-only", "-S", os.path.join(b.CSRC, "bb64_inst.hip"), "-o", out]
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
        elif name is not None and "bb64_kernel" in name:
            kernels.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return kernels


def test_both_bb64_instantiations_are_compiled(bb64_metadata):
    assert len(bb64_metadata) == 2, sorted(bb64_metadata)
    for name, fields in bb64_metadata.items():
        assert set(fields) == {"vgpr_spill_count", "private_segment_fixed_size"}, (name, fields)


def test_bb64_kernels_spill_no_vgpr_and_use_no_scratch(bb64_metadata):
    for name, fields in bb64_metadata.items():
        assert fields["vgpr_spill_count"] == 0, (name, fields)
        assert fields["private_segment_fixed_size"] == 0, (name, fields)
