"""conv4_kernel keeps every register in the register file: no spilled VGPR, no scratch memory.

conv4_kernel runs at 2 waves per SIMD with 112 accumulator registers per lane and one barrier per k-step; a register the compiler spills
is reloaded from scratch inside that loop behind an s_waitcnt vmcnt(0), which also waits for the LDS-DMA the loop keeps in flight.  Its
epilogues are the shared ones of conv_common.h, so a change there reaches this kernel's register allocation.  The translation unit is
compiled device-only to assembly with the flags of popnet_amd/build.py (hipcc cross-compiles without a GPU) and the two metadata fields
of the kernel are read -- nothing else of the assembly is looked at."""
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
def conv4_metadata(tmp_path_factory):
    b = _build_module()
    if not os.path.exists(b.HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("conv4") / "conv4_inst.s")
    cmd = [b.HIPCC] + b.FLAGS + ["--cuda-device-only", "-S", os.path.join(b.CSRC, "conv4_inst.hip"), "-o", out]
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
        elif name is not None and "conv4_kernel" in name:
            kernels.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return kernels


def test_exactly_one_conv4_kernel_is_compiled(conv4_metadata):
    assert len(conv4_metadata) == 1, sorted(conv4_metadata)
    for name, fields in conv4_metadata.items():
        assert set(fields) == {"vgpr_spill_count", "private_segment_fixed_size"}, (name, fields)


def test_conv4_kernel_spills_no_vgpr_and_uses_no_scratch(conv4_metadata):
    for name, fields in conv4_metadata.items():
        assert fields["vgpr_spill_count"] == 0, (name, fields)
        assert fields["private_segment_fixed_size"] == 0, (name, fields)
