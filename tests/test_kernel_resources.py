"""bb64x3_kernel and the planes / fp32 weight-gradient kernels keep every register in the register file and fit their occupancy budget.

bb64x3_kernel (eight waves per workgroup, one workgroup per CU) and wgrad_stream_kernel / wgrad_f32_kernel (__launch_bounds__(256, 2): two
waves per SIMD) are built from shared device functions (bx_kloop; wg_begin, wg_walk, wg_store), so a change in one of those reaches the register
allocation of every kernel that uses it.  Two waves per SIMD leave 256 VGPRs per lane; bb64x3_kernel and wgrad_stream_kernel<3, 2> sit at 234.  A
spilled register is reloaded from scratch behind an s_waitcnt vmcnt(0), which also waits for the LDS-DMA these kernels keep in flight.  The two
translation units are compiled device-only to assembly with the flags of popnet_amd/build.py (hipcc cross-compiles without a GPU) and four
metadata fields of each kernel are read -- nothing else of the assembly is looked at."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# translation unit -> the kernels checked in it, as the start of their mangled names (the template arguments follow: I = <, Li3ELi2E = 3, 2)
KERNELS = {
    "bb64x3_inst.hip": ["_Z13bb64x3_kernel"],
    "trainx.hip": ["_ZN2tx19wgrad_stream_kernelILi3ELi2EEE", "_ZN2tx19wgrad_stream_kernelILi1ELi2EEE",
                   "_ZN2tx16wgrad_f32_kernelILi3ELi2EEE", "_ZN2tx16wgrad_f32_kernelILi1ELi2EEE"],
}
FIELDS = ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")


def _build_module():
    spec = importlib.util.spec_from_file_location("_popnet_build_flags", os.path.join(ROOT, "popnet_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel prefix: [fields of every kernel whose name starts with it]}"""
    b = _build_module()
    if not os.path.exists(b.HIPCC):
        pytest.skip("hipcc not found")
    tmp = tmp_path_factory.mktemp("kernel_resources")
    found = {}
    for unit, prefixes in KERNELS.items():
        out = str(tmp / (unit[:-4] + ".s"))
        r = subprocess.run([b.HIPCC] + b.FLAGS + ["--cuda-device-only", "-S", os.path.join(b.CSRC, unit), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for p in prefixes:
            found[p] = []
        entry = None
        for line in open(out):
            m = re.match(r"\s*(?:- )?\.(name|%s):\s*(\S+)" % "|".join(FIELDS), line)
            if not m:
                continue
            if m.group(1) == "name":              # a kernel's .name comes before its three fields
                hits = [p for p in prefixes if m.group(2).startswith(p)]
                entry = {"name": m.group(2)} if hits else None
                if hits:
                    found[hits[0]].append(entry)
            elif entry is not None:
                entry[m.group(1)] = int(m.group(2))
    return found


@pytest.mark.parametrize("kernel", [p for ps in KERNELS.values() for p in ps])
def test_kernel_is_compiled_once_without_spills_inside_its_vgpr_budget(metadata, kernel):
    entries = metadata[kernel]
    assert len(entries) == 1, (kernel, entries)
    fields = entries[0]
    assert set(fields) == set(FIELDS) | {"name"}, fields
    assert fields["vgpr_spill_count"] == 0, fields
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields["vgpr_count"] <= 256, fields
