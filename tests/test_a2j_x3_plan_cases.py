"""bf16x3 A2J inference: the nets compile, and every kernel instance the deployed plans launch is one that tests/test_gpu_a2j_x3.py compares with
fp64 -- without a GPU.

Each net is compiled on a context without a device (pn_create(-1)), where conv_plan.h decides kernel, cout block and tile.

  a. every convolution of the bf16x3 nets the engines and scripts compile (288 x 288 at max_batch 32, 16 and 2, crop 96 at max_batch 2) has the
     instance key of a step that a row of tests/a2j_x3_plan_cases.py compares;
  b. every input plane of every convolution of those nets and of the rows is a multiple of 64 (the K loop wraps to the hi plane per 64-channel chunk);
  c. the stem and the max pool are two launches, the rest of the step list is the bf16 net's, convolution by convolution;
  d. the bf16 and fp32 A2J step lists are the committed ones (tests/golden/net_steps.json.gz): the mode changes no existing plan.
"""
import ctypes as C
import functools
import importlib.util
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import a2j_plan_cases as APC  # noqa: E402
import a2j_x3_plan_cases as XPC  # noqa: E402
from popnet_amd import _lib  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_net_steps", os.path.join(HERE, "golden", "make_golden_net_steps.py"))
MK = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MK)


@functools.lru_cache(None)
def _ctx():
    return _lib.lib().pn_create(-1)


@functools.lru_cache(None)
def net(prec, max_batch, H, W):
    """(pn_net_step_info(-1), [pn_net_step_info(k)]) of one A2J net."""
    L = _lib.lib()
    h = MK.compile_net(_ctx(), ("a2j", "a2j", prec, max_batch, H, W, False, {}))
    try:
        buf = C.create_string_buffer(1 << 16)
        out = []
        for k in range(-1, L.pn_net_num_steps(h)):
            assert L.pn_net_step_info(h, k, buf, len(buf)) == 0, (k, MK.last_error(_ctx()))
            out.append(json.loads(buf.value.decode()))
        return out[0], out[1:]
    finally:
        L.pn_net_destroy(h)


def steps(max_batch, H, W, prec=XPC.PREC):
    return net(prec, max_batch, H, W)[1]


def net_keys(max_batch, H, W):
    return {APC.instance_key(c) for st in steps(max_batch, H, W) if st["type"] == "conv" for c in st["convs"]}


def compared(cases):
    out = set()
    for _, prec, H, W, B, mb, which in cases:
        out |= APC.compared_keys(steps(mb, H, W), which)
    return out


def uncovered_deployed(cases):
    have = compared(cases)
    return [(H, W, mb, k) for H, W, mb in XPC.DEPLOYED for k in sorted(net_keys(mb, H, W) - have)]


def test_the_table_is_well_formed():
    for id_, prec, H, W, B, mb, which in XPC.CASES:
        assert id_ == APC.case_id(prec, H, W, B, mb) and prec == "bf16x3" and H % 16 == 0 and W % 16 == 0 and 1 <= B <= mb
        info, st = net(prec, mb, H, W)
        assert info["prec"] == "bf16x3" and info["max_batch"] == mb and (info["in_h"], info["in_w"]) == (H, W)
        # a row names no key that its own net does not launch, and selects something
        assert APC.key_part(which) <= net_keys(mb, H, W), (id_, sorted(APC.key_part(which) - net_keys(mb, H, W)))
        assert any(APC.selects(which)(s) for s in st), id_
    assert XPC.SMALL[6] == APC.ALL
    # the 288 x 288 rows name exactly the keys that the rows before them do not compare
    small = net_keys(3, 80, 96)
    assert set(XPC.KEYS_288_MAX_BATCH_32) == net_keys(32, 288, 288) - small
    assert set(XPC.KEYS_288_MAX_BATCH_2) == net_keys(2, 288, 288) - small - net_keys(32, 288, 288)
    # the wider pitch classes of the dilated steps
    for id_, prec, H, W, B, mb, which in XPC.WIDE:
        dil = [s for s in steps(mb, H, W) if APC.is_dilated(s)]
        assert len(dil) == 2 and all(c["pitch"] == XPC.WIDE_PITCH[W] and c["dil"] == 2 for s in dil for c in s["convs"]), [s["kernel"] for s in dil]


def test_a_every_convolution_of_the_deployed_plans_is_compared():
    miss = uncovered_deployed(XPC.CASES)
    assert not miss, "%d convolution instances of the deployed bf16x3 A2J nets are compared by no row of tests/a2j_x3_plan_cases.py:\n%s" % (
        len(miss), "\n".join("  %dx%d max_batch %d: %s" % m for m in miss))
    have = {k[0] for k in compared(XPC.CASES)}
    for H, W, mb in XPC.DEPLOYED:
        labels = {st["kernel"] for st in steps(mb, H, W) if st["type"] == "conv"}
        print("A2J bf16x3 %dx%d max_batch %d: %d steps, %d convolution labels, %d compared by no row" % (H, W, mb, len(steps(mb, H, W)), len(labels), len(labels - have)))
        assert labels <= have
    # the guard can fail: without the max_batch 32 row its keys are reported
    miss = uncovered_deployed([c for c in XPC.CASES if c is not XPC.LARGE_32])
    assert {m[3] for m in miss if m[:3] == (288, 288, 32)} == set(XPC.KEYS_288_MAX_BATCH_32)


def test_b_every_input_plane_is_a_multiple_of_64():
    nets = {(mb, H, W) for H, W, mb in XPC.DEPLOYED} | {(c[5], c[2], c[3]) for c in XPC.CASES}
    for mb, H, W in sorted(nets):
        info, st = net(XPC.PREC, mb, H, W)
        planes = [info["bufs"][c["in_buf"]][2] for s in st if s["type"] == "conv" for c in s["convs"]]
        assert len(planes) == 67 and all(p % 64 == 0 for p in planes), (mb, H, W, sorted(set(planes)))
        # ... and the heads' output planes are the 240 / 480 channels the vote reads as [hi | lo] rows
        outs = sorted(info["bufs"][c["out_buf"]][2] for s in st if APC.is_output(s) for c in s["convs"])
        assert outs == [240, 240, 480]


@pytest.mark.parametrize("shape", [(3, 80, 96), (32, 288, 288), (2, 288, 288)], ids=["80x96", "288_max_batch32", "288_max_batch2"])
def test_c_the_step_list_is_the_bf16_one_with_stem_and_pool_apart(shape):
    x3, bf = steps(*shape), steps(*shape, prec="bf16")
    assert [s["type"] for s in x3[:2]] == ["stem", "pool"] and x3[0]["kernel"] == "stem7x7_mfma_kernel<x3>" and x3[0]["pool_buf"] == -1
    assert x3[1]["kernel"] == "pool_kernel<1, split>" and x3[1]["mode"] == 1 and x3[1]["in_buf"] == x3[0]["out_buf"]
    assert bf[0]["kernel"] == "stem7x7_pool_kernel" and bf[0]["pool_buf"] == x3[1]["out_buf"]
    names = lambda st: [(c["w"], c["ks"], c["stride"], c.get("dil", 1), c["in_buf"], c["res_buf"], c["out_buf"]) for s in st if s["type"] == "conv" for c in s["convs"]]
    assert names(x3) == names(bf) and len(names(x3)) == 67
    assert not any("blocked_acc" in c for s in x3 if s["type"] == "conv" for c in s["convs"])          # blocked accumulation stays fp32-only


def test_d_the_bf16_and_fp32_step_lists_are_the_committed_ones():
    recorded = MK.load()
    rows = [n for n in MK.nets() if n[1] == "a2j"]
    assert len(rows) == len(APC.CASES) and {n[2] for n in rows} == {"bf16", "fp32"}
    for n in rows:
        assert MK.net_steps(_ctx(), n) == recorded[n[0]], n[0]
