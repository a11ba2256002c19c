"""The compiled step list of every inference net the GPU suites compile, against tests/golden/net_steps.json.gz -- without a GPU.

pn_net_finalize compiles a net on the host (net.hip::compile_net: levels, planner decisions, fusions, steps, packed images) and then uploads it; on a
context without a device it stops after the first phase and pn_net_step_info answers.  The recorded lists were dumped on an MI355X by the last commit
whose finalize needed a device (tests/golden/make_golden_net_steps.py has the recipe and the list of nets); every net must compile to the same list
here, step by step, and with a device (one GPU test, a few nets, no forward).
"""
import ctypes as C
import importlib.util
import json
import os

import pytest

from popnet_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_net_steps", os.path.join(HERE, "golden", "make_golden_net_steps.py"))
MK = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MK)

NETS = MK.nets()
PN_ERR_STATE = -3          # include/popnet_hip.h
BY_ID = {n[0]: n for n in NETS}


@pytest.fixture(scope="module")
def recorded():
    return MK.load()


@pytest.fixture(scope="module")
def no_device():
    return _lib.lib().pn_create(-1)


def _first_difference(got, want):
    """None, or a line naming the first step and field that differ."""
    if len(got) != len(want):
        return "%d steps, recorded %d" % (len(got) - 1, len(want) - 1)
    for k, (g, w) in enumerate(zip(got, want), -1):
        if g == w:
            continue
        g, w = json.loads(g), json.loads(w)
        for f in sorted(set(g) | set(w)):
            if f != "convs" and g.get(f) != w.get(f):
                return "step %d: %s = %r, recorded %r" % (k, f, g.get(f), w.get(f))
        gc, wc = g.get("convs", []), w.get("convs", [])
        if [c["w"] for c in gc] != [c["w"] for c in wc]:
            return "step %d: convolutions %s, recorded %s" % (k, [c["w"] for c in gc], [c["w"] for c in wc])
        for a, b in zip(gc, wc):
            for f in sorted(set(a) | set(b)):
                if a.get(f) != b.get(f):
                    return "step %d, %s: %s = %r, recorded %r" % (k, a["w"], f, a.get(f), b.get(f))
        return "step %d: the texts differ: %s | %s" % (k, g, w)
    return None


def test_the_recorded_file_covers_every_net(recorded):
    assert len(NETS) == 26 + 89 + 26 and set(recorded) == set(BY_ID)          # A2J: the 26 rows of tests/a2j_plan_cases.py (8 before the deployed plans)
    assert set(MK.GPU_IDS) <= set(BY_ID)


@pytest.mark.parametrize("net", NETS, ids=[n[0] for n in NETS])
def test_step_list_equals_the_recorded_one_without_a_device(no_device, recorded, net):
    diff = _first_difference(MK.net_steps(no_device, net), recorded[net[0]])
    assert diff is None, diff


def test_a_changed_fusion_changes_the_list(no_device, recorded):
    """The comparison can fail: without the fused 1x1 tails the bf16 net has other steps than the recorded ones."""
    id_, kind, prec, mb, H, W, default, env = BY_ID["rt_224_b5_bf16"]
    diff = _first_difference(MK.net_steps(no_device, (id_, kind, prec, mb, H, W, default, dict(env, POPNET_NO_TAILFUSE="1"))), recorded[id_])
    print(diff)
    assert diff is not None


def test_forwards_refuse_a_net_without_a_device(no_device):
    L = _lib.lib()
    fake = C.c_void_p(4096)          # never dereferenced: every call below returns before it touches the device
    stream = C.c_void_p(0)
    out = (C.c_float * 4)()

    def refused(rc):
        assert rc == PN_ERR_STATE and "no device" in MK.last_error(no_device), (rc, MK.last_error(no_device))

    handles = {kind: MK.compile_net(no_device, BY_ID[id_]) for kind, id_ in (("rtpose", "rt_8x8_b2_bf16"), ("yolo", "yolo_16x16_b2_bf16"), ("a2j", "a2j_80x96_b3_bf16"))}
    try:
        for h in handles.values():
            assert L.pn_net_num_steps(h) > 0 and L.pn_net_flops_per_frame(h) > 0
            refused(L.pn_net_read_activation(h, b"buf0", 1, out, 4, stream))
            refused(L.pn_net_copy_activation(h, b"buf0", 1, fake, stream))
            refused(L.pn_net_lock(h, 1))
        refused(L.pn_rtpose_forward(handles["rtpose"], fake, 1, fake, fake, fake, stream))
        refused(L.pn_yolo_forward(handles["yolo"], fake, 1, fake, stream))
        refused(L.pn_a2j_forward(handles["a2j"], fake, 1, None, None, None, stream))
    finally:
        for h in handles.values():
            L.pn_net_destroy(h)


@pytest.mark.gpu
def test_step_lists_equal_the_recorded_ones_on_the_device(gpu, recorded):
    """The four bench nets, the conv4 configuration and the smallest A2J net in bf16 and fp32, compiled on device 0: compile only, no forward."""
    ctx = _lib.Context.for_device(0).handle
    for id_ in MK.GPU_IDS:
        diff = _first_difference(MK.net_steps(ctx, BY_ID[id_]), recorded[id_])
        assert diff is None, "%s: %s" % (id_, diff)
