"""The census behind tests/net_history_cases.py (no GPU): the rows cover every kernel label of the max_batch 4 plans, each at the smallest frame.

All through pn_conv_level_plan_info on a device-less context (tests/plan_cases.py), as tests/test_plan_cases.py.
"""
import ctypes as C
import functools
import importlib.util
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2j_cases as AC  # noqa: E402
import a2j_plan_cases as APC  # noqa: E402
import a2j_x3_plan_cases as XPC  # noqa: E402
import net_history_cases as NH  # noqa: E402
import plan_cases as PC  # noqa: E402
import test_plan_cases as T  # noqa: E402
import numpy as np  # noqa: E402
from popnet_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_net_steps", os.path.join(ROOT, "tests", "golden", "make_golden_net_steps.py"))
MK = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MK)


def _own(kind, prec, H, W, env):
    return {c.p["kernel"] for c in PC.plan_net(kind, prec, NH.MAX_BATCH, NH.PROBE_B, H, W, env) if c.own}


@functools.lru_cache(None)
def _wanted():
    g = T.grid_pass((), (NH.MAX_BATCH,))
    assert not g["refused"] and not g["missing"]
    return frozenset(set(g["labels"]) - set(PC.LARGE_BATCH_ONLY))


@functools.lru_cache(None)
def _tiers():
    """[{label: smallest (H * W, H, W, precision order, network, precision, environment items)}] for the three tiers of candidates."""
    order = {p: i for i, p in enumerate(PC.ALL)}
    tiers = [{}, {}, {}]

    def reach(t, kind, prec, H, W, env):
        key = (H * W, H, W, order[prec], kind, prec, tuple(sorted(env.items())))
        for l in _own(kind, prec, H, W, env):
            if l not in tiers[t] or key < tiers[t][l]:
                tiers[t][l] = key
    for kind, H, W, _, _, env, precs, _ in PC.SWEEP:
        for prec in precs:
            reach(1 if env else 0, kind, prec, H, W, env)
    missing = _wanted() - set(tiers[0]) - set(tiers[1])
    for kind in ("rtpose", "yolo"):
        for prec in PC.ALL:
            for H, W in PC.grid(kind):
                if any(c.own and c.p["kernel"] in missing for c in PC.plan_net(kind, prec, NH.MAX_BATCH, NH.PROBE_B, H, W, {})):
                    reach(2, kind, prec, H, W, {})
    return tiers


def test_rows_cover_every_label_of_the_max_batch_4_plans():
    """Coverage: every label grid_pass((), (4,)) counts (LARGE_BATCH_ONLY exempt) is a key of LABEL_ROWS, its row is a case, and that case's own
    plan -- PC.plan_net(kind, prec, 4, 2, H, W, env) -- launches it as planned.  Removing a row from the table or a case from CASES fails here."""
    want = _wanted()
    print("\nNET HISTORY CENSUS: %d labels at max_batch %d, %d exempt (LARGE_BATCH_ONLY), %d rtpose / yolo cases over %d frames" % (
        len(want), NH.MAX_BATCH, len(set(T.grid_pass((), (NH.MAX_BATCH,))["labels"]) & set(PC.LARGE_BATCH_ONLY)), len(NH.CASES),
        len({(c[1], c[3], c[4], tuple(sorted(c[5].items()))) for c in NH.CASES})))
    assert len(want) > 40
    assert set(NH.LABEL_ROWS) == set(want), (sorted(want - set(NH.LABEL_ROWS)), sorted(set(NH.LABEL_ROWS) - want))
    by_key = {(c[1], c[3], c[4], c[2], tuple(sorted(c[5].items()))): c for c in NH.CASES}
    assert len(by_key) == len(NH.CASES) == len({c[0] for c in NH.CASES})
    covered = set()
    for label, (kind, H, W, prec, env) in NH.LABEL_ROWS.items():
        case = by_key.get((kind, H, W, prec, tuple(sorted(env.items()))))
        assert case is not None, (label, "its row is no case")
        assert label in _own(kind, prec, H, W, env), (label, case[0])
        assert label in NH.counted(case)
        covered |= _own(kind, prec, H, W, env)
    assert want <= covered
    # every case is there for a reason: it holds a counted label, or it is another precision of a frame that does
    frames = {(r[0], r[1], r[2], tuple(sorted(r[4].items()))) for r in NH.LABEL_ROWS.values()} | {(r[0], r[1], r[2], tuple(sorted(r[3].items()))) for r in NH.SWITCH_ROWS}
    assert {(c[1], c[3], c[4], tuple(sorted(c[5].items()))) for c in NH.CASES} == frames
    assert all(c[6] == NH.MAX_BATCH and c[7] == NH.PROBE_B and c[8] == NH.ALL_SEQ for c in NH.CASES)


def test_each_label_is_at_its_smallest_frame():
    """Minimality, tier by tier (the SWEEP without switches, the SWEEP's switch entries, the grid): the first tier that reaches a label names its
    smallest frame, and that is the table's row."""
    tiers = _tiers()
    for label in sorted(_wanted()):
        key = next(t[label] for t in tiers if label in t)
        assert NH.LABEL_ROWS[label] == (key[4], key[1], key[2], key[5], dict(key[6])), (label, NH.LABEL_ROWS[label], key)
    grid_tier = sorted(l for l in _wanted() if l not in tiers[0] and l not in tiers[1])
    print("\nlabels no SWEEP frame reaches at max_batch %d: %s" % (NH.MAX_BATCH, [(l, NH.LABEL_ROWS[l][:4]) for l in grid_tier]))
    assert len(grid_tier) <= 2             # the table takes its frames from the SWEEP; two labels need a larger map than it has


def test_precisions_and_switch_rows():
    # all the precisions of the SWEEP entry, for every frame taken from the SWEEP without switches
    ids = {c[0] for c in NH.CASES}
    for kind, H, W, prec, env in NH.LABEL_ROWS.values():
        e = NH.sweep_entry(kind, H, W, env)
        if e and not env:
            assert all(NH.case_id(kind, H, W, p, env) in ids for p in e[6]), (kind, H, W)
    # the switch entries: SWEEP entries, every switch once -- POPNET_CONV3_PT14 twice, with both of its values; each selects what the row says
    envs = [r[3] for r in NH.SWITCH_ROWS]
    assert sorted(k for e in envs for k in e) == sorted(NH.SWITCHES + ("POPNET_CONV3_PT14",))
    assert {e["POPNET_CONV3_PT14"] for e in envs if "POPNET_CONV3_PT14" in e} == {"1", "2"}
    sweep_switches = {k for e in PC.SWEEP for k in e[5]}
    assert sweep_switches == set(NH.SWITCHES)
    for kind, H, W, env, precs, labels in NH.SWITCH_ROWS:
        e = NH.sweep_entry(kind, H, W, env)
        assert e is not None and tuple(precs) == tuple(e[6]), (kind, H, W, env)
        for prec in precs:
            sel = _own(kind, prec, H, W, env) - _own(kind, prec, H, W, {})
            assert labels and set(labels) <= sel, (kind, H, W, env, prec, sorted(sel))
            assert NH.case_id(kind, H, W, prec, env) in ids


def test_bench_rows_take_both_bb64_paths():
    """The bench shape's two nets, each as planned and with POPNET_BB64_STRIP set against the default at B = 32; under POPNET_BB64_STRIP=0 the
    rtpose net's bb64_kernel hands tiles out by ticket at B = 32 and statically at B = 5 and 2 (NH.bb64_launch restates net_run.hip's rule;
    tests/test_gpu_bb64_strip.py and test_gpu_bb64_tiles.py hold it against the kernels)."""
    api = open(os.path.join(ROOT, "popnet_amd", "csrc", "api.hip")).read()
    import test_switches as TS
    start, end = TS._read_switches_span(api)
    assert "POPNET_BB64_STRIP" in re.findall(r'"(POPNET_[A-Z0-9_]+)"', api[start:end])
    assert NH.BENCH_WALK == (32, 5, 32, 2) and all(c[6] == 32 and c[2] == "bf16" and (c[3], c[4]) == (224, 224) and c[8] == (1, 2) for c in NH.BENCH_CASES)
    by_kind = {}
    for c in NH.BENCH_CASES:
        by_kind.setdefault(c[1], []).append(c[5].get("POPNET_BB64_STRIP"))
    assert set(by_kind) == {"rtpose", "yolo"}
    for kind, switches in by_kind.items():
        h, w = NH.BENCH_LAYER1[kind]
        default_strip = NH.bb64_launch(32, h, w, None)[0]
        assert switches == [None, "0" if default_strip else "1"], (kind, switches, default_strip)
        assert NH.bb64_launch(32, h, w, int(switches[1]))[0] != default_strip
    assert NH.bb64_launch(32, 112, 112, None) == (True, False)
    assert [NH.bb64_launch(B, 112, 112, 0) for B in NH.BENCH_WALK] == [(False, True), (False, False), (False, True), (False, False)]
    # bb64_kernel is in these plans at all: the layer1 pairs of both bf16 nets are fused (plan_cases.own_launch)
    for kind in ("rtpose", "yolo"):
        assert any(not c.own and c.name.startswith("model0.layer1.") for c in PC.plan_net(kind, "bf16", 32, 2, 224, 224, {}))


def test_a2j_rows_are_rows_of_the_a2j_tables():
    H, W, B = AC.SMALL
    small = [c for c in NH.A2J_CASES if (c[2], c[3]) == (H, W)]
    assert sorted(c[1] for c in small) == ["bf16", "bf16x3", "fp32"] and all(c[4] == B == 3 and c[5] == 2 and c[6] == (1, 2, 3, 4) for c in small)
    assert APC.find("bf16", H, W, B, B)[6] == APC.ALL and APC.find("fp32", H, W, B, B)[6] == APC.ALL
    # the smallest plane-pair row whose compared steps include the dilated ones
    with_dil = [c for c in XPC.CASES if c[6] == APC.ALL or APC.DIL_OUT in ((c[6],) if isinstance(c[6], str) else c[6])]
    smallest = min(with_dil, key=lambda c: (c[2] * c[3] * c[4], c[2]))
    assert (smallest[2], smallest[3]) == (H, W) and smallest is XPC.SMALL
    dep = NH.A2J_CASES[-1]
    assert dep[0] == APC.DEPLOYED_CASES[0][0] == "a2j_288x288_b2of32_bf16" and dep[1:6] == ("bf16", 288, 288, 32, 2) and dep[6] == (1,)
    assert all(c[2] <= 288 and c[3] <= 288 and c[4] <= 32 for c in NH.A2J_CASES) and all(c[3] <= 224 and c[4] <= 224 and c[6] <= 32 for c in NH.BENCH_CASES)


def _steps(net):
    """(net description, steps) of pn_net_step_info for a net compiled without a device."""
    L, ctx = _lib.lib(), PC._ctx()
    h = MK.compile_net(ctx, net)
    try:
        buf = C.create_string_buffer(1 << 16)
        out = []
        for k in range(-1, L.pn_net_num_steps(h)):
            assert L.pn_net_step_info(h, k, buf, len(buf)) == 0, MK.last_error(ctx)
            out.append(json.loads(buf.value.decode()))
        return out[0], out[1:]
    finally:
        L.pn_net_destroy(h)


def test_counted_labels_are_steps_and_pad_channels_exist_in_the_compiled_nets():
    """Every row compiled without a device: the labels the census counts for it are labels of plain convolution steps of the net itself (the GPU
    file repeats this on the net it runs), and the zeroed-once check is not vacuous -- every rtpose net has the stage-1 concat buffer of 192 channels
    of which no step writes 187..191, and every net has buffers at all."""
    pad_total = 0
    for id_, kind, prec, H, W, env, mb, b, _ in NH.CASES + NH.BENCH_CASES:
        info, steps = _steps((id_, kind, prec, mb, H, W, False, env))
        assert info["max_batch"] == mb and info["prec"] == prec
        case = next((c for c in NH.CASES if c[0] == id_), None)
        if case:
            assert NH.counted(case) <= NH.launched_as_planned(steps), (id_, sorted(NH.counted(case) - NH.launched_as_planned(steps)))
        written = NH.written_channels(info, steps)
        if kind == "rtpose":
            cat = [w for w, bf in zip(written, info["bufs"]) if bf[2] == 192]
            assert len(cat) == 1 and np.flatnonzero(~cat[0]).tolist() == [187, 188, 189, 190, 191], id_
        pad_total += sum(int((~w).sum()) for w in written)
    assert pad_total > 0
    for id_, prec, H, W, mb, b, _ in NH.A2J_CASES:
        info, steps = _steps((id_, "a2j", prec, mb, H, W, False, {}))
        written = NH.written_channels(info, steps)
        heads = [c for st in steps if st["type"] == "conv" for c in st["convs"] if c["w"].endswith(".output")]
        assert sorted(c["w"] for c in heads) == ["DepthRegressionModel.output", "classificationModel.output", "regressionModel.output"]
        print("\n%s: %d buffers, pad channels per buffer %s" % (id_, len(written), [int((~w).sum()) for w in written]))
