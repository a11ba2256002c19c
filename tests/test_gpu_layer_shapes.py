"""Every launch of the inference nets against fp64 at small and ragged frame sizes, and the plan view against the compiled nets.

tests/test_gpu_layers.py checks each step of the compiled nets at a few frame sizes, none with a side below 96 pixels; the launch planner
(popnet_amd/csrc/conv_plan.h) decides kernel, tiles and LDS pitch from the map's height and width.  The sweep of tests/plan_cases.py puts a
frame on either side of each of its rules (tests/test_plan_cases.py holds the census, without a GPU) and this file runs it with the machinery
and the two assertions of test_gpu_layers.py: every output element of every step within tests/layer_reference.py's derived allowance, and no
allowance vacuous.  No tolerance of its own.

The sizes at or below 128 (rtpose) / 112 (yolo) pixels wide are those whose 1x1 / stride-2 convolutions had no kernel instance at their LDS
pitch class before the planner consulted the instance table; they now run at the next wider class.  With that fallback no frame size of
either net is refused, so there is no refusal to assert here (the refusal of a level that has no instance in any class, and its message, is
asserted on the plan entry in tests/test_plan_cases.py).

Every case also compares pn_net_step_info's geometry of each convolution with what pn_conv_level_plan_info returns for the same level of
plan_cases' transcribed tables: the tables, the census and the recorded plans of tests/golden/plan_existing.json then cannot drift from the nets.
The plan view reports the UNFUSED plan of a convolution; what the census counts is narrower -- only convolutions launched as the kernel their plan
names (plan_cases.own_launch) -- and every case asserts that each such convolution sits in a plain conv step with that kernel label.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_cases as PC  # noqa: E402
from test_gpu_layers import CONFIGS, _Net, _model, _step_info  # noqa: E402
from popnet_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = []
for _e in PC.SWEEP:
    _kind, _H, _W, _B, _mb, _env, _precs, _ = _e
    for _p in _precs:
        _cfg_env = dict(_env, **({"POPNET_MAX_BATCH": str(_mb)} if _mb != _B else {}))
        CASES.append(((PC.sweep_id(_e) + "_" + _p, _kind, _p, _B, _H, _W, False, _cfg_env), _e))

# what a fused average pool changes after planning (net.hip::fuse_pool_tails: 8-row image, tiles of the pooled map)
POOL_FUSED = ("kernel", "rpg", "nbuf", "tiles_x", "tiles_per_img", "nblocks")


def _plan_view_matches(steps, planned):
    """pn_net_step_info's geometry of every convolution == the device-less plan of the same level; every table convolution is in the net; and every
    convolution plan_cases counts as launched as planned (Conv.own) sits in a plain conv step -- no fused tail, no fused pool, not a BasicBlock step,
    not conv3_mix_kernel -- whose kernel label is the plan's.  Returns the labels of the steps that launch exactly the kernel they name."""
    want = {c.name: c for c in planned}
    assert len(want) == len(planned)
    seen, bad, launched = set(), [], set()
    for k, st in enumerate(steps):
        convs = st.get("convs", ())
        plain = st["type"] == "conv" and not any(cv["tail"] or cv["pool"] for cv in convs)
        if plain:
            launched.add(st["kernel"])
        for cv in convs:
            seen.add(cv["w"])
            if cv["tail"]:
                seen.add(cv["tail"]["w"])
                assert not want[cv["tail"]["w"]].own, cv["tail"]["w"]
            c = want[cv["w"]]
            for f in PC.GEOM + ("kernel",):
                if cv["pool"] and f in POOL_FUSED:
                    continue
                if cv[f] != c.p[f]:
                    bad.append((k, cv["w"], f, cv[f], c.p[f]))
            if c.own and not (plain and st["kernel"] == c.p["kernel"]):
                bad.append((k, cv["w"], "counted as launched as planned, but the step is", st["type"], st["kernel"]))
    assert not bad, bad[:8]
    assert seen == set(want), sorted(seen ^ set(want))
    return launched


# the kernel a switch entry is there for must be the label of a step of that case, not only of a plan
MUST_LAUNCH = {
    "rt_96x240_b2of32_conv3_pt141_no_bblock1_bf16": "conv3_kernel<3, 2, 1, 1, 14, 8>",
    "rt_32x88_b2_conv3_pt142_bf16": "conv3_kernel<3, 4, 1, 1, 14, 8>",
    "rt_96x240_b2of32_conv3_nbuf21_bf16x3": "conv3_kernel<3, 2, 2, 2, 7, 4>",
    "rt_16x88_b2_conv3_nbuf21_bf16x3": "conv3_kernel<3, 2, 1, 2, 7, 4>",
    "rt_16x88_b2_conv3_nbuf21_bf16": "conv3_kernel<3, 4, 1, 2, 7, 4>",
    "rt_24x56_b2_conv3_rpg81_bf16": "conv3_kernel<3, 4, 1, 1, 7, 8>",
    "rt_24x240_b3_conv41_bf16": "conv4_kernel",
}
assert set(MUST_LAUNCH) <= {c[0][0] for c in CASES}, sorted(set(MUST_LAUNCH) - {c[0][0] for c in CASES})


@pytest.mark.parametrize("cfg,entry", CASES, ids=[c[0][0] for c in CASES])
def test_every_layer_within_fp64_allowance_small_and_ragged(gpu, golden, monkeypatch, cfg, entry):
    kind, H, W, B, mb, env, _, why = entry
    net = _Net(golden, cfg, gpu, monkeypatch)
    assert net.info["max_batch"] == mb and net.B == B
    launched = _plan_view_matches(net.steps, PC.plan_net(kind, cfg[2], mb, B, H, W, env))
    assert cfg[0] not in MUST_LAUNCH or MUST_LAUNCH[cfg[0]] in launched, sorted(launched)
    results = net.check_all()
    assert len(results) >= len(net.steps)
    worst = max(r[3]["worst"] for r in results)
    print("\nSHAPES %s: %d steps, %d outputs, worst |gpu - r| / allowance = %.4f  [%s]" % (cfg[0], len(net.steps), len(results), worst, why))
    bad = ["step %d %s %s: worst %.3g, %d elements over, at (frame, channel, row, col, ratio) %s" % (k, kern, name, rep["worst"], rep["n_bad"], rep["where"])
           for k, kern, name, rep in results if rep["n_bad"]]
    assert not bad, "\n".join(bad)
    # the allowance must not be vacuous: every checked output carries real data
    assert all(r[3]["worst"] > 0 for r in results if "pool1" not in r[2] and "pool2" not in r[2] and "maxpool" not in r[2]), \
        [(r[0], r[2]) for r in results if r[3]["worst"] == 0]
    net.m.invalidate()


def test_plan_view_matches_the_existing_configurations_and_small_batch_labels_are_launched(gpu, golden, monkeypatch):
    """The same comparison for test_gpu_layers.CONFIGS (reference-default topology apart: its heads have other widths than the tables), and
    the coverage guard over frame sizes: every kernel label that the plan grid (both sides 8..512, max_batch 1 and 3) gives to a convolution
    launched as planned is the label of a step that launches exactly that kernel -- in a CONFIGS net compiled here, or in a sweep case, whose
    own test asserts that the convolutions counted for it sit in such steps.  Labels reached at max_batch 32 only are exempt:
    plan_cases.LARGE_BATCH_ONLY (tests/test_plan_cases.py asserts that list)."""
    import test_plan_cases as T
    launched = set()
    for cfg in CONFIGS:
        _, kind, prec, B, H, W, default, env = cfg
        if default:
            continue
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = _model(golden, kind, default)
        m.precision = prec
        h = m._compile(gpu, B, H, W)
        for k in env:
            monkeypatch.delenv(k)
        steps = [_step_info(h, k) for k in range(_lib.lib().pn_net_num_steps(h))]
        launched |= _plan_view_matches(steps, PC.plan_net(kind, prec, B, B, H, W, env))
        m.invalidate()
    assert "conv4_kernel" in launched and any(l.startswith("conv_mfma_kernel<1, 3, 2") for l in launched)
    sweep = {c.p["kernel"] for (cfg, e) in CASES for c in PC.plan_net(e[0], cfg[2], e[4], e[3], e[1], e[2], e[5]) if c.own}
    small = {l for l, mbs in T.grid_pass((), (1, 3))["labels"].items()}
    assert not small & set(PC.LARGE_BATCH_ONLY)
    assert small <= launched | sweep, sorted(small - launched - sweep)
