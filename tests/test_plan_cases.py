"""The inference plan without a device: every accepted frame size has kernels, the sweep's census, and the existing shapes' plans (no GPU).

All through pn_conv_level_plan_info on a device-less context (tests/plan_cases.py), i.e. conv_plan.h's own rules.
"""
import ctypes as C
import functools
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_cases as PC  # noqa: E402
from popnet_amd import _lib  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_existing.json")
SWITCH_ENVS = ({"POPNET_CONV3_PT14": "1"}, {"POPNET_CONV3_PT14": "2"}, {"POPNET_CONV3_NBUF2": "1"}, {"POPNET_CONV3_RPG8": "1"})


def _heights(kind, coarse):
    """coarse: the first four heights and every fourth after them, 512 included.  A conv3_kernel variant depends on the map's height only
    through min(H, rows of a wave group) -- settled within the first heights -- and through tile-count thresholds, which are monotonic in H."""
    hs = sorted({h for h, _ in PC.grid(kind)})
    return [h for i, h in enumerate(hs) if not coarse or i < 4 or i % 4 == 3]


@functools.lru_cache(None)
def grid_pass(env_items=(), batches=(1, 3, 32)):
    """One pass over the grid of test a. (both nets, every frame size, max_batch 1 / 3 / 32) under an environment: what it plans, in sets.
    "labels" counts a convolution only where the compiled net certainly launches the planned kernel (Conv.own); the other sets count every plan.
    With switches only the bf16 / bf16x3 nets are planned -- the switches select conv3_kernel variants, which fp32 never runs -- at every
    width and the heights of _heights(coarse)."""
    env = dict(env_items)
    out = {"missing": [], "refused": [], "classes": set(), "conv3": set(), "labels": {}, "kern_w31": set(), "convs": 0, "sizes": 0}
    for kind in ("rtpose", "yolo"):
        heights = set(_heights(kind, coarse=bool(env)))
        for prec in (PC.ALL if not env else ("bf16", "bf16x3")):
            for mb in batches:
                for H, W in PC.grid(kind):
                    if H not in heights:
                        continue
                    out["sizes"] += 1
                    try:
                        convs = PC.plan_net(kind, prec, mb, mb, H, W, env)
                    except PC.Refused as e:
                        out["refused"].append((kind, prec, mb, H, W, str(e)))
                        continue
                    for c in convs:
                        out["convs"] += 1
                        if c.own:
                            out["labels"].setdefault(c.p["kernel"], set()).add(mb)
                        if c.W == 31:
                            out["kern_w31"].add(c.p["kern"])
                        if PC.generic(c):
                            out["classes"].add(PC.generic_class(c))
                            if not PC.has_instance(prec, c.ks, c.stride, c.p["pitch"], c.p["cfg"]):
                                out["missing"].append((kind, prec, mb, H, W, c.name, c.p["kernel"]))
                        elif c.p["kern"] == 3:
                            out["conv3"].add(PC.conv3_tuple(c))
    return out


@functools.lru_cache(None)
def planned_runs():
    """Every convolution the per-layer GPU tests plan: test_gpu_layers.CONFIGS (the reference-default topology apart: other head widths, same
    sizes) and the sweep, as [(run id, environment, [Conv])]."""
    import test_gpu_layers as GL
    runs = []
    for id_, kind, prec, B, H, W, default, env in GL.CONFIGS:
        if not default:
            runs.append((id_, env, PC.plan_net(kind, prec, B, B, H, W, env)))
    for e in PC.SWEEP:
        kind, H, W, B, mb, env, precs, _ = e
        for prec in precs:
            runs.append((PC.sweep_id(e) + "_" + prec, env, PC.plan_net(kind, prec, mb, B, H, W, env)))
    return runs


def test_a_every_accepted_size_has_kernels():
    """Both sides 8..512 step 8 (rtpose) / 16..512 step 16 (yolo), max_batch 1, 3, 32, three precisions, 256 CUs: every planned generic
    convolution names a built instance (pn_conv_has_instance), or the plan refuses the size.  On the planner before the pitch fallback this
    failed at every rtpose width <= 128 (1024 of 4096 sizes: the stage 1x1 convolutions at pitch 16; at width <= 64 layer2.0.downsample and
    model0.conv2 too) and at YoloPoseNet widths <= 112 (bf16 / bf16x3) or <= 128 (fp32, whose 1x1 stride-2 shortcut has the narrower halo):
    256 of 1024 sizes, the stride-2 level at pitch 16 / 32."""
    g = grid_pass()
    print("\nPLAN GRID: %d net plans, %d convolutions, %d refused, generic classes %s" % (g["sizes"], g["convs"], len(g["refused"]), sorted(g["classes"])))
    sizes = sorted({m[:5] for m in g["missing"]})
    assert not g["missing"], "%d plans name a kernel that is not built, e.g. %s" % (len(sizes), g["missing"][:5])
    # the two nets' convolutions all have a fallback class: nothing in the grid is refused (a refusal would be legitimate, and is then listed here)
    assert g["refused"] == []


def test_instance_predicate_and_entry_arguments():
    # the holes of the table the fallback exists for, and a few instances on either side of them
    assert not PC.has_instance("bf16", 1, 1, 16, PC.CFG_C128) and PC.has_instance("bf16", 1, 1, 32, PC.CFG_C128) and PC.has_instance("fp32", 3, 1, 16, PC.CFG_C16)
    assert not PC.has_instance("bf16", 3, 2, 32, PC.CFG_C128) and PC.has_instance("fp32", 3, 2, 64, PC.CFG_C64) and not PC.has_instance("bf16", 1, 2, 64, PC.CFG_C32)
    assert PC.has_instance("bf16", 3, 1, 64, PC.CFG_C64W) and not PC.has_instance("bf16", 1, 1, 64, PC.CFG_C64W) and not PC.has_instance("bf16", 3, 1, 48, PC.CFG_C64)
    assert _lib.lib().pn_conv_has_instance(2, 3, 1, 32, 0) == 0            # bf16x3 nets run the bf16 instances: PN_PREC_BF16X3 is no kernel precision
    # stride 2 on a 32- / 16-cout block has no instance in any class: refused with a reason, as pn_net_finalize would
    with pytest.raises(PC.Refused, match="conv 0: no generic kernel instance"):
        PC.plan_level("bf16", 2, 2, 8, 8, [(64, 32, 3, 2)], together=True)
    L, h, buf = _lib.lib(), PC._ctx(), C.create_string_buffer(4096)
    one = (C.c_int * 1)
    ok = (h, 1, 2, 256, 2, 8, 8, 1, 1, one(64), one(64), one(3), one(1))
    assert L.pn_conv_level_plan_info(*ok, buf, len(buf)) == 0 and set(PC.GEOM) | {"kernel"} == set(json.loads(buf.value.decode())["convs"][0])
    assert L.pn_conv_level_plan_info(*ok, buf, 8) == -1                       # cap too small
    assert L.pn_conv_level_plan_info(*ok[:4], 3, *ok[5:], buf, len(buf)) == -1   # B > max_batch
    assert L.pn_conv_level_plan_info(*ok[:8], 4, *ok[9:], buf, len(buf)) == -1   # more than three convolutions
    assert L.pn_conv_level_plan_info(*ok[:11], one(5), one(1), buf, len(buf)) == -1   # kernel size


def test_b_census_of_the_sweep():
    """Counted are only convolutions that the compiled net launches as the kernel the plan names (Conv.own, plan_cases.own_launch): a convolution
    fused into a BasicBlock kernel, run as a tail, or launched through conv3_mix_kernel exercises another kernel than its plan says."""
    runs = [(i, e, [c for c in cs if c.own]) for i, e, cs in planned_runs()]
    convs = [c for _, _, cs in runs for c in cs]
    g = grid_pass()
    counts = {name: sum(1 for c in convs if pred(c)) for name, pred in PC.CONDITIONS.items()}
    print("\nCENSUS over %d runs, %d convolutions launched as planned:" % (len(runs), len(convs)))
    for name, n in counts.items():
        print("  %-48s %d" % (name, n))
    for name in PC.UNREACHABLE:
        assert counts.pop(name) == 0
    assert all(counts.values()), [n for n, v in counts.items() if not v]
    # ... unreachable over the whole grid, not only unseen in the sweep: a map 31 wide never fills 75 % of a wave group (two 16-wide strips of
    # 4 rows hold 4 * 15.5 = 62 of 112 pixel slots), so conv3_kernel / conv4_kernel never see it; the generic kernel does
    assert g["kern_w31"] == {0}
    assert any(c.W == 31 and PC.generic(c) for c in convs)
    # every (ks, stride, pitch) class of the generic kernel the grid reaches, the classes reached through the fallback included
    classes = {PC.generic_class(c) for c in convs if PC.generic(c)}
    assert g["classes"] <= classes, sorted(g["classes"] - classes)
    assert {(1, 1, 32), (3, 2, 64), (1, 2, 64)} <= {PC.generic_class(c) for c in convs if PC.CONDITIONS["generic pitch widened by the fallback"](c)}
    # conv3_kernel: every variant the grid reaches with default switches ...
    seen = {PC.conv3_tuple(c) for _, env, cs in runs for c in cs if c.p["kern"] == 3 and not set(env) & {k for e in SWITCH_ENVS for k in e}}
    assert g["conv3"] <= seen, sorted(g["conv3"] - seen)
    # ... and under each switch: a variant is one kernel instantiation whatever selected it, so a variant the default plan reaches too is run by
    # the default runs; a variant only the switch reaches must be planned by a run compiled under that switch
    seen_any = {PC.conv3_tuple(c) for _, _, cs in runs for c in cs if c.p["kern"] == 3}
    for env in SWITCH_ENVS:
        reach = grid_pass(tuple(sorted(env.items())))["conv3"]
        seen_env = {PC.conv3_tuple(c) for _, e, cs in runs for c in cs if c.p["kern"] == 3 and all(e.get(k) == v for k, v in env.items())}
        print("  conv3 variants under %s: %s, of them new: %s" % (env, sorted(reach), sorted(reach - g["conv3"])))
        assert reach - g["conv3"], env                        # the switch does select something
        assert reach <= seen_any and reach - g["conv3"] <= seen_env, (env, sorted(reach - seen_env))
    # conv4 by block count and by the switch
    k4 = [(env.get("POPNET_CONV4"), c) for _, env, cs in runs for c in cs if c.p["kern"] == 4]
    assert any(e is None for e, _ in k4) and any(e == "1" for e, _ in k4)
    # the sweep itself: B <= 3 everywhere, one entry compiled for a larger batch than it runs
    assert all(e[3] <= 3 for e in PC.SWEEP) and any(e[4] > e[3] for e in PC.SWEEP)


def test_c_existing_shapes_keep_their_plan():
    """tests/golden/plan_existing.json: the plan of every convolution of test_gpu_layers.CONFIGS' sizes, recorded from the planner before the
    instance table reached it (the same dump, PC.existing_plans)."""
    with open(GOLDEN) as f:
        want = json.load(f)
    got = PC.existing_plans()
    assert sorted(got) == sorted(want)
    moved = [(k, a[0], a[1], b[1]) for k in want for a, b in zip(want[k], got[k]) if a != b]
    assert not moved, moved[:5]
    assert sum(len(v) for v in want.values()) > 300


def test_kernel_labels_of_small_batches_are_run():
    """Every kernel label the grid reaches at max_batch 1 or 3 is the label of a convolution that a run of the per-layer GPU tests launches as
    planned (Conv.own on both sides; tests/test_gpu_layer_shapes.py asserts per compiled net that such a convolution sits in a plain conv step
    with that label, and repeats this comparison on the labels the compiled nets report).  LARGE_BATCH_ONLY: reached at max_batch 32 only."""
    g = grid_pass()
    small = {l for l, mbs in g["labels"].items() if mbs & {1, 3}}
    run = {c.p["kernel"] for _, _, cs in planned_runs() for c in cs if c.own}
    assert small <= run, sorted(small - run)
    assert {l for l, mbs in g["labels"].items() if mbs == {32}} == set(PC.LARGE_BATCH_ONLY)
