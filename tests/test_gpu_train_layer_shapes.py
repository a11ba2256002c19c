"""The planes training step at small and ragged shapes, op by op: tests/train_plan_cases.py::SWEEP through the machinery of tests/test_gpu_train_layers.py.

For every sweep entry, in bf16x3 and fp32:
  * the plan the engine reports (pn_trainer_op_info) equals the transcription of train_plan_cases.step_ops field by field, planned for the device's own CU
    count; the classes the entry is there for are present in the reported plan of an op of the step;
  * every op against the fp64 reference with the allowances of train_layer_reference (Step.check_all; the assertions of
    test_every_op_of_the_training_step_within_fp64_allowance, nothing of its own);
  * the integer probes (integer_probes of test_gpu_train_layers.py), the impulses on both sides of every column-strip seam, block boundary and image seam.
The conv4-threshold entry (B = 31 at the bench size) checks only the convolutions whose kernel differs from the bench configuration's.
"""
import json
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_layer_reference as TL  # noqa: E402
import train_plan_cases as TP  # noqa: E402
import test_gpu_train_layers as GT  # noqa: E402
from test_gpu_train_layers import CHECKED, EXACT, QUIET, Step, _report, impulse_ops, impulse_spots, integer_probes, op_labels  # noqa: E402

pytestmark = pytest.mark.gpu

# (the conv4 decision exists on the bf16 kernels only: the threshold entry runs in bf16x3)
CONFIGS = [("%s_%s" % (e[0], prec), prec, e) for e in TP.SWEEP for prec in ("bf16x3", "fp32") if prec == "bf16x3" or e[0] not in TP.FILTERED]
IDS = [c[0] for c in CONFIGS]
LAUNCHED = {}                     # configuration id -> {(op kind, kernel label)} the engine reports for it
SECONDS = {}                      # configuration id -> seconds of its fp64 check and of its integer probes (printed by the coverage guard, the last test)


# Comparisons that are legitimately exact at B = 2 on 1 x 1 stage maps, by name (every other comparison with worst == 0 still fails as vacuous).  A channel
# reduction there is the float32 sum of TWO values, and that sum has no rounding error
#   * in bf16x3 where both are stored values of 16 significant bits whose exponents differ by less than 8 (the batch mean of a 64-channel BatchNorm input,
#     the bias gradients below; likewise dbeta and k2 = dbeta / 8 of model0.bn2, the sum of the eight 16-bit values of its 2 x 2 maps);
#   * in both precisions where the two have opposite signs and lie within a factor of two of each other (Sterbenz): the head gradients of the two frames
#     -- a BatchNorm over two values makes every activation of one frame the mirror image of the other's, and so the gradients that reach the stage-1 heads.
# Which sums these are depends on the values: the list belongs to the seeds of Step (state_dict_from_keys(seed=0), train_case_inputs(seed=40 + B + H)).  With
# other seeds or inputs other comparisons at this shape will be the exact ones; the list is then to be measured again, the kernels have not changed.
EXACT_HERE = {
    "b2_8x8_bf16x3": ("bn_fwd model1_3.10 mean", "bn_fwd model2_3.4 mean", "dbias model2_1.12", "dbias model1_2.12", "dbias model1_3.12", "bn_bwd model0.bn2 dbeta",
                      "bn_bwd model0.bn2 k2"),
    "b2_8x8_fp32": ("dbias model1_2.12", "dbias model1_3.12"),
}


def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def _bench_labels(prec, cus):
    """(layer, dgrad) -> kernel label of the bench configuration"""
    return {(p["layer"], p["dgrad"]): op["kernels"][0] for op in TP.step_ops(32, 224, 224, prec, cus) if op["kind"] == "conv" for p in op["problems"]}


def _which(entry, prec, cus):
    """None (every op), or for a FILTERED entry the predicate `a convolution launch with a problem that the bench configuration runs on another kernel`."""
    if entry[0] not in TP.FILTERED:
        return None
    bench = _bench_labels(prec, cus)
    return lambda op: op["kind"] == "conv" and any(bench[(p["layer"], p["dgrad"])] != op["kernels"][0] for p in op["problems"])


def reported_classes(st, table):
    """{class: [op index]} from what pn_trainer_op_info reports (weight gradients, reductions, heads, pools: from the report and the tensor sizes alone;
    convolutions: kernel label, R and Wt from the report, the level's block count and lds_two from the table op it was compared with)."""
    hw = lambda ref: tuple(st.net["tensors"][ref["t"]][:2])
    out = {}
    launching = [(k, op) for k, op in enumerate(st.ops) if op["kind"] not in QUIET + ("pack",)]
    assert len(launching) == len(table)
    for (k, op), t in zip(launching, table):
        kind = op["kind"]
        if kind == "wgrad":
            H, W = hw(op["dy"])
            cl = TP.wgrad_classes(dict(op, H=H, W=W, B=st.B))
        elif kind in ("bn_fwd", "bn_bwd"):
            cl = set()
            for p in op["problems"]:
                H, W = hw(p["x"])
                cl |= TP.red_classes(kind, dict(p, npix=st.B * H * W))
        elif kind == "dbias":
            H, W = hw(op["dy"])
            cl = TP.red_classes(kind, dict(op, npix=st.B * H * W))
        elif kind == "heads":
            H, W = hw(op["heads"][0]["dv"])
            cl = TP.classify(dict(kind="heads", **TP.head_plan(st.B, H, W)))
        elif kind in ("pool_fwd", "pool_bwd"):
            (H, W), (Ho, Wo) = (hw(op["x"]), hw(op["y"])) if kind == "pool_fwd" else (hw(op["dx"]), hw(op["dy"]))
            cl = TP.classify(dict(kind=kind, H=H, W=W, Ho=Ho, Wo=Wo))
        elif kind == "conv":
            probs = []
            for p, q in zip(op["problems"], t["problems"]):
                H, W = hw(p["in"])
                plan = dict(q["p"], kernel=op["kernels"][0], R=p["R"], Wt=p["Wt"], tiles_x=-(-W // p["Wt"]))
                probs.append(dict(q, p=plan, H=H, W=W, dgrad=p["dgrad"], res=p["res"], nchw=p["nchw"], ks=p["ks"], rows=p["rows"]))
            cl = {(c[0] + " " + st.prec,) + c[1:] for c in TP.classify(dict(kind="conv", kernels=op["kernels"], problems=probs))}
        else:
            cl = TP.classify(t)
        for c in cl:
            out.setdefault(c, []).append(k)
    return out


def compare_plan(st, table):
    """Every field pn_trainer_op_info reports against the table; returns the list of differences."""
    bad = []
    launching = [(k, op) for k, op in enumerate(st.ops) if op["kind"] not in QUIET + ("pack",)]
    if [op["kind"] for _, op in launching] != [t["kind"] for t in table]:
        return ["op kinds differ: engine %s, table %s" % ([op["kind"] for _, op in launching], [t["kind"] for t in table])]
    hw = lambda ref: tuple(st.net["tensors"][ref["t"]][:2])

    def eq(k, what, got, want):
        if got != want:
            bad.append("op %d %s: engine %r, table %r" % (k, what, got, want))
    for (k, op), t in zip(launching, table):
        kind = op["kind"]
        if kind == "conv":
            eq(k, "conv kernels", op["kernels"], t["kernels"])
            eq(k, "conv problems", [(p["layer"], p["dgrad"]) for p in op["problems"]], [(q["layer"], q["dgrad"]) for q in t["problems"]])
            for p, q in zip(op["problems"], t["problems"]):
                got = (p["ks"], p["rows"], p["R"], p["Wt"], p["in"]["c"], bool(p["res"]), bool(p["nchw"]), hw(p["in"]))
                eq(k, "conv %s (ks, rows, R, Wt, k plane, residual, nchw, map)" % p["layer"], got, (q["ks"], q["rows"], q["p"]["R"], q["p"]["Wt"], q["kplane"], bool(q["res"]), bool(q["nchw"]), (q["H"], q["W"])))
        elif kind == "wgrad":
            f = ("layer", "ks", "cin", "cout", "cat", "tiles_x", "Wt", "rows_per_block", "Sr")
            eq(k, "wgrad %s" % (f,), tuple(op[x] for x in f) + (hw(op["dy"]),), tuple(t[x] for x in f) + ((t["H"], t["W"]),))
        elif kind in ("bn_fwd", "bn_bwd"):
            eq(k, kind + " (bn, C, ppb, nblk, map)", [(p["bn"], p["C"], p["ppb"], p["nblk"], hw(p["x"])) for p in op["problems"]],
               [(q["bn"], q["C"], q["ppb"], q["nblk"], (t["H"], t["W"])) for q in t["problems"]])
        elif kind == "dbias":
            f = ("layer", "cout", "C", "ppb", "nblk")
            eq(k, "dbias %s" % (f,), tuple(op[x] for x in f) + (hw(op["dy"]),), tuple(t[x] for x in f) + ((t["H"], t["W"]),))
        elif kind == "heads":
            eq(k, "heads (stage, C, map)", (op["stage"], [h["C"] for h in op["heads"]], hw(op["heads"][0]["dv"])), (t["stage"], list(TP.HEAD_C), (t["H"], t["W"])))
        elif kind == "pool_fwd":
            eq(k, "pool_fwd maps", (hw(op["x"]), hw(op["y"])), ((t["H"], t["W"]), (t["Ho"], t["Wo"])))
        elif kind == "pool_bwd":
            eq(k, "pool_bwd maps", (hw(op["dx"]), hw(op["dy"])), ((t["H"], t["W"]), (t["Ho"], t["Wo"])))
        elif kind == "add":
            eq(k, "add (C, inputs, map)", (op["out"]["c"], len(op["ins"]), hw(op["out"])), (t["C"], t["n"], (t["H"], t["W"])))
        else:
            eq(k, "stem layer", op["layer"], t["layer"])
    return bad


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_sweep_shape_plan_and_every_op_within_fp64_allowance(gpu, golden, cfg):
    tag, prec, entry = cfg
    name, B, H, W, why = entry
    t0 = time.time()
    cus = _cus(gpu)
    st = Step(golden, gpu, prec, B, H, W, tag=tag)
    # the plan view
    table = TP.step_ops(B, H, W, prec, cus)
    bad = compare_plan(st, table)
    assert not bad, "\n".join(bad[:20])
    have = reported_classes(st, table)
    mine = [c for c in why if not c[0].endswith(("bf16x3", "fp32")) or c[0].endswith(prec)]
    if cus == TP.NUM_CUS:                          # the classes were chosen at 256 CUs: on another chip the plan comparison above still holds, the census need not
        assert set(mine) <= set(have), sorted(set(mine) - set(have), key=repr)
    else:
        print("TRAIN LAYER SHAPES %s: %d CUs, not %d -- the classes the entry is there for are not asserted" % (tag, cus, TP.NUM_CUS))
    LAUNCHED[tag] = {kl for kl in op_labels(st.ops) if kl[0] != "pack"}
    # every op against fp64
    which = _which(entry, prec, cus)
    results = st.check_all(which)
    bad = _report(tag, results)
    worst = max(r[4]["worst"] for r in results)
    SECONDS.setdefault(tag, [0.0, 0.0])[0] = time.time() - t0
    print("TRAIN LAYER SHAPES %s: %d ops, %d checks, worst |gpu - r| / allowance %.3f; mask disagreements %d; %.1f s" % (tag, len(st.ops), len(results), worst, st.flips, time.time() - t0))
    launching = [k for k, op in enumerate(st.ops) if op["kind"] not in QUIET + ("pack",) and (which is None or which(op))]
    assert launching and {r[0] for r in results} == set(launching)
    assert not bad, "\n".join(bad)
    assert st.flips == 0
    vacuous = [(r[0], r[3]) for r in results if r[4]["worst"] == 0 and not any(e in r[3] for e in EXACT) and r[3] not in EXACT_HERE.get(tag, ())]
    assert not vacuous, vacuous
    if which is not None:                          # the threshold entry: the stage levels' 3x3 convolutions run conv3_kernel where the bench configuration runs conv4_kernel
        kinds = {kern.split("<")[0] for k in launching for kern in st.ops[k]["kernels"]}
        assert "conv3_kernel" in kinds and "conv4_kernel" not in kinds and len(launching) >= 6, (kinds, launching)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_sweep_shape_integer_probes_are_bit_exact(gpu, golden, cfg):
    tag, prec, entry = cfg
    name, B, H, W, _ = entry
    t0 = time.time()
    conv_max, wgrad_max = TL.integer_limits(B, H, W)
    assert conv_max < 2 ** 16 and wgrad_max < 2 ** 24
    st = Step(golden, gpu, prec, B, H, W)
    which = _which(entry, prec, _cus(gpu))
    nconv, nwg, nimp, bad = integer_probes(st, tag, extended=True, which=which)          # (a filtered entry: its convolutions only, no impulses)
    SECONDS.setdefault(tag, [0.0, 0.0])[1] = time.time() - t0
    print("\nINTEGER PROBES %s: %d convolution problems, %d weight gradients, %d impulses; %d differ; %.1f s" % (tag, nconv, nwg, nimp, len(bad), time.time() - t0))
    if which is None:
        spots = sum(len(impulse_spots(op, B, *st.net["tensors"][op["dy"]["t"]][:2], True)) for _, op in impulse_ops(st, True))
        levels = {tuple(st.net["tensors"][op["x"]["t"]][:2]) for _, op in impulse_ops(st, True)}
        assert nconv >= 38 and nwg == sum(op["kind"] == "wgrad" for op in st.ops) and nimp == spots and len(levels) == 3 and spots >= 2 * len(impulse_ops(st, True))
    else:
        assert nconv >= 3
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("prec", ("bf16x3", "fp32"))
@pytest.mark.parametrize("shape", TP.REFUSED_SWEEP, ids=[r[0] for r in TP.REFUSED_SWEEP])
def test_one_frame_on_a_1x1_stage_map_is_refused_at_finalize(gpu, golden, shape, prec):
    """B = 1 at 8 x 8: every stage BatchNorm would see one value per channel.  pn_trainer_finalize answers PN_ERR_UNSUPPORTED and names the layer and the
    reason; nothing is launched.  The next shapes up (two frames, or a 1 x 2 stage map) are accepted: the sweep runs 2 x 8 x 8."""
    from popnet_amd import _lib
    from popnet_amd.train import TrainEngine
    from helpers import state_dict_from_keys
    _, B, H, W = shape
    eng = TrainEngine(state_dict_from_keys(golden.keys["rtpose_light3d"], seed=0), device=gpu, precision=prec)
    with pytest.raises(_lib.PopnetError, match=TP.REFUSAL) as e:
        eng._trainer(B, H, W)
    assert "batch 1 on a 1 x 1 stage map" in str(e.value) and "(-4)" in str(e.value)          # PN_ERR_UNSUPPORTED
    assert (B, H, W) not in eng._trainers
    assert eng._trainer(1, 8, 16) and eng._trainer(2, 8, 8)


def test_coverage_guard_every_kernel_of_the_small_grid_is_checked(gpu, golden):
    """The sibling of test_coverage_guard_every_bench_op_kernel_is_checked over the sweep: every convolution kernel label the planner gives to any grid shape
    within the sweep's size cap (tests/golden/train_plan_small_grid_labels.json, planned at 256 CUs and kept equal to the planner by
    tests/test_train_plan_cases.py; on a chip with another CU count the grid is planned here), and every (op kind, kernel label) pair that the engine reports
    for a sweep or SHAPES configuration, must be among the pairs whose outputs Step.check_all compared (CHECKED; a configuration not yet checked in this
    process is checked here, the bench shape apart -- its pairs are the other guard's)."""
    cus = _cus(gpu)
    for tag, prec, (name, B, H, W, _) in CONFIGS:
        if tag not in CHECKED or tag not in LAUNCHED:
            st = Step(golden, gpu, prec, B, H, W, tag=tag)
            st.check_all(_which((name, B, H, W, ()), prec, cus))
            LAUNCHED[tag] = {kl for kl in op_labels(st.ops) if kl[0] != "pack"}
    for tag, prec, B, H, W in GT.CONFIGS:
        if not tag.startswith("bench_") and (tag not in CHECKED or tag not in LAUNCHED):
            st = Step(golden, gpu, prec, B, H, W, tag=tag)
            st.check_all()
            LAUNCHED[tag] = {kl for kl in op_labels(st.ops) if kl[0] != "pack"}
    checked = set().union(*CHECKED.values())
    if cus == TP.NUM_CUS:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_plan_small_grid_labels.json")) as f:
            grid = {("conv", k) for labels in json.load(f).values() for k in labels}
    else:
        grid = {("conv", k) for B, H, W in TP.grid_shapes(TP.SIZE_CAP) if (B, H, W) not in [r[1:] for r in TP.REFUSED_SWEEP] for prec in ("bf16x3", "fp32")
                for op in TP.step_ops(B, H, W, prec, cus) if op["kind"] == "conv" for k in op["kernels"]}
    # the threshold entry launches the whole step and checks its stage convolutions only: what it launches is the bench configuration's, checked there
    launched = set().union(*[v for t, v in LAUNCHED.items() if not any(t.startswith(f) for f in TP.FILTERED)])
    print("\nsmall-grid convolution kernels: %d; (op kind, kernel) pairs launched by the sweep and SHAPES: %d; checked: %d" % (len(grid), len(launched), len(checked)))
    assert len(grid) > 20 and grid <= checked, sorted(grid - checked)
    assert len(launched) > 40 and launched <= checked, sorted(launched - checked)
    total = sum(a + b for a, b in SECONDS.values())
    print("TRAIN LAYER SHAPES seconds (fp64 check + integer probes): " + ", ".join("%s %.1f + %.1f" % (k, a, b) for k, (a, b) in SECONDS.items()))
    print("TRAIN LAYER SHAPES total: %.0f s over %d cases" % (total, len(SECONDS)))
