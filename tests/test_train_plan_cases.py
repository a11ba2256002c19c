"""The planes trainer's plan without a device (tests/train_plan_cases.py): the census of the shape sweep, the conditions of its integer probes, and
planted plan errors that the sweep's own allowances must report (no GPU).

The census counts classes -- (family, decision, value) tuples, train_plan_cases.classify -- over B in {1, 2, 3, 5, 8, 32} and both sides 8..256 step 8, at 256
CUs (tests/test_gpu_train_layer_shapes.py repeats the comparison of every plan field with the device's own CU count).
"""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_reference as LR  # noqa: E402
import train_layer_reference as TL  # noqa: E402
import train_plan_cases as TP  # noqa: E402
from test_train_layer_reference import _emu_wgrad, _f, _r, _worst  # noqa: E402

PRECS = ("bf16x3", "fp32")


def _entry(name):
    return next(e for e in TP.SWEEP if e[0] == name)


# ---- census -----------------------------------------------------------------------------------------------------------------------------------------
def test_every_class_of_the_grid_is_reached_by_the_sweep_or_exempt():
    g = TP.grid_classes()
    c = TP.census()
    print("\nTRAIN PLAN CENSUS: classes on the grid %d / reached by SHAPES %d / reached by SHAPES + SWEEP %d / exempt %d" % (c["grid"], c["shapes"], c["both"], c["exempt"]))
    assert not c["missing"], c["missing"]
    # the exemptions: each with a reason, each reached on the grid, and there only beyond the sweep's size cap; at most a tenth of the grid's classes
    assert all(isinstance(why, str) and why and "\n" not in why for why in TP.EXEMPT.values())
    assert set(TP.EXEMPT) <= set(g), sorted(set(TP.EXEMPT) - set(g), key=repr)
    small = {cl: px for cl, px in g.items() if cl in TP.EXEMPT and px <= TP.SIZE_CAP}
    assert not small, small
    assert 10 * len(TP.EXEMPT) <= len(g)
    # SHAPES alone leave classes for the sweep (else the sweep is idle), and the sweep's frames stay within the cap -- the conv4-threshold entry apart
    assert c["shapes"] < c["both"]
    over = [e[0] for e in TP.SWEEP if e[1] * e[2] * e[3] > TP.SIZE_CAP]
    assert over == [TP.K4_ENTRY], over
    ragged = 3 * 72 * 40
    assert sum(e[1] * e[2] * e[3] <= 2.5 * ragged for e in TP.SWEEP) >= len(TP.SWEEP) - 4          # almost every entry is about the `ragged` case's size


def test_one_frame_on_a_1x1_stage_map_is_refused_and_one_value_per_channel_has_a_class():
    """B = 1 at 8 x 8: pn_trainer_finalize refuses it (tests/test_gpu_train_layer_shapes.py asserts the engine's answer), so the table refuses it and the grid
    leaves it out; the reductions class `npix == 1` exists, and no accepted shape of the grid has it -- if one ever does, the census asks for a sweep shape."""
    for name, B, H, W in TP.REFUSED_SWEEP:
        with pytest.raises(TP.PC.Refused, match="model1_1.1: train-mode BatchNorm over one value per channel"):
            TP.step_ops(B, H, W, "fp32", convs=False)
    assert TP.step_ops(2, 8, 8, "fp32", convs=False) and TP.step_ops(1, 8, 16, "fp32", convs=False)
    assert ("bn_fwd", "npix == 1", True) in TP.red_classes("bn_fwd", TP.red_plan(1, 128)) and ("dbias", "npix == 1", False) in TP.red_classes("dbias", TP.red_plan(2, 64))
    g = TP.grid_classes()
    assert all((f, "npix == 1", False) in g and (f, "npix == 1", True) not in g for f in ("bn_fwd", "bn_bwd", "dbias"))


def test_small_grid_kernel_labels_file_equals_the_planner():
    """tests/golden/train_plan_small_grid_labels.json (read by the GPU coverage guard): the convolution kernel labels of every grid shape within the size cap."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_plan_small_grid_labels.json")) as f:
        assert json.load(f) == TP.small_grid_labels()


@pytest.mark.parametrize("entry", TP.SWEEP, ids=[e[0] for e in TP.SWEEP])
def test_sweep_entry_holds_the_classes_it_is_there_for(entry):
    name, B, H, W, why = entry
    assert why, name
    have = TP.entry_classes(name, B, H, W)
    assert set(why) <= have, sorted(set(why) - have, key=repr)
    conv_max, wgrad_max = TL.integer_limits(B, H, W)                  # the conditions of the integer probe
    assert conv_max < 2 ** 16 and wgrad_max < 2 ** 24


def test_the_issue_named_edges_are_in_the_sweep():
    """A full-width 3x3 strip (Wt == 30) and a full-width 1x1 strip (Wt == 32), Sr == 1, a single partial reduction block, rows_per_block below / at the
    five-row ring with a short last block, blocks that span whole columns of a multi-strip map, and a 1 x 1 stage map."""
    ops = {e[0]: TP.step_ops(e[1], e[2], e[3], "fp32", convs=False) for e in TP.SWEEP if e[0] not in TP.FILTERED}
    wg = [(n, o) for n, os_ in ops.items() for o in os_ if o["kind"] == "wgrad"]
    assert any(o["ks"] == 3 and o["Wt"] == 30 and o["Sr"] == 1 for _, o in wg)
    assert any(o["ks"] == 1 and o["Wt"] == 32 for _, o in wg)
    assert any(o["rows_per_block"] < TP.RING and o["rows_total"] % o["rows_per_block"] for _, o in wg)
    assert any(o["rows_per_block"] == TP.RING and o["rows_total"] % o["rows_per_block"] for _, o in wg)
    assert any(o["rows_per_block"] > o["H"] and o["tiles_x"] >= 2 and "whole column" in TP.wgrad_span(o, o["H"]) for _, o in wg)
    assert any(o["Sr"] == o["rows_total"] and o["rows_per_block"] == 1 for _, o in wg)
    red = [p for os_ in ops.values() for o in os_ if o["kind"] in ("bn_fwd", "bn_bwd") for p in o["problems"]]
    assert any(p["nblk"] == 1 and p["npix"] < p["ppb"] for p in red) and any(p["nblk"] > 64 for p in red)
    assert any((o["H"], o["W"], o["Ho"], o["Wo"]) == (2, 2, 1, 1) for os_ in ops.values() for o in os_ if o["kind"] == "pool_fwd")


# ---- the moved transcriptions -------------------------------------------------------------------------------------------------------------------------
def test_moved_plan_transcriptions_keep_their_values():
    p = TP._wgrad_plan(32, 28, 28, 256, 256, 3)
    assert set(p) == {"tiles_x", "Wt", "rows_per_block", "Sr"} and (p["rows_per_block"], p["Sr"]) == (56, 16) and (p["tiles_x"], p["Wt"]) == (1, 28)
    assert TP._wgrad_plan(1, 6, 40, 64, 64, 3) == dict(tiles_x=2, Wt=20, rows_per_block=1, Sr=12)
    assert TP._wgrad_plan(32, 112, 112, 64, 64, 3) == dict(tiles_x=4, Wt=28, rows_per_block=56, Sr=256)
    c = TP._red_chain(32 * 28 * 28, 128)
    assert (c["C"], c["ppb"], TL.chain(c)) == (128, 128, 8)
    c = TP._red_chain(32 * 112 * 112, 64)
    assert (c["ppb"], TL.chain(c)) == (416, 13)
    assert TP.NUM_CUS == 256
    assert TP.head_plan(3, 9, 5) == dict(total=[3780, 2160, 2025], nblk=[15, 9, 8]) and TP.pooled(13, 17) == (7, 9) and TP.pooled(2, 2) == (1, 1)
    assert TL.stem_depth(2 * 4 * 4) == TP.stem_plan(2, 8, 8)["pps"] + TP.stem_plan(2, 8, 8)["slices"]
    assert TL.stem_depth(32 * 112 * 112) == TP.stem_plan(32, 224, 224)["pps"] + TP.stem_plan(32, 224, 224)["slices"]


def test_step_table_has_every_layer_once_per_direction():
    ops = TP.step_ops(3, 72, 40, "bf16x3")
    wg = [o["layer"] for o in ops if o["kind"] == "wgrad"]
    fwd = [p["layer"] for o in ops if o["kind"] == "conv" for p in o["problems"] if not p["dgrad"]]
    dg = [p["layer"] for o in ops if o["kind"] == "conv" for p in o["problems"] if p["dgrad"]]
    assert len(wg) == len(set(wg)) == 38 and sorted(fwd) == sorted(wg) and sorted(dg) == sorted(wg)
    assert [o["layer"] for o in ops if o["kind"] == "dbias"] == ["model%d_%d.12" % (s, b) for s in (2, 1) for b in (1, 2, 3)]
    assert sum(o["kind"] == "bn_fwd" for o in ops) == sum(o["kind"] == "bn_bwd" for o in ops)


# ---- mutants: a planted plan error must be reported by the sweep's own allowance at the sweep shape that is there for the class -------------------------
def _table_op(name, pred):
    _, B, H, W, _ = _entry(name)
    return next(o for o in TP.step_ops(B, H, W, "fp32", convs=False) if o["kind"] == "wgrad" and pred(o))


# (mutant of _emu_wgrad, sweep entry, the op of its table the class sits in)
WGRAD_MUTANTS = [
    ("strip_col", "b1_8x240", lambda o: o["ks"] == 3 and o["Wt"] == 30 and o["Sr"] == 1),              # full-width 3x3 strip, one slice
    ("strip_col", "b2_16x120", lambda o: o["ks"] == 3 and o["Wt"] == 30 and o["H"] == 4),               # ... on the /4 map
    ("strip_col", "b2_16x128", lambda o: o["ks"] == 1 and o["Wt"] == 32),                               # full-width 1x1 strip
    ("strip_col", "b1_40x256", lambda o: o["ks"] == 1 and o["Wt"] == 32 and o["tiles_x"] == 2),
    ("last_slice", "b1_8x240", lambda o: o["Sr"] == 1 and o["ks"] == 3),                                # Sr == 1: the only slice
    ("last_slice", "b1_8x240", lambda o: o["Sr"] == 1 and o["ks"] == 1),
    ("last_slice", "b5_208x8", lambda o: o["rows_per_block"] == TP.RING and o["rows_total"] % TP.RING == 0 and o["ks"] == 3),
    ("last_block", "b5_208x8", lambda o: o["rows_per_block"] < TP.RING and o["rows_total"] % o["rows_per_block"] and o["ks"] == 1),
    ("last_block", "b8_136x8", lambda o: o["rows_per_block"] == TP.RING and o["rows_total"] % TP.RING and o["ks"] == 1),
    ("last_block", "b2_136x248", lambda o: o["rows_per_block"] == TP.RING and o["rows_total"] % TP.RING and o["ks"] == 3),
    ("last_block", "b8_176x8", lambda o: o["rows_per_block"] > TP.RING and o["rows_total"] % o["rows_per_block"] and o["ks"] == 1),
    ("reprime", "b5_208x8", lambda o: o["ks"] == 1 and "image seam" in TP.wgrad_span(o, o["H"])),
    ("reprime", "b2_136x248", lambda o: o["ks"] == 3 and o["tiles_x"] == 2 and "strip seam" in TP.wgrad_span(o, o["H"])),
    ("reprime", "b2_136x248", lambda o: o["ks"] == 3 and o["tiles_x"] >= 3 and {"strip seam", "image seam"} <= TP.wgrad_span(o, o["H"])),
    ("reprime", "b2_136x248", lambda o: o["ks"] == 1 and o["tiles_x"] == 2 and {"strip seam", "image seam"} <= TP.wgrad_span(o, o["H"])),
    ("reprime", "b32_8x248", lambda o: o["ks"] == 3 and o["tiles_x"] >= 3 and "whole column" in TP.wgrad_span(o, o["H"])),
]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", range(len(WGRAD_MUTANTS)), ids=["%s_%s_%d" % (m[0], m[1], i) for i, m in enumerate(WGRAD_MUTANTS)])
def test_weight_gradient_plan_mutants_are_reported(case, prec):
    """The blockwise float32 emulation under the op's own plan (8 of its channels) passes wgrad_ref's allowance in both slice orders; with the planted error
    it does not.  Integer operands: the same error shows bit for bit."""
    mutant, name, pred = WGRAD_MUTANTS[case]
    t = _table_op(name, pred)
    B, h, w_ = t["B"], t["H"], t["W"]
    op = dict(cout=8, cin=8, ks=t["ks"], cat=0, **{k: t[k] for k in ("tiles_x", "Wt", "rows_per_block", "Sr")})
    x, dy = TL.split_act(_r((B, 8, h, w_), 300 + case).clamp_min(0), prec), TL.split_act(_r((B, 8, h, w_), 400 + case), prec)
    r, a = TL.wgrad_ref(op, prec, x, dy)
    for order in (0, 1):
        assert 0 < _worst(_emu_wgrad(op, prec, x, dy, order), r, a) <= 1
    assert _worst(_emu_wgrad(op, prec, x, dy, 0, drop=mutant), r, a) > 1, (mutant, name, op)
    xi, dyi = TL.split_act(TL.integer_operand((B, 8, h, w_), 500 + case), prec), TL.split_act(TL.integer_operand((B, 8, h, w_), 600 + case), prec)
    exact = TL._cw(dyi.v, xi.v, t["ks"])
    assert torch.equal(_emu_wgrad(op, prec, xi, dyi, 0), exact) and not torch.equal(_emu_wgrad(op, prec, xi, dyi, 0, drop=mutant), exact)


def _emu_sums(v, plan, too_far=False):
    """reduce_kernel's sums of float32 v [C, npix] under red_plan `plan`: every (block, pixel lane) a float32 chain, the rest in double.  too_far: the last block
    reads a whole ppb -- what lies behind the tensor stands in as the tensor's first pixels."""
    C, npix = v.shape
    ppb, PL = plan["ppb"], plan["PL"]
    tot = torch.zeros(C, dtype=torch.float64)
    for b in range(plan["nblk"]):
        p0, p1 = b * ppb, min((b + 1) * ppb, npix)
        idx = torch.arange(p0, (b + 1) * ppb if too_far else p1) % npix
        blk = v[:, idx]
        blk = torch.nn.functional.pad(blk, (0, (-blk.shape[1]) % PL)).view(C, -1, PL)          # [C, chain step, lane]
        acc = torch.zeros((C, PL), dtype=torch.float32)
        for i in range(blk.shape[1]):
            acc = acc + blk[:, i]
        tot += acc.double().sum(1)
    return tot


# (sweep entry, level divisor, channels, what the entry's map is there for)
RED_CASES = [("b2_8x8", 8, 64, "one block, npix = 2 below PL"), ("b2_8x8", 8, 256, "one block, npix < ppb"), ("b2_8x8", 2, 64, "one block, npix = 32 < ppb = 256"),
             ("b5_16x240", 8, 64, "dbias: 2..64 blocks, the last partial"), ("b2_136x248", 2, 64, "more than 64 blocks, the last partial"),
             ("b1_8x240", 4, 128, "one partial block on a one-row-pair map")]


@pytest.mark.parametrize("case", RED_CASES, ids=["%s_l%d_c%d" % c[:3] for c in RED_CASES])
def test_reduction_plan_mutants_are_reported(case):
    """BatchNorm forward (mean), BatchNorm backward (dbeta, k2) and dbias through bn_stats_ref / bn_bwd_sums_ref / dbias_ref and their allowances: the
    emulation passes; the last partial block reading a whole ppb, and (single block) the division by ppb instead of npix, do not."""
    name, div, Cn, _ = case
    _, B, H, W, _ = _entry(name)
    h, w_ = H // div, W // div
    plan = TP.red_plan(B * h * w_, Cn)
    m, n = TL.chain(plan), B * h * w_
    partial = n % plan["ppb"] != 0
    assert partial
    x = TL.split_act(_r((B, Cn, h, w_), 700 + Cn + h, 1.5, 0.3), "fp32").v
    flat = lambda t: _f(t).permute(1, 0, 2, 3).reshape(Cn, -1)
    one = torch.ones(Cn, dtype=torch.float64)
    ref = TL.bn_stats_ref(x, one, 0 * one, 0 * one, one, m)
    mean = lambda **kw: _f(_emu_sums(flat(x), plan, **kw) / n).double()
    assert _worst(mean(), *ref["mean"]) <= 1 and _worst(mean(too_far=True), *ref["mean"]) > 1
    sums = TL.bn_bwd_sums_ref(x, x, None, ref["mean"][0], ref["invstd"][0], one, 0, m)            # g = x: act 0
    s = lambda **kw: _emu_sums(flat(x), plan, **kw)
    assert _worst(_f(s()).double(), *sums["dbeta"]) <= 1 and _worst(_f(s(too_far=True)).double(), *sums["dbeta"]) > 1
    assert _worst(_f(s() / n).double(), *sums["k2"]) <= 1 and _worst(_f(s(too_far=True) / n).double(), *sums["k2"]) > 1
    r, a = TL.dbias_ref(x, Cn, m)
    assert _worst(_f(s()).double(), r, a) <= 1 and _worst(_f(s(too_far=True)).double(), r, a) > 1
    if plan["nblk"] == 1:
        assert _worst(_f(s() / plan["ppb"]).double(), *ref["mean"]) > 1, "single block: divided by ppb"
        assert _worst(_f(s() / plan["ppb"]).double(), *sums["k2"]) > 1, "single block: divided by ppb"


def test_allowance_formulas_see_the_plan_through_chain_and_depth():
    """The allowances the GPU sweep uses are functions of the reported plan: chain() of ppb, wgrad_depth() of rows_per_block, Wt and Sr -- at Sr == 1,
    nblk == 1 and rows_per_block == 1 they take their smallest values."""
    assert TL.wgrad_depth(dict(rows_per_block=1, Wt=30, Sr=1), "bf16x3") == 90 + 1 + 16 and TL.wgrad_depth(dict(rows_per_block=1, Wt=1, Sr=2), "fp32") == 1 + 1 + 16
    assert TL.chain(TP.red_plan(2, 256)) == 8 and TL.chain(TP.red_plan(2, 64)) == 8
    assert LR.U == 2.0 ** -24
