"""A2J inference: every kernel instance the deployed plans launch is one that tests/test_gpu_a2j.py compares with fp64 -- without a GPU.

Each net is compiled on a context without a device (pn_create(-1), tests/golden/make_golden_net_steps.py::a2j_steps), which is where
conv_plan.h decides kernel, cout block and tile; tests/test_net_steps.py shows that a device compiles the same step list.  A convolution is
identified by its instance key (tests/a2j_plan_cases.py::instance_key), a row of the table by the keys of the steps it compares.

  a. every convolution of the nets the engines and scripts compile (288 x 288 at max_batch 32, 16 and 2, crop 96 at max_batch 2, bf16 and
     fp32) has the key of a compared step;
  b. so has every convolution of the census: square crops 32 .. 384 and the three non-square shapes at max_batch 1, 2, 16 and 32 (208 nets,
     about 40 s); no size is refused;
  c. the guard can fail: without the max_batch 32 rows, a. reports the labels that no test compared before those rows.
"""
import functools
import importlib.util
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2j_plan_cases as APC  # noqa: E402
from popnet_amd import _lib  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_net_steps", os.path.join(HERE, "golden", "make_golden_net_steps.py"))
MK = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MK)


@functools.lru_cache(None)
def _ctx():
    return _lib.lib().pn_create(-1)


@functools.lru_cache(None)
def steps(prec, max_batch, H, W):
    return MK.a2j_steps(_ctx(), prec, max_batch, H, W)


def net_keys(prec, max_batch, H, W):
    return {APC.instance_key(c) for st in steps(prec, max_batch, H, W) if st["type"] == "conv" for c in st["convs"]}


def compared(cases):
    """Instance keys of the steps the rows compare."""
    out = set()
    for _, prec, H, W, B, mb, which in cases:
        out |= APC.compared_keys(steps(prec, mb, H, W), which)
    return out


def uncovered_deployed(cases):
    """[(precision, H, W, max_batch, key)] of the deployed nets' convolutions that no row of `cases` compares."""
    have = compared(cases)
    return [(prec, H, W, mb, k) for H, W, mb in APC.DEPLOYED for prec in APC.PRECISIONS for k in sorted(net_keys(prec, mb, H, W) - have)]


def test_the_table_is_well_formed():
    assert len({c[0] for c in APC.CASES}) == len(APC.CASES)
    for id_, prec, H, W, B, mb, which in APC.CASES:
        assert id_ == APC.case_id(prec, H, W, B, mb) and prec in APC.PRECISIONS and H % 16 == 0 and W % 16 == 0 and 1 <= B <= mb
        # a row names no key that its own net does not launch: a stale key would compare nothing
        assert APC.key_part(which) <= net_keys(prec, mb, H, W), (id_, sorted(APC.key_part(which) - net_keys(prec, mb, H, W)))
        sel = APC.selects(which)
        assert any(sel(st) for st in steps(prec, mb, H, W)), id_
    # the deployed plans are compared step by step, at two crops
    for H, W, mb in APC.DEPLOYED[:3]:
        for prec in APC.PRECISIONS:
            if (prec, mb) != ("bf16", 2):          # 288 x 288, bf16, max_batch 2: the dilated and the output steps, its other keys through the rows beside it
                assert APC.find(prec, H, W, 2, mb)[6] == APC.ALL


def test_a_every_convolution_of_the_deployed_plans_is_compared():
    miss = uncovered_deployed(APC.CASES)
    assert not miss, "%d convolution instances of the deployed A2J nets are compared by no row of tests/a2j_plan_cases.py:\n%s" % (
        len(miss), "\n".join("  %s %dx%d max_batch %d: %s" % m for m in miss))
    # per 288 x 288 net: the labels, too, each in a step the table compares ("0 labels no A2J test compares")
    have = {k[0] for k in compared(APC.CASES)}
    for H, W, mb in APC.DEPLOYED:
        for prec in APC.PRECISIONS:
            labels = {st["kernel"] for st in steps(prec, mb, H, W) if st["type"] == "conv"}
            print("A2J %s %dx%d max_batch %d: %d steps, %d convolution labels, %d compared by no row" % (prec, H, W, mb, len(steps(prec, mb, H, W)), len(labels), len(labels - have)))
            assert labels <= have
    # the max_batch 32 plans launch every label that was new with them, in a step of their own row
    for prec in APC.PRECISIONS:
        _, _, H, W, B, mb, which = APC.find(prec, 288, 288, 2, 32)
        assert set(APC.NEW_LABELS[prec]) <= {k[0] for k in APC.compared_keys(steps(prec, mb, H, W), which)}


def test_b_census_over_crop_sizes():
    have = compared(APC.CASES)
    before = compared([c[:6] + (APC.ALL if c[6] == APC.ALL else APC.DIL_OUT,) for c in APC.CASES if c not in APC.CENSUS_CASES])
    first, refused, nets = {}, [], 0
    for H, W in sorted(APC.CENSUS_SIZES, key=lambda s: s[0] * s[1]):
        for mb in APC.CENSUS_MAX_BATCH:
            for prec in APC.PRECISIONS:
                nets += 1
                try:
                    keys = net_keys(prec, mb, H, W)
                except AssertionError as e:          # pn_net_finalize refused the size: legitimate with the planner's own message
                    refused.append((prec, H, W, mb, str(e)))
                    continue
                for k in keys:
                    first.setdefault(k, (prec, H, W, mb))
    print("\nA2J CENSUS: %d nets, %d refused, %d instance keys, %d of them compared only through a census row:" % (nets, len(refused), len(first), len(set(first) - before)))
    for k in sorted(first):
        print("  %-44s cfg %d pitch %3d wc %d wp %d nbuf %d pt %d rpg %d lds_two %d dil %d blocked_acc %d   first at %s %dx%d max_batch %d%s" % (
            k + first[k] + ("" if k in before else "   [census row]",)))
    # no size is refused; one that were must carry one of conv_plan.h's two reasons, not fail some other way
    assert all("halo width has no pitch class" in r[4] or "no generic kernel instance" in r[4] for r in refused), refused
    print("  refused:", refused)
    miss = sorted(set(first) - have)
    assert not miss, "instance keys the census reaches and no row compares (add the smallest crop and max_batch that produce each):\n%s" % "\n".join(
        "  %s first at %s" % (k, first[k]) for k in miss)
    # a census row is the smallest net (area, then max_batch) that produces its keys
    for id_, prec, H, W, B, mb, which in APC.CASES:
        for k in APC.key_part(which):
            assert first[k] == (prec, H, W, mb), (id_, k, first[k])


def test_c_without_the_max_batch_32_rows_the_guard_reports_their_labels():
    cases = [c for c in APC.CASES if c[5] != 32]
    miss = uncovered_deployed(cases)
    labels = {prec: {m[4][0] for m in miss if m[0] == prec and m[3] == 32} for prec in APC.PRECISIONS}
    print("\nwithout the max_batch 32 rows:", {p: sorted(v) for p, v in labels.items()})
    # bf16: every label of NEW_LABELS that a remaining row does not launch (the max_batch 16 plan shares the 1x1 generic ones, the census rows
    # two more); the 8-row conv3 tiles and the 128-cout 3x3 blocks at pitch 32 are the max_batch 32 plan's alone
    left = {k[0] for k in compared(cases)}
    assert labels["bf16"] >= set(APC.NEW_LABELS["bf16"]) - left
    assert {"conv3_kernel<1, 2, 2, 1, 7, 4>", "conv_mfma_kernel<1, 3, 1, 32, 0>", "conv_mfma_kernel<1, 3, 1, 32, 0, 2>"} <= labels["bf16"]
    # fp32 plans 288 x 288 alike at max_batch 32, 16 and 2: its rows stand in for one another
    assert labels["fp32"] == set()
    # ... and without every row that was added with the max_batch 32 ones: all of NEW_LABELS, in both precisions
    miss = uncovered_deployed([c for c in APC.CASES if c not in APC.DEPLOYED_CASES and c not in APC.CENSUS_CASES])
    for prec in APC.PRECISIONS:
        got = {m[4][0] for m in miss if m[0] == prec and m[3] == 32}
        print("without the deployed and census rows, %s max_batch 32: %s" % (prec, sorted(got)))
        assert set(APC.NEW_LABELS[prec]) <= got, (prec, sorted(set(APC.NEW_LABELS[prec]) - got))
