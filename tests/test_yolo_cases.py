"""CPU: the hand-built Yolo decode cases (tests/yolo_cases.py) contain what they were built for, and every mutant of the oracle is
seen by at least one of them.  The conditions below are conditions on the INPUTS of tests/test_gpu_yolo_edges.py, counted with
the oracle's own decode_maps and box_nms_keep; if one fails, a case is missing -- the condition stays."""
import numpy as np

from oracle import parse_yolo as O

import yolo_cases as YC

SHAPES = {(2, 14, 14), (1, 16, 32), (3, 13, 13), (1, 23, 22), (2, 1, 40), (3, 40, 1), (1, 1, 1), (2, 16, 16)}


def _all():
    return [(g, c) for g in YC.groups() for c in g.cases]


def test_decode_with_no_flag_restates_the_oracle():
    """the function the mutants are made of equals oracle.parse_yolo.parse_prior_pose when no flag is set, on every case, for
    both configurations; and the rank/keep it reports equal box_nms_keep"""
    for g, c in _all():
        for m, pv in YC.CONFIGS + ((2, False),):
            pm = YC.case_map(g.key, c.name, pv)
            assert YC.outputs_differ(YC.decode(pm, g, m, pv), YC.reference(g, c, m, pv)) is None, (g.key, c.name, m, pv)


def test_shapes_and_builder():
    assert {g.shape for g in YC.groups()} >= SHAPES
    for g in YC.groups():
        assert g.A * g.h * g.w <= YC.MAX_CAND and (g.h == g.w or g.w_out != g.h_out)
        for c in g.cases:
            a, b = YC.case_map(g.key, c.name, False), YC.case_map(g.key, c.name, True)
            assert a.shape == (g.A * (5 + 3 * YC.J), g.h, g.w) and b.shape == (g.A * (5 + 4 * YC.J), g.h, g.w) and a.dtype == b.dtype == np.float32
            assert np.array_equal(b.reshape(g.A, -1, g.h, g.w)[:, :5 + 3 * YC.J].reshape(a.shape), a)
            conf = a.reshape(g.A, -1, g.h, g.w)[:, 4]
            placed = np.zeros(conf.shape, bool)
            for p in c.places:
                placed[p[0], p[1], p[2]] = True
            assert (conf[~placed] < 0.3).all()                         # every other cell stays below the threshold
    assert sum(g.A * g.h * g.w == 512 for g in YC.groups()) >= 1 and any(g.h * g.w > 256 for g in YC.groups())


def test_case_set_meets_its_conditions():
    cen = {(g.key, c.name): YC.census(g, c) for g, c in _all()}
    for k, v in cen.items():
        print(k, {a: b for a, b in v.items() if a not in ("on_bound", "off_bound")})
    allc = list(cen.values())
    counts = {c["n"] for c in allc}
    assert {0, 1, 2, 3, 64, 65, 256, 257, 512} <= counts
    assert {63, 64, 65} <= {c["survivors"] for c in allc}
    assert any(c["all_tied_disjoint"] and c["n"] >= 32 for c in allc)                  # order decided by the tie rule alone
    assert sum(c["tied_conflicts"] for c in allc) >= 2                                 # and ties that decide who survives
    for A in (1, 2, 3):                                                               # every anchor slot of every anchor count
        slots = set()
        for g in YC.groups():
            if g.A == A:
                for c in g.cases:
                    slots |= set(cen[(g.key, c.name)]["slots"])
        assert slots == set(range(A)), (A, slots)
    assert sum(c["conf_on_thr"] for c in allc) >= 1 and sum(c["conf_step_above"] for c in allc) >= 1
    assert sum(c["iou_on_thr"] for c in allc) >= 1 and sum(c["zero_area_pairs"] for c in allc) >= 1
    # the chain of the issue: four candidates, the oracle keeps A and C
    g = YC.group("2x1x40")
    chain = cen[("2x1x40", "chain")]
    assert chain["n"] == 4 and chain["survivors"] == 2 and chain["freed"] == 1 and g.nms_thr == 0.45
    ref = YC.reference(g, next(c for c in g.cases if c.name == "chain"), 0, False)
    assert np.array_equal(ref["bbox"][:, 4], np.array([0.9, 0.9 - 0.04], np.float32))
    assert sum(c["two_suppressors_one_suppressed"] for c in allc if c["n"] <= 8) >= 1
    # n = 2 and 3 with conflicts: the loop's range is empty / one row
    assert cen[("2x14x14", "two_conflict")]["survivors"] == 1 and cen[("2x14x14", "three_chain")]["freed"] == 1
    # the high s_conf words and the later rounds of the suppression and survivor loops, in frames whose record holds every survivor
    full = [c for c in allc if c["survivors"] <= YC.MAX_DET]
    assert sum(c["conflict_col_256"] for c in full) >= 100 and sum(c["conflict_row_64"] for c in full) >= 100
    assert sum(c["returning_rows_64"] for c in full) >= 100 and sum(c["freed"] for c in full if c["n"] > 256) >= 10
    assert any(c["n"] == 512 and c["survivors"] <= YC.MAX_DET for c in allc) and any(c["n"] == 512 and c["survivors"] > YC.MAX_DET for c in allc)
    assert sum(c["cell_256_up"] for c in allc) >= 100                                  # candidates from cells past the first 256 of a slot
    # joints on every visibility bound and on the nearest reachable value outside it, for both margins, in every group but 1x1x1
    for g in YC.groups():
        if g.shape == (1, 1, 1):
            continue
        on, off = {}, {}
        for c in g.cases:
            for k, v in cen[(g.key, c.name)]["on_bound"].items():
                on[k] = on.get(k, 0) + v
            for k, v in cen[(g.key, c.name)]["off_bound"].items():
                off[k] = off.get(k, 0) + v
        assert len(on) == 8 and min(on.values()) >= 1 and min(off.values()) >= 1, (g.key, on, off)
    # one batch holds frames with no, a few and many candidates
    for g in YC.groups():
        ns = [cen[(g.key, c.name)]["n"] for c in g.cases]
        assert min(ns) <= 1 and (g.shape == (1, 1, 1) or (any(2 <= n <= 8 for n in ns) and max(ns) >= min(64, g.A * g.h * g.w)))
    # status: only more than 64 survivors set bit 0
    for g, c in _all():
        ref = YC.reference(g, c, 0, False)
        assert ref["status"] == (1 if cen[(g.key, c.name)]["survivors"] > YC.MAX_DET else 0) and ref["n_det"] == min(ref["n_survivors"], YC.MAX_DET)
    assert YC.reference(YC.group("2x14x14"), next(c for c in YC.group("2x14x14").cases if c.name == "survivors64"), 0, False)["status"] == 0


def test_every_mutant_is_seen_by_a_case():
    seen = {}
    for name in YC.MUTANTS:
        seen[name] = []
        for g, c in _all():
            for m, pv in YC.CONFIGS:
                pm = YC.case_map(g.key, c.name, pv)
                what = YC.outputs_differ(YC.reference(g, c, m, pv), YC.decode(pm, g, m, pv, **{name: True}))
                if what:
                    seen[name].append("%s/%s/m%d(%s)" % (g.key, c.name, m, what))
        print("%-12s %d: %s" % (name, len(seen[name]), ", ".join(seen[name][:6]) or "-- unseen --"))
    assert not [k for k, v in seen.items() if not v]
