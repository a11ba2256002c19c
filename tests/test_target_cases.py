"""CPU: the hand-placed target annotations (tests/target_cases.py) contain what they were built for, and every mutant of the
oracle is seen by at least one of them.  The conditions are conditions on the INPUTS of tests/test_gpu_target_edges.py, counted
with the oracle's arithmetic; if one fails, a case is missing -- the condition stays."""
import numpy as np

from oracle import targets as OT

import target_cases as TC


def test_restatement_with_no_flag_equals_the_oracle():
    for c in TC.cases():
        got = TC.ground_truth(c.kp2d, c.kp_z, c.depth, c.geom)
        ref = TC.reference(c)
        for name, a, b in zip(("heat", "paf", "z", "fg"), got, ref):
            assert a.dtype == b.dtype and np.array_equal(a, b), (c.name, c.geom, name)


def test_geometries():
    want = {(224, 224, 8, 2), (232, 200, 8, 2), (200, 232, 8, 1), (224, 224, 4, 3), (64, 24, 8, 2), (8, 8, 8, 2)}
    assert {g[:4] for g in TC.by_geometry()} >= want
    assert TC.grid((232, 200, 8, 2, 7.0)) == (25, 29) and TC.grid((224, 224, 4, 3, 7.0)) == (56, 56) and TC.grid((8, 8, 8, 2, 7.0)) == (1, 1)
    for geom, cs in TC.by_geometry().items():
        for c in cs:
            assert TC.reference(c)[0].shape == TC.grid(geom) + (16,) and len(c.kp2d) <= 5


def test_case_set_meets_its_conditions():
    cen = {(c.name, c.geom): TC.census(c) for c in TC.cases()}
    for k, v in cen.items():
        print(k, v)
    allc = list(cen.values())
    total = lambda key: sum(c[key] for c in allc)
    for geom in TC.GEOMETRIES:                                            # every geometry has joints on 0, on the input size and just below it
        b = cen[("bounds", geom)]
        assert b["at_zero"] >= 4 and b["at_input"] >= 4 and b["just_below_input"] >= 4 and b["one_end_out"] >= 3, geom
        assert cen[("nobody", geom)]["persons"] == 0
    square = [v for (n, g), v in cen.items() if g[0] == g[1]]
    oblong = [v for (n, g), v in cen.items() if g[0] != g[1]]
    for part in (square, oblong):
        assert sum(c["edges_half"] for c in part) > 0                     # box edges that differ between half-even and half-away
        assert sum(c["zero_limbs"] for c in part) >= 1
        for kind in ("horizontal", "vertical", "diagonal"):
            assert sum(c["dist1"].get(kind, 0) for c in part) >= 1, kind
        assert max(c["limb_cnt_max"] for c in part) >= 3
        assert sum(c["added_to_clamped"] for c in part) >= 1
        assert sum(c["nearer_second"] for c in part) >= 1 and sum(c["behind_never_fg"] for c in part) >= 1
        assert sum(c["cut_last_inside"] for c in part) >= 1 and sum(c["cut_first_outside"] for c in part) >= 1
    assert total("cut_exact") >= 1
    # the integer search of the cut at sigma 7: 450.5 / 98 <= 4.6052 < 451.5 / 98
    assert 450.5 / 98 <= TC.CUT < 451.5 / 98


def test_every_mutant_is_seen_by_a_case_and_the_equivalent_variants_by_none():
    seen = {}
    for name in TC.MUTANTS + TC.EQUIVALENT:
        seen[name] = []
        for c in TC.cases():
            what = TC.outputs_differ(TC.reference(c), TC.ground_truth(c.kp2d, c.kp_z, c.depth, c.geom, **{name: True}))
            if what:
                seen[name].append("%s@%dx%d/%d(%s)" % ((c.name,) + c.geom[:3] + (what,)))
        print("%-15s %d: %s" % (name, len(seen[name]), ", ".join(seen[name][:8]) or "-- unseen --"))
    assert not [k for k in TC.MUTANTS if not seen[k]]
    assert not [k for k in TC.EQUIVALENT if seen[k]]                      # see the module docstring of target_cases
    # the grid mix-up is seen on a grid that is not square
    assert any("232x200" in s or "200x232" in s for s in seen["swap_grid"])


def test_compositor_cases_hold_their_inputs():
    names = set()
    for name, d, m, n_src, bg in TC.compose_cases():
        B, S, H, W = d.shape
        names.add((H, W))
        assert {0, 1, 2, 255} <= set(np.unique(m).tolist())
        assert {0, 1, S, S + 2} <= set(n_src.tolist())
        assert (d == 0).any() and (d < 0).any() and (d > 2 * OT.DEPTH_MAX).any()
        assert np.array_equal(d.astype(np.float16).astype(np.float32), d) and np.array_equal(bg.astype(np.float16).astype(np.float32), bg)
    assert names >= {(1, 1), (1, 300), (17, 19)} and any(d.shape[1] == 1 for _, d, *_ in TC.compose_cases())
    assert (1 * 300) % 256 and (17 * 19) % 256
