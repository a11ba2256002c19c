"""CPU: the hand-built parse cases (tests/parse_cases.py) contain what they were built for, and every mutant of the oracle is
seen by at least one of them.  The conditions below are conditions on the INPUTS of tests/test_gpu_parse_edges.py, counted
with the oracle's own stage functions; if one fails, a case is missing -- the condition stays."""
import numpy as np

from oracle import parse_paf as O

import parse_cases as PC

FIXED = [c.name for c in PC.cases() if c.name not in PC.TINY_CASES]


def _census():
    return {c.name: PC.census(c) for c in PC.cases()}


def test_variants_with_default_flags_restate_the_oracle():
    """the stage variants the census and the mutants are made of equal the oracle's functions when no flag is set"""
    for c in PC.cases():
        ref = PC.reference(c)
        per_type, jl = ref["peaks"], ref["rec"]["joint_list"]
        plain = O.frame_to_records(c.heat.copy(), c.paf.copy(), c.z.copy())            # the oracle untouched, not through the stage wrappers
        assert PC.outputs_differ(ref, dict(ref, rec=plain, assoc=plain["assoc"])) is None
        assert np.array_equal(np.asarray(plain["joint_list"]), np.asarray(jl))
        for j in range(PC.J):
            assert np.array_equal(PC.find_peaks_variant(O.THRESH_HEATMAP, c.heat[:, :, j]), O.find_peaks(O.THRESH_HEATMAP, c.heat[:, :, j]))
        got = PC.connect_variant(c.paf_up, per_type)
        for a, b in zip(got, ref["connected"]):
            assert np.array_equal(np.asarray(a).reshape(-1, 5), np.asarray(b).reshape(-1, 5))
        assert np.array_equal(PC.group_variant(ref["connected"], jl).reshape(-1, PC.J + 2), np.asarray(ref["assoc"]).reshape(-1, PC.J + 2))
    rng = np.random.default_rng(0)
    hm, dm = rng.uniform(-0.2, 1, (9, 7)).astype(np.float32), rng.standard_normal((9, 7)).astype(np.float32)
    for r in (1, 2, 3):
        for ctr in ((0, 0), (6, 8), (3, 4), (0, 5)):
            assert PC.retrieve_variant(ctr, dm, hm.copy(), r) == O.retrieve_depth_heat_weighted(ctr, dm, hm.copy(), r)


def test_case_set_meets_its_conditions():
    cen = _census()
    for name, c in cen.items():
        print(name, PC.case(name).shape, c)
    fixed = [cen[n] for n in FIXED]
    tiny = [cen[n] for n in PC.TINY_CASES]
    patches = set(k for c in fixed for k in c["patch"])
    assert {(pw, ph) for pw in (3, 4, 5) for ph in (3, 4, 5)} <= patches
    assert any(min(k) <= 2 for c in tiny for k in c["patch"])
    allc = list(cen.values())
    assert sum(c["repeated_max"] for c in allc) >= 1
    assert sum(c["cnt"][8] for c in allc) >= 1 and sum(c["cnt"][9] for c in allc) >= 1
    assert sum(c["pen_accepted"] for c in allc) >= 1 and sum(c["pen_rejected"] for c in allc) >= 1
    assert sum(c["ties_shared"] for c in fixed) >= 1 and sum(c["ties_apart"] for c in fixed) >= 1
    for n in (4, 6, 9):
        assert sum(c["windows"].get(n, 0) for c in allc) >= 1, n
    assert sum(c["windows_negative"] for c in allc) >= 10
    assert sum(c["pruned_count"] for c in allc) >= 1 and sum(c["pruned_score"] for c in allc) >= 1
    assert cen["peaks32"]["peaks_max"] == 32 and cen["peaks33"]["peaks_max"] == 33
    assert cen["rows32"]["open_rows"] == 32 and cen["rows33"]["open_rows"] == 33 and cen["rows33"]["kept"] <= 32
    assert cen["persons16"]["kept"] == 16 and cen["persons17"]["kept"] == 17
    assert all(c["hit_max"] <= 1 for c in allc)            # the limb tree makes the merge branches unreachable (parse_cases docstring)
    # the capacity cases overflow exactly what they are named for, every other case fits the fixed-size records
    want = {"peaks33": 1, "rows33": 2}
    for name, c in cen.items():
        assert PC.expected_status(c) == want.get(name, 0), name
    for name in ("plateau_9x13", "plateau_5x7", "const_3x3"):
        assert cen[name]["peaks_max"] <= 32


def test_every_mutant_is_seen_by_a_case():
    seen = {}
    for m in PC.MUTANTS:
        seen[m.name] = []
        for c in PC.cases():
            what = PC.outputs_differ(PC.reference(c), PC.reference(c, m))
            if what:
                seen[m.name].append("%s(%s)" % (c.name, what))
        print("%-24s %s" % (m.name, ", ".join(seen[m.name]) or "-- unseen --"))
    assert not [k for k, v in seen.items() if not v]
