"""CPU: the edge-case depth frames (tests/preproc_cases.py) contain what they were built for, and every mutant of the pre-processing
arithmetic is seen by at least one of them.  The conditions are conditions on the INPUTS of tests/test_gpu_preproc_edges.py, counted
with the oracle; if one fails, a case is missing -- the condition stays."""
import numpy as np

import preproc_cases as PC


def test_restatement_with_no_flag_equals_the_oracle():
    for c in PC.cases():
        ref = PC.reference(c)
        assert ref.shape == (PC.B, 1, c.S, c.S) and ref.dtype == np.float32
        for b in range(PC.B):
            assert PC.same(PC.restate(c.frames[b], c.S, c.consts), ref[b, 0]), (c.name, b)      # NaN positions and the sign of zeros count


def test_sizes_and_geometries():
    assert set(PC.RT_S) >= {8, 32, 40, 136, 224} and set(PC.YOLO_S) >= {16, 32, 112, 224, 240} and set(PC.PRE_S) == {1, 17}
    assert sorted(S // 2 for S in (8, 32, 40, 136, 224)) == [4, 16, 20, 68, 112]          # stem maps: below one 16-tile, one, ragged, ragged, exact
    assert [S // 2 % 16 for S in (8, 32, 40, 136, 224)] == [4, 0, 4, 4, 0]
    assert sorted(S // 4 for S in (16, 32, 112, 224, 240)) == [4, 8, 28, 56, 60]          # pooled maps against 8 x 7 blocks
    assert sum(1 for S in PC.ALL_S if (S * S) % 256 != 0) >= 3
    for S in PC.ALL_S:
        got = {n: (H, W) for n, H, W in PC.geometries(S)}
        assert (2 * S, 2 * S) not in got.values() and PC.refused(S) == (2 * S, 2 * S)
        assert all(H >= 2 and W >= 2 for H, W in got.values())
        if S == 1:
            assert set(got.values()) == {(2, 3), (7, 5)}
            continue
        assert set(got) == set(PC.GEOMETRY_NAMES), (S, sorted(got))
        assert got["down"] == (2 * S + S // 2 + 1, 3 * S - 1) and got["up"] == (max(2, S // 3 + 1), max(2, S // 2 - 1))
        assert got["mixed2x"] == (2 * S, S // 2 + 1) and got["identity"] == (S, S) and got["min"] == (2, 2)
        assert got["thin"] == (2, 5 * S) and got["tall"] == (5 * S, 2)
        assert got["up"][0] < S and got["up"][1] < S and got["down"][0] > 2 * S and got["down"][1] > 2 * S
    names = [c.name for c in PC.cases()]
    assert len(names) == len(set(names))
    for S in PC.ALL_S:                       # every geometry in float16 and float32, every constant set at every S
        cs = PC.cases_for(S)
        assert {(c.geom, c.dtype) for c in cs if c.values == "plain"} == {(n, d) for n, _, _ in PC.geometries(S) for d in (np.float16, np.float32)}
        assert {c.consts for c in cs} == set(PC.CONSTANTS)
        for c in cs:
            assert c.frames.shape == (PC.B, c.H, c.W) and c.frames.dtype == c.dtype
            assert not np.array_equal(c.frames[0], c.frames[1], equal_nan=True) and not np.array_equal(c.frames[1], c.frames[2], equal_nan=True)
    assert (6.0, 3.0, 2.0) in PC.CONSTANTS and (5.0, 3.0, 2.0) in PC.CONSTANTS and (4.5, 2.7, 1.3) in PC.CONSTANTS


def test_case_set_meets_its_conditions():
    cen = {c.name: PC.census(c) for c in PC.cases()}
    print("%d cases, %d pre-processed pixels" % (len(cen), sum(v["pixels"] for v in cen.values())))
    worst = 0.0
    for c in PC.cases():
        v = cen[c.name]
        assert v["at_low"] >= 1 and v["at_high"] >= 1, (c.name, v)              # pixels at both clamp values
        if c.values == "nonfinite":
            assert min(c.H, c.W) >= 5 and c.geom != "identity"
            assert np.isnan(c.frames[:, 0, 0]).all() and np.isposinf(c.frames[:, :, -1].astype(np.float32)).all()
            assert np.isneginf(c.frames[:, c.H // 2, c.W // 2].astype(np.float32)).all() and np.isposinf(c.frames[:, c.H - 1, 1].astype(np.float32)).all()
            if c.dtype == np.float16:
                assert (c.frames == np.float16(65504)).any() and ((c.frames > 0) & (c.frames < np.float16(6.2e-5))).any()      # max and a subnormal
            assert 1 <= v["nan"] <= 0.10 * v["pixels"], (c.name, v)
            worst = max(worst, v["nan"] / v["pixels"])
        else:
            assert np.isfinite(c.frames.astype(np.float32)).all() and v["nan"] == 0
            assert (c.frames < 0).any() and (c.frames > 6).any()
        if c.geom == "identity":            # cv2 copies: the bilinear path with weights (1, 0) equals clamp + normalise of the frame itself
            dmax, mean, std = (np.float32(k) for k in c.consts)
            want = (np.clip(c.frames.astype(np.float32), np.float32(0), dmax) - mean) / std
            assert want.dtype == np.float32 and PC.same(PC.reference(c)[:, 0], want), c.name
    print("largest NaN share of a nonfinite case: %.4f" % worst)
    nf = [c for c in PC.cases() if c.values == "nonfinite"]
    for S in PC.ALL_S:
        if S > 1:
            assert {c.geom for c in nf if c.S == S} >= {"down", "mixed2x"}, S
    assert {c.S for c in nf if c.geom == "up"} >= {17, 32, 40, 48, 112, 136, 224, 240}      # up-sampled on both axes, at least 5 x 5


def test_every_mutant_is_seen_by_a_case_and_the_equivalent_variants_by_none():
    seen = {}
    for name in PC.MUTANTS + PC.EQUIVALENT:
        seen[name] = []
        for c in PC.cases():
            ref = PC.reference(c)
            if any(not PC.same(PC.restate(c.frames[b], c.S, c.consts, **{name: True}), ref[b, 0]) for b in range(PC.B)):
                seen[name].append(c)
        print("%-17s %3d: %s" % (name, len(seen[name]), ", ".join(c.name for c in seen[name][:4]) or "-- unseen --"))
    assert not [k for k in PC.MUTANTS if not seen[k]]
    assert not [k for k in PC.EQUIVALENT if seen[k]]                       # see the module docstring of preproc_cases
    # multiplying by the reciprocal shows only where the std is no power of two
    assert all(c.consts[2] == 1.3 for c in seen["recip"])
    # multiplying in the right-border tail shows only on +Inf in the last column of an up-sampled axis
    assert all(c.values == "nonfinite" and c.W < c.S for c in seen["no_tail_copy"])
    assert {c.dtype for c in seen["no_tail_copy"]} == {np.float16, np.float32}
