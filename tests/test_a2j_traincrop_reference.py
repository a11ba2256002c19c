"""CPU: the host half of A2J's crop-level augmentation (popnet_amd/a2j_crops.py) and the numpy restatement of the kernel
(tests/a2j_traincrop_reference.py) against the reference's own outputs (tests/golden/a2j_traincrop.npz, made by
tests/golden/make_golden_a2j_traincrop.py from dataPreprocess / transform / errorCompute / writeTxt themselves)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2j_traincrop_cases as TC  # noqa: E402
import a2j_traincrop_reference as TR  # noqa: E402
import cv2_warp_reference as WR  # noqa: E402
from popnet_amd import _lib, a2j_crops as AJ, warp_affine  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "a2j_traincrop.npz"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def itop_case_items(g, i):
    """records and labels of ITOP case i, built by the host module from the case table"""
    name, fset, fi, lt, rb, c, draws, (cw, ch) = TC.ITOP_CASES[i]
    rec, labels = AJ.itop_items([i], TC.itop_centres(), g["itop_lefttop"], g["itop_rightbottom"], TC.itop_keypoints(), TC.SETS[fset],
                                draws=None if draws is None else [TC.draws_of(draws)], crop_w=cw, crop_h=ch, frames=[fi])
    return rec, labels


def box_case_items(i):
    name, fi, box, draws, (cw, ch) = TC.BOX_CASES[i]
    bnd, k2, k3 = TC.box_arrays()
    return AJ.box_items([i], bnd, k2, k3, TC.SETS["b"], draws=None if draws is None else [TC.draws_of(draws)], crop_w=cw, crop_h=ch,
                        img_wh=TC.IMG_WH_B, frames=[fi])


def golden_crop(g, form, i):
    cases = TC.ITOP_CASES if form == "itop" else TC.BOX_CASES
    large = [k for k, c in enumerate(cases) if c[-1][0] == TC.LARGE]
    if i in large:
        assert form != "bg"
        return g[form + "_crops_large"][large.index(i)]
    return g[form + "_crops"][[k for k in range(len(cases)) if k not in large].index(i)]


def composed_frames_b():
    fg = TC.frames("b")
    mask, bg = TC.masks_and_backgrounds("b")
    return np.where(mask > 0, fg, bg)


def test_the_case_table_is_the_goldens():
    g = np.load(os.path.join(GOLDEN, "a2j_traincrop.npz"))
    assert [str(n) for n in g["itop_names"]] == [c[0] for c in TC.ITOP_CASES] and [str(n) for n in g["box_names"]] == [c[0] for c in TC.BOX_CASES]
    assert g["itop_crops"].shape == (len(TC.ITOP_CASES) - 1, TC.CROP_H, TC.CROP_W) and g["itop_crops_large"].shape == (1, TC.LARGE, TC.LARGE)
    assert g["box_crops"].shape == g["bg_crops"].shape == (len(TC.BOX_CASES) - 1, TC.CROP_H, TC.CROP_W)
    assert os.path.getsize(os.path.join(GOLDEN, "a2j_traincrop.npz")) < 1 << 20
    assert str(g["numpy_version"]).split(".")[0] == np.__version__.split(".")[0], "the golden was made under another numpy major version"
    nan = {str(n): int(k) for n, k in zip(g["itop_names"], g["itop_nan_count"])}
    assert all((nan[n] > 0) == (n in TC.NAN_CASES) for n in nan)


@pytest.mark.parametrize("i", range(len(TC.ITOP_CASES)), ids=[c[0] for c in TC.ITOP_CASES])
def test_itop_items_labels_and_restated_crops_equal_the_reference(g, i):
    name, fset, fi, lt, rb, c, draws, (cw, ch) = TC.ITOP_CASES[i]
    rec, labels = itop_case_items(g, i)
    crops, flags = TR.train_crops(TC.frames(fset), rec, cw, ch, TC.ITOP_MEAN, TC.ITOP_STD)
    assert flags.tolist() == [int(g["itop_flags"][i])]
    want = golden_crop(g, "itop", i)
    assert np.array_equal(bits(crops[0]), bits(want)), "%s: %d pixels differ" % (name, int((bits(crops[0]) != bits(want)).sum()))
    assert int(np.isnan(crops[0]).sum()) == int(g["itop_nan_count"][i])
    if not flags[0]:
        assert labels.dtype == np.float32 and np.array_equal(bits(labels[0]), bits(g["itop_labels"][i])), name
    assert rec[0].warp == (0 if draws is None else 1) and rec[0].window == 1 and rec[0].padded == 0


# every box case through train_a2j_base.py, and through train_a2j_bgaug_new.py (the background swap) except the 288 x 288 one, whose crop
# is stored for the base form only
BOX_RUNS = [(i, False) for i in range(len(TC.BOX_CASES))] + [(i, True) for i, c in enumerate(TC.BOX_CASES) if c[-1][0] != TC.LARGE]


@pytest.mark.parametrize("i,swap", BOX_RUNS, ids=["%s-%s" % (TC.BOX_CASES[i][0], "bgaug" if s else "base") for i, s in BOX_RUNS])
def test_box_items_labels_and_restated_crops_equal_the_reference(g, i, swap):
    name, fi, box, draws, (cw, ch) = TC.BOX_CASES[i]
    rec, labels = box_case_items(i)
    frames = composed_frames_b() if swap else TC.frames("b")
    crops, flags = TR.train_crops(frames, rec, cw, ch, 3, 2)
    tag = "bg" if swap else "box"
    assert flags.tolist() == [int(g[tag + "_flags"][i])] == [0]
    want = golden_crop(g, tag, i)
    assert np.array_equal(bits(crops[0]), bits(want)), "%s: %d pixels differ" % (name, int((bits(crops[0]) != bits(want)).sum()))
    assert np.array_equal(bits(labels[0]), bits(g[tag + "_labels"][i])), name
    assert rec[0].window == 0 and rec[0].warp == (0 if draws is None else 1)


def test_padded_and_unpadded_boxes_are_both_covered():
    pads = [box_case_items(i)[0][0].padded for i in range(len(TC.BOX_CASES))]
    assert 0 in pads and 1 in pads and sum(pads) >= 6


def test_itop_boxes_equal_the_scripts_construction(g):
    lt, rb = AJ.itop_boxes(TC.itop_centres())
    assert lt.dtype == np.float32 and np.array_equal(bits(lt), bits(g["itop_boxes_lefttop"])) and np.array_equal(bits(rb), bits(g["itop_boxes_rightbottom"]))
    assert (AJ.A2J_ITOP.fx, AJ.A2J_ITOP.fy, AJ.A2J_ITOP.u0, AJ.A2J_ITOP.v0, AJ.A2J_ITOP.xy_thres, AJ.A2J_ITOP.depth_thres) == (286, -286, 160, 120, 120, 0.4)


def test_map_back_rows_file_and_both_errors_equal_the_reference(g, tmp_path):
    votes, target, centres = TC.map_back_inputs()
    rows = AJ.write_txt_rows(votes, centres)
    assert rows.shape == (len(votes), 45) and np.array_equal(bits(rows), bits(g["txt_rows"]))
    AJ.write_txt(tmp_path / "result.txt", rows)
    assert open(tmp_path / "result.txt").read() == str(g["txt_text"])
    ref = AJ.error_compute(votes, target, centres, as_reference=True)
    assert isinstance(ref, np.float32) and bits(ref) == bits(g["err_reference"])
    err = AJ.error_compute(votes, target, centres)
    assert bits(err) == bits(g["err_default"]) and bits(err) != bits(ref)
    # the script's own box has no width: every joint lands on the centre pixel, whatever the votes say
    moved = votes.copy()
    moved[:, :, :2] += 17.0
    assert bits(AJ.error_compute(moved, target, centres, as_reference=True)) == bits(ref)
    assert bits(AJ.error_compute(moved, target, centres)) != bits(err)


class _Recorder:
    def __init__(self, monkeypatch):
        self.log = []
        monkeypatch.setattr(np.random, "randint", lambda lo, hi: (self.log.append("randint(%d, %d)" % (lo, hi)), 701 if hi == 1700 else 1)[1])
        monkeypatch.setattr(np.random, "rand", lambda: (self.log.append("rand()"), 0.25)[1])
        monkeypatch.setattr(np.random, "normal", lambda mu, sigma, n: (self.log.append("normal(%g, %g, %d)" % (mu, sigma, n)), np.zeros(n))[1])


@pytest.mark.parametrize("form,key", [("itop", "itop_draw_log"), ("box", "box_draw_log")])
def test_sampler_draws_in_the_references_order(g, monkeypatch, form, key):
    want = [str(s) for s in g[key]]
    assert len(want) == 7 and want[4].startswith("normal(")
    rec = _Recorder(monkeypatch)
    d = AJ.A2JCropSampler(form, TC.CROP_W, TC.CROP_H, exact_stream=True).draw()
    assert rec.log == want
    assert d == dict(offsets=(1, 1, 1, 1), rotate=1, scale=0.25 * 1.0 + 0.5 if form == "itop" else 701 / 1000)
    rec.log.clear()
    AJ.A2JCropSampler(form, TC.CROP_W, TC.CROP_H).draw()
    assert rec.log == want[:4] + want[5:]


def test_rotation_matrix_and_inversion_equal_the_restated_opencv():
    for (cx, cy), rot, scale in (((32.0, 24.0), -10, 0.5), ((144.0, 144.0), 9, 1.699), ((32.0, 24.0), 0, 1)):
        M = warp_affine.rotation_matrix((cx, cy), rot, scale)
        assert np.array_equal(M, WR.getRotationMatrix2D((cx, cy), rot, scale))
        assert warp_affine.invert_affine(M) == WR.invert_affine(M)


def test_items_refuse_non_finite_boxes_and_count_their_draws():
    bnd, k2, k3 = TC.box_arrays()
    bad = bnd.copy()
    bad[0, 2] = np.nan
    with pytest.raises(_lib.PopnetError, match="item 0"):
        AJ.box_items([0], bad, k2, k3, TC.SETS["b"])
    rec, labels = AJ.box_items([], bnd, k2, k3, TC.SETS["b"])
    assert len(rec) == 0 and labels.shape == (0, 15, 3)


def test_read_centres_drops_the_frame_of_an_invalid_line(tmp_path):
    p = tmp_path / "center_test.txt"
    p.write_text("150.5 110.25 2.75\ninvalid invalid invalid\n20 200 3.125\n")
    centres, kept, n = AJ.read_centres(p)
    assert centres.shape == (2, 1, 3) and centres.dtype == np.float32 and kept.tolist() == [0, 2] and n == 3
    assert centres[1, 0].tolist() == [20.0, 200.0, 3.125]


@pytest.mark.parametrize("lines", [2, 4], ids=["fewer", "more"])
def test_itop_a2j_set_refuses_a_centre_file_of_another_length(tmp_path, lines):
    """Three frames: a centre file with two or four lines (invalid ones count) is refused, one with three is taken."""
    import json
    from popnet_amd import targets
    json.dump({"f%d" % i: [{"3d_joints": [[1.0, 2.0, 3.0]] * 15}] for i in range(3)}, open(tmp_path / "labels.json", "w"))
    (tmp_path / "c.txt").write_text("invalid invalid invalid\n" + "10 20 2.5\n" * (lines - 1))
    with pytest.raises(_lib.PopnetError, match="%d lines" % lines):
        targets.ItopA2JSet(str(tmp_path), str(tmp_path / "labels.json"), str(tmp_path / "c.txt"), device="cpu")
    (tmp_path / "c.txt").write_text("invalid invalid invalid\n" + "10 20 2.5\n" * 2)
    s = targets.ItopA2JSet(str(tmp_path), str(tmp_path / "labels.json"), str(tmp_path / "c.txt"), device="cpu")
    assert s.ids == ["f1", "f2"] and s.keypoints.shape == (2, 15, 3)
