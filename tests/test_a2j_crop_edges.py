"""The rows of tests/a2j_crop_cases.py without a GPU: the numpy restatement of the inference crop (tests/a2j_crop_reference.py) against the
reference's own outputs on every row (tests/golden/a2j_crop_edges.npz: digests and flags of dataPreprocess itself), against the 11 stored
crops of a2j_crops.npz, and against the other derivation of the same rule, popnet_amd.a2j_crops.box_items + the training-crop restatement;
the explicit paste loop against the vectorised paste; and the census: how many rows sit in each class, counted from the restatement's own
intermediate values.  Measured on both sets together (1468 rows): 215 rows on which the reference raises, 105 / 96 with a negative slice end in x / y (44 of them
unpadded and valid: the far-edge rule of Python's slice decides their crop), 53 whose paste is bounded by the crop's own size."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2j_cases as AC  # noqa: E402
import a2j_crop_cases as CC  # noqa: E402
import a2j_crop_reference as CR  # noqa: E402
import a2j_traincrop_reference as TR  # noqa: E402
from popnet_amd import a2j_crops as AJ  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [(name, cwh, None) for name in CC.SETS for cwh in CC.CROPS] + [(name, CC.LARGE, "large") for name in CC.SETS]
f32 = np.float32


def case_rows(name, which):
    rows = CC.rows(name)
    return rows if which is None else rows[CC.large_index(name)]


@pytest.fixture(scope="module")
def restated():
    """(set, crop size) -> (rows, crops, flags, infos) of the restatement, computed once and left unchanged"""
    out = {}
    for name, cwh, which in SIZES:
        rows = case_rows(name, which)
        out[(name, cwh)] = (rows,) + CR.crops(CC.frames(name), rows, CC.IMG_WH, cwh)
    return out


def same_bits(a, b):
    nan = np.isnan(b)
    return bool(np.isnan(a[nan]).all()) and np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan])


@pytest.mark.parametrize("name,cwh,which", SIZES, ids=["%s_%dx%d" % (n, c[0], c[1]) for n, c, _ in SIZES])
def test_restatement_equals_the_reference_on_every_row(restated, name, cwh, which):
    g = np.load(os.path.join(GOLDEN, "a2j_crop_edges.npz"))
    rows, crops, flags, _ = restated[(name, cwh)]
    key = "%s_%dx%d" % (name, cwh[0], cwh[1])
    assert np.array_equal(g["%s_rows" % name].view(np.uint32), CC.rows(name).view(np.uint32))          # the fixture is of these rows
    assert len(g[key + "_flags"]) == len(rows) == (CC.N_LARGE if which else len(CC.rows(name)))
    assert np.array_equal(flags, g[key + "_flags"].astype(np.int32)), np.nonzero(flags != g[key + "_flags"])[0]
    bad = [k for k in range(len(rows)) if not np.array_equal(CR.digest(crops[k]), g[key + "_sha256"][k])]
    assert not bad, "%d rows differ from the reference, the first: %s" % (len(bad), rows[bad[0]])
    assert all(not crops[k].any() for k in np.nonzero(flags)[0])


def test_restatement_equals_the_stored_crops_of_the_large_frame():
    g = np.load(os.path.join(GOLDEN, "a2j_crops.npz"))
    crops, flags, _ = CR.crops(AC.depth_frames(AC.SEED + 2, 1), g["rows"], (480, 512), (288, 288))
    assert len(crops) == 11 and not flags.any()
    for k, name in enumerate(g["names"]):
        assert np.array_equal(crops[k].view(np.uint32), g["crops"][k].view(np.uint32)), name


@pytest.mark.parametrize("name", list(CC.SETS))
def test_explicit_paste_loop_equals_the_vectorised_paste_on_every_row(restated, name):
    rows, crops, flags, infos = restated[(name, CC.CROPS[0])]
    c2, f2, i2 = CR.crops(CC.frames(name), rows, CC.IMG_WH, CC.CROPS[0], paste=CR.paste_loop)
    assert np.array_equal(flags, f2)
    assert all(same_bits(a, b) for a, b in zip(c2, crops))
    assert [(i.get("pasted"), i.get("size_bound")) for i in infos] == [(i.get("pasted"), i.get("size_bound")) for i in i2]
    assert sum(1 for i in infos if i.get("pasted", 0) > 0) > 150


@pytest.mark.parametrize("name,cwh,which", SIZES, ids=["%s_%dx%d" % (n, c[0], c[1]) for n, c, _ in SIZES])
def test_box_items_and_the_training_restatement_give_the_same_crops(restated, name, cwh, which):
    """The host geometry the trainers upload (box_items without draws: no warp) and the inference rule, on every row above the confidence
    threshold with finite coordinates: equal crops, equal flags."""
    rows, crops, flags, _ = restated[(name, cwh)]
    keep = [k for k, r in enumerate(rows) if r[5] > f32(0.01) and np.isfinite(r[1:5]).all()]
    assert len(keep) > (0.9 * len(rows) if which is None else 5)
    P = 15
    items, _ = AJ.box_items(keep, rows[:, 1:5], np.zeros((len(rows), P, 2), f32), np.zeros((len(rows), P, 3), f32), CC.SETS[name], draws=None,
                            crop_w=cwh[0], crop_h=cwh[1], img_wh=CC.IMG_WH, frames=[int(rows[k][0]) for k in keep])
    got, gflags = TR.train_crops(CC.frames(name), items, cwh[0], cwh[1], 3, 2)
    assert np.array_equal(gflags, flags[keep])
    bad = [k for j, k in enumerate(keep) if not same_bits(got[j], crops[k])]
    assert not bad, "%d rows differ, the first: %s" % (len(bad), rows[bad[0]])


def census():
    """class -> number of rows, both sets together, from the rows and the restatement's intermediate values at 64 x 48"""
    n = {}

    def count(name, cond):
        n[name] = n.get(name, 0) + int(bool(cond))

    iw, ih = CC.IMG_WH
    for name, (H, W) in CC.SETS.items():
        rows = CC.rows(name)
        _, flags, infos = CR.crops(CC.frames(name), rows, CC.IMG_WH, CC.CROPS[0])
        for r, fl, i in zip(rows, flags, infos):
            fr, x0, y0, x1, y1, conf = r
            t, ok = i["taken"], i["taken"] and not fl
            sides = (x0 < 0, y0 < 0, x1 > iw, y1 > ih)
            count("unpadded_inside", ok and not i["padded"])
            for k, side in enumerate(("left", "top", "right", "bottom")):
                count(side + "_alone", ok and sides == tuple(j == k for j in range(4)))
            count("all_four_sides", ok and all(sides))
            count("image_not_frame_x", ok and iw < x1 <= W - 1)
            count("frame_not_image_x", ok and W - 1 < x1 <= iw)
            count("image_not_frame_y", ok and ih < y1 <= H - 1)
            count("frame_not_image_y", ok and H - 1 < y1 <= ih)
            count("negative_end_x", t and i.get("cx1", 0) < 0)
            count("negative_end_y", t and i.get("cy1", 0) < 0)
            count("negative_end_unpadded_valid", ok and not i["padded"] and (i["cx1"] < 0 or i["cy1"] < 0))
            count("start_past_frame_x", t and i.get("cx0", 0) >= W)
            count("start_past_frame_y", t and i.get("cy0", 0) >= H)
            count("i_equals_start", ok and i["padded"] and i["start1"] > 0 and i["start1"] == int(i["start1"]) and i["start1"] < min(i["end1"], i["sh"]) and i["pasted"] > 0)
            count("j_equals_start", ok and i["padded"] and i["start2"] > 0 and i["start2"] == int(i["start2"]) and i["start2"] < min(i["end2"], i["sw"]) and i["pasted"] > 0)
            for tag, vals, lo, hi in (("x", (0.0, -0.0, iw, np.nextafter(f32(iw), f32(np.inf)), W - 1, W), x0, x1), ("y", (0.0, -0.0, ih, np.nextafter(f32(ih), f32(np.inf)), H - 1, H), y0, y1)):
                for k, v in enumerate(vals):
                    hit = lambda e: e == f32(v) and (v != 0 or bool(np.signbit(e)) == (k == 1))
                    count("%s_edge_at_%s" % (tag, ("0", "-0", "img", "img_next", "size-1", "size")[k]), t and (hit(lo) or hit(hi)))
            for pad in (True, False):
                p = "padded" if pad else "unpadded"
                count("height_0_%s" % p, t and i["padded"] == pad and i.get("sh") == 0 and fl)
                count("width_0_%s" % p, t and i["padded"] == pad and i.get("sw") == 0 and fl)
                count("height_1_%s" % p, ok and i["padded"] == pad and i["sh"] == 1)
                count("width_1_%s" % p, ok and i["padded"] == pad and i["sw"] == 1)
            count("float32_height_truncates_apart", ok and i["padded"] and int(y1 - y0) != int(float(y1) - float(y0)))
            count("float32_width_truncates_apart", ok and i["padded"] and int(x1 - x0) != int(float(x1) - float(x0)))
            count("conf_at_threshold", conf == f32(0.01))
            count("conf_next_above_threshold", conf == np.nextafter(f32(0.01), f32(1)))
            count("conf_0", conf == 0)
            count("conf_nan", np.isnan(conf))
            count("low_conf_nan_coordinates", not t and np.isnan(r[1:5]).any())
            count("no_detection", np.array_equal(r[1:], f32([-1, -1, -1, -1, 0])))
            count("last_frame", fr == CC.N_FRAMES - 1)
            count("paste_bound_by_the_crops_size", ok and i.get("size_bound", 0) > 0)
            count("reference_raises", fl)
            count("rows", True)
    return n


def test_class_census():
    n = census()
    print("\nA2J CROP CENSUS: " + ", ".join("%s %d" % kv for kv in n.items()))
    assert len(n) == 49
    small = {k: v for k, v in n.items() if v < 8}
    assert not small, small
    # the threshold itself is not above the threshold, its neighbour is: both as the script's float32 comparison has them
    assert not (f32(0.01) > 0.01) and np.nextafter(f32(0.01), f32(1)) > 0.01


def test_hostile_and_bad_frame_rows_are_flagged_by_the_restatement():
    for name in CC.SETS:
        for rows in (CC.hostile_rows(name), CC.bad_frame_rows(name)):
            crops, flags, _ = CR.crops(CC.frames(name), rows, CC.IMG_WH, CC.CROPS[1])
            assert flags.all() and not crops.any()
        assert len(CC.hostile_rows(name)) == 16
        allr, ia, ib = CC.all_rows(name)
        assert np.array_equal(allr[ia].view(np.uint32), CC.rows(name).view(np.uint32)) and np.array_equal(allr[ib].view(np.uint32), CC.hostile_rows(name).view(np.uint32))
        assert len(allr) == len(ia) + len(ib) and ib.min() > 0 and ib.max() < len(allr) - 1      # each has a row before and after it


@pytest.mark.parametrize("name", list(CC.SETS))
def test_the_size_test_of_the_paste_implies_its_end_test(restated, name):
    """`end = size + start` is implied by `int(i - start) < size`: leaving the ends at the paste image's size changes no pixel of any row.  So
    the wrong reference of the GPU test is end = size (the start dropped), which does change the rows that cross a near and a far side."""
    rows, crops, flags, _ = restated[(name, CC.CROPS[0])]
    none = CR.crops(CC.frames(name), rows, CC.IMG_WH, CC.CROPS[0], end_rule="none")
    assert np.array_equal(none[1], flags) and all(same_bits(a, b) for a, b in zip(none[0], crops))
    wrong = CR.crops(CC.frames(name), rows, CC.IMG_WH, CC.CROPS[0], end_rule="no_start")
    assert sum(1 for a, b in zip(wrong[0], crops) if not same_bits(a, b)) >= 8
