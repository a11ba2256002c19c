"""CPU: the numpy restatement of the parse outside its default arguments (tests/parse_options_reference.py) equals the reference's own
output (tests/golden/parse_options.npz, written by tests/golden/make_golden_parse_options.py) bit for bit for every stored entry; its frozen
Gaussian weights are scipy's; and each rule it adds to oracle/parse_paf.py is visible in some stored case: a mutant of the rule differs
from the golden there."""
import functools
import os

import numpy as np
import pytest

import parse_cases as PC
import parse_options_reference as PR
from oracle import cv2_resize as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parse_options.npz")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


@functools.lru_cache(maxsize=None)
def paf_up(name, f):
    return R.resize(np.ascontiguousarray(PC.case(name).paf), None, fx=f, fy=f, interpolation=R.INTER_CUBIC)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b)


def nms_differs(name, f, refine, gauss, **mut):
    g = golden()
    key = "nms/%s/%s" % (name, PR.nms_key(f, refine, gauss))
    peaks, counts = PR.flat_peaks(PR.nms(PC.case(name).heat, f, refine, gauss, **mut))
    return not (same(peaks, g[key + "/peaks"]) and np.array_equal(counts, g[key + "/counts"]))


def parse_differs(name, f, n, **mut):
    g = golden()
    key = "parse/%s/%s" % (name, PR.parse_key(f, n))
    c = PC.case(name)
    jl, assoc, conn = PR.paf_to_pose(c.heat, c.paf, f, n, paf_up=paf_up(name, f), **mut)
    return not (same(np.asarray(jl).reshape(-1, 5), g[key + "/joint_list"]) and same(np.asarray(assoc).reshape(-1, PR.J + 2), g[key + "/assoc"])
                and same(PR.flat_connections(conn), g[key + "/conn"]))


def test_the_golden_holds_every_case_and_option_set_of_the_lists():
    g = golden()
    assert tuple(g["nms_cases"]) == PR.NMS_CASES and tuple(g["parse_cases"]) == PR.PARSE_CASES
    assert [tuple(o) for o in g["nms_options"]] == [(f, int(r), int(x)) for f, r, x in PR.NMS_OPTIONS]
    assert [tuple(o) for o in g["parse_options"]] == list(PR.PARSE_OPTIONS)
    want = {"nms/%s/%s/%s" % (c, PR.nms_key(*o), leaf) for c in PR.NMS_CASES for o in PR.NMS_OPTIONS for leaf in ("peaks", "counts")}
    want |= {"nms/%s/%s/%s" % (PR.NMS_BIG[0], PR.nms_key(*PR.NMS_BIG[1]), leaf) for leaf in ("peaks", "counts")}
    want |= {"parse/%s/%s/%s" % (c, PR.parse_key(*o), leaf) for c in PR.PARSE_CASES for o in PR.PARSE_OPTIONS for leaf in ("joint_list", "assoc", "conn")}
    assert {k for k in g if "/" in k} == want
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_frozen_gaussian_weights_are_the_goldens_and_scipys_bit_for_bit():
    assert np.array_equal(PR.GAUSS_W, golden()["gauss_weights"])
    from scipy.ndimage import _filters
    w = _filters._gaussian_kernel1d(3.0, 0, PR.GAUSS_RADIUS)
    assert w.dtype == np.float64 and np.array_equal(w[:13], PR.GAUSS_W) and np.array_equal(w[::-1][:13], PR.GAUSS_W)


def test_gaussian_restatement_equals_scipy_on_random_float32_patches():
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(3)
    for h, w in [(3, 3), (3, 4), (5, 3), (4, 5), (5, 5), (6, 10), (12, 20), (24, 25), (40, 40), (48, 80), (80, 80)]:
        x = rng.standard_normal((h, w)).astype(np.float32)
        got, want = PR.gaussian_sigma3(x), gaussian_filter(x, sigma=3)
        assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want), (h, w)


@pytest.mark.parametrize("name", PR.NMS_CASES)
def test_nms_restatement_equals_the_reference_for_every_option_set(name):
    bad = [o for o in PR.NMS_OPTIONS if nms_differs(name, *o)]
    assert not bad, bad


def test_nms_restatement_equals_the_reference_on_the_largest_map_with_the_filter():
    assert not nms_differs(PR.NMS_BIG[0], *PR.NMS_BIG[1])


@pytest.mark.parametrize("name", PR.PARSE_CASES)
def test_parse_restatement_equals_the_reference_for_every_option_set(name):
    bad = [o for o in PR.PARSE_OPTIONS if parse_differs(name, *o)]
    assert not bad, bad


def test_the_default_call_of_the_reference_is_among_the_stored_option_sets():
    assert (1, True, False) in PR.NMS_OPTIONS and (8, 10) in PR.PARSE_OPTIONS


# ---- one mutant per new rule: the stored cases can see it ----
def _some(differs, cases, options, **mut):
    return [(c, o) for c in cases for o in options if differs(c, *o, **mut)]


def test_mutant_gaussian_axes_swapped_differs_on_a_stored_case():
    assert _some(nms_differs, ("corners", "plateau_5x7"), [(8, True, True), (1, True, True)], swap_axes=True)


def test_mutant_edge_border_instead_of_reflect_differs_on_a_stored_case():
    assert _some(nms_differs, ("corners", "plateau_5x7"), [(8, True, True), (1, True, True)], edge=True)


def test_mutant_sequential_mean_at_16_points_differs_on_a_stored_case():
    assert _some(parse_differs, ("corners", "wide", "cnt"), [(8, 16)], seq_mean=True)


def test_mutant_criterion1_with_ge_differs_on_a_stored_case():
    assert _some(parse_differs, ("cnt", "plateau_5x7", "corners"), [(8, 10), (1, 5)], cnt_ge=True)


def test_unfiltered_and_filtered_and_unrefined_peaks_differ_so_the_flags_are_seen():
    g = golden()
    a, b, c = (g["nms/corners/%s/peaks" % PR.nms_key(8, r, x)] for r, x in ((True, False), (True, True), (False, False)))
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(c, g["nms/corners/%s/peaks" % PR.nms_key(8, False, True)])      # the filter flag is ignored without refinement
