"""CPU: the random training transform without a GPU.

  * tests/cv2_warp_reference.augment_reference (pure numpy) == the reference's own Rotate / RenderDepth / Crop / Resize classes run
    through KDH3D_Keypoints.__getitem__ (tests/golden/augment.npz), item by item: image, integer geometry, z and boxes bit for bit;
    the rotated 2-D joints within 1 float32 ulp (they are float64 3-term dot products rounded to float32, and a BLAS that fuses
    differently can move the float64 result by one of its ulps, hence at most one float32 step).
  * the package's host half (popnet_amd.targets.augmentation / AugmentationBatch.transform_labels) == the same golden, same bars.
  * a seeded MPAugSampler.batch(augment=True) reproduces the golden's source picks and draws in order; augment=False consumes the
    draws the sampler consumed before the option existed.
"""
import random

import numpy as np
import pytest

import augment_helpers as ah
import cv2_warp_reference as cw
from augment_helpers import G


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    d = tmp_path_factory.mktemp("augment_tree")
    ah.write_tree(d)
    return d


def test_the_golden_covers_the_boundary_cases():
    shapes = {str(G["names"][ci]): G["it%d_shapes" % ci].tolist() for ci in range(ah.N)}
    draws = {str(G["names"][ci]): G["it%d_draws" % ci] for ci in range(ah.N)}
    assert ah.N >= 6 and sum(not bool(G["it%d_scripted" % ci]) for ci in range(ah.N)) >= 2
    assert {draws[n][0] for n in draws} >= {0.0, 10.0, -10.0} and {draws[n][1] for n in draws} >= {0.7, 1.7}
    assert tuple(draws["rot0_a0.7_crop0"][2:]) == (0, 0, 0, 0) and tuple(draws["rot10_a1.7_crop0.1"][2:]) == (0.1, 0.1, 0.1, 0.1)
    assert shapes["rot-10_mixed"][1] == [ah.H + 3, ah.W + 2]      # zero image, dx = 0, dy = 1: (new_ymax + 1 + 1) x (new_xmax + 1)
    assert shapes["both_truncate"][1] == [ah.H, ah.W]             # the a <= 1 slice with its end clamped to the frame
    assert "list indices must be integers or slices" in str(G["json_list_error"])


def test_augment_reference_equals_the_reference_classes_on_every_item(tree):
    from oracle import cv2_resize, targets as ot
    for ci in range(ah.N):
        image, persons = ah.composed(tree, ci)
        img, labels, geo = cw.augment_reference(image, persons, ah.item_params(ci))
        want_shapes = G["it%d_shapes" % ci].tolist()
        assert [list(geo["rotate_shape"]), list(geo["render_shape"]), list(geo["crop_shape"]), list(img.shape)] == want_shapes, ci
        kp = np.stack([lb["2d_joints"] for lb in labels])
        assert kp.dtype == np.float32 and ah.ulp_distance_f32(kp, G["it%d_kp2d" % ci]).max() <= 1, ci
        assert np.array_equal(np.stack([lb["3d_joints"] for lb in labels]), G["it%d_kp3d" % ci]), ci
        assert np.array_equal(np.stack([lb["bbox"] for lb in labels]), G["it%d_bbox" % ci]), ci
        x = cw.network_input(img, 6.0, 3.0, 2.0)
        assert np.array_equal(x[None], G["it%d_image" % ci]), (ci, np.abs(x[None] - G["it%d_image" % ci]).max())
        # the four target maps from the golden's own labels and this image: the rest of __getitem__, as oracle.targets states it
        clamped = cw.network_input(img, 6.0, 0.0, 1.0)
        dr = cv2_resize.resize(clamped, (28, 28), interpolation=cv2_resize.INTER_LINEAR)
        heat, paf, z, fg = ot.ground_truth(G["it%d_kp2d" % ci], G["it%d_kp3d" % ci], dr)
        for name, a in (("heat", heat), ("paf", paf), ("z", z), ("fg", fg)):
            assert np.array_equal(a.transpose(2, 0, 1).astype(np.float32), G["it%d_%s" % (ci, name)]), (ci, name)


def test_host_geometry_and_label_transform_equal_the_reference_classes(tree):
    from popnet_amd import targets
    for ci in range(ah.N):
        p = ah.item_params(ci)
        it = targets.augmentation(p["rot"], p["a"], p["crops"], ah.H, ah.W, p["cx"], p["cy"], p["input_size"])
        shapes = G["it%d_shapes" % ci].tolist()
        assert [it["render_h"], it["render_w"]] == shapes[1] and [it["src_h"], it["src_w"]] == shapes[2], ci
        _, _, geo = cw.augment_reference(*ah.composed(tree, ci), p)
        assert it["render_corner"] == geo["render_corner"] and it["render_a"] == geo["render_a"] and it["crop_bounds"] == geo["crop_bounds"], ci
        assert list(it["inv_mat"]) == cw.invert_affine(cw.getRotationMatrix2D((p["cx"], p["cy"]), p["rot"], 1.0)), ci
        _, _, _, persons = ah.item_sources(tree, ci)
        k2 = np.array([ps["2d_joints"] for ps in persons], dtype=np.float32)[None]
        k3 = np.array([ps["3d_joints"] for ps in persons], dtype=np.float64)[None]
        bb = np.array([ps["bbox"] for ps in persons], dtype=np.float64)[None]
        kp, kz, bx = targets.AugmentationBatch([it]).transform_labels(k2, k3, bb)
        assert kp.dtype == np.float32 and ah.ulp_distance_f32(kp[0], G["it%d_kp2d" % ci]).max() <= 1, ci
        assert np.array_equal(kz[0], G["it%d_kp3d" % ci][:, :, 2]) and np.array_equal(bx[0], G["it%d_bbox" % ci]), ci
        assert np.array_equal(k2[0], np.array([ps["2d_joints"] for ps in persons], dtype=np.float32))      # the inputs are left alone


def test_geometry_the_reference_cannot_run_is_refused():
    from popnet_amd import _lib, targets
    with pytest.raises(_lib.PopnetError, match="empty"):
        targets.augmentation(0.0, 0.001, (0, 0, 0, 0), 32, 32, 16.0, 16.0)
    with pytest.raises(_lib.PopnetError, match="Crop"):
        targets.augmentation(0.0, 1.0, (0.6, 0.6, 0, 0), 32, 32, 16.0, 16.0)


def _sources_as_before(set_sizes, n_bg, index):
    """MPAugSampler.sources as it stood before `augment` existed: the draws of KDH3D_Keypoints.__getitem__ (:234-262)."""
    from popnet_amd.targets import AUG_MODS
    mod = AUG_MODS[random.randint(0, len(AUG_MODS) - 1)]
    src = [(ii, index % set_sizes[ii]) for ii in mod if not random.uniform(0, 1) > 0.8]
    if not src:
        ii = random.randint(0, len(set_sizes) - 1)
        src.append((ii, index % set_sizes[ii]))
    return src, index % n_bg


def test_seeded_sampler_reproduces_the_goldens_picks_and_draws_in_order():
    from popnet_amd.targets import MPAugSampler
    seeded = [ci for ci in range(ah.N) if not bool(G["it%d_scripted" % ci])]
    assert seeded == list(range(len(seeded)))                 # the seeded items come first in the recipe
    s = MPAugSampler([G["ids"].shape[1]] * G["ids"].shape[0], len(G["bgs"]))
    random.seed(9)                                            # the recipe's seed before its first item
    src, n_src, bg, aug = s.batch([int(G["it%d_index" % ci]) for ci in seeded], augment=True, H=ah.H, W=ah.W, cx=ah.CX, cy=ah.CY, max_ratio=1.7, input_size=ah.S)
    for r, ci in enumerate(seeded):
        assert src[r, :n_src[r], 0].tolist() == G["it%d_picks" % ci].tolist(), ci
        it = aug.items[r]
        assert [it["rot"], it["a"]] + list(it["crops"]) == G["it%d_draws" % ci].tolist(), ci
    assert random.random() == float(G["next_after_random_items"])


def test_default_batch_consumes_the_draws_it_consumed_before():
    from popnet_amd.targets import MPAugSampler
    sizes, indices = [7, 5, 9, 4, 6], list(range(40))
    for seed in (0, 1, 2):
        random.seed(seed)
        want = [_sources_as_before(sizes, 3, i) for i in indices]
        after = random.random()
        for kw in ({}, {"augment": False}):
            random.seed(seed)
            src, n_src, bg = MPAugSampler(sizes, 3).batch(indices, **kw)
            assert random.random() == after
            for r, (s_, b_) in enumerate(want):
                assert [tuple(v) for v in src[r, :n_src[r]].tolist()] == s_ and int(bg[r]) == b_
        random.seed(seed)
        MPAugSampler(sizes, 3).batch(indices, augment=True, H=64, W=48, cx=20.0, cy=30.0)
        assert random.random() != after                       # six more draws per item
