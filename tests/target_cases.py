"""Hand-placed annotations for the training-target rasteriser and the depth compositor, a census of what they contain, and
mutants of the oracle (no GPU).

rasterize_kernel and compose_depth_kernel (popnet_amd/csrc/targets.hip) promise agreement with oracle/targets.py: fg, z and paf
bit for bit, heat within one float32 ulp at 1.  The golden annotations only run them at 224 x 224 with stride 8; the cases here
use network inputs that are not square (so that x / y and gh / gw cannot change places unseen), stride 4, a 3 x 8 and a one-cell
grid, and put joints on the kernel's decision points: exactly on 0 and on input_x / input_y, limb ends on pixel s*m + s/2 (the
PAF box edges min - 1 and max + 1 are then exact halves, which separate round-half-even from half-away), a zero-length limb,
cells at distance exactly 1 from a limb, three persons on one limb cell, saturated heat, overlapping z windows, and cells next to
and exactly on the exponent cut 4.6052.

  GEOMETRIES     (input_x, input_y, stride, z_radius, sigma)
  cases()        annotations per geometry: kp2d [P,15,2] float32, kp_z [P,15] float64, depth_resize [gh,gw] float32
  ground_truth   a restatement of oracle.targets.ground_truth with flags: no flag == the oracle (asserted in
                 test_target_cases.py), one flag == a mutant
  census         what a case contains, counted with the same arithmetic as oracle.targets
  MUTANTS        every one must change the compared output of some case
  compose_cases  inputs of the compositor

Three variants look like mutants and are not, because no input can tell them from the oracle:
  * flooring the z window instead of truncating it: int() and floor differ only below zero, and the window's lower edge is
    clamped at 0, its upper edge cx + r is never negative for a joint that passed the bounds test;
  * the clamp at 1 applied once after all persons: every addend is >= 0, so once the sum passes 1 it stays clamped and
    min(1, .) of the running sum equals the running clamp, in the same order of additions;
  * the z map written by the nearest person: that IS what the oracle computes.  ``zk[new] = pz[new]`` only ever fires where
    the map holds 2 * depth_max or a value >= depth_max, where min(pz, z) is pz already, so z = the minimum over the persons
    whose window covers the cell, whoever comes first; fg is 1 if any of them is nearer than depth_max.  The mutant that can be
    seen is the opposite one, first_writer_z: the first foreground person keeps the cell.
And one is a mutant only in the last bits of a float64 intermediate: persons visited in reverse.  The heat sum, the PAF mean
and the z minimum do not depend on the order except through the rounding of float64 additions, which the float32 maps that are
compared show only on a rounding boundary; no case here sits on one.  (A mean of unit vectors weighted by the count is the plain
mean over the persons that cover the cell, so the two mutants of the average that can be seen are plain_mean, which divides by
every person who has the limb, and pair_mean, which halves the value so far.)
EQUIVALENT lists these three; test_target_cases.py asserts that no case tells them apart.
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import targets as OT

f32 = np.float32
CUT = 4.6052
OUT = -1000.0                      # a joint that is not annotated: outside the input
PAD = 1.0e9                        # what padded person slots hold

#            input_x, input_y, stride, z_radius, sigma
GEOMETRIES = ((224, 224, 8, 2, 7.0),
              (232, 200, 8, 2, 7.0),
              (200, 232, 8, 1, 7.0),
              (224, 224, 4, 3, 7.0),
              (64, 24, 8, 2, 7.0),
              (8, 8, 8, 2, 7.0))


def grid(geom):
    return int(geom[1] / geom[2]), int(geom[0] / geom[2])          # gh, gw


# ---------------------------------------------------------------------------------------------
# the oracle with room for a mutant
# ---------------------------------------------------------------------------------------------
def _round(v, half_away):
    return int(np.floor(v + 0.5) if v >= 0 else -np.floor(-v + 0.5)) if half_away else int(round(v))


def ground_truth(kp2d, kp3d_z, depth_resize, geom, half_away=False, clamp_once=False, plain_mean=False, pair_mean=False, nearest_z=False,
                 first_writer_z=False, cut_lt=False, bounds_gt=False, swap_grid=False, reverse=False, info=None):
    """oracle.targets.ground_truth, restated.  kp3d_z [P,15].  swap_grid: the cell index is taken apart with gh in place of gw."""
    input_x, input_y, stride, z_radius, sigma = geom
    DEPTH_MAX, DEPTH_MEAN, DEPTH_STD = OT.DEPTH_MAX, OT.DEPTH_MEAN, OT.DEPTH_STD
    kp2d = np.asarray(kp2d, dtype=np.float64).reshape(-1, 15, 2)
    kz = np.asarray(kp3d_z, dtype=np.float64).reshape(-1, 15)
    if reverse:
        kp2d, kz = kp2d[::-1], kz[::-1]
    P = kp2d.shape[0]
    gh, gw = int(input_y / stride), int(input_x / stride)
    if bounds_gt:
        bad = (kp2d[:, :, 0] > input_x) | (kp2d[:, :, 0] < 0) | (kp2d[:, :, 1] > input_y) | (kp2d[:, :, 1] < 0)
    else:
        bad = (kp2d[:, :, 0] >= input_x) | (kp2d[:, :, 0] < 0) | (kp2d[:, :, 1] >= input_y) | (kp2d[:, :, 1] < 0)
    inb = (~bad).astype(np.float64)
    cell = np.arange(gh * gw)
    if swap_grid:
        ys, xs = (cell // gh).reshape(gh, gw).astype(np.float64), (cell % gh).reshape(gh, gw).astype(np.float64)
    else:
        ys, xs = np.mgrid[0:gh, 0:gw].astype(np.float64)
    start = stride / 2.0 - 0.5
    heat = np.zeros((gh, gw, 16))
    for i in range(15):
        acc = np.zeros((gh, gw))
        for j in range(P):
            if inb[j, i] <= 0.5:
                continue
            d2 = (xs * stride + start - kp2d[j, i, 0]) ** 2 + (ys * stride + start - kp2d[j, i, 1]) ** 2
            e = d2 / 2.0 / sigma / sigma
            acc = acc + ((e < CUT) if cut_lt else (e <= CUT)) * np.exp(-e)
            if not clamp_once:
                acc[acc > 1.0] = 1.0
            if info is not None:
                info.setdefault("e", []).append(e)
        acc[acc > 1.0] = 1.0
        heat[:, :, i] = acc
    heat[:, :, 15] = np.maximum(1 - heat[:, :, :15].max(axis=2), 0.0)

    paf = np.zeros((gh, gw, 28))
    for l, (k1, k2) in enumerate(OT.LIMBS):
        vx, vy, cnt = np.zeros((gh, gw)), np.zeros((gh, gw)), np.zeros((gh, gw))
        sx, sy, nlimb = np.zeros((gh, gw)), np.zeros((gh, gw)), 0
        for j in range(P):
            if not (inb[j, k1] > 0.5 and inb[j, k2] > 0.5):
                if info is not None and (inb[j, k1] > 0.5) != (inb[j, k2] > 0.5):
                    info["one_end_out"] = info.get("one_end_out", 0) + 1
                continue
            a, b = kp2d[j, k1] / stride, kp2d[j, k2] / stride
            v = b - a
            n = np.linalg.norm(v)
            if n == 0.0:
                if info is not None:
                    info["zero_limbs"] = info.get("zero_limbs", 0) + 1
                continue
            u = v / n
            raw = (min(a[0], b[0]) - 1, max(a[0], b[0]) + 1, min(a[1], b[1]) - 1, max(a[1], b[1]) + 1)
            x0, x1 = max(_round(raw[0], half_away), 0), min(_round(raw[1], half_away), gw - 1)
            y0, y1 = max(_round(raw[2], half_away), 0), min(_round(raw[3], half_away), gh - 1)
            box = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
            width = np.abs((xs - a[0]) * u[1] - (ys - a[1]) * u[0])
            m = box & (width < 1)
            if info is not None:
                info["edges_half"] = info.get("edges_half", 0) + sum(1 for r in raw if _round(r, True) != _round(r, False))
                kind = "horizontal" if v[1] == 0 else "vertical" if v[0] == 0 else "diagonal"
                info.setdefault("dist1", {}).setdefault(kind, 0)
                info["dist1"][kind] += int((box & (width == 1.0)).sum())
            wx, wy = m * u[0], m * u[1]
            hit = (np.abs(wx) > 0) | (np.abs(wy) > 0)
            sx, sy = sx + wx, sy + wy
            nlimb += 1
            if pair_mean:                    # the mean of the value so far and the new one, not weighted by the count
                first = cnt == 0
                vx, vy = np.where(hit, np.where(first, wx, (vx + wx) / 2), vx), np.where(hit, np.where(first, wy, (vy + wy) / 2), vy)
                cnt = cnt + hit
                continue
            vx, vy = vx * cnt + wx, vy * cnt + wy
            cnt = cnt + hit
            div = np.where(cnt == 0, 1.0, cnt)
            vx, vy = vx / div, vy / div
        if plain_mean:                       # the mean over every person who has the limb, whether it covers the cell or not
            vx, vy = sx / max(nlimb, 1), sy / max(nlimb, 1)
        if info is not None:
            info["limb_cnt_max"] = max(info.get("limb_cnt_max", 0), int(cnt.max()) if cnt.size else 0)
        paf[:, :, 2 * l], paf[:, :, 2 * l + 1] = vx, vy

    zorg = np.repeat(np.asarray(depth_resize)[:, :, None], 15, axis=2)
    dt = zorg.dtype.type
    z = np.ones_like(zorg) * 2 * DEPTH_MAX
    fg = np.zeros((gh, gw, 15))
    seen_near = np.full((gh, gw, 15), np.inf)
    for j in range(P):
        for k in range(15):
            if inb[j, k] < 0.5:
                continue
            cx, cy = kp2d[j, k] / stride
            x0, x1 = max(int(int(cx - z_radius)), 0), min(int(int(cx + z_radius)), gw - 1)
            y0, y1 = max(int(int(cy - z_radius)), 0), min(int(int(cy + z_radius)), gh - 1)
            win = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
            pz = np.where(win, dt(kz[j, k]), dt(DEPTH_MAX))
            if info is not None:
                info["nearer_second"] = info.get("nearer_second", 0) + int((win & (fg[:, :, k] > 0) & (pz < z[:, :, k])).sum())
                info["behind_never_fg"] = info.get("behind_never_fg", 0) + int((win & (dt(kz[j, k]) >= DEPTH_MAX)).sum())
            if nearest_z:
                zk = np.minimum(pz, z[:, :, k])
                new = (pz < DEPTH_MAX) & (fg[:, :, k] == 0)
            elif first_writer_z:
                zk = z[:, :, k].copy()
                new = (pz < DEPTH_MAX) & (fg[:, :, k] == 0)
                zk[new] = pz[new]
            else:
                zk = np.minimum(pz, z[:, :, k])
                new = (pz < DEPTH_MAX) & (fg[:, :, k] == 0)
                zk[new] = pz[new]
            z[:, :, k] = zk
            fg[:, :, k] = np.logical_or(fg[:, :, k], new)
    z[fg == 0] = zorg[fg == 0]
    z[z < 0] = 0
    z[z > DEPTH_MAX] = DEPTH_MAX
    z = (z - DEPTH_MEAN) / DEPTH_STD
    return heat, paf, z, fg


MUTANTS = ("half_away", "plain_mean", "pair_mean", "first_writer_z", "cut_lt", "bounds_gt", "swap_grid")
EQUIVALENT = ("clamp_once", "nearest_z", "reverse")


def outputs_differ(a, b):
    for name, x, y in zip(("heat", "paf", "z", "fg"), a, b):
        if x.shape != y.shape or not np.array_equal(x.astype(f32), y.astype(f32)):
            return name
    return None


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def _person(joints, z=3.0):
    """{joint: (x, y) or (x, y, z)} -> (kp2d [15,2] float32, kp_z [15]); the other joints are not annotated"""
    kp, kz = np.full((15, 2), OUT, f32), np.full(15, float(z))
    for j, v in joints.items():
        kp[j] = v[:2]
        if len(v) > 2:
            kz[j] = v[2]
    return kp, kz


def _case(name, geom, persons, seed=0):
    gh, gw = grid(geom)
    rng = np.random.default_rng(seed + 1000 * gh + gw)
    depth = rng.uniform(-1.0, 8.0, (gh, gw)).astype(f32)                 # the clamps at 0 and at depth_max both fire on the background
    kp = np.stack([p[0] for p in persons]).astype(f32) if persons else np.zeros((0, 15, 2), f32)
    kz = np.stack([p[1] for p in persons]).astype(np.float64) if persons else np.zeros((0, 15))
    for a in (depth, kp, kz):
        a.setflags(write=False)
    return SimpleNamespace(name=name, geom=geom, kp2d=kp, kp_z=kz, depth=depth)


def _below(v):
    return np.nextafter(f32(v), f32(0))


def find_exact_cut_sigma(d2=512.0):
    """a sigma near 7 for which d2 / 2 / sigma / sigma is the double 4.6052 exactly (searched over the neighbours of the root)"""
    for D in (d2, 320.0, 640.0, 576.0, 832.0, 1024.0):          # 64 * (k^2 + l^2): offsets of whole cells
        s = np.sqrt(D / 2.0 / CUT)
        lo = hi = s
        for _ in range(4000):
            for c in (lo, hi):
                if D / 2.0 / c / c == CUT:
                    return float(c), D
            lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, 100.0)
    raise AssertionError("no sigma puts a cell on the cut")


def _cases_for(geom):
    X, Y, s, r, _ = geom
    gh, gw = grid(geom)
    h = s / 2.0
    C = []
    px = lambda m: s * m + h                                              # pixel s*m + s/2: the cell coordinate m + 0.5
    C.append(_case("nobody", geom, []))
    # joints on the bounds: 0 and the last float32 below input_x / input_y are inside, input_x / input_y are outside; limbs 1-2, 2-4
    # and 1-3 have one end outside, 8-9 and 1-0 lie along the right and the bottom edge
    C.append(_case("bounds", geom, [_person({0: (0, 0), 1: (_below(X), 0), 2: (X, h), 4: (h, Y), 3: (X, Y), 8: (_below(X), _below(Y)),
                                             9: (_below(X), 0), 5: (0, _below(Y)), 7: (h, _below(Y)), 10: (0, Y), 11: (X, 0)}, z=2.0)], seed=1))
    if gh == 1 and gw == 1:
        C.append(_case("one_cell_two_persons", geom, [_person({0: (1, 1, 4.0), 8: (2, 2, 5.0), 9: (6, 5, 5.0), 1: (3, 3)}),
                                                       _person({0: (4, 4, 2.5), 8: (6, 1, 7.0), 9: (1, 6, 1.0), 1: (3, 3, 6.0)})], seed=2))
        return C
    if gh < 8:
        # 3 x 8 cells: a horizontal limb on exact halves through the middle row, two more persons on it, windows clipped on every side
        C.append(_case("strip", geom, [_person({8: (px(1), px(1), 4.0), 9: (px(5), px(1), 4.5), 11: (px(5), px(2), 3.0), 0: (px(3), px(1), 5.0)}),
                                       _person({8: (px(0), px(0), 2.0), 9: (px(6), px(2), 2.5), 0: (px(3) + 3, px(1), 4.0)}),
                                       _person({8: (px(2), px(1), 6.0), 9: (px(7), px(1), 1.0), 0: (px(3), px(1) + 3, 3.0)})], seed=3))
        return C
    # limb ends on s*m + s/2: horizontal 8-9, vertical 9-11, diagonal 8-10, and a zero-length 10-12
    C.append(_case("halves", geom, [_person({8: (px(3), px(5)), 9: (px(9), px(5)), 11: (px(9), px(12)), 10: (px(8), px(10)), 12: (px(8), px(10)),
                                             1: (px(0), px(0)), 2: (px(gw - 1), px(0)), 0: (px(0), px(gh - 1))})], seed=4))
    # cells at distance exactly 1: a horizontal limb on y = 5 cells, a vertical one on x = 9 cells, a 3-4-5 diagonal (u = (0.6, 0.8))
    C.append(_case("distance_one", geom, [_person({8: (s * 2, s * 5), 9: (s * 9, s * 5), 11: (s * 9, s * 12), 1: (s * 2, s * 2), 2: (s * 8, s * 10),
                                                   4: (s * 14, s * 18), 10: (s * 2, s * 11), 12: (s * 2, s * 12.5)})], seed=5))
    # three persons crossing on one cell of limb 8-9 (and of 1-2 with a fourth who misses), different directions
    C.append(_case("crossing", geom, [_person({8: (s * 6.2, s * 10.3), 9: (s * 14.1, s * 10.6), 1: (s * 3.3, s * 4.1), 2: (s * 9.2, s * 4.4)}),
                                      _person({8: (s * 10.4, s * 6.1), 9: (s * 10.1, s * 15.2), 1: (s * 6.4, s * 1.2), 2: (s * 6.1, s * 8.3)}),
                                      _person({8: (s * 6.3, s * 6.4), 9: (s * 14.2, s * 14.9), 1: (s * 3.2, s * 1.3), 2: (s * 9.4, s * 7.2)}),
                                      _person({8: (s * 14.3, s * 6.2), 9: (s * 6.1, s * 14.4), 1: (s * 15.1, s * 15.3), 2: (s * 17.2, s * 15.1)})], seed=6))
    # the same joints 3 px apart: the heat of two persons passes 1 next to them, a third is added to the clamped value
    C.append(_case("saturated", geom, [_person({0: (px(6), px(7)), 3: (s * 11, s * 4)}), _person({0: (px(6) + 3, px(7)), 3: (s * 11, s * 4 + 3)}),
                                       _person({0: (px(6) + 6, px(7) + 1), 3: (s * 11 + 2, s * 4)})], seed=7))
    # overlapping z windows: the nearer person second (joint 0), first (joint 1), a person at and behind depth_max (2, 3), negative depth (4)
    C.append(_case("z_windows", geom, [_person({0: (s * 5.5, s * 5.5, 4.0), 1: (s * 12.5, s * 5.5, 2.0), 2: (s * 5.5, s * 12.5, 6.0), 3: (s * 12.5, s * 12.5, 7.5),
                                                4: (s * 9.5, s * 17.5, -0.5), 5: (0, 0, 3.0)}),
                                       _person({0: (s * 6.5, s * 6.5, 2.5), 1: (s * 13.5, s * 6.5, 4.5), 2: (s * 6.5, s * 13.5, 3.0), 3: (s * 13.5, s * 13.5, 5.0),
                                                4: (s * 10.5, s * 18.5, 1.0), 5: (s * 1.5, s * 1.5, 5.999)}),
                                       _person({0: (s * 7.5, s * 5.5, 3.25), 2: (s * 7.5, s * 12.5, 6.5)})], seed=8))
    # next to the exponent cut: joints on integer pixels put cell centres at half-integer offsets; d2 = 20.5^2 + 5.5^2 = 450.5 is the
    # last value inside the cut at sigma 7 (450.5 / 98 <= 4.6052 < 451.5 / 98)
    C.append(_case("cut", geom, [_person({0: (s * 5 + (h - 0.5) - 20.5, s * 3 + (h - 0.5) - 5.5), 1: (s * 10 + (h - 0.5) - 16, s * 10 + (h - 0.5) - 14)})], seed=9))        # and 16^2 + 14^2 = 452, the first outside
    return C


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for geom in GEOMETRIES:
        out += _cases_for(geom)
    # a sigma that puts cells exactly ON the cut: the joint sits on a cell centre, d2 is an integer sum of squares
    sigma, D = find_exact_cut_sigma()
    geom = (232, 200, 8, 2, sigma)
    out.append(_case("cut_exact", geom, [_person({0: (8 * 12 + 3.5, 8 * 11 + 3.5), 1: (8 * 3 + 3.5, 8 * 3 + 3.5)})], seed=10))
    return tuple(out)


def by_geometry():
    out = {}
    for c in cases():
        out.setdefault(c.geom, []).append(c)
    return out


_BASE = {}


def reference(c):
    """the oracle's own maps of the case"""
    if id(c) not in _BASE:
        X, Y, s, r, sigma = c.geom
        kp3d = np.zeros((len(c.kp2d), 15, 3))
        kp3d[:, :, 2] = c.kp_z
        _BASE[id(c)] = OT.ground_truth(c.kp2d, kp3d, c.depth, X, Y, s, r, sigma)
    return _BASE[id(c)]


def census(c):
    info = {}
    ground_truth(c.kp2d, c.kp_z, c.depth, c.geom, info=info)
    X, Y, s, r, sigma = c.geom
    kp = c.kp2d.astype(np.float64)
    out = {"persons": len(kp), "at_zero": int((kp == 0).sum()), "at_input": int((kp[:, :, 0] == X).sum() + (kp[:, :, 1] == Y).sum()),
           "just_below_input": int((c.kp2d[:, :, 0] == _below(X)).sum() + (c.kp2d[:, :, 1] == _below(Y)).sum()),
           "one_end_out": info.get("one_end_out", 0), "zero_limbs": info.get("zero_limbs", 0), "edges_half": info.get("edges_half", 0),
           "dist1": info.get("dist1", {}), "limb_cnt_max": info.get("limb_cnt_max", 0), "nearer_second": info.get("nearer_second", 0),
           "behind_never_fg": info.get("behind_never_fg", 0)}
    es = info.get("e", [])
    lim = CUT * 2 * sigma * sigma
    out["cut_last_inside"] = int(sum(((e * 2 * sigma * sigma <= lim) & (e * 2 * sigma * sigma + 1 > lim) & (e <= CUT)).sum() for e in es))
    out["cut_first_outside"] = int(sum(((e > CUT) & (e * 2 * sigma * sigma - 1 < lim)).sum() for e in es))
    out["cut_exact"] = int(sum((e == CUT).sum() for e in es))
    # heat that passed 1 before the last person was added
    heat_sat = 0
    for i in range(15):
        acc = None
        for j in range(len(kp)):
            if not (0 <= kp[j, i, 0] < X and 0 <= kp[j, i, 1] < Y):
                continue
            gh, gw = grid(c.geom)
            ys, xs = np.mgrid[0:gh, 0:gw].astype(np.float64)
            e = ((xs * s + s / 2.0 - 0.5 - kp[j, i, 0]) ** 2 + (ys * s + s / 2.0 - 0.5 - kp[j, i, 1]) ** 2) / 2.0 / sigma / sigma
            g = (e <= CUT) * np.exp(-e)
            if acc is not None:
                heat_sat += int(((acc >= 1.0) & (g > 0)).sum())
            acc = g if acc is None else np.minimum(acc + g, 1.0)
    out["added_to_clamped"] = heat_sat
    return out


# ---------------------------------------------------------------------------------------------
# the compositor
# ---------------------------------------------------------------------------------------------
def compose_cases():
    """(name, fg_depth [B,S,H,W] float32 values that float16 holds exactly, fg_mask uint8, n_src int32, bg [B,H,W])"""
    out = []
    for name, S, H, W, seed in (("1x1", 3, 1, 1, 1), ("1x300", 3, 1, 300, 2), ("17x19", 3, 17, 19, 3), ("one_source", 1, 17, 19, 4)):
        rng = np.random.default_rng(seed)
        B = 6
        d = (rng.integers(-16, 160, (B, S, H, W)) / 8.0).astype(f32)          # -2 .. 20 in steps of 1/8: zero, negative and above 2 * depth_max
        d[0].flat[::5] = 0.0
        m = rng.choice(np.array([0, 0, 1, 1, 2, 255], np.uint8), (B, S, H, W))
        bg = (rng.integers(0, 56, (B, H, W)) / 8.0).astype(f32)
        n_src = np.array([0, 1, S, S + 2, 0 if S == 1 else S - 1, S], np.int32)
        m[5] = 0
        out.append((name, d, m, n_src, bg))
    return out
