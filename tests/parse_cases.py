"""Hand-built edge-case maps for the part-affinity parse, a census of what they contain, and mutants of the oracle (no GPU).

The parse kernels (popnet_amd/csrc/parse_*.hip) promise bit-exact agreement with oracle/parse_paf.py.  The cases here put
that promise where random planted persons never go: corner patches, non-square and tiny maps, the largest map, the record
capacities on both sides, bit-equal candidate scores, the 8-of-10 rule, the length penalty, negative heat in the read-out.

  build_maps   explicit placements -> (heat [h,w,16], paf [h,w,28], z [h,w,15]) float32 HWC
  CASES        the case list, grouped by map shape (one shape = one batch)
  reference    the oracle's stage outputs of a case (peaks, connections, records), optionally under a mutant
  census       what a case contains, counted with the oracle's own stage functions
  MUTANTS      tests-side variants of the oracle's stages; every one must change the compared outputs of some case

Two facts about the 14-limb tree save cases.  Every destination joint type belongs to exactly one limb and matching is one to
one, so a connection can hit an open row only through its source id, which is unique to one row: ``len(hit)`` in
group_limbs_of_same_person is always 0 or 1, and the merge branch, the 2-hit overlap branch and the >= 3-hit fall-through
cannot be reached from any maps (the census counts ``len(hit)`` to confirm it).  And np.round never sees an exact .5 in the
sample coordinates: peak coordinates are integers and i * d / 9 = m + 0.5 has no integer solution.
"""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np

from oracle import cv2_resize as R
from oracle import parse_paf as O

J, L = O.NUM_KEYPOINTS, O.NUM_LIMBS
W_ORG, H_ORG = 480, 640

# a 15-joint stick figure, offsets in cells from the pelvis (joint 8); 5 cells wide, 7 high at scale 1
STICK = {8: (0, 0), 1: (0, -2), 0: (0, -3), 2: (-1, -1), 4: (-2, 0), 6: (-2, 1), 3: (1, -1), 5: (2, 0), 7: (2, 1),
         9: (-1, 1), 11: (-1, 2), 13: (-1, 3), 10: (1, 1), 12: (1, 2), 14: (1, 3)}


def stick(ax, ay, sx=1, sy=1, joints=None, transpose=False):
    p = {j: (ax + sx * dx, ay + sy * dy) for j, (dx, dy) in STICK.items() if joints is None or j in joints}
    return {j: (y, x) for j, (x, y) in p.items()} if transpose else p


def build_maps(h, w, persons=(), amps=None, paf_mag=None, zero_pts=None, extra_peaks=(), paf_blocks=(), seed=0, noise=1.0,
               heat_planes=None, paf_const=None):
    """persons: list of {joint: (x, y)} cell placements.  amps[p] (scalar or {joint: amp}, default 0.9): peak amplitudes.
    paf_mag[(p, limb)] (default 1): length of the constant PAF vector written in a band of 1 cell around the limb segment.
    zero_pts[(p, limb)] = sample indices (0..9): the band is zeroed in the 3x3 cells around those sample points of the limb.
    extra_peaks: (joint, x, y, amp) strays.  paf_blocks: (limb, x0, x1, y0, y1, vx, vy) constant rectangles (inclusive),
    written last.  heat_planes {joint: [h,w] array} / paf_const {limb: (vx, vy)} replace whole planes (plateau maps).
    Background heat is uniform(-0.08, 0.06) * noise - 0.03125 * (noise == 0): below the threshold, negative values included."""
    rng = np.random.default_rng(seed)
    heat = (rng.uniform(-0.08, 0.06, (h, w, J + 1)) * noise).astype(np.float32)
    if noise == 0:
        heat[:] = -0.03125
    paf = np.zeros((h, w, 2 * L), np.float32)
    z = (rng.standard_normal((h, w, J)) * 0.3).astype(np.float32)
    amps, paf_mag, zero_pts = amps or {}, paf_mag or {}, zero_pts or {}
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    for p, person in enumerate(persons):
        a = amps.get(p, 0.9)
        for j, (x, y) in person.items():
            assert 0 <= x < w and 0 <= y < h, (p, j, x, y)
            heat[y, x, j] = a[j] if isinstance(a, dict) else a
        for limb, (s, d) in enumerate(O.LIMBS):
            if s not in person or d not in person:
                continue
            (x0, y0), (x1, y1) = person[s], person[d]
            vx, vy = float(x1 - x0), float(y1 - y0)
            n2 = vx * vx + vy * vy
            assert n2 > 0, "zero-length limb"
            t = np.clip(((xx - x0) * vx + (yy - y0) * vy) / n2, 0.0, 1.0)
            dist = np.hypot(xx - (x0 + t * vx), yy - (y0 + t * vy))
            band = dist <= 1.0
            m = paf_mag.get((p, limb), 1.0)
            paf[band, 2 * limb] = np.float32(m * vx / np.sqrt(n2))
            paf[band, 2 * limb + 1] = np.float32(m * vy / np.sqrt(n2))
            for k in zero_pts.get((p, limb), ()):
                cx, cy = int(round(x0 + vx * k / 9.0)), int(round(y0 + vy * k / 9.0))
                paf[max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2, 2 * limb:2 * limb + 2] = 0.0
    for j, x, y, a in extra_peaks:
        heat[y, x, j] = a
    for limb, x0, x1, y0, y1, vx, vy in paf_blocks:
        paf[y0:y1 + 1, x0:x1 + 1, 2 * limb] = vx
        paf[y0:y1 + 1, x0:x1 + 1, 2 * limb + 1] = vy
    for j, plane in (heat_planes or {}).items():
        heat[:, :, j] = plane
    for limb, (vx, vy) in (paf_const or {}).items():
        paf[:, :, 2 * limb], paf[:, :, 2 * limb + 1] = vx, vy
    return heat, paf, z


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def _mirror(person, w, h, fx, fy):
    return {j: ((w - 1 - x) if fx else x, (h - 1 - y) if fy else y) for j, (x, y) in person.items()}


# joints of one person around the top-left corner: every clipped patch size (pw, ph) in {3, 4, 5}^2 occurs
_CORNER = {8: (0, 0), 9: (1, 0), 11: (3, 0), 13: (5, 1), 10: (0, 1), 12: (0, 3), 14: (1, 5), 1: (1, 1), 0: (3, 3), 2: (3, 1),
           4: (5, 0), 6: (7, 0), 3: (1, 3), 5: (0, 5), 7: (0, 7)}


def _fragments(n3, n2, low=()):
    """n3 three-joint fragments (8, 9, 11: kept) and n2 two-joint fragments (2, 4: pruned by count) on a 4 x 9 grid of a 28x28
    map; fragments of the two kinds share cells (their joints and limbs live in other planes).  low: indices of three-joint
    fragments with peaks and PAF so weak that the row is pruned by score per count."""
    cells = [(1 + 7 * c, 1 + 3 * r) for r in range(9) for c in range(4)]
    persons, amps, mag = [], {}, {}
    for k in range(n3):
        x, y = cells[k]
        persons.append({8: (x, y), 9: (x + 1, y), 11: (x + 2, y)})
        if k in low:
            amps[len(persons) - 1] = 0.12
            mag[(len(persons) - 1, 0)] = mag[(len(persons) - 1, 1)] = 0.08
    for k in range(n2):
        x, y = cells[k]
        persons.append({2: (x, y), 4: (x + 1, y)})
    return dict(persons=persons, amps=amps, paf_mag=mag)


def _plateau(h, w, seed, joints):
    rng = np.random.default_rng(seed)
    levels = np.array([0.1, 0.35, 0.6], np.float32)      # three levels; the lowest is the threshold itself: `>` makes none of its cells a peak
    planes = {j: levels[rng.choice(3, (h, w), p=(0.72, 0.18, 0.1))] for j in joints}
    ang = {limb: 0.4 + 0.45 * limb for limb in range(L)}
    return dict(heat_planes=planes, paf_const={limb: (np.float32(np.cos(a)), np.float32(np.sin(a))) for limb, a in ang.items()}, seed=seed)


def _grid_peaks(joint, n, w=28):
    pts = [(x, y) for y in range(0, 28, 2) for x in range((y // 2) % 2, w, 3)]
    return [(joint, x, y, 0.5 + 0.01 * (k % 7)) for k, (x, y) in enumerate(pts[:n])]


def _quarter_strays(h, w, joint=0):
    """peaks on both sides of each boundary between the four quarter scans, Q = (hw + 3) / 4"""
    q = (h * w + 3) // 4
    out = []
    for k in (1, 2, 3):
        for cell in (k * q - 1, k * q):
            out.append((joint, cell % w, cell // w, 0.6))
    return out


def _layout_2036(transpose):
    h, w = (36, 20) if transpose else (20, 36)
    t = (lambda x, y: (y, x)) if transpose else (lambda x, y: (x, y))
    persons = [
        stick(8, 8, sx=2, sy=2, transpose=transpose),
        {8: t(2, 17), 9: t(33, 17), 11: t(34, 12)},                 # a limb of 31 cells along the long axis
        {8: t(20, 1), 10: t(20, 18), 12: t(24, 18)},                # and one of 17 cells along the short axis
        stick(28, 6, transpose=transpose),
    ]
    strays = _quarter_strays(h, w) + [(13, w - 1, h - 1, 0.7), (14, 0, h - 1, 0.7), (6, w - 1, 0, 0.7)]
    return dict(h=h, w=w, persons=persons, extra_peaks=strays, seed=11)


def _spread(h, w, seed):
    persons = [stick(8, 10, 3, 3), stick(w - 9, 10, 3, 3), stick(8, h - 11, 3, 3), stick(w - 9, h - 11, 3, 3), stick(w // 2, h // 2, 2, 2),
               {8: (w - 1, h - 1), 9: (w - 4, h - 1), 11: (w - 1, h - 5)}, {8: (0, h - 1), 10: (3, h - 2), 12: (7, h - 1)},
               {1: (w - 1, 0), 0: (w - 1, 4), 2: (w - 5, 0)}]
    strays = [(5, w - 1, y, 0.5) for y in range(1, h, 9)] + [(7, x, h - 1, 0.5) for x in range(1, w, 9)] + _quarter_strays(h, w, joint=6)
    return dict(h=h, w=w, persons=persons, extra_peaks=strays, seed=seed)


def _line(n, vertical):
    xs = {8: 18, 9: 22, 11: 26, 13: 31, 10: 14, 12: 9, 14: 3, 1: 20, 0: 39, 2: 24}
    person = {j: ((0, x) if vertical else (x, 0)) for j, x in xs.items()}
    return dict(h=n if vertical else 1, w=1 if vertical else n, persons=[person], extra_peaks=[(6, 0, 0, 0.4)], seed=5)


def _specs():
    S = []
    add = lambda name, **kw: S.append(dict(dict(h=28, w=28), name=name, **kw))
    add("corners", persons=[_mirror(_CORNER, 28, 28, fx, fy) for fy in (0, 1) for fx in (0, 1)], seed=1)
    add("edges", persons=[{8: (13, 0), 9: (16, 1), 11: (19, 0), 10: (10, 1), 12: (7, 0)}, {8: (13, 27), 9: (16, 26), 11: (19, 27), 10: (10, 26), 12: (7, 27)},
                          {8: (0, 13), 9: (1, 16), 11: (0, 19), 10: (1, 10), 12: (0, 7)}, {8: (27, 13), 9: (26, 16), 11: (27, 19), 10: (26, 10), 12: (27, 7)}], seed=2)
    # two whole-cell translations of one person (tied candidates that share no peak); one pelvis with two hips at mirrored
    # offsets inside a constant PAF block (bicubic of a constant is exact, so the two candidates score bit-equal and share the pelvis)
    add("ties", persons=[stick(5, 5), stick(15, 12), {8: (5, 21), 9: (9, 19), 11: (13, 19)}, {9: (9, 23), 11: (13, 23)}],
        paf_blocks=[(0, 2, 12, 16, 26, np.float32(1.0), np.float32(0.0))], noise=0.0, seed=3)
    add("cnt", persons=[{8: (2, 4), 9: (24, 4), 11: (24, 8)}, {8: (2, 13), 9: (24, 13), 11: (24, 17)}, {8: (2, 22), 9: (24, 22), 11: (24, 26)}],
        zero_pts={(0, 0): (4,), (1, 0): (3, 6)}, seed=4)
    add("penalty", persons=[{8: (1, 4), 9: (26, 4), 11: (26, 8)}, {8: (1, 14), 9: (26, 14), 11: (26, 18)}, {8: (3, 23), 9: (6, 23), 11: (9, 23)}],
        paf_mag={(1, 0): 0.3}, amps={2: 0.12}, seed=5, **{})
    S[-1]["paf_mag"].update({(2, 0): 0.08, (2, 1): 0.08})
    S.append(dict(name="wide", **_layout_2036(False)))
    S.append(dict(name="tall", **_layout_2036(True)))
    S.append(dict(name="plateau_9x13", h=9, w=13, **_plateau(9, 13, 21, (8, 9, 11, 1))))
    S.append(dict(name="plateau_5x7", h=5, w=7, **_plateau(5, 7, 22, (8, 9, 11, 13, 1, 0))))
    S.append(dict(name="const_3x3", h=3, w=3, heat_planes={j: np.full((3, 3), 0.5, np.float32) for j in range(J)},
                  paf_const=_plateau(3, 3, 23, ())["paf_const"], seed=23))
    S.append(dict(name="max_map", **_spread(64, 64, 31)))
    S.append(dict(name="max_map_60", **_spread(64, 60, 32)))
    add("peaks32", persons=[stick(14, 14, 2, 2)], extra_peaks=_grid_peaks(0, 31), seed=6)
    add("peaks33", persons=[stick(14, 14, 2, 2)], extra_peaks=_grid_peaks(0, 32), seed=6)
    add("rows32", seed=7, **_fragments(16, 16, low=(3,)))
    add("rows33", seed=7, **_fragments(17, 16, low=(3,)))
    add("persons16", seed=8, **_fragments(16, 0))
    add("persons17", seed=8, **_fragments(17, 0))
    S.append(dict(name="line_1x40", **_line(40, False)))
    S.append(dict(name="line_40x1", **_line(40, True)))
    return S


class Case(SimpleNamespace):
    @property
    def shape(self):
        return (self.h, self.w)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for s in _specs():
        s = dict(s)
        name, h, w = s.pop("name"), s.pop("h"), s.pop("w")
        heat, paf, z = build_maps(h, w, **s)
        for a in (heat, paf, z):
            a.setflags(write=False)
        out.append(Case(name=name, h=h, w=w, heat=heat, paf=paf, z=z))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


LINE_CASES = ("line_1x40", "line_40x1")
TINY_CASES = ("plateau_9x13", "plateau_5x7", "const_3x3") + LINE_CASES


def shapes():
    """{(h, w): [cases]} in case order -- one shape is one batch"""
    out = {}
    for c in cases():
        out.setdefault(c.shape, []).append(c)
    return out


# ---------------------------------------------------------------------------------------------
# the oracle by stages, with room for a mutant
# ---------------------------------------------------------------------------------------------
STAGES = ("nms", "find_connected_joints", "group_limbs_of_same_person", "glue")


class Mutant(SimpleNamespace):
    """stage: the first stage whose output it changes.  patch: {attribute of oracle.parse_paf: replacement}; swap_org: the glue's
    w_org / h_org change places."""


@contextlib.contextmanager
def _patched(repl):
    old = {k: getattr(O, k) for k in repl}
    try:
        for k, v in repl.items():
            setattr(O, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(O, k, v)


_BASE = {}


def reference(c, mutant=None):
    """One O.frame_to_records run of the case with every stage function wrapped: returns its stage outputs
    {'peaks': per-type list, 'connected': per-limb list, 'assoc', 'rec': the records dict}.  Under a mutant the stages in front
    of the mutant's own are replayed from the unmutated run (their inputs are the same), which keeps the mutant table quick."""
    if mutant is None and c.name in _BASE:
        return _BASE[c.name]
    base = None if mutant is None else reference(c)
    first = 0 if mutant is None else STAGES.index(mutant.stage)
    got = {}
    patch = {} if mutant is None else dict(mutant.patch)
    real = {k: patch.get(k, getattr(O, k)) for k in STAGES[:3]}

    def wrap(idx, key):
        def f(*a, **kw):
            got[key] = base[key] if idx < first else real[STAGES[idx]](*a, **kw)
            return got[key]
        return f

    def resize(img, *a, **kw):
        if img.ndim == 3:                      # the PAF up-sampling: the same for every run of the case
            if "paf_up" not in c.__dict__:
                c.paf_up = R.resize(img, *a, **kw)
            return c.paf_up
        return patch["_resize"](img, *a, **kw) if "_resize" in patch else R.resize(img, *a, **kw)

    repl = {"nms": wrap(0, "peaks"), "find_connected_joints": wrap(1, "connected"), "group_limbs_of_same_person": wrap(2, "assoc"),
            "cv2_resize": SimpleNamespace(resize=resize, INTER_CUBIC=R.INTER_CUBIC, INTER_NEAREST=R.INTER_NEAREST)}
    for k, v in patch.items():
        if k not in STAGES and k != "_resize":
            repl[k] = v
    worg, horg = (H_ORG, W_ORG) if (mutant is not None and getattr(mutant, "swap_org", False)) else (W_ORG, H_ORG)
    with _patched(repl):
        rec = O.frame_to_records(c.heat.copy(), c.paf.copy(), c.z.copy(), w_org=worg, h_org=horg)
    got["rec"] = rec
    if mutant is None:
        _BASE[c.name] = got
    return got


def outputs_differ(a, b):
    """the compared outputs of two runs: peaks, connections (count, ids, score), records"""
    def same(x, y):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        return x.shape == y.shape and np.array_equal(x, y)
    if not all(same(p, q) for p, q in zip(a["peaks"], b["peaks"])):
        return "peaks"
    if not all(same(np.asarray(p).reshape(-1, 5), np.asarray(q).reshape(-1, 5)) for p, q in zip(a["connected"], b["connected"])):
        return "connections"
    if not same(np.asarray(a["assoc"]).reshape(-1, J + 2), np.asarray(b["assoc"]).reshape(-1, J + 2)):
        return "persons"
    for k in ("humans_2d", "humans_3d", "conf", "visibility"):
        if not same(a["rec"][k], b["rec"][k]):
            return k
    return None


# ---------------------------------------------------------------------------------------------
# variants of the stages: default flags restate the oracle (asserted in test_parse_cases.py), a flag makes a mutant
# ---------------------------------------------------------------------------------------------
def find_peaks_variant(thresh, img, ge=False, conn8=False, colmajor=False):
    m = img.copy()
    m[1:, :] = np.maximum(m[1:, :], img[:-1, :])
    m[:-1, :] = np.maximum(m[:-1, :], img[1:, :])
    m[:, 1:] = np.maximum(m[:, 1:], img[:, :-1])
    m[:, :-1] = np.maximum(m[:, :-1], img[:, 1:])
    if conn8:
        m[1:, 1:] = np.maximum(m[1:, 1:], img[:-1, :-1])
        m[1:, :-1] = np.maximum(m[1:, :-1], img[:-1, 1:])
        m[:-1, 1:] = np.maximum(m[:-1, 1:], img[1:, :-1])
        m[:-1, :-1] = np.maximum(m[:-1, :-1], img[1:, 1:])
    binary = (m == img) * ((img >= thresh) if ge else (img > thresh))
    if colmajor:
        xs, ys = np.nonzero(binary.T)
        return np.array([xs, ys]).T
    return np.array(np.nonzero(binary)[::-1]).T


class _LastMax(np.ndarray):
    def argmax(self, *a, **kw):
        flat = np.asarray(self).ravel()
        return flat.size - 1 - int(flat[::-1].argmax())


def _resize_last_max(img, *a, **kw):
    return R.resize(img, *a, **kw).view(_LastMax)


def nms_whole_map(heatmaps, upsamp=O.DOWNSAMPLE, num_keypoints=J, thresh=O.THRESH_HEATMAP):
    """O.nms with the patch cut out of the up-sampled WHOLE map: the border is replicated at the map edge, not the patch edge"""
    out, cnt = [], 0
    for joint in range(num_keypoints):
        m = heatmaps[:, :, joint]
        up = R.resize(np.ascontiguousarray(m), None, fx=upsamp, fy=upsamp, interpolation=R.INTER_CUBIC)
        coords = O.find_peaks(thresh, m)
        peaks = np.zeros((len(coords), 4))
        for i, peak in enumerate(coords):
            x_min, y_min = np.maximum(0, peak - O.WIN_SIZE)
            x_max, y_max = np.minimum(np.array(m.T.shape) - 1, peak + O.WIN_SIZE)
            pu = up[y_min * upsamp:(y_max + 1) * upsamp, x_min * upsamp:(x_max + 1) * upsamp]
            loc = np.unravel_index(pu.argmax(), pu.shape)
            peaks[i] = (x_min * upsamp + loc[1], y_min * upsamp + loc[0], pu[loc], cnt)
            cnt += 1
        out.append(peaks)
    return out


def candidate_table(paf_up, per_type, seq_mean=False, pen_w=False):
    """every (src, dst) pair of every limb: (i, j, cnt, mean, penalty, score), the oracle's arithmetic"""
    H = paf_up.shape[1] if pen_w else paf_up.shape[0]
    table = []
    for limb, (js_t, jd_t) in enumerate(O.LIMBS):
        rows = []
        for i, js in enumerate(per_type[js_t]):
            for j, jd in enumerate(per_type[jd_t]):
                d = jd[:2] - js[:2]
                dist = np.sqrt(np.sum(d ** 2)) + 1e-8
                d = d / dist
                xs = np.round(np.linspace(js[0], jd[0], num=10)).astype(np.intp)
                ys = np.round(np.linspace(js[1], jd[1], num=10)).astype(np.intp)
                pts = paf_up[ys, xs, 2 * limb].astype(np.float64) * d[0] + paf_up[ys, xs, 2 * limb + 1].astype(np.float64) * d[1]
                if seq_mean:
                    mean = 0.0
                    for v in pts:
                        mean = mean + v
                    mean = mean / 10
                else:
                    mean = O._pairwise_mean10(pts)
                pen = min(0.5 * H / dist - 1, 0)
                rows.append((i, j, int(np.count_nonzero(pts > O.THRESH_PAF)), mean, pen, mean + pen))
        table.append(rows)
    return table


def connect_variant(paf_up, per_type, seq_mean=False, pen_w=False, cnt_ge=False, tie_rev=False, **_):
    out = []
    for limb, rows in enumerate(candidate_table(paf_up, per_type, seq_mean, pen_w)):
        src, dst = per_type[O.LIMBS[limb][0]], per_type[O.LIMBS[limb][1]]
        if len(src) == 0 or len(dst) == 0:
            out.append([])
            continue
        cand = [r for r in rows if ((r[2] >= 8) if cnt_ge else (r[2] > 8)) and r[5] > 0]
        cand = sorted(cand[::-1] if tie_rev else cand, key=lambda r: r[5], reverse=True)
        conn = np.empty((0, 5))
        for i, j, _c, _m, _p, s in cand:
            if i not in conn[:, 3] and j not in conn[:, 4]:
                conn = np.vstack([conn, [src[i][3], dst[j][3], s, i, j]])
                if len(conn) >= min(len(src), len(dst)):
                    break
        out.append(conn)
    return out


def group_variant(connected, joint_list, count_le3=False, info=None, **_):
    """O.group_limbs_of_same_person; info (a dict) receives len(hit) per connection and the rows before pruning"""
    persons, hits = [], []
    for limb, (s_t, d_t) in enumerate(O.LIMBS):
        for c in connected[limb]:
            hit = [p for p, row in enumerate(persons) if row[s_t] == c[0] or row[d_t] == c[1]]
            hits.append(len(hit))
            if len(hit) == 1:
                row = persons[hit[0]]
                if row[d_t] != c[1]:
                    row[d_t] = c[1]
                    row[-1] += 1
                    row[-2] += joint_list[c[1].astype(int), 2] + c[2]
            elif len(hit) == 2:
                r1, r2 = persons[hit[0]], persons[hit[1]]
                if not ((r1 >= 0) & (r2 >= 0))[:-2].any():
                    r1[:-2] += (r2[:-2] + 1)
                    r1[-2:] += r2[-2:]
                    r1[-2] += c[2]
                    persons.pop(hit[1])
                else:
                    r1[d_t] = c[1]
                    r1[-1] += 1
                    r1[-2] += joint_list[c[1].astype(int), 2] + c[2]
            else:
                row = -1 * np.ones(J + 2)
                row[s_t], row[d_t], row[-1] = c[0], c[1], 2
                row[-2] = sum(joint_list[c[:2].astype(int), 2]) + c[2]
                persons.append(row)
    if info is not None:
        info["hits"] = hits
        info["rows"] = [r.copy() for r in persons]
    lim = 4 if count_le3 else 3
    return np.array([r for r in persons if not (r[-1] < lim or r[-2] / r[-1] < 0.2)])


def retrieve_variant(center, depthmap, heatmap, radius=1, dup=False, no_clamp=False, seq_sum=False):
    if not no_clamp:
        heatmap[heatmap < 0] = 0
    gx, gy = depthmap.shape[1], depthmap.shape[0]
    if dup:                                                        # border cells repeated instead of the window being clipped
        xs = [min(max(int(center[0]) + k, 0), gx - 1) for k in range(-radius, radius + 1)]
        ys = [min(max(int(center[1]) + k, 0), gy - 1) for k in range(-radius, radius + 1)]
    else:
        xs = list(range(min(max(int(center[0] - radius), 0), gx - 1), max(min(int(center[0] + radius), gx - 1), 0) + 1))
        ys = list(range(min(max(int(center[1] - radius), 0), gy - 1), max(min(int(center[1] + radius), gy - 1), 0) + 1))
    xx, yy = np.meshgrid(xs, ys)
    w = heatmap[yy, xx] + 0.000000001
    d = depthmap[yy, xx]
    if seq_sum:
        sp, sw = np.float32(-0.0), np.float32(-0.0)
        for a, b in zip((d * w).ravel(), w.ravel()):
            sp, sw = sp + a, sw + b
        return sp / sw
    return np.sum(d * w) / np.sum(w)


def _mean_seq(s):
    res = s[0]
    for v in s[1:]:
        res = res + v
    return res / len(s)


def _conn(**kw):
    def f(paf_up, per_type, *a, **k):
        return connect_variant(paf_up, per_type, **kw)
    return f


def _peaks(**kw):
    return lambda thresh, img: find_peaks_variant(thresh, img, **kw)


def _retr(**kw):
    return lambda center, depthmap, heatmap, radius=1: retrieve_variant(center, depthmap, heatmap, radius, **kw)


MUTANTS = (
    Mutant(name="argmax_last", stage="nms", patch={"_resize": _resize_last_max}),
    Mutant(name="border_at_map_edge", stage="nms", patch={"nms": nms_whole_map}),
    Mutant(name="peak_ge_thresh", stage="nms", patch={"find_peaks": _peaks(ge=True)}),
    Mutant(name="filter_8_connected", stage="nms", patch={"find_peaks": _peaks(conn8=True)}),
    Mutant(name="ids_column_major", stage="nms", patch={"find_peaks": _peaks(colmajor=True)}),
    Mutant(name="mean_sequential", stage="find_connected_joints", patch={"_pairwise_mean10": _mean_seq}),
    Mutant(name="penalty_from_width", stage="find_connected_joints", patch={"find_connected_joints": _conn(pen_w=True)}),
    Mutant(name="cnt_ge_8", stage="find_connected_joints", patch={"find_connected_joints": _conn(cnt_ge=True)}),
    Mutant(name="tie_order_reversed", stage="find_connected_joints", patch={"find_connected_joints": _conn(tie_rev=True)}),
    Mutant(name="window_duplicated", stage="glue", patch={"retrieve_depth_heat_weighted": _retr(dup=True)}),
    Mutant(name="no_negative_clamp", stage="glue", patch={"retrieve_depth_heat_weighted": _retr(no_clamp=True)}),
    Mutant(name="readout_sum_sequential", stage="glue", patch={"retrieve_depth_heat_weighted": _retr(seq_sum=True)}),
    Mutant(name="prune_count_le_3", stage="group_limbs_of_same_person",
           patch={"group_limbs_of_same_person": lambda conn, jl, **k: group_variant(conn, jl, count_le3=True)}),
    Mutant(name="org_size_swapped", stage="glue", patch={}, swap_org=True),
)


# ---------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------
def census(c):
    ref = reference(c)
    heat, h, w = c.heat, c.h, c.w
    out = {"patch": {}, "repeated_max": 0, "cnt": {8: 0, 9: 0, 10: 0}, "pen_accepted": 0, "pen_rejected": 0,
           "ties_shared": 0, "ties_apart": 0, "windows": {}, "windows_negative": 0}
    per_type = ref["peaks"]
    out["peaks"] = int(sum(len(p) for p in per_type))
    out["peaks_max"] = max(len(p) for p in per_type)
    for j in range(J):
        for x, y in O.find_peaks(O.THRESH_HEATMAP, heat[:, :, j]):
            x0, y0, x1, y1 = max(0, x - 2), max(0, y - 2), min(w - 1, x + 2), min(h - 1, y + 2)
            key = (x1 - x0 + 1, y1 - y0 + 1)
            out["patch"][key] = out["patch"].get(key, 0) + 1
            up = R.resize(np.ascontiguousarray(heat[y0:y1 + 1, x0:x1 + 1, j]), None, fx=8, fy=8, interpolation=R.INTER_CUBIC)
            out["repeated_max"] += int(np.count_nonzero(up == up.max()) > 1)
    table = candidate_table(c.paf_up, per_type)
    for rows in table:
        ok = []
        for i, j, cnt, mean, pen, score in rows:
            if cnt in out["cnt"]:
                out["cnt"][cnt] += 1
            if cnt > 8 and pen < 0 and mean > 0:
                out["pen_accepted" if score > 0 else "pen_rejected"] += 1
            if cnt > 8 and score > 0:
                ok.append((i, j, score))
        for s in sorted(set(r[2] for r in ok)):
            grp = [r for r in ok if r[2] == s]
            if len(grp) > 1:
                shared = len(set(r[0] for r in grp)) < len(grp) or len(set(r[1] for r in grp)) < len(grp)
                out["ties_shared" if shared else "ties_apart"] += 1
    out["connections"] = int(sum(len(x) for x in ref["connected"]))
    info = {}
    jl = ref["rec"]["joint_list"]
    keep = group_variant(ref["connected"], jl, info=info)
    out["hit_max"] = max(info["hits"], default=0)
    out["open_rows"] = len(info["rows"])
    out["pruned_count"] = sum(1 for r in info["rows"] if r[-1] < 3)
    out["pruned_score"] = sum(1 for r in info["rows"] if r[-1] >= 3 and r[-2] / r[-1] < 0.2)
    out["kept"] = len(keep)
    for row in keep:
        for j in range(J):
            if row[j] < 0:
                continue
            cx, cy = int(jl[int(row[j]), 0] / 8), int(jl[int(row[j]), 1] / 8)
            x0, x1 = min(max(cx - 1, 0), w - 1), max(min(cx + 1, w - 1), 0)
            y0, y1 = min(max(cy - 1, 0), h - 1), max(min(cy + 1, h - 1), 0)
            n = (x1 - x0 + 1) * (y1 - y0 + 1)
            out["windows"][n] = out["windows"].get(n, 0) + 1
            out["windows_negative"] += int((heat[y0:y1 + 1, x0:x1 + 1, j] < 0).any())
    return out


def expected_status(cen):
    """the overflow bits the fixed-size record of a case must carry (PN_FRAME_OVERFLOW_PEAKS = 1, _PERSONS = 2)"""
    return (1 if cen["peaks_max"] > 32 else 0) | (2 if cen["open_rows"] > 32 else 0)
