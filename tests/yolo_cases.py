"""Hand-built edge-case maps for the Yolo-Pose+ decode, a census of what they contain, and mutants of the oracle (no GPU).

parse_yolo_kernel (popnet_amd/csrc/parse_yolo.hip) promises bit-exact agreement with oracle/parse_yolo.py.  The cases here put
that promise where random 14 x 14 maps with two anchors never go: one and three anchors, non-square and one-cell maps, every
candidate count at which a loop of the kernel takes another round (64 | 65, 256 | 257, 512 = the capacity), 63 | 64 | 65 survivors,
bit-equal scores, a score and an IoU exactly on their thresholds, zero-area boxes, suppression chains that give votes back,
conflicts among the low-ranked candidates, and joints exactly on the visibility bounds.

  build_map    explicit placements -> a raw map [A*(5+3J), h, w] float32 ([A*(5+4J), h, w] with pred_vis)
  groups()     the case list, grouped by (A, h, w): one group is one batch, with its anchors, output size and thresholds
  decode       a restatement of oracle.parse_yolo.parse_prior_pose for one frame with flags: no flag set == the oracle
               (asserted in test_yolo_cases.py), one flag set == a mutant
  record       what the fixed-size pn_yolo_frame of a frame must hold, from the oracle's own parse_prior_pose
  census       what a case contains, counted with the oracle's own decode_maps and box_nms_keep
  MUTANTS      every one must change the compared output of some case

The reference's suppression loop runs over rows 1 .. n-2 only (prior_pose_align.py:112-115).  That quirk cannot change any
result: row 0 never has keep > 0 (column 0 of an upper-triangular matrix is empty), and row n-1 of an upper-triangular matrix
is empty, so neither row could subtract anything.  It is therefore not a mutant.  For the same reason the vote-returning loop
keeps exactly the boxes plain greedy NMS keeps "if suppressed boxes do not suppress"; the mutant is the NMS that lets them.

Box width and height of a placement are given in CELLS and converted to the raw channel value with the anchor of the slot
(raw = cells / anchor); joints are raw channel values {joint: (vx, vy, vz[, vvis])}.
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import parse_yolo as O

f32 = np.float32
J = 15
MAX_DET = 64            # PN_YOLO_MAX_DET
MAX_CAND = 512          # YMAXC
CONFIGS = ((0, False), (2, True))          # (vis_margin, pred_vis): every group is compared under both
W_ORG, H_ORG, GLUE_INPUT = 480, 640, 224
DEPTH_MEAN, DEPTH_STD = 3, 2
INTRINSICS = {"fx": 365.0, "fy": 366.5, "cx": 255.5, "cy": 210.25}


class Group(SimpleNamespace):
    @property
    def shape(self):
        return (self.A, self.h, self.w)

    @property
    def key(self):
        return "%dx%dx%d" % self.shape


def _group(A, h, w, anchors, w_out, h_out, conf_thr=0.5, nms_thr=0.5):
    assert len(anchors) == A and A * h * w <= MAX_CAND
    assert len(set(a[0] for a in anchors)) == A and len(set(a[1] for a in anchors)) == A and all(a[0] != a[1] for a in anchors)
    return Group(A=A, h=h, w=w, anchors=tuple((float(a), float(b)) for a, b in anchors), w_out=w_out, h_out=h_out,
                 conf_thr=conf_thr, nms_thr=nms_thr, cases=[])


def P(a, row, col, conf, bw, bh, dx=0.5, dy=0.5, joints=None):
    return (a, row, col, conf, bw, bh, dx, dy, joints)


def build_map(g, places, seed=0, pred_vis=False):
    """Every cell that holds no placement has objectness in [0, 0.3), below every threshold used here; the other channels of
    those cells are random and must never be read into a result.  The 5 + 3J channels of an anchor are the same with and
    without pred_vis; pred_vis appends J visibility channels in (0, 1) per anchor."""
    rng = np.random.default_rng(seed)
    A, h, w = g.shape
    base = rng.uniform(-1, 1, (A, 5 + 3 * J, h, w)).astype(f32)
    base[:, 2:4] = rng.uniform(0.5, 2, (A, 2, h, w))
    base[:, 4] = rng.uniform(0, 0.3, (A, h, w))
    vis = rng.uniform(0.05, 1, (A, J, h, w)).astype(f32)
    seen = set()
    for a, row, col, conf, bw, bh, dx, dy, joints in places:
        assert 0 <= a < A and 0 <= row < h and 0 <= col < w and (a, row, col) not in seen, (a, row, col)
        seen.add((a, row, col))
        base[a, 0, row, col], base[a, 1, row, col] = dx, dy
        base[a, 2, row, col] = f32(bw) / f32(g.anchors[a][0])
        base[a, 3, row, col] = f32(bh) / f32(g.anchors[a][1])
        base[a, 4, row, col] = conf
        for j, v in (joints or {}).items():
            base[a, 5 + j, row, col], base[a, 5 + J + j, row, col], base[a, 5 + 2 * J + j, row, col] = v[0], v[1], v[2]
            if len(v) > 3:
                vis[a, j, row, col] = v[3]
    full = np.concatenate([base, vis], axis=1) if pred_vis else base
    return np.ascontiguousarray(full.reshape(-1, h, w))


# ---------------------------------------------------------------------------------------------
# the decode of one frame, with room for a mutant
# ---------------------------------------------------------------------------------------------
def decode(pm, g, vis_margin=0, pred_vis=False, info=None, tie_rev=False, conf_ge=False, iou_ge=False, no_return=False,
           cell_major=False, colrow_h=False, swap01=False, swap12=False, vis_excl=False, no_margin=False, keep_last=False):
    """oracle.parse_yolo.parse_prior_pose for ONE frame, then the fixed-size record: the first MAX_DET survivors and status bit 0
    when there are more.  info (a dict) receives the conflict matrix and the keep counts before and after the loop."""
    A, h, w = g.shape
    hw = h * w
    anchors = list(g.anchors)
    if swap01 and A >= 2:
        anchors[0], anchors[1] = anchors[1], anchors[0]
    if swap12 and A >= 3:
        anchors[1], anchors[2] = anchors[2], anchors[1]
    x = np.asarray(pm, dtype=f32).reshape(A, -1, hw).copy()
    F = x.shape[1]
    assert F == 5 + (4 if pred_vis else 3) * J
    cell = np.arange(hw)
    lin_x = (cell % h if colrow_h else cell % w).astype(f32)
    lin_y = (cell // h if colrow_h else cell // w).astype(f32)
    aw = np.array([a[0] for a in anchors], dtype=f32).reshape(A, 1)
    ah = np.array([a[1] for a in anchors], dtype=f32).reshape(A, 1)
    x[:, 0] = (x[:, 0] + lin_x) / f32(w)
    x[:, 1] = (x[:, 1] + lin_y) / f32(h)
    x[:, 2] = (x[:, 2] * aw) / f32(w)
    x[:, 3] = (x[:, 3] * ah) / f32(h)
    aw3, ah3 = (aw / f32(2.0)).reshape(A, 1, 1), (ah / f32(2.0)).reshape(A, 1, 1)
    x[:, 5:5 + J] = (x[:, 5:5 + J] * aw3 + lin_x) / f32(w)
    x[:, 5 + J:5 + 2 * J] = (x[:, 5 + J:5 + 2 * J] * ah3 + lin_y) / f32(h)
    x[:, 5 + 2 * J:5 + 3 * J] = x[:, 5 + 2 * J:5 + 3 * J] * f32(DEPTH_STD) + f32(DEPTH_MEAN)
    det = x.transpose(2, 0, 1).reshape(hw * A, F) if cell_major else x.transpose(0, 2, 1).reshape(A * hw, F)
    thr = f32(g.conf_thr)
    boxes = det[(det[:, 4] >= thr) if conf_ge else (det[:, 4] > thr)].copy()
    n = len(boxes)
    rec = {"n_candidates": n}
    if n:
        a, b = boxes[:, :2], boxes[:, 2:4]
        bb = np.concatenate([a - b / f32(2), a + b / f32(2)], 1).astype(f32)
        scores = boxes[:, 4]
        order = (n - 1 - np.argsort(-scores[::-1], kind='stable')) if tie_rev else np.argsort(-scores, kind='stable')
        x1, y1, x2, y2 = [bb[order][:, i:i + 1] for i in range(4)]
        dx = np.clip(np.minimum(x2, x2.T) - np.maximum(x1, x1.T), 0, None).astype(f32)
        dy = np.clip(np.minimum(y2, y2.T) - np.maximum(y1, y1.T), 0, None).astype(f32)
        inter = dx * dy
        areas = (x2 - x1) * (y2 - y1)
        unions = (areas + areas.T) - inter
        with np.errstate(divide='ignore', invalid='ignore'):
            ious = inter / unions
        nt = f32(g.nms_thr)
        conflicting = np.triu(((ious >= nt) if iou_ge else (ious > nt)).astype(np.int32), 1)
        keep = conflicting.sum(0).astype(np.int32)
        if info is not None:
            info.update(conflicting=conflicting, ious=ious, keep0=keep.copy(), returned=[], scores=scores[order], areas=areas[:, 0])
        if not no_return:
            for i in range(1, n - 1):
                if keep[i] > 0:
                    if info is not None and conflicting[i].any():
                        info["returned"].append(i)
                    keep -= conflicting[i]
        if info is not None:
            info["keep"] = keep.copy()
        boxes = boxes[order][keep == 0].copy()
    ns = len(boxes)
    rec["n_survivors"] = ns
    rec["status"] = 1 if ns > MAX_DET else 0
    boxes = boxes[-MAX_DET:] if keep_last else boxes[:MAX_DET]
    w_out, h_out = g.w_out, g.h_out
    boxes[:, 0] *= f32(w_out)
    boxes[:, 2] *= f32(w_out)
    boxes[:, 1] *= f32(h_out)
    boxes[:, 3] *= f32(h_out)
    boxes[:, 0] -= boxes[:, 2] / f32(2)
    boxes[:, 1] -= boxes[:, 3] / f32(2)
    boxes[:, 2] += boxes[:, 0]
    boxes[:, 3] += boxes[:, 1]
    boxes[:, 5:5 + J] *= f32(w_out)
    boxes[:, 5 + J:5 + 2 * J] *= f32(h_out)
    human = boxes[:, 5:5 + 3 * J].reshape(-1, 3, J).transpose(0, 2, 1).copy()
    m = 0 if no_margin else vis_margin
    hx, hy = human[:, :, 0], human[:, :, 1]
    if vis_excl:
        inside = (hx > 0 + m) & (hx < w_out - 1 - m) & (hy > 0 + m) & (hy < h_out - 1 - m)
    else:
        inside = (hx >= 0 + m) & (hx <= w_out - 1 - m) & (hy >= 0 + m) & (hy <= h_out - 1 - m)
    rec.update(n_det=len(boxes), bbox=boxes[:, :5].copy(), human=human, visibility=inside.astype(np.int32))
    if pred_vis:
        rec["vis_pred"] = (inside * boxes[:, 5 + 3 * J:]).astype(f32)
    return rec



def record(pm, g, vis_margin=0, pred_vis=False):
    """the same record from the oracle's own parse_prior_pose (the GPU tests compare with this one)"""
    bb, hh, vv = O.parse_prior_pose(np.asarray(pm)[None].copy(), list(g.anchors), J, g.w_out, g.h_out, DEPTH_MEAN, DEPTH_STD,
                                    g.conf_thr, g.nms_thr, vis_margin, pred_vis)
    bb, hh, vv = bb[0], hh[0], vv[0]
    ns = len(bb)
    dec = O.decode_maps(np.asarray(pm)[None], list(g.anchors), J, DEPTH_MEAN, DEPTH_STD)
    rec = {"n_candidates": int((dec[0, :, 4, :] > f32(g.conf_thr)).sum()), "n_survivors": ns, "status": 1 if ns > MAX_DET else 0}
    bb, hh, vv = bb[:MAX_DET], hh[:MAX_DET], vv[:MAX_DET]
    k = len(bb)
    rec.update(n_det=k, bbox=np.array(bb, dtype=f32).reshape(k, 5), human=np.array(hh, dtype=f32).reshape(k, J, 3))
    v = np.array(vv).reshape(k, J)
    if pred_vis:          # the record carries the in-bounds test as well: the oracle's, from the same channels without the visibility ones
        A = g.A
        base = np.ascontiguousarray(np.asarray(pm).reshape(A, 5 + 4 * J, g.h, g.w)[:, :5 + 3 * J].reshape(-1, g.h, g.w))
        rec["vis_pred"] = v.astype(f32)
        rec["visibility"] = record(base, g, vis_margin, False)["visibility"]
    else:
        rec["visibility"] = v.astype(np.int32)
    return rec


def glue(rec, g):
    """joints_2d / joints_3d / bbox_org of the record under the glue cfg of the GPU test"""
    n = rec["n_det"]
    return O.frame_glue([b for b in rec["bbox"]], [h for h in rec["human"]], J, GLUE_INPUT, W_ORG, H_ORG, INTRINSICS) if n else None


FIELDS = ("n_candidates", "n_survivors", "status", "n_det", "bbox", "human", "visibility", "vis_pred")


def outputs_differ(a, b):
    for k in FIELDS:
        if (k in a) != (k in b):
            return k
        if k in a and not (np.shape(a[k]) == np.shape(b[k]) and np.array_equal(a[k], b[k])):
            return k
    return None


MUTANTS = ("tie_rev", "conf_ge", "iou_ge", "no_return", "cell_major", "colrow_h", "swap01", "swap12", "vis_excl", "no_margin", "keep_last")


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def _decode_joint(g, a, pos, axis, v):
    """the oracle's float32 chain for one joint coordinate: ((v * anchor / 2 + cell) / cells) * out"""
    anc, cells, out = (g.anchors[a][0], g.w, g.w_out) if axis == 0 else (g.anchors[a][1], g.h, g.h_out)
    return ((f32(v) * (f32(anc) / f32(2.0)) + f32(pos)) / f32(cells)) * f32(out)


def solve_joint(g, a, pos, target, axis, outside=0):
    """The raw joint value whose decoded coordinate (the oracle's float32 chain ((v * anchor / 2 + cell) / cells) * out) is
    exactly `target` (outside == 0), or the reachable coordinate closest to `target` strictly below (outside == -1) or above
    (outside == +1).  Searched over the float32 neighbours of the float64 solution."""
    anc, cells, out = (g.anchors[a][0], g.w, g.w_out) if axis == 0 else (g.anchors[a][1], g.h, g.h_out)
    half = f32(anc) / f32(2.0)
    dec = lambda v: _decode_joint(g, a, pos, axis, v)

    v0 = f32((float(target) / out * cells - pos) / float(half))
    best, v_lo, v_hi = None, v0, v0
    cand = [v0]
    step = max(abs(float(v0)), float(pos) / float(half)) * 2.0 ** -25          # below the float32 spacing of the sum v * half + pos
    for k in range(1, 400):
        v_lo, v_hi = np.nextafter(v_lo, f32(-np.inf)), np.nextafter(v_hi, f32(np.inf))
        cand += [v_lo, v_hi, f32(float(v0) - k * step), f32(float(v0) + k * step)]
    for v in cand:
        x = dec(v)
        if outside == 0:
            if x == f32(target):
                return f32(v)
        elif (x < f32(target)) if outside < 0 else (x > f32(target)):
            if best is None or abs(float(x) - target) < abs(float(dec(best)) - target):
                best = v
    return None if best is None else f32(best)


def edge_places(g, slots, conf=0.9):
    """Candidates whose joints sit exactly on the four visibility bounds and on the nearest reachable value outside each, for
    vis_margin 0 and 2.  slots: (a, row, col) of three candidates with tiny disjoint boxes."""
    combos = []
    for m in (0, 2):
        for axis, hi in ((0, g.w_out - 1 - m), (1, g.h_out - 1 - m)):
            combos += [(axis, m, 0), (axis, m, -1), (axis, hi, 0), (axis, hi, +1)]
    joints = [dict() for _ in slots]
    for n, (axis, target, outside) in enumerate(combos):
        best = None
        for k in [(n + d) % len(slots) for d in range(len(slots))]:        # the slot from which the value is reached best
            a, row, col = slots[k]
            v = solve_joint(g, a, col if axis == 0 else row, target, axis, outside)
            if v is None or len(joints[k]) >= J:
                continue
            err = abs(float(_decode_joint(g, a, col if axis == 0 else row, axis, v)) - target)
            if best is None or err < best[0]:
                best = (err, k, v)
        assert best is not None, (g.key, axis, target, outside)
        _, k, v = best
        a, row, col = slots[k]
        mid = solve_joint(g, a, row if axis == 0 else col, ((g.h_out if axis == 0 else g.w_out) // 2), 1 - axis, +1)
        joints[k][len(joints[k])] = (v, mid, 0.25, 0.75) if axis == 0 else (mid, v, 0.25, 0.75)
    return [P(a, row, col, conf - 0.01 * k, 0.25, 0.25, joints=joints[k]) for k, (a, row, col) in enumerate(slots)]


def _dense(g, n, seed, size=(1.0, 3.0), conf=None, slots=None):
    """n candidates with distinct scores on random (anchor, cell) slots, box sides uniform in `size` cells"""
    rng = np.random.default_rng(seed)
    A, h, w = g.shape
    if slots is None:
        slots = rng.choice(A * h * w, n, replace=False)
    lo, hi = conf or (g.conf_thr + 0.02, 0.98)
    confs = rng.permutation(np.linspace(lo, hi, n)).astype(f32)
    assert len(set(confs.tolist())) == n
    out = []
    for k, s in enumerate(slots):
        a, cell = divmod(int(s), h * w)
        out.append(P(a, cell // w, cell % w, confs[k], rng.uniform(*size), rng.uniform(*size), rng.uniform(0, 1), rng.uniform(0, 1)))
    return out


def _disjoint(g, n, extra=0, conf=None, a=0, first=0):
    """n disjoint 0.75-cell boxes on distinct cells of anchor slot a (all survive); `extra` of the cells carry a copy of the box
    with a lower score in the next anchor slot (all suppressed)"""
    A, h, w = g.shape
    cells = [(r, c) for r in range(h) for c in range(w)][first:first + n]
    assert len(cells) == n
    out = [P(a, r, c, (0.95 - 0.005 * k) if conf is None else conf, 0.75, 0.75) for k, (r, c) in enumerate(cells)]
    out += [P((a + 1) % A, r, c, 0.55 - 0.001 * k, 0.75, 0.75) for k, (r, c) in enumerate(cells[:extra])]
    return out


def _line(g, start, n=4, a=0, vertical=False, conf=0.9, step=1.0):
    """n boxes 3 cells long, `step` cells apart along the map's long axis, scores descending: neighbours conflict (IoU 2/4), second
    neighbours do not (1/5): the first suppresses the second, whose returned vote frees the third"""
    out = []
    for k in range(n):
        pos = start + k * step
        cell, frac = int(pos), pos - int(pos)
        out.append(P(a, cell, 0, conf - 0.02 * k, 0.5, 3.0, dy=0.5 + frac) if vertical else P(a, 0, cell, conf - 0.02 * k, 3.0, 0.5, dx=0.5 + frac))
    return out


def _build_groups():
    G = []
    add = lambda g, name, places, seed=0: g.cases.append(SimpleNamespace(name=name, places=list(places), seed=seed))

    # ---- 2 x 14 x 14, the network's own shape and anchors, the wrapper's default objectness threshold ----
    g = _group(2, 14, 14, ((6, 3), (12, 6)), 224, 224, conf_thr=0.35, nms_thr=0.5)
    thr = f32(0.35)
    add(g, "empty", [])
    add(g, "one", [P(1, 13, 13, 0.6, 2.0, 1.0)])
    add(g, "two_conflict", [P(0, 5, 5, 0.8, 2.0, 2.0), P(1, 5, 5, 0.7, 2.0, 2.0)])
    add(g, "three_chain", [P(0, 3, 3, 0.9, 3.5, 0.5), P(1, 3, 4, 0.8, 3.5, 0.5), P(0, 3, 5, 0.7, 3.5, 0.5)])
    add(g, "conf_on_threshold", [P(0, 2, 2, thr, 1.0, 1.0), P(1, 2, 9, np.nextafter(thr, f32(1)), 1.0, 1.0), P(0, 9, 2, np.nextafter(thr, f32(0)), 1.0, 1.0),
                                 P(1, 9, 9, 0.6, 1.0, 1.0)])
    add(g, "ties_disjoint", _disjoint(g, 20, conf=0.75, a=1) + _disjoint(g, 20, conf=0.75, a=0, first=30))
    add(g, "ties_overlap", [P(1, 4, 4, 0.75, 2.0, 2.0), P(0, 4, 5, 0.75, 2.0, 2.0, dx=0.0), P(0, 10, 10, 0.75, 2.0, 2.0, dx=0.25), P(0, 10, 9, 0.75, 2.0, 2.0, dx=0.75),
                            P(1, 10, 3, 0.5, 1.0, 1.0), P(0, 12, 3, 0.5, 1.0, 1.0)])
    add(g, "survivors63", _disjoint(g, 63, extra=10))
    add(g, "survivors64", _disjoint(g, 64, extra=10))
    add(g, "survivors65", _disjoint(g, 65, extra=10))
    add(g, "cand64", _dense(g, 64, 11), seed=1)
    add(g, "cand65", _dense(g, 65, 12), seed=2)
    add(g, "edges", edge_places(g, [(0, 0, 0), (1, 13, 13), (0, 12, 6)]), seed=3)
    G.append(g)

    # ---- 1 x 16 x 32: A*h*w is the capacity itself ----
    g = _group(1, 16, 32, ((4, 2),), 320, 192)
    add(g, "full512", _dense(g, 512, 21, size=(8.0, 16.0), slots=range(512)), seed=4)
    add(g, "full512_small", _dense(g, 512, 22, size=(0.5, 1.5), slots=range(512)), seed=5)
    add(g, "cand257", _dense(g, 257, 23, size=(8.0, 14.0)), seed=6)
    add(g, "few", _dense(g, 5, 24) + edge_places(g, [(0, 0, 0), (0, 15, 31), (0, 8, 17)]), seed=7)
    add(g, "empty", [], seed=8)
    G.append(g)

    # ---- 3 x 13 x 13 = 507 ----
    g = _group(3, 13, 13, ((6, 3), (12, 6), (3, 9)), 224, 224)
    add(g, "each_slot", [P(0, 2, 2, 0.9, 2.0, 2.0), P(1, 2, 8, 0.8, 2.0, 2.0), P(2, 8, 2, 0.7, 2.0, 2.0), P(2, 8, 8, 0.65, 2.0, 2.0), P(1, 8, 8, 0.6, 2.0, 2.0)])
    add(g, "full507", _dense(g, 507, 31, size=(6.0, 12.0), slots=range(507)), seed=9)
    add(g, "cand300", _dense(g, 300, 32, size=(5.0, 10.0)), seed=10)
    add(g, "edges", edge_places(g, [(2, 0, 12), (1, 12, 0), (0, 6, 6)]), seed=11)
    add(g, "empty", [], seed=101)
    G.append(g)

    # ---- 1 x 23 x 22: h != w, more than 256 cells in one anchor slot ----
    g = _group(1, 23, 22, ((5, 7),), 218, 232, conf_thr=0.35)
    add(g, "cand256", _dense(g, 256, 41, size=(7.0, 14.0)), seed=12)
    add(g, "cand257", _dense(g, 257, 42, size=(7.0, 14.0)), seed=13)
    add(g, "last_cells", [P(0, 22, 20, 0.9, 2.0, 1.0), P(0, 22, 0, 0.8, 2.0, 1.0), P(0, 0, 21, 0.7, 1.0, 2.0), P(0, 11, 14, 0.6, 3.0, 1.0)]
        + edge_places(g, [(0, 0, 0), (0, 22, 21), (0, 12, 3)], conf=0.5), seed=14)
    add(g, "empty", [], seed=102)
    G.append(g)

    # ---- 2 x 1 x 40 ----
    g = _group(2, 1, 40, ((6, 3), (12, 6)), 402, 24, nms_thr=0.45)
    add(g, "chain", _line(g, 10))
    add(g, "two_suppressors", [P(0, 0, 20, 0.9, 3.0, 0.5), P(0, 0, 21, 0.8, 3.0, 0.5), P(1, 0, 20, 0.7, 3.0, 0.5, dx=1.0), P(1, 0, 30, 0.6, 3.0, 0.5)])
    add(g, "chains_everywhere", _line(g, 1, n=9) + _line(g, 14, n=7, a=1, conf=0.88) + _line(g, 26, n=10, conf=0.97) + _line(g, 26.5, n=10, a=1, conf=0.945), seed=15)
    add(g, "full80", _dense(g, 80, 51, size=(0.4, 3.0), slots=range(80)), seed=16)
    add(g, "edges", edge_places(g, [(0, 0, 0), (1, 0, 39), (0, 0, 22)]), seed=17)
    add(g, "empty", [], seed=103)
    G.append(g)

    # ---- 3 x 40 x 1 ----
    g = _group(3, 40, 1, ((6, 3), (12, 6), (3, 9)), 16, 402, nms_thr=0.45)
    add(g, "chain", _line(g, 10, a=2, vertical=True))
    add(g, "full120", _dense(g, 120, 61, size=(0.4, 3.0), slots=range(120)), seed=18)
    add(g, "edges", edge_places(g, [(2, 0, 0), (1, 39, 0), (0, 17, 0)]), seed=19)
    add(g, "empty", [], seed=104)
    G.append(g)

    # ---- 1 x 1 x 1 ----
    g = _group(1, 1, 1, ((6, 3),), 224, 224)
    add(g, "empty", [])
    add(g, "one", [P(0, 0, 0, 0.7, 0.5, 0.5, joints={0: (0.0, 0.0, 0.5, 0.5)})])
    G.append(g)

    # ---- 2 x 16 x 16: power-of-two geometry, every decoded box coordinate is exact ----
    g = _group(2, 16, 16, ((4, 2), (8, 16)), 256, 256)
    add(g, "iou_on_threshold", [P(0, 4, 4, 0.9, 4.0, 4.0), P(1, 4, 4, 0.8, 2.0, 4.0),            # B inside A, half its area: IoU == 0.5
                                P(0, 10, 4, 0.9, 4.0, 4.0), P(1, 10, 4, 0.8, 2.5, 4.0),           # 0.625 > 0.5: a conflict
                                P(0, 4, 11, 0.7, 0.0, 0.0), P(1, 4, 11, 0.6, 0.0, 0.0),           # a zero-area pair: IoU 0 / 0
                                P(0, 11, 11, 0.7, 2.0, 2.0), P(1, 11, 11, 0.6, 0.0, 2.0)])        # zero area inside a box: IoU 0
    add(g, "cand256", _dense(g, 256, 71, size=(6.0, 12.0)), seed=20)
    add(g, "full512", _dense(g, 512, 72, size=(6.0, 12.0), slots=range(512)), seed=21)
    add(g, "edges", edge_places(g, [(0, 0, 0), (1, 15, 15), (1, 3, 9)]), seed=22)
    add(g, "empty", [], seed=23)
    G.append(g)
    return G


@functools.lru_cache(maxsize=None)
def groups():
    return tuple(_build_groups())


def group(key):
    return next(g for g in groups() if g.key == key)


@functools.lru_cache(maxsize=None)
def case_map(key, name, pred_vis=False):
    g = group(key)
    c = next(c for c in g.cases if c.name == name)
    pm = build_map(g, c.places, c.seed, pred_vis)
    pm.setflags(write=False)
    return pm


_REF = {}


def reference(g, c, vis_margin, pred_vis):
    k = (g.key, c.name, vis_margin, pred_vis)
    if k not in _REF:
        _REF[k] = record(case_map(g.key, c.name, pred_vis), g, vis_margin, pred_vis)
    return _REF[k]


# ---------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------
def census(g, c):
    """counted with the oracle's own decode_maps and box_nms_keep"""
    pm = case_map(g.key, c.name)
    dec = O.decode_maps(pm[None], list(g.anchors), J, DEPTH_MEAN, DEPTH_STD)[0]            # [A, F, hw]
    A, h, w = g.shape
    det = dec.transpose(0, 2, 1).reshape(A * h * w, -1)
    conf = det[:, 4]
    thr = f32(g.conf_thr)
    sel = conf > thr
    n = int(sel.sum())
    out = {"n": n, "slots": sorted(set((np.nonzero(sel)[0] // (h * w)).tolist())), "conf_on_thr": int((conf == thr).sum()),
           "conf_step_above": int((conf == np.nextafter(thr, f32(1))).sum()), "cell_256_up": int((np.nonzero(sel)[0] % (h * w) >= 256).sum()),
           "survivors": 0, "iou_on_thr": 0, "zero_area_pairs": 0, "conflict_col_256": 0, "conflict_row_64": 0, "returning_rows": 0,
           "returning_rows_64": 0, "freed": 0, "two_suppressors_one_suppressed": 0, "tied_scores": 0, "tied_conflicts": 0, "all_tied_disjoint": False}
    if n:
        info = {}
        decode(pm, g, info=info)
        order, keep = O.box_nms_keep(det[sel], g.nms_thr)
        assert np.array_equal(keep, info["keep"] == 0)
        conf_m, ious, keep0 = info["conflicting"], info["ious"], info["keep0"]
        out["survivors"] = int(keep.sum())
        iu = np.triu_indices(n, 1)
        out["iou_on_thr"] = int((ious[iu] == f32(g.nms_thr)).sum())
        out["zero_area_pairs"] = int(np.isnan(ious[iu]).sum())
        out["conflict_col_256"] = int(conf_m[:, 256:].sum())
        out["conflict_row_64"] = int(conf_m[64:].sum())
        out["returning_rows"] = len(info["returned"])
        out["returning_rows_64"] = sum(1 for i in info["returned"] if i >= 64)
        out["freed"] = int(((keep0 > 0) & keep).sum())                        # suppressed by column sum, kept after the votes came back
        sup = ~keep
        out["two_suppressors_one_suppressed"] = int(sum(1 for j in range(n) if keep0[j] >= 2 and (conf_m[:, j] & sup.astype(np.int32)).sum() >= 1
                                                        and (conf_m[:, j] & keep.astype(np.int32)).sum() >= 1))
        sc = info["scores"]
        out["tied_scores"] = int((sc[1:] == sc[:-1]).sum())
        out["tied_conflicts"] = int(sum(1 for i, j in zip(*np.nonzero(conf_m)) if sc[i] == sc[j]))
        out["all_tied_disjoint"] = bool(n > 2 and (sc == sc[0]).all() and conf_m.sum() == 0)
    # joints of the survivors on the visibility bounds, and just outside them
    out["on_bound"], out["off_bound"] = {}, {}
    for m in (0, 2):
        rec = reference(g, c, m, False)
        for axis, lo, hi in ((0, m, g.w_out - 1 - m), (1, m, g.h_out - 1 - m)):
            v = rec["human"][:, :, axis].ravel() if rec["n_det"] else np.zeros(0, f32)
            for name, b, side in (("lo", lo, -1), ("hi", hi, +1)):
                out["on_bound"][(m, axis, name)] = int((v == f32(b)).sum())
                tol = max(abs(b), 1e-30) * 2.0 ** -22
                out["off_bound"][(m, axis, name)] = int((((v < f32(b)) if side < 0 else (v > f32(b))) & (np.abs(v.astype(np.float64) - b) <= tol)).sum())
    return out
