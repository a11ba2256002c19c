"""numpy restatement of the inference crop, dataPreprocess of third_party_methods/A2J_experiments/a2j_test_pred_box_new.py:268-313, that
pn_a2j_crop (csrc/a2j.hip) replaces: box rows -> crops, one numpy / Python operation per operation of the script, so that every value has
the type the script gives it (the box array is float32; `float32 scalar - 0`, `int + float32 scalar` and `float32 scalar > 0.01` stay float32
under the numpy the goldens are made with, 2.x).  Test infrastructure: slow and explicit, written from the script's lines and NOT from
popnet_amd.a2j_crops.box_items -- tests/test_a2j_crop_edges.py compares the two derivations on every row of tests/a2j_crop_cases.py, and this
one with the reference's own outputs (tests/golden/a2j_crop_edges.npz).

Where the script raises, the row's flag is 1 and its crop zeros (the project's rule, include/popnet_hip.h).  One rule is added to the
script's own exceptions: an int() of a value past what a C int holds (|v| > 2^31 - 128, the largest float32 below 2^31) counts as a raise --
in the script it stands for a zero image, a slice or a loop of that size, which ends in a MemoryError or never.
"""
import numpy as np

INT_LIMIT = 2147483520.0


class Raised(Exception):
    pass


def _int(v):
    """int() as the script calls it; a NaN and an infinity raise by themselves"""
    if not (-INT_LIMIT <= float(v) <= INT_LIMIT) and np.isfinite(v):
        raise OverflowError("int() of %r: past a C int" % (v,))
    return int(v)


def nearest(img, crop_w, crop_h):
    """cv2.resize(img, (crop_w, crop_h), interpolation=cv2.INTER_NEAREST): source index min(floor(d * (1 / (dsize / ssize))), ssize - 1) in double"""
    sh, sw = img.shape
    if sh == 0 or sw == 0:
        raise Raised("cv2.resize of an empty image")
    xs = np.minimum(np.floor(np.arange(crop_w) * (1.0 / (crop_w / sw))).astype(np.int64), sw - 1)
    ys = np.minimum(np.floor(np.arange(crop_h) * (1.0 / (crop_h / sh))).astype(np.int64), sh - 1)
    return img[ys][:, xs]


def paste_loop(canvas, cut, start1, start2, end1, end2, info, less=lambda a, b: a < b):
    """:295-299, pixel by pixel.  `less`: the comparison of the four inequalities (the GPU test swaps it to show that it can fail)."""
    pasted = bound = 0
    for i in range(canvas.shape[0]):
        for j in range(canvas.shape[1]):
            if less(start1, i) and less(i, end1) and less(start2, j) and less(j, end2):
                if int(i - start1) < cut.shape[0] and int(j - start2) < cut.shape[1]:
                    canvas[i][j] = cut[int(i - start1)][int(j - start2)]
                    pasted += 1
                else:
                    bound += 1
    info.update(pasted=pasted, size_bound=bound)


def paste_vector(canvas, cut, start1, start2, end1, end2, info):
    """The same paste with one mask per axis: every condition of the loop concerns i alone or j alone."""
    def axis(n, start, end, size):
        k = np.arange(n).astype(np.float32)                  # a Python int against a float32 scalar is a float32 (exact: n < 2^24)
        d = k - np.float32(start)                            # int - float32 scalar: float32; int - 0: the int itself
        ineq = (start < k) & (k < end)
        src = np.where(ineq, d, 0).astype(np.int64)          # int(): truncation; ineq implies d > 0
        return ineq, ineq & (src < size), src
    iy, oky, py = axis(canvas.shape[0], start1, end1, cut.shape[0])
    ix, okx, px = axis(canvas.shape[1], start2, end2, cut.shape[1])
    canvas[np.ix_(oky, okx)] = cut[np.ix_(py[oky], px[okx])]
    pasted = int(oky.sum()) * int(okx.sum())
    info.update(pasted=pasted, size_bound=int(iy.sum()) * int(ix.sum()) - pasted)


def preprocess(frame, box, img_w, img_h, crop_w, crop_h, mean=3, std=2, paste=paste_vector, end_rule="script", info=None):
    """One row.  frame [H, W], box: float32 (x0, y0, x1, y1, conf) -> [crop_h, crop_w] float32; raises where the script raises.
    info (a dict) receives the intermediate values the class census reads.  end_rule: "script"; "no_start" is the deliberately wrong
    end = size (the `+ start` dropped) of the GPU test; "none" leaves both ends at the paste image's size, which changes no pixel: the
    size test int(i - start) < size already implies i < size + start (tests/test_a2j_crop_edges.py shows it on every row)."""
    info = {} if info is None else info
    box = np.asarray(box, dtype=np.float32)
    depth = np.asarray(frame).astype(np.float64)
    out = np.zeros((crop_h, crop_w, 1), dtype="float32")
    info.update(taken=bool(box[4] > 0.01), padded=False, raised=False)
    if box[4] > 0.01:
        xmin = max(box[0], 0)
        ymin = max(box[1], 0)
        xmax = min(box[2], depth.shape[1] - 1)
        ymax = min(box[3], depth.shape[0] - 1)
        cy0, cy1, cx0, cx1 = _int(ymin), _int(ymax), _int(xmin), _int(xmax)
        cut = depth.copy()[cy0:cy1, cx0:cx1]
        info.update(cy0=cy0, cy1=cy1, cx0=cx0, cx1=cx1, ih=cut.shape[0], iw=cut.shape[1])
        if box[0] < 0 or box[1] < 0 or box[2] > img_w or box[3] > img_h:
            info.update(padded=True)
            sh, sw = _int(box[3] - box[1]), _int(box[2] - box[0])
            info.update(sh=sh, sw=sw)
            canvas = np.zeros((sh, sw))
            start1 = start2 = 0
            end1, end2 = canvas.shape[0], canvas.shape[1]
            if box[1] < 0:
                start1 = 0 - box[1]
            if box[0] < 0:
                start2 = 0 - box[0]
            if box[3] > img_h and end_rule != "none":
                end1 = cut.shape[0] + (start1 if end_rule == "script" else 0)
            if box[2] > img_w and end_rule != "none":
                end2 = cut.shape[1] + (start2 if end_rule == "script" else 0)
            info.update(start1=start1, start2=start2, end1=end1, end2=end2)
            paste(canvas, cut, start1, start2, end1, end2, info)
            cut = canvas
        else:
            info.update(sh=cut.shape[0], sw=cut.shape[1])
        img = nearest(np.asarray(cut, np.float32), crop_w, crop_h)
        img = np.asarray(img, dtype="float32")
        with np.errstate(invalid="ignore"):
            img = (img - mean) / std
        out[:, :, 0] = img
    return np.asarray(out).transpose(2, 0, 1)[0]


def crops(frames, rows, img_wh, crop_wh, mean=3, std=2, **kw):
    """frames [F, H, W], rows [n, 6] float32 (frame, x0, y0, x1, y1, conf) -> (crops [n, crop_h, crop_w] float32, flags [n] int32, infos).
    A frame index that names none of the F frames raises: the script has no such file to load, whatever the confidence."""
    rows = np.asarray(rows, dtype=np.float32)
    n, (cw, ch) = len(rows), crop_wh
    out, flags, infos = np.zeros((n, ch, cw), np.float32), np.zeros((n,), np.int32), []
    for k, r in enumerate(rows):
        info = {}
        try:
            if not (0 <= r[0] < len(frames)):
                raise Raised("no frame %r" % (r[0],))
            out[k] = preprocess(frames[int(r[0])], r[1:], img_wh[0], img_wh[1], cw, ch, mean, std, info=info, **kw)
        except (Raised, ValueError, OverflowError, ZeroDivisionError, MemoryError) as e:
            info.update(raised=True, why=type(e).__name__)
            flags[k] = 1
        infos.append(info)
    return out, flags, infos


def digest(crop):
    """SHA-256 of a crop's float32 bytes, every NaN replaced by one NaN first (the payload is not compared) -> [32] uint8"""
    import hashlib
    c = np.array(crop, dtype=np.float32)
    c[np.isnan(c)] = np.float32("nan")
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(c).tobytes()).digest(), dtype=np.uint8)
