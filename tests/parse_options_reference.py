"""numpy restatement of the pose parse for every argument the reference accepts (tpm/lib/utils/paf_to_pose.py:75
NMS(heatmaps, upsampFactor, bool_refine_center, bool_gaussian_filt); MODEL.DOWNSAMPLE and TEST.NUM_INTERMED_PTS_BETWEEN_KEYPOINTS in
find_connected_joints :156-264).  What the HIP parse kernels' run-time instantiations and gen_peaks_kernel (popnet_amd/csrc/parse_device.h, parse_peaks.hip) are written against, and itself pinned
by tests/golden/parse_options.npz -- the reference's own functions under the cv2.resize restatement and the installed scipy
(tests/test_parse_options_reference.py).

The rules beyond oracle/parse_paf.py:

  gaussian_sigma3   scipy.ndimage.gaussian_filter(patch, sigma=3) on float32 without scipy: radius int(4 * 3 + 0.5) = 12, the 13 distinct
                    weights frozen below, axis 0 then axis 1, each output a float64 accumulation
                    x[l] w[12] + sum_{k=-12..-1} (x[l+k] + x[l-k]) w[k+12] rounded to float32, boundary 'reflect'
  nms               refined (patch up-sampled by f, optional filter, first arg-max) or not ((p + 0.5) f - 0.5 and the map's own value)
  mean_pairwise     np.mean of n contiguous float64 values: n < 8 a running sum, else eight accumulators over whole blocks of eight,
                    ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remaining elements one by one
  connect           n sample points, each scored x * dx + y * dy in float64 with both products rounded (oracle/parse_paf.py's form of
                    intermed_paf.dot(limb_dir)), score = mean + min(0.5 (h f) / dist - 1, 0), criterion 1 = count > 0.8 n in float64

The flags (swap_axes, edge, seq_mean, cnt_ge) make the mutants of tests/test_parse_options_reference.py; their defaults are the contract.
"""
import numpy as np

from oracle import cv2_resize as R
from oracle import parse_paf as O

J, L = O.NUM_KEYPOINTS, O.NUM_LIMBS
FACTORS = (1, 2, 4, 8, 16)
NMS_OPTIONS = tuple((f, r, g) for f in FACTORS for r in (True, False) for g in (False, True))
PARSE_OPTIONS = ((8, 10), (8, 2), (8, 7), (8, 8), (8, 9), (8, 16), (8, 17), (8, 32), (4, 10), (16, 10), (1, 5))
# cases of tests/parse_cases.py the golden stores: the workload's shape, both non-square shapes, the three tiny maps, a frame whose
# record overflows (peaks33: second pass) and one with 33 open rows; max_map (64 x 64) for NMS at f = 16 with the filter only
NMS_CASES = ("corners", "edges", "ties", "wide", "tall", "plateau_9x13", "plateau_5x7", "const_3x3", "peaks33")
NMS_BIG = ("max_map", (16, True, True))
PARSE_CASES = ("corners", "edges", "ties", "cnt", "penalty", "wide", "tall", "plateau_9x13", "plateau_5x7", "const_3x3", "peaks33", "rows33")

GAUSS_RADIUS = 12
# scipy.ndimage._filters._gaussian_kernel1d(3.0, 0, 12)[0:13] ([12] is the centre; the kernel is symmetric)
GAUSS_W = np.array([float.fromhex(v) for v in (
    "0x1.763a210dfb306p-15", "0x1.4fbe39149e277p-13", "0x1.0d8a5ad43c165p-11", "0x1.8345966f69518p-10", "0x1.f1e9915139406p-9",
    "0x1.1e6bccad344bap-7", "0x1.26defcaeb0202p-6", "0x1.0fa58939b528fp-5", "0x1.bfde9c12bec92p-5", "0x1.4a614d1afd337p-4",
    "0x1.b42a57d56c0bep-4", "0x1.01a25f86eb137p-3", "0x1.105a329f98197p-3")], dtype=np.float64)


def nms_key(f, refine, gauss):
    return "f%d_r%d_g%d" % (f, int(refine), int(gauss))


def parse_key(f, n):
    return "f%d_n%d" % (f, n)


def _border(i, n, edge):
    if edge:
        return np.clip(i, 0, n - 1)
    m = np.mod(i, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def _filter_axis(x, axis, edge):
    """one pass of scipy's correlate1d with the symmetric 25-tap kernel along `axis` of a float32 array -> float32"""
    x = np.moveaxis(np.asarray(x, dtype=np.float32), axis, 0)
    n = x.shape[0]
    xd = x.astype(np.float64)
    l = np.arange(n)
    tmp = xd * GAUSS_W[GAUSS_RADIUS]
    for k in range(-GAUSS_RADIUS, 0):
        tmp = tmp + (xd[_border(l + k, n, edge)] + xd[_border(l - k, n, edge)]) * GAUSS_W[k + GAUSS_RADIUS]
    return np.moveaxis(tmp.astype(np.float32), 0, axis)


def gaussian_sigma3(patch, swap_axes=False, edge=False):
    axes = (1, 0) if swap_axes else (0, 1)
    out = np.asarray(patch, dtype=np.float32)
    for a in axes:
        out = _filter_axis(out, a, edge)
    return out


def nms(heatmaps, f, refine=True, gauss=False, thresh=O.THRESH_HEATMAP, num_keypoints=J, swap_axes=False, edge=False):
    """-> per joint type a float64 [n, 4] array (x, y, score, running id)"""
    out, cnt = [], 0
    for joint in range(num_keypoints):
        m = heatmaps[:, :, joint]
        h, w = m.shape
        coords = O.find_peaks(thresh, m)
        peaks = np.zeros((len(coords), 4))
        for i, (px, py) in enumerate(coords):
            if refine:
                x0, y0, x1, y1 = max(0, px - 2), max(0, py - 2), min(w - 1, px + 2), min(h - 1, py + 2)
                up = R.resize(np.ascontiguousarray(m[y0:y1 + 1, x0:x1 + 1]), None, fx=f, fy=f, interpolation=R.INTER_CUBIC)
                if gauss:
                    up = gaussian_sigma3(up, swap_axes, edge)
                my, mx = np.unravel_index(up.argmax(), up.shape)
                peaks[i] = (f * x0 + mx, f * y0 + my, up[my, mx], cnt)
            else:
                peaks[i] = ((px + 0.5) * f - 0.5, (py + 0.5) * f - 0.5, m[py, px], cnt)
            cnt += 1
        out.append(peaks)
    return out


def mean_pairwise(s):
    n = len(s)
    if n < 8:
        res = 0.0
        for v in s:
            res = res + v
        return res / n
    r = [s[j] for j in range(8)]
    i = 8
    while i < n - (n % 8):
        for j in range(8):
            r[j] = r[j] + s[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for k in range(i, n):
        res = res + s[k]
    return res / n


def mean_sequential(s):
    res = 0.0
    for v in s:
        res = res + v
    return res / len(s)


def connect(paf_up, per_type, n, thresh_paf=O.THRESH_PAF, seq_mean=False, cnt_ge=False):
    """find_connected_joints with n sample points -> per limb a float64 [m, 5] array (src_id, dst_id, score, i, j) or []"""
    H = paf_up.shape[0]
    out = []
    for limb, (js_t, jd_t) in enumerate(O.LIMBS):
        src, dst = per_type[js_t], per_type[jd_t]
        if len(src) == 0 or len(dst) == 0:
            out.append([])
            continue
        cand = []
        for i, js in enumerate(src):
            for j, jd in enumerate(dst):
                d = jd[:2] - js[:2]
                dist = np.sqrt(np.sum(d ** 2)) + 1e-8
                d = d / dist
                xs = np.round(np.linspace(js[0], jd[0], num=n)).astype(np.intp)
                ys = np.round(np.linspace(js[1], jd[1], num=n)).astype(np.intp)
                pts = paf_up[ys, xs, 2 * limb].astype(np.float64) * d[0] + paf_up[ys, xs, 2 * limb + 1].astype(np.float64) * d[1]
                score = (mean_sequential(pts) if seq_mean else mean_pairwise(pts)) + min(0.5 * H / dist - 1, 0)
                count = np.count_nonzero(pts > thresh_paf)
                c1 = (count >= 0.8 * n) if cnt_ge else (count > 0.8 * n)
                if c1 and score > 0:
                    cand.append((i, j, score))
        cand = sorted(cand, key=lambda c: c[2], reverse=True)
        conn = np.empty((0, 5))
        for i, j, s in cand:
            if i not in conn[:, 3] and j not in conn[:, 4]:
                conn = np.vstack([conn, [src[i][3], dst[j][3], s, i, j]])
                if len(conn) >= min(len(src), len(dst)):
                    break
        out.append(conn)
    return out


def paf_to_pose(heat, paf, f, n, paf_up=None, **mut):
    """-> (joint_list [N, 5], person_to_joint_assoc [P, J + 2], connected limbs); paf_up: the up-sampled PAF when the caller has it"""
    per_type = nms(heat, f)
    joint_list = np.array([tuple(p) + (jt,) for jt, peaks in enumerate(per_type) for p in peaks])
    if paf_up is None:
        paf_up = R.resize(np.ascontiguousarray(paf), None, fx=f, fy=f, interpolation=R.INTER_CUBIC)
    connected = connect(paf_up, per_type, n, **mut)
    assoc = O.group_limbs_of_same_person(connected, joint_list)
    return joint_list, assoc, connected


def flat_peaks(per_type):
    """the per-type list as one [N, 4] array and the J counts (how the golden stores it)"""
    counts = np.array([len(p) for p in per_type], dtype=np.int32)
    return np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 4) for p in per_type]), counts


def flat_connections(connected):
    """the per-limb list as one [M, 6] array (limb, src_id, dst_id, score, i, j)"""
    rows = [np.concatenate([np.full((len(c), 1), float(l)), np.asarray(c, dtype=np.float64).reshape(-1, 5)], axis=1)
            for l, c in enumerate(connected)]
    return np.concatenate(rows).reshape(-1, 6)
