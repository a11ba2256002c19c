"""Edge-case depth frames for the pre-processing (pn_preprocess) and for the 7x7 stems that compute their own input tile from the raw
frames (pn_*_forward_frames), a census of what the frames contain, and mutants of the pre-processing arithmetic (no GPU).

preprocess_kernel (popnet_amd/csrc/api.hip) and the SRC = 1 | 2 instantiations of stem7x7_mfma_kernel / stem7x7_pool_kernel
(popnet_amd/csrc/conv_misc.hip) share popnet_amd/csrc/preproc_pixel.h and promise oracle.preproc.preprocess_frame bit for bit.  The
cases here are the inputs of tests/test_gpu_preproc_edges.py; tests/test_preproc_cases.py holds the conditions they must meet.

  RT_S, YOLO_S, PRE_S   the net sizes S (square S x S input): stem maps S / 2 = 4, 16, 20, 68, 112 (below one 16 x 16 stem tile, exactly one,
                        ragged, ragged, exact) and pooled maps S / 4 = 4, 8, 28, 56, 60 against the fused stem + pool kernel's 8-row x
                        7-column blocks; 48 is the yolo bf16x3 net and the engines' second size; 1 and 17 run the stand-alone
                        pre-processing only (S * S = 1 and 289: a ragged last block of its 256-thread launch, like 8, 40 and 136)
  geometries(S)         frame sizes H x W per S: decimating, up-sampled, one axis exactly 2x (must run: only 2x on BOTH axes makes
                        cv2.resize switch to INTER_AREA), identity, 2 x 2, two pixels high, two pixels wide
  refused(S)            2S x 2S: refused by every entry point
  cases()               (S, geometry, dtype, values, constants) with B = 3 different frames each
  restate               the kernel's arithmetic (preproc_pixel.h) with one flag per plausible error: no flag == the oracle, one flag ==
                        a mutant
  census                what a case contains, counted on the oracle's output

Values.  "plain": uniform(-1, 8), below 0 and above every depth clamp, with the corner pixels of tests/test_gpu_ablation.py (-4, 9.5
and exactly 6).  At S = 1 the one output pixel per frame reads no corner, so there frame 0 is moved below 0 and frame 2 above every
clamp as a whole.  "nonfinite" (frames of at least 5 x 5, not the identity): uniform(0.3, 5.5) with the last column +Inf, [0, 0] NaN,
the centre -Inf (seven pixels wide along an axis that decimates by more than 2, where the taps skip single pixels), [H - 1, 1] +Inf
and, in float16, 65504 at [1, 1] and the smallest subnormal at [1, 2].  What these are for:
  * the last column on an up-sampled axis is read by OpenCV's right-border tail, which copies (D = S[sx]) where the body would compute
    Inf * 1 + Inf * 0 = NaN;
  * [H - 1, 1] is the second tap of the LEFT border columns, where OpenCV does multiply by the clamped weight 0: NaN there is right;
  * -Inf is the only source of the lower clamp value in these frames.
The identity stays finite: cv2 copies there, and the bilinear path equals a copy only while x * 1 + neighbour * 0 == x.  One-pixel
outputs (S = 1) stay finite too: one NaN among three output pixels could not meet the 10 % bound of the census.

Two variants look like mutants and are not (EQUIVALENT; test_preproc_cases.py asserts that no case tells them from the oracle):
  * no_right_clamp: the weight clamp "sx >= W - 1 -> fx = 0" dropped alone.  The source column never exceeds W - 1
    ((S - 0.5) W / S - 0.5 < W - 0.5), and at sx == W - 1 the tail copy overrides the weights;
  * scale_div: scale = W / S in place of 1 / (S / W).  The doubles differ in the last bit for some sizes, the float32 coordinates for
    none of the sizes here.
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import preproc as OP

f32 = np.float32
B = 3

RT_S = (8, 32, 40, 136, 224)
YOLO_S = (16, 32, 48, 112, 224, 240)
PRE_S = (1, 17)
ALL_S = tuple(sorted(set(RT_S + YOLO_S + PRE_S)))

#            depth_max, depth_mean, depth_std: MP-3DHP's, ITOP's, and a std that is no power of two (x / std != x * (1 / std))
CONSTANTS = ((6.0, 3.0, 2.0), (5.0, 3.0, 2.0), (4.5, 2.7, 1.3))

GEOMETRY_NAMES = ("down", "up", "mixed2x", "identity", "min", "thin", "tall")


def geometries(S):
    """[(name, H, W)] without the exact 2x decimation on both axes and without repeats"""
    if S == 1:
        g = [("down", 2, 3), ("down2", 7, 5)]
    else:
        g = [("down", 2 * S + S // 2 + 1, 3 * S - 1), ("up", max(2, S // 3 + 1), max(2, S // 2 - 1)), ("mixed2x", 2 * S, S // 2 + 1),
             ("identity", S, S), ("min", 2, 2), ("thin", 2, 5 * S), ("tall", 5 * S, 2)]
    out, seen = [], set()
    for name, H, W in g:
        if (H == 2 * S and W == 2 * S) or (H, W) in seen:
            continue
        seen.add((H, W))
        out.append((name, H, W))
    return out


def refused(S):
    return (2 * S, 2 * S)


# ---------------------------------------------------------------------------------------------
# the kernel's arithmetic with room for a mutant
# ---------------------------------------------------------------------------------------------
MUTANTS = ("fma_h", "fma_v", "coord_f32", "trunc", "clamp_first", "swap_scale", "y_clamp_weight", "recip", "no_tail_copy", "no_clamp_no_tail")
EQUIVALENT = ("no_right_clamp", "scale_div")


def _mix(v0, w0, v1, w1, fma):
    """v0 * w0 + v1 * w1 in float32, summed left to right; fma: the second product contracted into the sum (one rounding)"""
    if fma:
        return (v1.astype(np.float64) * w1.astype(np.float64) + (v0 * w0).astype(f32).astype(np.float64)).astype(f32)
    return ((v0 * w0).astype(f32) + (v1 * w1).astype(f32)).astype(f32)


def _axis(S, scale, coord_f32, trunc):
    d = np.arange(S)
    if coord_f32:
        c = ((d.astype(f32) + f32(0.5)) * f32(scale) - f32(0.5)).astype(f32)
    else:
        c = ((d + 0.5) * scale - 0.5).astype(f32)
    s = (np.trunc(c) if trunc else np.floor(c)).astype(np.int64)
    return s, (c - s.astype(f32)).astype(f32)


def restate(frame, S, consts, fma_h=False, fma_v=False, coord_f32=False, trunc=False, clamp_first=False, swap_scale=False, y_clamp_weight=False,
            recip=False, no_tail_copy=False, no_clamp_no_tail=False, no_right_clamp=False, scale_div=False):
    """pn_preproc_axis_x / _y / _combine (popnet_amd/csrc/preproc_pixel.h) on one [H, W] frame -> float32 [S, S]"""
    dmax, mean, std = (f32(v) for v in consts)
    f = np.asarray(frame).astype(f32)
    H, W = f.shape
    with np.errstate(invalid="ignore", over="ignore"):
        if clamp_first:
            f = np.where(f < 0, f32(0), f)
            f = np.where(f > dmax, dmax, f)
        scale_x, scale_y = (W / S, H / S) if scale_div else (1.0 / (S / W), 1.0 / (S / H))
        if swap_scale:
            scale_x, scale_y = scale_y, scale_x
        sx, fx = _axis(S, scale_x, coord_f32, trunc)
        sy, fy = _axis(S, scale_y, coord_f32, trunc)
        fx[sx < 0] = 0
        sx[sx < 0] = 0
        if not (no_right_clamp or no_clamp_no_tail):
            fx[sx >= W - 1] = 0
        sx = np.minimum(sx, W - 1)
        x1 = np.minimum(sx + 1, W - 1)
        tail = sx + 1 >= W
        if y_clamp_weight:
            fy[(sy < 0) | (sy >= H - 1)] = 0
        y0, y1 = np.clip(sy, 0, H - 1), np.clip(sy + 1, 0, H - 1)
        a0, a1 = (f32(1) - fx).astype(f32)[None, :], fx[None, :]
        rows = []
        for y in (y0, y1):
            r = f[y]
            h = _mix(r[:, sx], a0, r[:, x1], a1, fma_h)
            if not (no_tail_copy or no_clamp_no_tail):
                h[:, tail] = r[:, sx[tail]]                  # HResizeLinear's tail: D = S[sx]
            rows.append(h)
        v = _mix(rows[0], (f32(1) - fy).astype(f32)[:, None], rows[1], fy[:, None], fma_v)
        if not clamp_first:
            v = np.where(v < 0, f32(0), v)
            v = np.where(v > dmax, dmax, v)
        if recip:
            return ((v - mean).astype(f32) * (f32(1) / std)).astype(f32)
        return ((v - mean).astype(f32) / std).astype(f32)


def bits(a):
    """int32 view of a float32 array with every NaN as ONE pattern: NaN positions, the sign of zeros and every bit of every number count.
    For the restatement and its mutants on the CPU, where a contracted or reordered operation may hand on another NaN of its operands;
    the GPU tests compare the raw int32 views."""
    a = np.ascontiguousarray(a, dtype=f32)
    out = a.view(np.int32).copy()
    out[np.isnan(a)] = 0x7FC00000
    return out


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def _plain(rng, S, H, W, dtype):
    fr = rng.uniform(-1.0, 8.0, (B, H, W))
    if S == 1:
        fr[0] -= 9.0
        fr[2] += 9.0
    fr = fr.astype(dtype)
    fr[0, 0, 0], fr[0, -1, -1], fr[2, 0, -1] = -4.0, 9.5, 6.0
    return fr


def _nonfinite(rng, S, H, W, dtype):
    fr = rng.uniform(0.3, 5.5, (B, H, W)).astype(dtype)
    fr[:, :, -1] = np.inf
    fr[:, 0, 0] = np.nan
    # an axis that decimates by more than 2 (here: by less than 3) skips single pixels; seven in a row hold two whole tap pairs, and the
    # fractions of two pairs are not both 0, where -Inf * 1 + -Inf * 0 would be NaN and not the lower clamp
    ry, rx = (3 if H > 2 * S else 0), (3 if W > 2 * S else 0)
    fr[:, H // 2 - ry:H // 2 + ry + 1, W // 2 - rx:W // 2 + rx + 1] = -np.inf
    fr[:, H - 1, 1] = np.inf
    if dtype == np.float16:
        fr[:, 1, 1] = 65504.0
        fr[:, 1, 2] = np.float16(2.0 ** -24)
    return fr


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for S in ALL_S:
        for name, H, W in geometries(S):
            kinds = ["plain"] + (["nonfinite"] if S > 1 and min(H, W) >= 5 and name != "identity" else [])
            for values in kinds:
                for dtype in (np.float16, np.float32):
                    i = len(out)
                    rng = np.random.default_rng(7919 * S + 31 * H + W + (1 << 20) * (values == "nonfinite") + (1 << 21) * (dtype == np.float32))
                    fr = _plain(rng, S, H, W, dtype) if values == "plain" else _nonfinite(rng, S, H, W, dtype)
                    fr.setflags(write=False)
                    out.append(SimpleNamespace(name="%s_%d_%dx%d_%s_%s_c%d" % (name, S, H, W, "f16" if dtype == np.float16 else "f32", values, i % 3),
                                               S=S, geom=name, H=H, W=W, dtype=dtype, values=values, consts=CONSTANTS[i % 3], frames=fr))
    return tuple(out)


def cases_for(S, geoms=None):
    return [c for c in cases() if c.S == S and (geoms is None or c.geom in geoms)]


_REF = {}


def reference(c):
    """the oracle's own output of the case, float32 [B, 1, S, S], computed once and read-only"""
    if c.name not in _REF:
        with np.errstate(invalid="ignore", over="ignore"):
            r = OP.preprocess_batch(c.frames, input_size=c.S, depth_max=c.consts[0], depth_mean=c.consts[1], depth_std=c.consts[2])
        r.setflags(write=False)
        _REF[c.name] = r
    return _REF[c.name]


def clamp_values(consts):
    dmax, mean, std = (f32(v) for v in consts)
    return (f32(0) - mean) / std, (dmax - mean) / std


def census(c):
    r = reference(c)
    lo, hi = clamp_values(c.consts)
    return {"pixels": int(r.size), "nan": int(np.isnan(r).sum()), "at_low": int((r == lo).sum()), "at_high": int((r == hi).sum()),
            "up_x": c.W < c.S, "up_y": c.H < c.S, "ragged_block": (c.S * c.S) % 256 != 0}
