"""Known answers for the cv2.warpAffine / cv2.getRotationMatrix2D restatement (tests/cv2_warp_reference.py), the way tests/test_cv2_kat.py
pins cv2.resize.

OpenCV cannot be run where this suite runs, so "equal to cv2" means: equal to OpenCV 4.2's generic C++ path as written down in
cv2_warp_reference.py's docstring.  Agreement with a LIVE cv2 build is UNVERIFIED.  Newer OpenCV releases route float32 warpAffine
through different SIMD code whose rounding may differ.  What this file does pin, independently of the restatement's numpy code:

  * `_kat_pixel` derives one destination pixel with exact rationals (fractions.Fraction), operation by operation, rounding to
    binary64 / binary32 with its own round-half-even (`_rnd`) exactly where the C++ rounds.  It shares no code with the restatement
    (only math.cos / math.sin of the angle, which no rational arithmetic can supply).
  * The restatement must give the same bits on a small patch at several angles -- interior pixels, footprints partly outside the
    source and footprints wholly outside.
  * Hex-float answers frozen from that derivation must keep holding, so neither side can drift.
  * Rotation by 0 degrees reproduces the interior of the image exactly.
"""
import math
from fractions import Fraction as Fr

import numpy as np

import cv2_warp_reference as cw


def _rnd(v, p):
    """v (Fraction) rounded to the nearest binary floating-point number with p significant bits, ties to even (no subnormals here)."""
    if v == 0:
        return Fr(0)
    s, a = (-1 if v < 0 else 1), abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fr(2) ** e > a:
        e -= 1
    q = Fr(2) ** (e - p + 1)
    return s * Fr(round(a / q)) * q          # round(Fraction) is round-half-even


def _d(v):
    return _rnd(v, 53)


def _f(v):
    return _rnd(v, 24)


def _kat_matrix(cx, cy, rot):
    """getRotationMatrix2D followed by warpAffine's inversion, every double operation rounded once."""
    cx, cy = Fr(float(np.float32(cx))), Fr(float(np.float32(cy)))
    ang = float(_d(Fr(rot) * _d(Fr(math.pi) / 180)))
    al, be = Fr(math.cos(ang)), Fr(math.sin(ang))
    m = [al, be, _d(_d(_d(1 - al) * cx) - _d(be * cy)), -be, al, _d(_d(be * cx) + _d(_d(1 - al) * cy))]
    D = _d(_d(m[0] * m[4]) - _d(m[1] * m[3]))
    D = _d(1 / D) if D != 0 else Fr(0)
    A11, A22 = _d(m[4] * D), _d(m[0] * D)
    m[0], m[1], m[3], m[4] = A11, _d(m[1] * -D), _d(m[3] * -D), A22
    b1 = _d(_d(-m[0] * m[2]) - _d(m[1] * m[5]))
    b2 = _d(_d(-m[3] * m[2]) - _d(m[4] * m[5]))
    m[2], m[5] = b1, b2
    return m


def _kat_pixel(src, m, x, y):
    """One pixel of warpAffine(src, M, ..., INTER_LINEAR), border constant 0.  -> (value as float32, 'interior' | 'partial' | 'outside')"""
    H, W = src.shape
    adelta = round(_d(_d(m[0] * x) * 1024))
    bdelta = round(_d(_d(m[3] * x) * 1024))
    X0 = round(_d(_d(_d(m[1] * y) + m[2]) * 1024)) + 16
    Y0 = round(_d(_d(_d(m[4] * y) + m[5]) * 1024)) + 16
    X, Y = (X0 + adelta) >> 5, (Y0 + bdelta) >> 5
    sx, sy = max(min(X >> 5, 32767), -32768), max(min(Y >> 5, 32767), -32768)
    fx, fy = Fr(X & 31, 32), Fr(Y & 31, 32)
    taps = [(sy, sx, _f(_f(1 - fy) * _f(1 - fx))), (sy, sx + 1, _f(_f(1 - fy) * fx)), (sy + 1, sx, _f(fy * _f(1 - fx))), (sy + 1, sx + 1, _f(fy * fx))]
    inside = [0 <= r < H and 0 <= c < W for r, c, _ in taps]
    acc = None
    for (r, c, w), ok in zip(taps, inside):
        t = _f((Fr(float(src[r, c])) if ok else Fr(0)) * w)
        acc = t if acc is None else _f(acc + t)
    kind = "interior" if all(inside) else ("partial" if any(inside) else "outside")
    return np.float32(float(acc)), kind


def _patch():
    rng = np.random.default_rng(2024)
    return rng.uniform(0.3, 5.9, (9, 11)).astype(np.float32)


CENTRE = (4.3, 3.9)
ANGLES = (-10.0, -3.3, 0.0, 7.25, 10.0, 37.0)


def test_restatement_equals_the_exact_rational_derivation_bit_for_bit():
    src = _patch()
    kinds = set()
    for rot in ANGLES:
        M = cw.getRotationMatrix2D(CENTRE, rot, 1.0)
        m = _kat_matrix(CENTRE[0], CENTRE[1], rot)
        assert [float(v) for v in m] == cw.invert_affine(M), rot
        got = cw.warpAffine(src, M, (src.shape[1], src.shape[0]))
        assert got.dtype == np.float32 and got.shape == src.shape
        for y in range(src.shape[0]):
            for x in range(src.shape[1]):
                want, kind = _kat_pixel(src, m, x, y)
                kinds.add(kind)
                assert got[y, x].tobytes() == want.tobytes(), (rot, x, y, kind, float(got[y, x]).hex(), float(want).hex())
    assert kinds == {"interior", "partial", "outside"}


# (angle, x, y, footprint, hex of the float32 answer) -- frozen from _kat_pixel
FROZEN = [
    (-10.0, 5, 4, "interior", "0x1.0bb52e0000000p+0"),
    (7.25, 3, 6, "interior", "0x1.7130000000000p+0"),
    (37.0, 6, 3, "interior", "0x1.c7e94a0000000p+1"),
    (10.0, 0, 0, "partial", "0x1.5769520000000p-1"),
    (-10.0, 10, 8, "partial", "0x1.971f660000000p+0"),
    (-3.3, 10, 4, "partial", "0x1.1e52100000000p+1"),
    (0.0, 10, 8, "partial", "0x1.95d8500000000p-1"),
    (37.0, 10, 0, "outside", "0x0.0p+0"),
    (37.0, 0, 8, "outside", "0x0.0p+0"),
]


def test_frozen_answers_hold():
    src = _patch()
    assert float(src[4, 5]).hex() == "0x1.bc17e00000000p-2"      # the patch itself is part of the known answer
    seen = set()
    for rot, x, y, kind, hx in FROZEN:
        m = _kat_matrix(CENTRE[0], CENTRE[1], rot)
        want, k = _kat_pixel(src, m, x, y)
        got = cw.warpAffine(src, cw.getRotationMatrix2D(CENTRE, rot, 1.0), (src.shape[1], src.shape[0]))[y, x]
        assert k == kind and float(want).hex() == hx and float(got).hex() == hx, (rot, x, y, k, float(want).hex(), float(got).hex())
        seen.add(kind)
    assert seen == {"interior", "partial", "outside"}


def test_rotation_by_zero_reproduces_the_interior_exactly():
    rng = np.random.default_rng(5)
    src = rng.uniform(0, 6, (40, 30)).astype(np.float32)
    for centre in ((15.0, 20.0), (11.7421875, 17.626403808593750), (0.0, 0.0)):
        M = cw.getRotationMatrix2D(centre, 0.0, 1.0)
        assert np.array_equal(M, np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
        out = cw.warpAffine(src, M, (30, 40))
        assert np.array_equal(out[:-1, :-1], src[:-1, :-1])
        # the last row / column: the 2 x 2 footprint reaches one past the source with weight 0 -- value * 1 + 0 * 0
        assert np.array_equal(out, src)


def test_a_wider_destination_and_a_translation_read_zero_outside():
    src = _patch()
    M = np.array([[1.0, 0.0, 2.5], [0.0, 1.0, -1.25]])          # dst(x, y) = src(x - 2.5, y + 1.25)
    out = cw.warpAffine(src, M, (14, 9))
    assert out.shape == (9, 14) and np.all(out[:, 0:2] == 0) and np.all(out[-1, :] == 0)
    m = [Fr(v) for v in cw.invert_affine(M)]
    for y, x in ((0, 2), (3, 7), (7, 13), (8, 5)):
        assert out[y, x].tobytes() == _kat_pixel(src, m, x, y)[0].tobytes()
