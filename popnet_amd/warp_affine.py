"""The product's one copy of the two pieces of OpenCV 4.2 arithmetic its host code needs to drive the bit-exact warp kernels
(csrc/augment.hip, csrc/a2j_traincrop.hip): cv2.getRotationMatrix2D and the inversion cv2.warpAffine applies to its matrix (imgwarp.cpp).
Used by targets.augmentation (Rotate about the principal point) and a2j_crops (A2J's rotation and scale about the crop centre).  Tests
compare both with tests/cv2_warp_reference.py, which tests/test_cv2_warp_kat.py pins against an exact-rational derivation."""
import math

import numpy as np


def rotation_matrix(center, angle, scale):
    """getRotationMatrix2D: the centre is a Point2f (float32); angle in degrees; alpha, beta in double.  -> [2, 3] float64"""
    cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))
    angle = angle * (math.pi / 180)
    alpha, beta = math.cos(angle) * scale, math.sin(angle) * scale
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


def invert_affine(M):
    """warpAffine's inversion of a matrix given without WARP_INVERSE_MAP, in its operation order.  -> six Python floats, row major"""
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m
