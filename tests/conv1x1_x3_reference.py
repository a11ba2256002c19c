"""fp64 host references of the split-bf16 1x1 convolution entries (csrc/conv1x1_x3.hip) that tests/nchw_layer_reference.py does not hold:
the weight gradient with its depth read from pn_conv1x1_x3_plan_info, and deliberately WRONG forward / data-gradient / weight-gradient
references (a product term dropped, a channel shifted) for the tests that show the allowance can reject.

Definitions (csrc/conv1x1_x3_kernels.h): both operands split as NR.split does, hi = RNE_bf16(v), lo = RNE_bf16(fp32(v - hi)); a product sum is
a_hi b_hi + a_hi b_lo + a_lo b_hi in fp32, no lo * lo.  Forward / data gradient: NR.conv_fwd_ref / NR.conv_dgrad_ref with ks = 1, x3 = True
(n = 3 K + bias + accumulate).  Weight gradient: a block adds the pixels of its slice (per_slice pixels, chunk padding included, x 3 products)
in fp32, then the slices are added in order: depth = 3 x per_slice + slices, |error| <= depth U S + float32 rounding."""
import torch
import torch.nn.functional as F

import nchw_layer_reference as NR
from layer_reference import U, allowance, f32

TERMS = ("hi hi", "hi lo", "lo hi")


def wgrad_depth(p):
    assert p["per_slice_unit"] == "pixels"
    return 3 * p["per_slice"] + p["slices"]


def wgrad_ref(x, dy, p, drop=None, shift=0):
    """x [N, Cin, h, w], dy [N, Cout, h, w] float64 of float32 values, p: the plan.  -> (dw [Cout, Cin, 1, 1], allowance).
    drop: a term of TERMS (dy x) left out; shift: x's channels rolled by that many -- wrong references."""
    x, dy = f32(x), f32(dy)
    if shift:
        x = torch.roll(x, shift, 1)
    xh, xl = NR.split(x)
    dh, dl = NR.split(dy)
    pairs = [(dh, xh), (dh, xl), (dl, xh)]
    r = sum(NR._cw(a, b, 1, 1, 0) for t, (a, b) in zip(TERMS, pairs) if t != drop)
    S = sum(NR._cw(a.abs(), b.abs(), 1, 1, 0) for a, b in pairs)
    return r, NR._round32(r, wgrad_depth(p) * U * S)


def fwd_ref(x, w, bias, prev, drop=None, shift=0):
    """NR.conv_fwd_ref(ks = 1, x3 = True) with a term of TERMS (w x) dropped or x's channels rolled: wrong references (drop = None, shift = 0: the right one)."""
    x, w = f32(x), f32(w)
    if shift:
        x = torch.roll(x, shift, 1)
    xh, xl = NR.split(x)
    wh, wl = NR.split(w)
    pairs = [(wh, xh), (wh, xl), (wl, xh)]                     # a = the weight pack, b = the activations
    r = sum(F.conv2d(b, a) for t, (a, b) in zip(TERMS, pairs) if t != drop)
    S = sum(F.conv2d(b.abs(), a.abs()) for a, b in pairs)
    n = 3 * w.shape[1]
    if bias is not None:
        b = f32(bias).view(1, -1, 1, 1)
        r, S, n = r + b, S + b.abs(), n + 1
    if prev is not None:
        r, S, n = r + f32(prev), S + f32(prev).abs(), n + 1
    return r, allowance(r, n * U * S, "fp32")


def dgrad_ref(dy, w, prev, drop=None, shift=0):
    """NR.conv_dgrad_ref(ks = 1, x3 = True) the same way: the pack is w transposed, the activations dy."""
    dy, w = f32(dy), f32(w)
    if shift:
        dy = torch.roll(dy, shift, 1)
    dh, dl = NR.split(dy)
    wh, wl = NR.split(w)
    pairs = [(wh, dh), (wh, dl), (wl, dh)]
    r = sum(F.conv_transpose2d(b, a) for t, (a, b) in zip(TERMS, pairs) if t != drop)
    S = sum(F.conv_transpose2d(b.abs(), a.abs()) for a, b in pairs)
    n = 3 * w.shape[0]
    if prev is not None:
        r, S, n = r + f32(prev), S + f32(prev).abs(), n + 1
    return r, allowance(r, n * U * S, "fp32")
