"""What the bf16x3 FORMAT alone costs the A2J net: an fp64 torch emulation, independent of the kernels (no GPU, no library call).

Every number the bf16x3 net stores is a pair hi = RNE_bf16(v), lo = RNE_bf16(float32(v - hi)); every product it forms is
x_hi W_hi + x_lo W_hi + x_hi W_lo.  This module runs A2J_model (ResNet-50 with the dilated layer4, three heads, the anchor vote) with exactly
those roundings and nothing else: all sums in float64, so neither a summation order nor an fp32 accumulator is in it.

  weights      folded as net_pack.hip does: BatchNorm scale in double, w_f = float32(w * scale), W_hi = RNE_bf16(w_f), W_lo = RNE_bf16(float32(w_f - W_hi));
               the stem's [64, 3, 7, 7] weights summed over Cin in double first (three identical input channels); the bias float32((b - mean) * scale + beta)
  convolution  conv(x_hi + x_lo, W_hi) + conv(x_hi, W_lo) in float64, + bias, + the residual hi + lo, then the activation
  storage      every stored tensor (the stem's input included) is re-split into hi and lo; the max pool runs on hi + lo
  vote         the float64 softmax vote of the reference on the heads hi + lo

Inputs: the two shapes of tests/golden/a2j.npz -- AC.SMALL (80 x 96, 3 crops) and AC.LARGE (288 x 288, 2 crops), weights and crops as tests/a2j_cases.py
makes them.  DEVIATION holds max |emulated joints - golden fp64 joints| over the crops and joints of each shape, as (pixels over y and x, z); printed by

    python tests/a2j_x3_emulation.py            # both shapes: the large one is about 200 GFLOP of float64, minutes on a desktop CPU

tests/test_a2j_x3_emulation.py recomputes the small shape and asserts the constant; tests/test_gpu_a2j_x3.py bounds the GPU's bf16x3 joints by
2 x DEVIATION + the golden's fp32 joints tolerance.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import a2j_cases as AC  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "a2j.npz")

# max |emulated joints - golden fp64 joints|: (pixels over y and x, z), by `python tests/a2j_x3_emulation.py`
DEVIATION = {"s": (2.81513e-05, 3.4794e-06), "l": (0.000112058, 7.20124e-06)}

NBLOCKS, STRIDES, DILS = (3, 4, 6, 3), (1, 2, 2, 1), (1, 1, 1, 2)
HEADS = (("classificationModel", "x3"), ("regressionModel", "x4"), ("DepthRegressionModel", "x4"))


def rne_bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def f32(t):
    return t.to(torch.float32).to(torch.float64)


def split(v):
    """float64 tensor -> (hi, lo) as float64: the two stored planes of float32(v)."""
    v = f32(v)
    hi = rne_bf16(v)
    return hi, rne_bf16(f32(v - hi))


def folded(sd, conv, bn, sum_cin=False):
    """(W_hi, W_lo, bias) of a convolution with its BatchNorm folded in (bn = None: the convolution's own bias alone)."""
    w = sd[conv + ".weight"].double()
    if sum_cin:
        w = w.sum(1, keepdim=True)
    b = sd.get(conv + ".bias")
    shift = torch.zeros(w.shape[0], dtype=torch.float64) if b is None else b.double()
    if bn is not None:
        scale = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + 1e-5)
        shift = (shift - sd[bn + ".running_mean"].double()) * scale + sd[bn + ".bias"].double()
        w = w * scale.view(-1, 1, 1, 1)
    hi, lo = split(w)
    return hi, lo, f32(shift)


def conv(x, sd, name, bn, stride=1, dil=1, relu=True, res=None, sum_cin=False):
    """x, res: (hi, lo) pairs.  -> the stored (hi, lo) pair of the convolution's output."""
    w_hi, w_lo, bias = folded(sd, name, bn, sum_cin)
    pad = dil * (w_hi.shape[2] // 2)
    y = F.conv2d(x[0] + x[1], w_hi, stride=stride, padding=pad, dilation=dil) + F.conv2d(x[0], w_lo, stride=stride, padding=pad, dilation=dil)
    y = y + bias.view(1, -1, 1, 1)
    if res is not None:
        y = y + (res[0] + res[1])
    return split(y.clamp_min(0) if relu else y)


def forward(sd, x):
    """x [B, 1, H, W] float32 crops -> the three heads as float64 NCHW tensors (hi + lo): cls [B, 240, h, w], reg [B, 480, h, w], dep [B, 240, h, w]."""
    a = conv(split(torch.as_tensor(x).double()), sd, "Backbone.model.conv1", "Backbone.model.bn1", stride=2, sum_cin=True)
    a = split(F.max_pool2d(a[0] + a[1], 3, 2, 1))
    feats = {}
    for l in range(4):
        for i in range(NBLOCKS[l]):
            p = "Backbone.model.layer%d.%d." % (l + 1, i)
            s = STRIDES[l] if i == 0 else 1
            idn = conv(a, sd, p + "downsample.0", p + "downsample.1", stride=s, relu=False) if i == 0 else a
            t = conv(a, sd, p + "conv1", p + "bn1")
            t = conv(t, sd, p + "conv2", p + "bn2", stride=s, dil=1 if i == 0 else DILS[l])
            a = conv(t, sd, p + "conv3", p + "bn3", res=idn)
        feats["x%d" % (l + 1)] = a
    heads = []
    for name, src in HEADS:
        t = feats[src]
        for i in (1, 2, 3, 4):
            t = conv(t, sd, "%s.conv%d" % (name, i), "%s.bn%d" % (name, i))
        t = conv(t, sd, name + ".output", None, relu=False)
        heads.append(t[0] + t[1])
    return heads


def generate_anchors():
    v = np.array([2.0, 6.0, 10.0, 14.0])
    return np.stack([np.repeat(v, 4), np.tile(v, 4)], 1)


def shift(h, w, stride=16):
    """anchor.py:20-42: the 16 anchors on every cell, cells column by column."""
    col, row = np.divmod(np.arange(h * w), h)
    cells = np.stack([row, col], 1) * stride
    return (cells[:, None, :] + generate_anchors()[None]).reshape(-1, 2)


def vote(heads, A=16, P=15):
    """post_process.forward (anchor.py:57-82) in float64 -> [B, P, 3] (y, x, z)."""
    cls, reg, dep = heads
    B, _, h, w = cls.shape
    lay = lambda t, *tail: t.permute(0, 3, 2, 1).reshape(B, w * h * A, P, *tail)
    c, r, d = lay(cls), lay(reg, 2), lay(dep)
    wgt = torch.softmax(c, 1)
    anchors = torch.from_numpy(shift(h, w))
    yx = (wgt[..., None] * (anchors[None, :, None, :] + r)).sum(1)
    z = (wgt * d).sum(1)
    return torch.cat([yx, z[..., None]], -1).numpy()


def state_dict():
    g = np.load(GOLDEN)
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(g["shapes"], g["ndim"])]
    return AC.state_dict_for_seed(int(g["seed"]), [str(k) for k in g["keys"]], shapes)


def deviation(size, sd=None):
    """size "s" or "l" -> (pixels, z): max |emulated joints - golden fp64 joints|."""
    H, W, B = AC.SMALL if size == "s" else AC.LARGE
    sd = state_dict() if sd is None else sd
    with torch.no_grad():
        joints = vote(forward(sd, AC.net_input(AC.SEED + H, B, H, W)))
    d = np.abs(joints - np.load(GOLDEN)["%s_joints" % size])
    return float(d[..., :2].max()), float(d[..., 2].max())


if __name__ == "__main__":
    sd = state_dict()
    for size in sys.argv[1:] or ("s", "l"):
        px, z = deviation(size, sd)
        print('"%s": (%.6g, %.6g),' % (size, px, z), flush=True)
