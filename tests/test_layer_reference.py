"""The per-layer checker's own sensitivity (CPU): tests/layer_reference.py must accept an independent fp32 emulation
of a layer (torch float32 convolution of the same bf16-valued operands, the fp32 epilogue, then the store rounding)
and reject each of six injected faults of the kind a tiled kernel makes, at the network's real K values."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_reference as LR  # noqa: E402

H, W, COUT = 13, 62, 48          # 30-column strips (boundaries at columns 30, 60), a ragged last 4-row tile (row 12)
LAYERS = {                        # name: (input channels read, ks, cin_map or None)
    "k64x9": (64, 3, None), "k128x9": (128, 3, None), "k256x9": (256, 3, None),
    "map205": (256, 3, "map"), "k128x1": (128, 1, None), "k256x1": (256, 1, None),
}
FAULTS = ["tap_dropped_on_strip_edge_column", "last_row_tile_shifted", "input_channels_swapped", "residual_missing_on_row",
          "leaky_slope", "bias_from_neighbour"]


def _layer(name, prec, seed=0):
    cin, ks, cmap = LAYERS[name]
    g = torch.Generator().manual_seed(seed)
    if cmap:                                                   # the stage-2 layout: 205 reference channels spread over 256, pads = -1
        cmap = [-1] * cin
        slots = torch.randperm(cin, generator=g)[:205].sort().values.tolist()
        for ref, slot in enumerate(torch.randperm(205, generator=g).tolist()):
            cmap[slots[ref]] = slot
        cin_ref = 205
    else:
        cin_ref = cin
    K = cin_ref * ks * ks
    sd = {"c.weight": torch.randn(COUT, cin_ref, ks, ks, generator=g) / K ** 0.5,
          "bn.weight": torch.rand(COUT, generator=g) + 0.5, "bn.bias": torch.randn(COUT, generator=g) * 0.3,
          "bn.running_mean": torch.randn(COUT, generator=g) * 0.3, "bn.running_var": torch.rand(COUT, generator=g) * 1.5 + 0.5}
    spec = {"w": "c", "bn": "bn", "ks": ks, "stride": 1, "act": LR.ACT_LEAKY, "cin_map": cmap or [], "cout": COUT}
    x = F.leaky_relu(torch.randn(1, cin, H, W, generator=g), 0.1).to(torch.float64)
    res = torch.randn(1, COUT, H, W, generator=g).to(torch.float64)
    if prec == "bf16":
        x, res = LR.rne_bf16(x), LR.rne_bf16(res)
        xin = LR.Act(x)
    else:
        hi = LR.rne_bf16(x)
        xin = LR.Act(hi + LR.rne_bf16(LR.f32(x - hi)), hi)
        rh = LR.rne_bf16(res)
        res = rh + LR.rne_bf16(LR.f32(res - rh))
    return spec, sd, xin, res


def _emulate(spec, sd, xin, res, prec, fault=None):
    """The kernel's operation in float32 (a different summation order from the fp64 reference), optionally faulty."""
    cin = xin.v.shape[1]
    Ws, bias, _ = LR.conv_weights(sd, spec, prec, cin)
    ks = spec["ks"]
    if fault == "input_channels_swapped":
        used = [i for i, m in enumerate(spec["cin_map"] or range(cin)) if m >= 0]
        perm = list(range(cin))
        perm[used[3]], perm[used[4]] = used[4], used[3]
        xin = LR.Act(xin.v[:, perm], None if xin.hi is None else xin.hi[:, perm])
    hi = xin.hi if xin.hi is not None else xin.v
    planes = [(xin.v.float(), Ws[0].float())] if prec == "bf16" else \
        [(hi.float(), Ws[0].float()), ((xin.v - hi).float(), Ws[0].float()), (hi.float(), Ws[1].float())]
    conv = lambda a, w: F.conv2d(a, w, padding=ks // 2)
    acc = sum(conv(a, w) for a, w in planes)
    if fault == "tap_dropped_on_strip_edge_column":          # one k-step (one tap x 32 channels) missing at column 30
        w = torch.zeros_like(planes[0][1])
        w[:, :32, 0, 0] = planes[0][1][:, :32, 0, 0]
        acc[..., 30] -= conv(planes[0][0], w)[..., 30]
    if fault == "last_row_tile_shifted":                      # the halo of the last 4-row tile read one row low
        shifted = [(torch.roll(a, 1, dims=2), w) for a, w in planes]
        acc[..., 12:, :] = sum(conv(a, w) for a, w in shifted)[..., 12:, :]
    b = bias.float().clone()
    if fault == "bias_from_neighbour":
        b[7] = b[8]
    v = acc + b.view(1, -1, 1, 1)
    r = res.float().clone()
    if fault == "residual_missing_on_row":
        r[..., 5, :] = 0
    v = v + r
    slope = np.float32(0.125 if fault == "leaky_slope" else 0.1)
    v = torch.where(v > 0, v, v * float(slope))
    out = LR.rne_bf16(v)
    if prec == "bf16x3":
        out = out + LR.rne_bf16(v - out.float())
    return out


def _check(name, prec, fault):
    spec, sd, xin, res = _layer(name, prec)
    Ws, bias, used = LR.conv_weights(sd, spec, prec, xin.v.shape[1])
    r, d = LR.conv_ref(xin, Ws, bias, used, spec["ks"], 1, spec["act"], res=res, x3_res=prec == "bf16x3")
    return LR.compare(_emulate(spec, sd, xin, res, prec, fault), r, LR.allowance(r, d, "x3" if prec == "bf16x3" else "bf16"))


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
@pytest.mark.parametrize("name", list(LAYERS))
def test_checker_accepts_an_fp32_emulation(name, prec):
    rep = _check(name, prec, None)
    assert rep["n_bad"] == 0, rep
    assert rep["worst"] > 0


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
@pytest.mark.parametrize("name", list(LAYERS))
def test_checker_rejects_injected_fault(name, prec, fault):
    rep = _check(name, prec, fault)
    assert rep["n_bad"] > 0, (name, prec, fault, rep["worst"])
    if fault == "tap_dropped_on_strip_edge_column":
        assert {w[3] for w in rep["where"]} == {30}, rep["where"]
    if fault == "residual_missing_on_row":
        assert {w[2] for w in rep["where"]} == {5}, rep["where"]


def test_allowance_orders_of_magnitude():
    """A regression guard on the bound's size at K = 2304: it is the worst case of any fp32 order of the K (bf16x3:
    3K) terms, about 1 % (bf16) and 3 % (bf16x3) of the value at the median -- loose against the arithmetic, yet
    every fault above stays out of it.  It must not grow."""
    for prec, hi in (("bf16", 2.0 ** -6), ("bf16x3", 2.0 ** -5)):
        spec, sd, xin, res = _layer("k256x9", prec)
        Ws, bias, used = LR.conv_weights(sd, spec, prec, 256)
        r, d = LR.conv_ref(xin, Ws, bias, used, 3, 1, spec["act"], res=res, x3_res=prec == "bf16x3")
        rel = float((LR.allowance(r, d, "x3" if prec == "bf16x3" else "bf16") / r.abs().clamp_min(1e-3)).median())
        assert rel < hi, (prec, rel)


def test_half_ulp_and_splits():
    a = torch.tensor([1.0, 1.5, 2.0 ** -10, 3.0, 0.0], dtype=torch.float64)
    assert LR.half_ulp(a, "bf16").tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -18, 2.0 ** -7, 0.0]
    assert LR.half_ulp(a, "fp32").tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -34, 2.0 ** -23, 0.0]
    assert LR.rne_bf16(torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8])).tolist() == [1.0, 1 + 2.0 ** -6]   # ties to even
