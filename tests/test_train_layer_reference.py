"""tests/train_layer_reference.py on the CPU (no GPU): the reference accepts a float32 emulation of each op of the planes training step evaluated
in two summation orders, and rejects injected faults, at the stage-level map sizes of every configuration of tests/test_gpu_train_layers.py
(28x28 at B = 32 -- reduced to 4 frames for the element-wise ops --, 13x17 at B = 1, 9x5 at B = 3) and at the ragged quarter-size maps for the pools; and at
the maps of the shape sweep (tests/train_plan_cases.py::SWEEP) that bring a summation chain those three do not have: one slice, one row per block, a single
partial reduction block (NEW_CHAINS).  The transcriptions of plan_wgrad / red_blocks live in tests/train_plan_cases.py.

Which check catches which fault (none may go uncaught):
  per-element allowance of test_gpu_train_layers.py: a shifted tap, a dropped halo row / column at an image edge (convolutions), the missing lo * hi
    term (convolutions at every shape; weight gradients at the two ragged shapes only, see below), a wrong channel of the stage-2 map, a pad channel given weight, biased instead of
    unbiased running variance, k2 / k3 divided by n - 1, the mask taken from the wrong tensor in one element (also counted by mask_disagreements), a
    missing * 4 in a head, the dextra slice of the wrong head, / (valid taps) instead of / 9 in the pool backward, a shifted tap of the weight gradient;
  (a row / column dropped per image or per column strip of a weight gradient is seen by the chain-depth allowance at every configured shape, the bench
    shape included: 1 of 112 of an element's products against an allowance of 3e-4 of their absolute sum;)
  exact integer probe (bit-for-bit): the same dropped rows / columns / seams, and what the allowance cannot see at the bench shape: a single dropped pixel
    (1 of 401 408 products; asserted below) -- on integer operands every fp32 summation order gives the same bits, so any missing product shows;
  NEITHER of the two at the bench shape: the missing lo * hi term of a weight gradient.  It is a 2^-9 relative, sign-random perturbation of each product, so
    it sinks inside the chain-depth allowance at every level of the bench shape (asserted below for 112 x 112 with the 64-channel plan and for 28 x 28 with the
    plan the 256-channel stage layers get: 0.06 and 0.3 of the allowance), and integer operands have no lo planes.  There this fault is caught only by the same
    kernel's per-element check at the two ragged configurations (asserted above) and by the whole step forced onto the engine's masks
    (test_gpu_train.py, 1e-4 per tensor: the fault moves the tensor by 1e-3, asserted below).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_reference as LR
import train_layer_reference as TL
import train_plan_cases as TP
from train_plan_cases import NUM_CUS, _red_chain, _wgrad_plan          # the transcriptions of red_blocks / plan_wgrad (moved there: one copy)

PRECS = ("bf16x3", "fp32")
STAGE_MAPS = [(name, B, H // 8, W // 8) for name, B, H, W in TL.SHAPES]
QUARTER_MAPS = [(name, B, H // 4, W // 4) for name, B, H, W in TL.SHAPES]


def _new_chains():
    """The sweep shapes (tests/train_plan_cases.py::SWEEP) whose stage maps bring a summation chain SHAPES does not have: the first with one slice
    (Sr == 1), with one row per block (rows_per_block == 1, Sr > 1) and with a single partial reduction block (nblk == 1, npix < ppb)."""
    want = {"Sr == 1": lambda w, r: w["Sr"] == 1, "rows_per_block == 1": lambda w, r: w["rows_per_block"] == 1 and w["Sr"] > 1,
            "nblk == 1": lambda w, r: r["nblk"] == 1 and r["npix"] < r["ppb"]}
    out = {}
    for name, B, H, W, _ in TP.SWEEP:
        w, r = TP.wgrad_plan(B, H // 8, W // 8, 64, 64, 3), TP.red_plan(B * (H // 8) * (W // 8), 128)
        for k, pred in want.items():
            if k not in out and name not in TP.FILTERED and pred(w, r):
                out[k] = (name, B, H, W)
    assert set(out) == set(want), sorted(set(want) - set(out))
    return sorted(set(out.values()))


NEW_CHAINS = _new_chains()
STAGE_MAPS_SWEEP = [(name, B, H // 8, W // 8) for name, B, H, W in NEW_CHAINS]
QUARTER_MAPS_SWEEP = [(name, B, H // 4, W // 4) for name, B, H, W in NEW_CHAINS]


def _r(shape, seed, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale + shift).to(torch.float64)


def _worst(got, r, a):
    return LR.compare(got.double().reshape(1, -1, 1, 1), r.reshape(1, -1, 1, 1), a.reshape(1, -1, 1, 1))["worst"]


def _f(t):
    return t.to(torch.float32)


def _stored(v32, prec):
    """what a planes tensor holds after storing the float32 value v32"""
    return TL.split_act(v32.double(), prec).v


# ---- convolutions ---------------------------------------------------------------------------------------
def _emu_conv(p, prec, w, bias, x, res, order, cat_map=None, drop_lo_hi=False, w_edit=None, edge=None):
    """float32 emulation of a convolution problem; order 1 permutes the k channels (another summation order)."""
    old = TL.CAT_MAP
    if cat_map is not None:
        TL.CAT_MAP = cat_map
    W, _ = TL.conv_weights(w, p, prec, x.v.shape[1])
    TL.CAT_MAP = old
    if w_edit is not None:
        W = [w_edit(a.clone()) for a in W]
    perm = torch.randperm(x.v.shape[1], generator=torch.Generator().manual_seed(5)) if order else torch.arange(x.v.shape[1])
    conv = lambda a, ww: F.conv2d(_f(a[:, perm]), _f(ww[:, perm]), padding=p["ks"] // 2)

    def full(xx):
        if prec == "bf16x3":
            hi = xx.hi
            y = conv(hi, W[0]) + conv(hi, W[1])
            return y if drop_lo_hi else y + conv(xx.v - hi, W[0])
        return conv(xx.v, W[0])
    y = full(x)
    if edge is not None:                     # the last output row / column computed without the input row / column next to it
        z = LR.Act(x.v.clone(), None if x.hi is None else x.hi.clone())
        for t in (z.v, z.hi):
            if t is not None:
                if edge == "row":
                    t[:, :, -2] = 0
                else:
                    t[:, :, :, -2] = 0
        yz = full(z)
        if edge == "row":
            y[:, :, -1] = yz[:, :, -1]
        else:
            y[:, :, :, -1] = yz[:, :, :, -1]
    if bias is not None:
        y = y + _f(bias).view(1, -1, 1, 1)
    if res is not None:
        y = y + _f(res.v)
    return _stored(y, prec)


def _conv_case(prec, B, h, w_, dgrad, seed):
    wt = _r((128, 187, 3, 3), seed, 0.05)
    if not dgrad:
        p = dict(dgrad=0, cat=1, rows=128, ks=3, act=0, bias=1)
        xv = _r((B, 192, h, w_), seed + 1)
        xv[:, 187:] = 0
        return p, wt, _r((128,), seed + 2), TL.split_act(xv, prec), None
    p = dict(dgrad=1, cat=1, rows=192, ks=3, act=0, bias=0)
    return p, wt, None, TL.split_act(_r((B, 128, h, w_), seed + 1), prec), TL.split_act(_r((B, 192, h, w_), seed + 3), prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", STAGE_MAPS, ids=[s[0] for s in STAGE_MAPS])
@pytest.mark.parametrize("dgrad", [0, 1])
def test_convolution_reference_accepts_fp32_orders_and_rejects_faults(shape, prec, dgrad):
    _, B, h, w_ = shape
    p, wt, bias, x, res = _conv_case(prec, min(B, 4), h, w_, dgrad, seed=11 + h)
    r, d = TL.conv_ref(p, prec, wt, bias, x, res)
    a = LR.allowance(r, d, TL.fmt_of(prec))
    for order in (0, 1):
        assert 0 < _worst(_emu_conv(p, prec, wt, bias, x, res, order), r, a) <= 1
    shifted = lambda W: torch.cat([torch.roll(W[:1], 1, 3), W[1:]], 0)          # the taps of output row 0 moved by one column
    faults = {"tap shifted": dict(w_edit=shifted), "halo row dropped": dict(edge="row"), "halo column dropped": dict(edge="col")}
    swapped = list(TL.CAT_MAP)
    swapped[128], swapped[156] = swapped[156], swapped[128]
    faults["wrong channel of the stage-2 map"] = dict(cat_map=swapped)
    padded = list(TL.CAT_MAP)
    padded[187] = 0
    if dgrad:
        faults["pad channel given weight"] = dict(cat_map=padded)
    if prec == "bf16x3":
        faults["lo * hi left out"] = dict(drop_lo_hi=True)
    for name, kw in faults.items():
        assert _worst(_emu_conv(p, prec, wt, bias, x, res, 0, **kw), r, a) > 1, name
    if not dgrad:                            # forward: a weight on a pad channel shows as soon as that channel is not zero -- the reference holds it at zero weight
        x.v[:, 187] = 1.0
        if x.hi is not None:
            x.hi[:, 187] = 1.0
        r, d = TL.conv_ref(p, prec, wt, bias, x, res)
        assert _worst(_emu_conv(p, prec, wt, bias, x, res, 0, cat_map=padded), r, LR.allowance(r, d, TL.fmt_of(prec))) > 1


# ---- BatchNorm ------------------------------------------------------------------------------------------
def _emu_bn_stats(x, gamma, beta, rm, rv, m, order, biased=False):
    """per-thread float32 chains of m pixels, the rest in double (order 1: the pixels in reverse)"""
    B, Cn = x.shape[:2]
    flat = _f(x).permute(1, 0, 2, 3).reshape(Cn, -1)
    if order:
        flat = flat.flip(1)
    n = flat.shape[1]
    pad = (-n) % m
    flat = F.pad(flat, (0, pad)).view(Cn, -1, m)
    s, ss = torch.zeros(Cn, flat.shape[1]), torch.zeros(Cn, flat.shape[1])
    for i in range(m):
        s = s + flat[:, :, i]
        ss = ss + flat[:, :, i] * flat[:, :, i]
    s, ss = s.double().sum(1), ss.double().sum(1)
    mean = s / n
    var = (ss / n - mean * mean).clamp_min(0)
    istd = 1 / torch.sqrt(var + TL.EPS)
    sc = gamma * istd
    unb = var if biased else var * n / (n - 1)
    out = dict(mean=mean, invstd=istd, scale=sc, shift=beta - mean * sc, running_mean=(1 - TL.MOMENTUM) * rm + TL.MOMENTUM * mean,
               running_var=(1 - TL.MOMENTUM) * rv + TL.MOMENTUM * unb)
    return {k: _f(v).double() for k, v in out.items()}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", STAGE_MAPS + STAGE_MAPS_SWEEP, ids=[s[0] for s in STAGE_MAPS + STAGE_MAPS_SWEEP])
def test_batchnorm_reference_accepts_fp32_orders_and_rejects_faults(shape, prec):
    _, B, h, w_ = shape
    Cn = 128
    p = _red_chain(B * h * w_, Cn)
    m = TL.chain(p)
    x = TL.split_act(_r((B, Cn, h, w_), 3 + h, 1.5, 0.3), prec).v
    gamma, beta, rm, rv = TL.f32(_r((Cn,), 4, 0.2, 1.0)), TL.f32(_r((Cn,), 5, 0.3)), TL.f32(_r((Cn,), 6, 0.1)), TL.f32(_r((Cn,), 7, 0.1, 1.0))
    ref = TL.bn_stats_ref(x, gamma, beta, rm, rv, m)
    for order in (0, 1):
        got = _emu_bn_stats(x, gamma, beta, rm, rv, m, order)
        for k, (r, a) in ref.items():
            assert _worst(got[k], r, a) <= 1, k
    got = _emu_bn_stats(x, gamma, beta, rm, rv, m, 0, biased=True)
    assert _worst(got["running_var"], *ref["running_var"]) > 1, "biased running variance"
    # apply, LeakyReLU with a residual
    sc, sf = _emu_bn_stats(x, gamma, beta, rm, rv, m, 0)["scale"], _emu_bn_stats(x, gamma, beta, rm, rv, m, 0)["shift"]
    xs, res = LR.Act(x[:4]), TL.split_act(_r((min(B, 4), Cn, h, w_), 9), prec)
    r, d = TL.bn_apply_ref(xs, sc, sf, res, 2)
    a = LR.allowance(r, d, TL.fmt_of(prec))
    y = _f(xs.v) * _f(sc).view(1, -1, 1, 1) + _f(sf).view(1, -1, 1, 1)
    for y32 in (y + _f(res.v), _f(res.v) + y):
        y32 = torch.where(y32 > 0, y32, y32 * np.float32(0.1))
        assert 0 < _worst(_stored(y32, prec), r, a) <= 1
    # backward
    dy = TL.split_act(_r((B, Cn, h, w_), 12, 1.0, 1.0) + 0.5 * (x - x.mean((0, 2, 3), keepdim=True)), prec).v
    got = _emu_bn_stats(x, gamma, beta, rm, rv, m, 0)
    mean, istd = got["mean"], got["invstd"]
    for act in (0, 1, 2):
        mask = (x * sc.view(1, -1, 1, 1) + sf.view(1, -1, 1, 1)) > 0
        sums = TL.bn_bwd_sums_ref(x, dy, mask, mean, istd, gamma, act, m)
        n = B * h * w_

        def emu(order, div=n, flip=None):
            mk = mask.clone()
            if flip is not None:
                mk.view(-1)[flip] = ~mk.view(-1)[flip]
            ga = _f(dy) if act == 0 else torch.where(mk, _f(dy), _f(dy) * np.float32(0.1 if act == 2 else 0.0))          # the apply kernel's g
            g = _f(dy) if act == 0 else torch.where(mask, _f(dy), _f(dy) * np.float32(0.1 if act == 2 else 0.0))         # the reduction's
            xh = (_f(x) - _f(mean).view(1, -1, 1, 1)) * _f(istd).view(1, -1, 1, 1)
            t = g * xh
            fl = lambda v: (v.permute(1, 0, 2, 3).reshape(Cn, -1).flip(1) if order else v.permute(1, 0, 2, 3).reshape(Cn, -1))
            cs = lambda v: F.pad(fl(v), (0, (-n) % m)).view(Cn, -1, m)
            s, sx = torch.zeros(Cn, cs(g).shape[1]), torch.zeros(Cn, cs(g).shape[1])
            for i in range(m):
                s, sx = s + cs(g)[:, :, i], sx + cs(t)[:, :, i]
            s, sx = s.double().sum(1), sx.double().sum(1)
            k1 = _f(gamma) * _f(istd)
            k2, k3 = _f(s / div), _f(sx / div)
            dx = k1.view(1, -1, 1, 1) * (ga - k2.view(1, -1, 1, 1) - xh * k3.view(1, -1, 1, 1))
            return dict(dbeta=_f(s).double(), dgamma=_f(sx).double(), k1=k1.double(), k2=k2.double(), k3=k3.double()), _stored(dx[:4], prec), _stored(ga[:4], prec)
        for order in (0, 1):
            vec, dx, g = emu(order)
            for k, (r, a) in sums.items():
                assert _worst(vec[k], r, a) <= 1, (act, k)
            r, d, gr, dg = TL.bn_bwd_apply_ref(x[:4], dy[:4], mask[:4], mean, istd, vec["k1"], vec["k2"], vec["k3"], act)
            assert 0 < _worst(dx, r, LR.allowance(r, d, TL.fmt_of(prec))) <= 1
            assert _worst(g, gr, LR.allowance(gr, dg, TL.fmt_of(prec))) <= 1
            assert TL.mask_disagreements(dx, x[:4], dy[:4], mask[:4], mean, istd, vec["k1"], vec["k2"], vec["k3"], act, TL.fmt_of(prec)) == 0
        vec, _, _ = emu(0, div=n - 1)
        assert _worst(vec["k2"], *sums["k2"]) > 1 and _worst(vec["k3"], *sums["k3"]) > 1, "k2 / k3 divided by n - 1"
        if act:
            good, _, _ = emu(0)
            _, dx, _ = emu(0, flip=777 % min(mask.numel(), 4 * Cn * h * w_))
            r, d, _, _ = TL.bn_bwd_apply_ref(x[:4], dy[:4], mask[:4], mean, istd, good["k1"], good["k2"], good["k3"], act)
            assert _worst(dx, r, LR.allowance(r, d, TL.fmt_of(prec))) > 1, "mask from the wrong tensor in one element"
            assert TL.mask_disagreements(dx, x[:4], dy[:4], mask[:4], mean, istd, good["k1"], good["k2"], good["k3"], act, TL.fmt_of(prec)) == 1


# ---- heads, pools, add ----------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", STAGE_MAPS + STAGE_MAPS_SWEEP, ids=[s[0] for s in STAGE_MAPS + STAGE_MAPS_SWEEP])
def test_heads_reference_accepts_fp32_and_rejects_faults(shape, prec):
    _, B, h, w_ = shape
    dcat = TL.split_act(_r((B, TL.CAT_PLANE, h, w_), 21, 1e-4), prec).v
    for b, (Cn, kind) in enumerate(zip(TL.HEAD_C, (1, 0, 1))):
        s = torch.sigmoid(_r((B, Cn, h, w_), 22 + b))
        o = TL.f32((s - 0.5) * 4 if kind else s)
        t, fg = TL.f32(_r((B, Cn, h, w_), 25 + b, 0.5)), ((_r((B, Cn, h, w_), 28) > 0.5).double() if b == 2 else None)
        de = dcat[:, TL.CAT_OFF[b]:TL.CAT_OFF[b] + Cn]
        r, d, loss, la = TL.heads_ref(o, t, fg, de, kind)
        a = LR.allowance(r, d, TL.fmt_of(prec))

        def emu(mul4=True, dextra=de, order=0):
            o32, t32 = _f(o), _f(t)
            s32 = o32 * np.float32(0.25) + np.float32(0.5) if kind else o32
            dd = o32 - t32
            w32 = (np.float32(0.1) + _f(fg) * np.float32(0.9)) if fg is not None else torch.ones_like(o32)
            e = (dd * dd * w32).double()
            g = np.float32(2.0) * dd * w32 * np.float32(1.0 / o.numel()) + _f(dextra)
            if kind and mul4:
                g = g * np.float32(4.0)
            dv = g * (np.float32(1.0) - s32) * s32 if not order else (s32 * (np.float32(1.0) - s32)) * g
            return _stored(dv, prec), _f((e.flatten().flip(0) if order else e.flatten()).sum() / o.numel()).double()
        for order in (0, 1):
            dv, ls = emu(order=order)
            assert 0 < _worst(dv, r, a) <= 1 and _worst(ls.view(1), loss.view(1), la.view(1)) <= 1
        if kind:
            assert _worst(emu(mul4=False)[0], r, a) > 1, "missing * 4"
        off = TL.CAT_OFF[(b + 1) % 3]
        assert _worst(emu(dextra=dcat[:, off:off + Cn])[0], r, a) > 1, "dextra slice of the wrong head"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", QUARTER_MAPS + STAGE_MAPS + QUARTER_MAPS_SWEEP, ids=["quarter_" + s[0] for s in QUARTER_MAPS] + ["stage_" + s[0] for s in STAGE_MAPS] + ["quarter_" + s[0] for s in QUARTER_MAPS_SWEEP])
def test_pool_and_add_references_accept_fp32_and_reject_faults(shape, prec):
    _, B, H, W = shape
    B = min(B, 2)
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = TL.split_act(_r((B, 8, ho, wo), 31, 1.0, 0.5), prec).v
    r, d = TL.pool_bwd_ref(dy, H, W)
    a = LR.allowance(r, d, TL.fmt_of(prec))

    def autograd(include_pad):
        x = torch.zeros((B, 8, H, W), dtype=torch.float32, requires_grad=True)
        F.avg_pool2d(x, 3, 2, 1, count_include_pad=include_pad).backward(_f(dy))
        return x.grad
    wt = torch.ones((8, 1, 3, 3))
    second = F.conv_transpose2d(_f(dy), wt, stride=2, padding=1, output_padding=(H - (2 * ho - 1), W - (2 * wo - 1)), groups=8) / np.float32(9.0)
    assert 0 < _worst(_stored(autograd(True), prec), r, a) <= 1 and 0 < _worst(_stored(second, prec), r, a) <= 1
    assert _worst(_stored(autograd(False), prec), r, a) > 1, "/ (valid taps) instead of / 9"
    ins = [TL.split_act(_r((B, 8, H, W), 40 + i), prec).v for i in range(4)]
    r, d = TL.add_ref(ins)
    a = LR.allowance(r, d, TL.fmt_of(prec))
    assert _worst(_stored(((_f(ins[0]) + _f(ins[1])) + _f(ins[2])) + _f(ins[3]), prec), r, a) <= 1
    assert _worst(_stored((_f(ins[3]) + _f(ins[2])) + (_f(ins[1]) + _f(ins[0])), prec), r, a) <= 1
    assert _worst(_stored((_f(ins[0]) + _f(ins[1])) + _f(ins[2]), prec), r, a) > 1, "an input left out"


# ---- weight gradient ------------------------------------------------------------------------------------
def _emu_wgrad(op, prec, x, dy, order, drop=None, lo_hi=True, shift_tap=False):
    """Blocks of rows_per_block rows of the flattened (image, column strip, row) space summed in float32, then the slices in float32 (order 1:
    slices in reverse).  drop: ("row" | "col" | "seam", ...) leaves out the x halo row below each image's last row pair / the x column right of the
    last column / the x column across the column-strip seam, as a kernel that does not fetch it would.  The plan mutants of tests/test_train_plan_cases.py:
    "strip_col" leaves out dy column Wt - 1 of every full-width strip, "reprime" the first row of a segment a block enters after a column seam, "last_block"
    the short last block, "last_slice" slice Sr - 1."""
    cout, cin, ks, Wt, tiles_x, rpb = op["cout"], op["cin"], op["ks"], op["Wt"], op["tiles_x"], op["rows_per_block"]
    B, _, H, W = dy.v.shape
    pad = ks // 2
    sel = [TL.CAT_MAP.index(c) for c in range(cin)] if op["cat"] else list(range(cin))
    parts = [(dy.v[:, :cout], x.v[:, sel])] if prec != "bf16x3" else \
        [(dy.hi[:, :cout], x.hi[:, sel]), (dy.hi[:, :cout], (x.v - x.hi)[:, sel])] + ([((dy.v - dy.hi)[:, :cout], x.hi[:, sel])] if lo_hi else [])
    rows = [(b, t, y) for b in range(B) for t in range(tiles_x) for y in range(H)]
    slices = []
    for s0 in range(0, len(rows), rpb):
        acc = torch.zeros((cout, cin, ks, ks), dtype=torch.float32)
        for i, (b, t, y) in enumerate(rows[s0:s0 + rpb]):
            x0, x1 = t * Wt, min(W, (t + 1) * Wt)
            if drop == "reprime" and i > 0 and y == 0:
                continue
            for d_, x_ in parts:
                drow = _f(d_[b, :, y, x0:x1]).clone()                                     # [cout, px]
                if drop == "strip_col" and x1 - x0 == 32 - 2 * pad:
                    drow[:, -1] = 0
                for ky in range(ks):
                    yy = y + ky - pad
                    if not 0 <= yy < H or (drop == "row" and y == H - 2 and yy == H - 1):
                        continue
                    for kx in range(ks):
                        lo, hi_ = x0 + kx - pad, x1 + kx - pad
                        xs = torch.zeros((cin, x1 - x0), dtype=torch.float32)
                        a0, a1 = max(lo, 0), min(hi_, W)
                        seg = _f(x_[b, :, yy, a0:a1]).clone()
                        if drop == "col" and a1 == W and kx == 2 * pad and pad:
                            seg[:, -1] = 0
                        if drop == "seam" and t + 1 < tiles_x and hi_ > x1 and pad:
                            seg[:, x1 - a0:] = 0
                        xs[:, a0 - lo:a1 - lo] = seg
                        acc[:, :, ky, (kx + 1) % ks if shift_tap else kx] += drow @ xs.t()
        slices.append(acc)
    if (drop == "last_block" and len(rows) % rpb) or drop == "last_slice":
        slices[-1] = torch.zeros_like(slices[-1])
    if order:
        slices = slices[::-1]
    tot = torch.zeros_like(slices[0])
    for s in slices:
        tot = tot + s
    return tot.double()


def _wgrad_case(prec, B, h, w_, seed, integer=False, channels=64, planned=64):
    op = dict(cout=channels, cin=channels, ks=3, cat=0, **_wgrad_plan(B, h, w_, planned, planned, 3))
    if integer:
        return op, TL.split_act(TL.integer_operand((B, channels, h, w_), seed), prec), TL.split_act(TL.integer_operand((B, channels, h, w_), seed + 1), prec)
    return op, TL.split_act(_r((B, channels, h, w_), seed).clamp_min(0), prec), TL.split_act(_r((B, channels, h, w_), seed + 1), prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", STAGE_MAPS[1:] + [("wide", 1, 6, 40)], ids=[s[0] for s in STAGE_MAPS[1:]] + ["two_column_strips"])
def test_weight_gradient_reference_accepts_fp32_orders_and_rejects_faults(shape, prec):
    _, B, h, w_ = shape
    op, x, dy = _wgrad_case(prec, B, h, w_, 51)
    r, a = TL.wgrad_ref(op, prec, x, dy)
    for order in (0, 1):
        assert 0 < _worst(_emu_wgrad(op, prec, x, dy, order), r, a) <= 1
    faults = {"tap shifted": dict(shift_tap=True), "halo row dropped at the image edge": dict(drop="row"), "halo column dropped at the image edge": dict(drop="col")}
    if op["tiles_x"] > 1:
        faults["halo column dropped at a column-strip seam"] = dict(drop="seam")
    if prec == "bf16x3":
        faults["lo * hi left out"] = dict(lo_hi=False)
    for name, kw in faults.items():
        assert _worst(_emu_wgrad(op, prec, x, dy, 0, **kw), r, a) > 1, name
    # the integer probe sees the same faults bit for bit
    op, x, dy = _wgrad_case(prec, B, h, w_, 61, integer=True)
    exact = TL._cw(dy.v, x.v, 3)
    assert torch.equal(_emu_wgrad(op, prec, x, dy, 0), exact) and torch.equal(_emu_wgrad(op, prec, x, dy, 1), exact)
    for name, kw in faults.items():
        if name != "lo * hi left out":
            assert not torch.equal(_emu_wgrad(op, prec, x, dy, 0, **kw), exact), name


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", STAGE_MAPS_SWEEP, ids=[s[0] for s in STAGE_MAPS_SWEEP])
def test_weight_gradient_allowance_at_the_sweeps_new_chain_lengths(shape, prec):
    """One slice (Sr == 1: the reduce kernel adds nothing, depth = Wt (3 | 1) + 1 + 16) and one row per block (rows_per_block == 1) on one-row stage maps:
    both summation orders pass, a shifted tap and (bf16x3) the missing lo * hi term do not.  (A one-row map has no halo row or column to drop.)"""
    _, B, h, w_ = shape
    op, x, dy = _wgrad_case(prec, B, h, w_, 53)
    assert op["rows_per_block"] == 1 and TL.wgrad_depth(op, prec) == op["Wt"] * (3 if prec == "bf16x3" else 1) + 1 + 16
    r, a = TL.wgrad_ref(op, prec, x, dy)
    for order in (0, 1):
        assert 0 < _worst(_emu_wgrad(op, prec, x, dy, order), r, a) <= 1
    assert _worst(_emu_wgrad(op, prec, x, dy, 0, shift_tap=True), r, a) > 1
    if prec == "bf16x3":
        assert _worst(_emu_wgrad(op, prec, x, dy, 0, lo_hi=False), r, a) > 1


def test_at_the_bench_shape_a_dropped_row_is_seen_by_the_allowance_and_a_single_dropped_pixel_needs_the_integer_probe():
    """B = 32, 112 x 112 (the first level of the bench shape; 8 of the 64 channels, planned as the 64 -> 64 layer).  One halo row dropped per image (1 of 112
    of the products of an element) is outside the chain-depth allowance.  ONE pixel of one image (1 of 401 408) is inside it -- that is what the integer probe
    is for: on integer operands every fp32 summation order gives the same bits, so a single missing product shows.  The missing dy_lo x_hi term is inside it too
    (and invisible to integers, whose lo planes are zero): it moves the tensor by 1e-3, which the mask-forced whole step's 1e-4 bar sees."""
    prec, (B, h, w_) = "bf16x3", (32, 112, 112)
    op, x, dy = _wgrad_case(prec, B, h, w_, 71, channels=8)
    r, a = TL.wgrad_ref(op, prec, x, dy)
    full = TL._cw(dy.v, x.hi, 3) + TL._cw(dy.hi, x.v - x.hi, 3)
    assert torch.allclose(full, r, rtol=0, atol=1e-9)

    def row_term(d, xx):                     # the products of output row h - 2 with x row h - 1 (tap row ky = 2): [co, ci, kx]
        xp = F.pad(xx[:, :, h - 1], (1, 1))
        return torch.stack([torch.einsum("bow,biw->oi", d[:, :, h - 2], xp[:, :, kx:kx + w_]) for kx in range(3)], -1)

    def pixel_term(d, xx, b=B - 1, y=h - 1, xc=w_ - 1):          # every product of dy[b, :, y, xc]: [co, ci, ky, kx]
        xp = F.pad(xx[b], (1, 1, 1, 1))
        return torch.einsum("o,ikl->oikl", d[b, :, y, xc], xp[:, y:y + 3, xc:xc + 3])
    dropped = full.clone()
    dropped[:, :, 2] -= row_term(dy.v, x.hi)
    assert _worst(dropped, r, a) > 1
    no_lo_hi = TL._cw(dy.hi, x.hi, 3) + TL._cw(dy.hi, x.v - x.hi, 3)
    assert _worst(no_lo_hi, r, a) <= 1                                                # a 2^-9 relative, sign-random perturbation of each product: inside
    assert float((no_lo_hi - r).norm() / r.norm()) > 1e-4                             # ... and past the 1e-4 bar of the mask-forced whole step
    one = full - pixel_term(dy.v, x.hi)
    assert float((one - full).abs().max()) > 0 and _worst(one, r, a) <= 1          # inside the allowance
    op, xi, dyi = _wgrad_case(prec, B, h, w_, 81, integer=True, channels=8)
    exact = TL._cw(dyi.v, xi.v, 3)
    assert float(exact.abs().max()) < 2 ** 24
    assert not torch.equal(exact - pixel_term(dyi.v, xi.v), exact)                    # bit for bit: seen
    assert not torch.equal(exact[:, :, 2] - row_term(dyi.v, xi.v), exact[:, :, 2])


def test_at_the_bench_shape_stage_level_a_missing_lo_hi_term_is_left_to_the_other_configurations_and_the_forced_step():
    """B = 32, 28 x 28, planned as a 256 -> 256 stage layer (rows_per_block 56, Sr 16: depth 4 721; 8 of the channels): the missing dy_lo x_hi term is inside
    the allowance and moves the tensor by more than the 1e-4 bar of the mask-forced whole step."""
    op, x, dy = _wgrad_case("bf16x3", 32, 28, 28, 91, channels=8, planned=256)
    assert (op["rows_per_block"], op["Sr"]) == (56, 16)
    r, a = TL.wgrad_ref(op, "bf16x3", x, dy)
    no_lo_hi = TL._cw(dy.hi, x.hi, 3) + TL._cw(dy.hi, x.v - x.hi, 3)
    assert 0 < _worst(no_lo_hi, r, a) <= 1
    assert float((no_lo_hi - r).norm() / r.norm()) > 1e-4


# ---- integer probes: a condition on the inputs ----------------------------------------------------------
@pytest.mark.parametrize("shape", TL.SHAPES + NEW_CHAINS, ids=[s[0] for s in TL.SHAPES + NEW_CHAINS])
def test_integer_probe_operands_are_exact_at_every_configured_shape(shape):
    _, B, H, W = shape
    conv_max, wgrad_max = TL.integer_limits(B, H, W)
    assert conv_max < 2 ** 16 and wgrad_max < 2 ** 24
    v = torch.arange(-70000, 70001, dtype=torch.float64)
    assert torch.equal(TL.split_act(v, "bf16x3").v[torch.abs(v) <= 2 ** 16], v[torch.abs(v) <= 2 ** 16])          # exact as hi + lo planes
    assert torch.equal(TL.split_act(v, "fp32").v, v)
    h, w_ = H // 8, W // 8
    x, wt, dy = TL.integer_operand((min(B, 2), 256, h, w_), 1), TL.integer_operand((256, 256, 3, 3), 2), TL.integer_operand((min(B, 2), 256, h, w_), 3)
    y = F.conv2d(x, wt, padding=1)
    dx = torch.nn.grad.conv2d_input(x.shape, wt, dy, padding=1)
    dw = torch.nn.grad.conv2d_weight(x, wt.shape, dy, padding=1)
    for t, lim in ((y, conv_max), (dx, conv_max), (dw, wgrad_max)):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= lim
    assert float(TL.split_act(x, "bf16x3").v.sub(x).abs().max()) == 0 and float((TL.split_act(x, "bf16x3").v - TL.split_act(x, "bf16x3").hi).abs().max()) == 0
