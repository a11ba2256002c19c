"""CPU: the checker of tests/test_gpu_train_nchw_layers.py checks what it claims to.

For every primitive, an fp32 (and split-bf16) emulation of the kernel's operation, summed in a shuffled order, must be ACCEPTED by the fp64
reference and allowance of tests/nchw_layer_reference.py at the shapes the GPU tests use, and the same emulation with one fault injected must
be REJECTED: a missing tap, the halo row / column off by one under stride 2, pad off by one, the last ragged channel dropped, the bias added
twice under accumulate, an unflipped data-gradient weight, a missing lo * hi term, BatchNorm's n for n - 1 in the running variance, the mask
taken from the wrong tensor, the average pool divided by the valid-tap count, the max-pool tie going to the last maximum, Nesterov without the
momentum look-ahead.  Also: the plan description's labels for the GPU table, so a planner change shows here, without a GPU, first.

Shapes at which a fault is invisible (by construction, not by tolerance): "halo off by one under stride 2" needs stride 2 and is injected at
the stride-2 rows only; "missing lo * hi" needs a split kernel, i.e. bf16x3 rows with Cin >= 32 (and in the weight gradient Cin >= 16); "pad off
by one" is invisible to a 1x1 convolution with pad 0 only if the shift keeps every pixel in range -- it is injected at the 3x3 rows; "last
ragged channel dropped" is injected at rows whose channel count is not a multiple of 16 / 64 but would show at any row; the average pool's
valid-tap division changes border outputs only (every map has them); the max-pool tie needs equal values in a window (the coarse 0.5-step
operands of the GPU test); a missing bottom-left tap is invisible on the one-column map 106 x 1 (it reads padding only): the bottom-centre tap
is removed there.  The convolution shapes are the table rows of the GPU test, which hold the replayed steps' critical layers (YoloPoseNet's
layer2.0 3x3 and 1x1 at stride 2 on 3 x 64 x 24 x 32, the 128 -> 100 head on 6 x 8, the 7x7 stem, a 56-column three-image map); the BatchNorm shapes are
those of its BatchNorm test and of the stem's maps.  The heavy table rows (Cout / Cin >= 832) are left to the GPU run: their faults are those of the light rows of the
same kernels."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nchw_layer_reference as NR
import test_gpu_train_nchw_layers as GT
import yolo_reference as yr

LIGHT = [r for r in GT.ROWS if r[0][1] * r[0][4] <= 128 * 128]
IDS = [i for r, i in zip(GT.ROWS, GT.ROW_IDS) if r in LIGHT]
ENV = ("POPNET_TRAIN_X3_WIDE", "POPNET_TRAIN_WGRAD_NOVEC")


def _env(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _ok(got, r, a):
    return NR.compare(GT._4d(got.double()), GT._4d(r), GT._4d(a))


def _perm(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))


def _bf(t):
    hi = t.to(torch.bfloat16).float()
    return hi, (t - hi).to(torch.bfloat16).float()


# ---- fp32 emulations (channel order shuffled: another summation order) -------------------------------------------
def emu_fwd(o, stride, pad, x3, bias, prev, fault=None):
    x, w = o["x"], o["w"]
    if fault == "tap":
        w = w.clone()
        w[:, :, -1, 0 if x.shape[3] > 1 else w.shape[3] // 2] = 0
    if fault == "channel":
        w = w.clone()
        w[:, -1] = 0
    pm = _perm(x.shape[1], 5)
    x, w = x[:, pm], w[:, pm]
    if fault == "halo":                                        # the strided gather starts one row and column late
        x = F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:]
    conv = lambda a, b: F.conv2d(a, b, stride=stride, padding=pad)           # noqa: E731
    if fault == "pad":
        conv = lambda a, b: F.conv2d(F.pad(a, (pad + 1, max(pad - 1, 0), pad + 1, max(pad - 1, 0))), b, stride=stride)[:, :, :o["y0"].shape[2], :o["y0"].shape[3]]   # noqa: E731
    if x3:
        (xh, xl), (wh, wl) = _bf(x), _bf(w)
        y = conv(xh, wh) + conv(xh, wl)
        if fault != "lohi":
            y = y + conv(xl, wh)
    else:
        y = conv(x, w)
    if bias:
        y = y + o["b"].view(1, -1, 1, 1) * (2 if fault == "bias2" else 1)
    if prev:
        y = y + o["y0"]
    return y


def emu_dgrad(o, stride, pad, x3, prev, fault=None):
    dy, w = o["dy"], o["w"]
    if fault == "unflipped":
        w = w.flip(2, 3)
    if fault == "channel":
        w = w.clone()
        w[-1] = 0
    pm = _perm(dy.shape[1], 6)
    dy, w = dy[:, pm], w[pm]
    H, W = o["x"].shape[2:]
    k = w.shape[2]
    op = (H + 2 * pad - k - (dy.shape[2] - 1) * stride, W + 2 * pad - k - (dy.shape[3] - 1) * stride)
    tr = lambda a, b: F.conv_transpose2d(a, b, stride=stride, padding=pad, output_padding=op)       # noqa: E731
    if x3:
        (dh, dl), (wh, wl) = _bf(dy), _bf(w)
        dx = tr(dh, wh) + tr(dh, wl)
        if fault != "lohi":
            dx = dx + tr(dl, wh)
    else:
        dx = tr(dy, w)
    if fault == "halo":
        dx = F.pad(dx, (0, 1, 0, 1))[:, :, 1:, 1:]
    return dx + o["dx0"] if prev else dx


def emu_wgrad(o, ks, stride, pad, x3, fault=None):
    x, dy = o["x"], o["dy"]
    if fault == "halo":
        x = F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:]
    if fault == "pad":
        x = F.pad(x, (1, 0, 1, 0))[:, :, :-1, :-1]
    cw = lambda a, b: NR._cw(a, b, ks, stride, pad)          # noqa: E731  (float32 in, float32 sums)
    if x3:
        (xh, xl), (dh, dl) = _bf(x), _bf(dy)
        dw = cw(dh, xh) + cw(dh, xl)
        if fault != "lohi":
            dw = dw + cw(dl, xh)
    else:
        dw = cw(dy, x)
    if fault == "tap":
        dw = dw.clone()
        dw[:, :, 0, -1] = 0
    if fault == "channel":
        dw = dw.clone()
        dw[:, -1] = 0
    return dw


# ---- the table's plan labels, without a GPU -------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_plan_description_gives_the_labels_the_gpu_table_expects(monkeypatch, prec):
    h = NR.plan_context(prec == "bf16x3")
    seen = set()
    for row in GT.ROWS:
        _env(monkeypatch, row[1])
        plans = GT._row_labels(h, row[0], row[4])
        assert {k: p["kernel"] for k, p in plans.items()} == GT._expected(row, prec), row[0]
        seen |= {p["kernel"] for p in plans.values()}
        for p in plans.values():
            tiled = p["kernel"].startswith("tconv3_")
            assert (p["TW"] > 0 and p["R"] > 0 and p["tiles_x"] * p["tiles_y"] > 0) == tiled, p
            assert p["x3"] == (prec == "bf16x3") and all(g >= 1 for g in p["grid"])
        if "wgrad" in plans:
            p = plans["wgrad"]
            N, Cin, H, W, Cout, ks, stride, pad = row[0]
            P = N * p["Ho"] * p["Wo"]
            per = p["per_slice"] * (p["R"] * p["TW"] if p["per_slice_unit"] == "tiles" else 1)
            assert p["slices"] >= 1 and p["slices"] * per >= P > (p["slices"] - 1) * per * (0 if p["per_slice_unit"] == "tiles" else 1), p      # the slices cover every pixel
            assert p["t_slices"] == NR.reduce_slices(h, N, Cout, p["Ho"] * p["Wo"]) >= 1
    # (in bf16x3 the fp32 tile weight gradient cannot be reached: t_tile_geometry_wx3 refuses no shape)
    every = {GT.T, GT.F1, GT.F3, GT.F7, GT.G1, GT.G3, GT.G7, GT.S1, GT.S3} | ({GT.X, GT.XW, GT.W3, GT.WPP, GT.WV} if prec == "bf16x3" else {GT.WT})
    assert every <= seen, sorted(every - seen)


def test_plan_description_rejects_bad_arguments():
    from popnet_amd import _lib
    import ctypes as C
    L, h = _lib.lib(), NR.plan_context(False)
    buf = C.create_string_buffer(1024)
    ok = (2, 16, 9, 7, 16, 3, 1, 1)
    assert L.pn_train_conv_plan_info(h, 0, *ok, buf, 1024) == 0
    assert L.pn_train_conv_plan_info(h, 0, *ok, buf, 8) == GT.PN_ERR_INVALID                    # cap too small
    assert L.pn_train_conv_plan_info(h, 4, *ok, buf, 1024) == GT.PN_ERR_INVALID
    assert L.pn_train_conv_plan_info(h, 0, 2, 16, 9, 7, 16, 5, 1, 1, buf, 1024) == GT.PN_ERR_INVALID      # kernel size
    assert L.pn_train_conv_plan_info(h, 2, 2, 16, 9, 7, 16, 7, 2, 3, buf, 1024) == GT.PN_ERR_INVALID      # the strided data gradient takes 1 and 3
    assert L.pn_train_conv_plan_info(h, 0, 2, 16, 1, 1, 16, 3, 1, 0, buf, 1024) == GT.PN_ERR_INVALID      # empty output
    assert L.pn_train_conv_plan_info(None, 0, *ok, buf, 1024) == GT.PN_ERR_INVALID
    assert L.pn_train_reduce_slices(h, 0, 4, 4) == GT.PN_ERR_INVALID


# ---- convolutions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("row", LIGHT, ids=IDS)
def test_convolution_references_accept_emulations_and_reject_faults(monkeypatch, row, prec):
    shape, env, _, _, ops = row
    _env(monkeypatch, env)
    N, Cin, H, W, Cout, ks, stride, pad = shape
    h = NR.plan_context(prec == "bf16x3")
    plans = GT._row_labels(h, shape, ops)
    o = GT._operands(shape, False, sum(shape))
    d = {k: v.double() for k, v in o.items()}
    rejected = {}

    def judge(name, faults, emu, ref):
        r, a = ref
        rep = _ok(emu(None), r, a)
        assert rep["n_bad"] == 0 and 0 < rep["worst"] <= 1, (name, rep)
        for f in faults:
            rejected[(name, f)] = _ok(emu(f), r, a)["n_bad"] > 0

    if "forward" in plans:
        x3 = NR.is_x3(plans["forward"]["kernel"])
        faults = ["tap", "channel"] + (["halo"] if stride == 2 else []) + (["pad"] if ks == 3 else []) + (["lohi"] if x3 else [])
        judge("forward", faults, lambda f: emu_fwd(o, stride, pad, x3, True, False, f), NR.conv_fwd_ref(d["x"], d["w"], d["b"], None, stride, pad, x3))
        judge("forward +=", ["bias2"], lambda f: emu_fwd(o, stride, pad, x3, True, True, f), NR.conv_fwd_ref(d["x"], d["w"], d["b"], d["y0"], stride, pad, x3))
        judge("forward += (no bias)", [], lambda f: emu_fwd(o, stride, pad, x3, False, True, f), NR.conv_fwd_ref(d["x"], d["w"], None, d["y0"], stride, pad, x3))
    for which in ("dgrad", "dgrad_strided"):
        if which in plans:
            x3 = NR.is_x3(plans[which]["kernel"])
            faults = ["channel"] + (["unflipped"] if ks > 1 else []) + (["halo"] if stride == 2 else []) + (["lohi"] if x3 else [])
            for prev in (False, True):
                judge(which + (" +=" if prev else ""), faults if not prev else [], lambda f: emu_dgrad(o, stride, pad, x3, prev, f),
                      NR.conv_dgrad_ref(d["dy"], d["w"], d["dx0"] if prev else None, tuple(o["x"].shape), stride, pad, x3))
    if "wgrad" in plans:
        p = plans["wgrad"]
        x3 = NR.is_x3(p["kernel"])
        faults = ["channel"] + (["tap"] if ks > 1 else []) + (["halo"] if stride == 2 else []) + (["pad"] if ks == 3 else []) + (["lohi"] if x3 else [])
        judge("wgrad", faults, lambda f: emu_wgrad(o, ks, stride, pad, x3, f), NR.conv_wgrad_ref(d["x"], d["dy"], ks, stride, pad, p))
        r, a = NR.conv_dbias_ref(d["dy"])
        db = o["dy"].double().sum((0, 2, 3)).float()
        assert _ok(db, r, a)["n_bad"] == 0
        assert _ok((o["dy"][:, :, :-1].double().sum((0, 2, 3))).float(), r, a)["n_bad"] > 0          # the last row of dy left out
    missed = [k for k, v in rejected.items() if not v]
    assert not missed, missed


def test_integer_operands_are_exact_at_the_table_shapes():
    for row in LIGHT:
        N, Cin, H, W, Cout, ks, stride, pad = row[0]
        o = {k: v.double() for k, v in GT._operands(row[0], True, 3).items()}
        assert all(float(v.abs().max()) <= 3 and bool((v == v.round()).all()) for v in o.values())
        y, _ = NR.conv_fwd_ref(o["x"], o["w"], o["b"], o["y0"], stride, pad, True)
        y2, _ = NR.conv_fwd_ref(o["x"], o["w"], o["b"], o["y0"], stride, pad, False)
        assert torch.equal(y, y2) and float(y.abs().max()) < 2 ** 24               # lo planes are zero: the split reference is the plain one
        assert torch.equal(emu_fwd({k: v.float() for k, v in o.items()}, stride, pad, True, True, True).double(), y)
    conv_max, wgrad_max = NR.integer_limits(3, 112, 260)                          # the largest table map (56 x 130) at that function's H / 2, W / 2
    assert conv_max < 2 ** 16 and wgrad_max < 2 ** 24


# ---- BatchNorm --------------------------------------------------------------------------------------------------------
def _bn_emu(x, gamma, beta, res, rm, rv, act, fault=None):
    n = x.shape[0] * x.shape[2] * x.shape[3]
    xd = x.double()
    mean = xd.mean((0, 2, 3))
    var = ((xd * xd).mean((0, 2, 3)) - mean * mean).clamp_min(0)
    mu, istd = mean.float(), (1.0 / torch.sqrt(var + NR.EPS)).float()
    unb = var * (n / (n if fault == "n" else n - 1.0))
    rm2 = ((1 - NR.MOMENTUM) * rm.double() + NR.MOMENTUM * mean).float()
    rv2 = ((1 - NR.MOMENTUM) * rv.double() + NR.MOMENTUM * unb).float()
    v = lambda t: t.view(1, -1, 1, 1)          # noqa: E731
    y = ((x - v(mu)) * v(istd)) * v(gamma) + v(beta)
    if res is not None:
        y = y + res
    y = F.relu(y) if act == 1 else torch.where(y > 0, y, y * np.float32(0.1)) if act == 2 else y
    return mu, istd, rm2, rv2, y


def _bn_bwd_emu(x, dy, mask, mu, istd, gamma, act, prev):
    n = x.shape[0] * x.shape[2] * x.shape[3]
    v = lambda t: t.view(1, -1, 1, 1)          # noqa: E731
    g = dy if act == 0 else torch.where(mask, dy, dy * np.float32(0.1) if act == 2 else torch.zeros_like(dy))
    xm = x - v(mu)
    sg, sgx = g.double().sum((0, 2, 3)), (g.double() * xm.double()).sum((0, 2, 3))
    dbeta, dgamma = sg.float(), (sgx * istd.double()).float()
    inv = np.float32(1.0 / n)
    mg, k2 = dbeta * inv, sgx.float() * inv * istd * istd
    dx = (g - v(mg) - xm * v(k2)) * v(istd) * v(gamma)
    return dbeta, dgamma, dx, (g if prev is None else prev + g)


@pytest.mark.parametrize("N,Cc,H,W", [(3, 70, 13, 9), (3, 64, 48, 64)])
@pytest.mark.parametrize("act,with_res", [(0, False), (1, True), (2, False)])
def test_batchnorm_references_accept_emulations_and_reject_faults(N, Cc, H, W, act, with_res):
    g = torch.Generator().manual_seed(N + Cc + H + act)
    shape = (N, Cc, H, W)
    x = torch.randn(shape, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)
    res = torch.randn(shape, generator=g) if with_res else None
    rm, rv = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    dy, d0 = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    mu, istd, rm2, rv2, y = _bn_emu(x, gamma, beta, res, rm, rv, act)
    st = NR.bn_stats_ref(x.double(), rm.double(), rv.double())
    for k, got in (("mean", mu), ("invstd", istd), ("running_mean", rm2), ("running_var", rv2)):
        assert _ok(got, *st[k])["n_bad"] == 0, k
    assert _ok(_bn_emu(x, gamma, beta, res, rm, rv, act, fault="n")[3], *st["running_var"])["n_bad"] > 0          # n for n - 1
    ya = NR.bn_apply_ref(x.double(), mu.double(), istd.double(), gamma.double(), beta.double(), None if res is None else res.double(), act)
    rep = _ok(y, *ya)
    assert rep["n_bad"] == 0 and rep["worst"] > 0
    if with_res:
        assert _ok(_bn_emu(x, gamma, beta, None, rm, rv, act)[4], *ya)["n_bad"] > 0                                # the residual left out
    mask = y > 0
    for prev in (None, d0):
        dbeta, dgamma, dx, dres = _bn_bwd_emu(x, dy, mask, mu, istd, gamma, act, prev)
        args = (x.double(), dy.double(), mask, mu.double(), istd.double(), gamma.double(), act, dbeta.double())
        ref = NR.bn_bwd_ref(*args, dres_prev=None if prev is None else prev.double())
        for k, got in (("dbeta", dbeta), ("dgamma", dgamma), ("dx", dx), ("dres", dres)):
            assert _ok(got, *ref[k])["n_bad"] == 0, (k, _ok(got, *ref[k]))
        assert NR.mask_disagreements(dx.double(), *args) == 0
    if act:
        wrong = x > 0                                                        # the mask taken from the wrong tensor (x for out)
        assert int((wrong != mask).sum()) > 0
        dbeta, dgamma, dx, dres = _bn_bwd_emu(x, dy, wrong, mu, istd, gamma, act, None)
        args = (x.double(), dy.double(), mask, mu.double(), istd.double(), gamma.double(), act, dbeta.double())
        ref = NR.bn_bwd_ref(*args)
        assert all(_ok(got, *ref[k])["n_bad"] > 0 for k, got in (("dbeta", dbeta), ("dx", dx), ("dres", dres)))
        # one element on the other branch, the sums as they should be: counted as a mask disagreement
        good, _, dx1, _ = _bn_bwd_emu(x, dy, mask, mu, istd, gamma, act, None)
        slope = np.float32(0.1) if act == 2 else np.float32(0.0)
        e = dy[0, 0, 0, 0]
        ge, go = (e, e * slope) if bool(mask[0, 0, 0, 0]) else (e * slope, e)
        dx1 = dx1.clone()
        dx1[0, 0, 0, 0] += (go - ge) * istd[0] * gamma[0]
        assert NR.mask_disagreements(dx1.double(), x.double(), dy.double(), mask, mu.double(), istd.double(), gamma.double(), act, good.double()) == 1


# ---- pools, heads, copies, optimiser, loss ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(14, 10), (13, 9)])
def test_pool_references_accept_emulations_and_reject_faults(H, W):
    g = torch.Generator().manual_seed(H)
    x = torch.randn((2, 5, H, W), generator=g)
    r, a = NR.avgpool_fwd_ref(x.double())
    assert _ok(F.avg_pool2d(x, 3, 2, 1), r, a)["n_bad"] == 0
    assert _ok(F.avg_pool2d(x, 3, 2, 1, count_include_pad=False), r, a)["n_bad"] > 0                   # divided by the valid-tap count
    dy = torch.randn(r.shape, generator=g)
    xr = x.clone().requires_grad_()
    F.avg_pool2d(xr, 3, 2, 1).backward(dy)
    rb, ab = NR.avgpool_bwd_ref(dy.double(), H, W)
    assert _ok(xr.grad, rb, ab)["n_bad"] == 0
    xr.grad = None
    F.avg_pool2d(xr, 3, 2, 1, count_include_pad=False).backward(dy)
    assert _ok(xr.grad, rb, ab)["n_bad"] > 0
    # max pool: first maximum of a tie
    xm = torch.randint(-3, 4, x.shape, generator=g).float() * 0.5
    for k, st, pad in ((3, 2, 1), (2, 2, 0)):
        yr_, ir = NR.maxpool_fwd_ref(xm, k, st, pad)
        cols = F.unfold(xm, k, padding=pad, stride=st) if pad == 0 else F.unfold(F.pad(xm, (pad,) * 4, value=-float("inf")), k, stride=st)
        cols = cols.view(2, 5, k * k, -1)
        last = (k * k - 1) - cols.flip(2).argmax(2)                                                    # the LAST maximum of each window
        first = cols.argmax(2)
        assert int((last != first).sum()) > 0                                                          # ties exist: the rule matters
        Wo = ir.shape[3]
        oy, ox = torch.arange(ir.shape[2]).view(-1, 1).expand(ir.shape[2:]).reshape(-1), torch.arange(Wo).repeat(ir.shape[2])
        to_flat = lambda t: ((oy * st - pad + t // k) * W + (ox * st - pad + t % k)).view(ir.shape)    # noqa: E731
        assert torch.equal(to_flat(first), ir) and not torch.equal(to_flat(last), ir)
        dym = torch.randn(yr_.shape, generator=g)
        xg = xm.clone().requires_grad_()
        F.max_pool2d(xg, k, st, pad).backward(dym)
        rb, ab = NR.maxpool_bwd_ref(dym.double(), ir, H, W)
        assert _ok(xg.grad, rb, ab)["n_bad"] == 0
        rl, _ = NR.maxpool_bwd_ref(dym.double(), to_flat(last), H, W)
        assert _ok(rl.float(), rb, ab)["n_bad"] > 0


def test_head_copy_sgd_and_yolo_references_accept_emulations_and_reject_faults():
    g = torch.Generator().manual_seed(2)
    N, Cc, h, w = 2, 15, 6, 5
    for kind, weighted in ((1, True), (0, False)):
        v, t = torch.randn((N, Cc, h, w), generator=g) * 2, torch.randn((N, Cc, h, w), generator=g)
        fg = (torch.rand((N, Cc, h, w), generator=g) < 0.3).float() if weighted else None
        ex = torch.randn((N, Cc, h, w), generator=g)
        s = 1 / (1 + torch.exp(-v))
        o = (s - 0.5) * 4 if kind else s
        rs, as_, ro, ao = NR.head_fwd_ref(v.double(), kind)
        assert _ok(s, rs, as_)["n_bad"] == 0 and _ok(o, ro, ao)["n_bad"] == 0
        assert _ok((s - 0.5) * 2 if kind else s * 2, ro, ao)["n_bad"] > 0
        wt = (np.float32(0.1) + fg * np.float32(0.9)) if weighted else torch.ones_like(v)
        d = o - t
        loss = ((d * d * wt).double().sum() / v.numel()).float()
        rl, al = NR.head_loss_ref(o.double(), t.double(), None if fg is None else fg.double())
        assert _ok(loss, rl, al)["n_bad"] == 0
        assert _ok(((d * d).double().sum() / v.numel()).float(), rl, al)["n_bad"] > (0 if weighted else -1)          # the fg weight left out
        inv = np.float32(1.0 / v.numel())
        gr = (2 * d * wt * inv + ex) * (4 if kind else 1) * (1 - s) * s
        rb, ab = NR.heads_bwd_ref(s.double(), t.double(), None if fg is None else fg.double(), ex.double(), kind)
        rep = _ok(gr, rb, ab)
        assert rep["n_bad"] == 0 and rep["worst"] > 0
        assert _ok(2 * d * wt * inv * (4 if kind else 1) * (1 - s) * s, rb, ab)["n_bad"] > 0                           # dextra left out
    # slice copy
    src, d0 = torch.randn((2, 6, 3, 5), generator=g), torch.randn((2, 6, 3, 5), generator=g)
    assert _ok(src, *NR.slice_copy_ref(src.double(), None))["n_bad"] == 0 and _ok(src + d0, *NR.slice_copy_ref(src.double(), d0.double()))["n_bad"] == 0
    assert _ok(src, *NR.slice_copy_ref(src.double(), d0.double()))["n_bad"] > 0
    # Nesterov SGD
    p, gr, buf = torch.randn(1000, generator=g), torch.randn(1000, generator=g), torch.randn(1000, generator=g)
    for first, wd, gs in ((True, 0.0, 1.0), (False, 0.0, 1.0), (False, 1e-2, 0.5)):
        lr, mu = np.float32(0.7), np.float32(0.9)
        dd = gr * np.float32(gs) + (np.float32(wd) * p if wd else 0)
        b = dd if first else mu * buf + dd
        ref = NR.sgd_ref(p.double(), gr.double(), buf.double(), 0.7, 0.9, wd, first, gs)
        assert _ok(p - lr * (dd + mu * b), *ref["p"])["n_bad"] == 0 and _ok(b, *ref["buf"])["n_bad"] == 0
        assert _ok(p - lr * b, *ref["p"])["n_bad"] > 0                                                  # without the momentum look-ahead
    # YOLO loss: the per-element definition equals yolo_reference.loss_terms; an fp32 evaluation is accepted
    for weighted in (True, False):
        prior, conf, coord, weight = [torch.from_numpy(a) for a in yr.yolo_case_targets(seed=5, B=2, H=80, W=112)]
        v = torch.randn(prior.shape, generator=g) * 2
        ref = NR.yolo_loss_ref(v.double(), prior.double(), conf.double(), coord.double(), weight.double() if weighted else None, 2, 15)
        v64 = v.double().requires_grad_()
        sg = v64.view(2, 2, 50, 5, 7).sigmoid()
        o64 = torch.cat([(sg[:, :, :2] - 0.5) * 2, sg[:, :, 2:4] * 2, sg[:, :, 4:5], (sg[:, :, 5:] - 0.5) * 4], 2).view(v.shape)
        t64 = yr.loss_terms(o64, prior.double(), conf.double(), coord.double(), weight.double() if weighted else None)
        t64[0].backward()
        assert torch.allclose(ref["terms"][0], t64.detach(), rtol=1e-12, atol=0) and torch.allclose(ref["dv"][0], v64.grad, rtol=1e-10, atol=1e-18)
        assert torch.allclose(ref["out"][0], o64.detach(), rtol=1e-13, atol=1e-16)
        v32 = v.clone().requires_grad_()
        s32 = v32.view(2, 2, 50, 5, 7).sigmoid()
        o32 = torch.cat([(s32[:, :, :2] - 0.5) * 2, s32[:, :, 2:4] * 2, s32[:, :, 4:5], (s32[:, :, 5:] - 0.5) * 4], 2).view(v.shape)
        t32 = yr.loss_terms(o32.double(), prior.double(), conf.double(), coord.double(), weight.double() if weighted else None)
        t32[0].backward()
        assert _ok(o32.detach(), *ref["out"])["n_bad"] == 0 and _ok(t32.detach().float(), *ref["terms"])["n_bad"] == 0
        assert _ok(v32.grad, *ref["dv"])["n_bad"] == 0
        assert _ok(v32.grad * (1 + 1e-5), *ref["dv"])["n_bad"] > 0 and _ok((t32.detach() * (1 + 1e-5)).float(), *ref["terms"])["n_bad"] > 0


# ---- the dilated arms (pn_conv2d_forward_dil / _dgrad_dil / _wgrad_dil) ----------------------------------------------------------
# N, Cin, H, W, Cout, dil, pad.  The first two are shapes of tests/test_gpu_train_a2j.py's primitive test; in both pad = dil, so the data
# gradient's padding 2 dil - pad IS pad and "pad for 2 dil - pad" changes nothing there: that fault is injected at the third shape (pad 1, dil 2).
DIL = [(2, 5, 7, 9, 7, 2, 2), (1, 20, 9, 13, 70, 3, 3), (2, 8, 6, 5, 8, 2, 1)]


@pytest.mark.parametrize("shape", DIL, ids=["%dx%dx%dx%d_to_%d_d%dp%d" % s for s in DIL])
def test_dilated_references_equal_autograd_accept_fp32_and_reject_faults(shape):
    N, Cin, H, W, Cout, dil, pad = shape
    Ho, Wo = H + 2 * pad - 2 * dil, W + 2 * pad - 2 * dil
    g = torch.Generator().manual_seed(sum(shape))
    x, w, b = torch.randn((N, Cin, H, W), generator=g), torch.randn((Cout, Cin, 3, 3), generator=g) / np.sqrt(9.0 * Cin), torch.randn(Cout, generator=g)
    dy, y0, dx0 = torch.randn((N, Cout, Ho, Wo), generator=g), torch.randn((N, Cout, Ho, Wo), generator=g), torch.randn((N, Cin, H, W), generator=g)
    p = NR.dil_wgrad_plan(NR.plan_context(False), N, Cin, Ho, Wo, Cout)
    assert p["slices"] >= 1 and p["slices"] * p["per_slice"] >= N * Ho * Wo > (p["slices"] - 1) * p["per_slice"]
    # the references are torch autograd in fp64
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    y64 = F.conv2d(x64, w64, b.double(), padding=pad, dilation=dil)
    dx64, dw64 = torch.autograd.grad(y64, (x64, w64), dy.double())
    refs = {"forward": NR.conv_fwd_ref(x.double(), w.double(), b.double(), None, 1, pad, False, dilation=dil),
            "forward +=": NR.conv_fwd_ref(x.double(), w.double(), b.double(), y0.double(), 1, pad, False, dilation=dil),
            "dgrad": NR.conv_dgrad_ref(dy.double(), w.double(), None, tuple(x.shape), 1, pad, False, dilation=dil),
            "dgrad +=": NR.conv_dgrad_ref(dy.double(), w.double(), dx0.double(), tuple(x.shape), 1, pad, False, dilation=dil),
            "wgrad": NR.conv_wgrad_ref(x.double(), dy.double(), 3, 1, pad, p, dilation=dil)}
    close = lambda a, r: torch.allclose(a, r, rtol=1e-12, atol=1e-13)          # noqa: E731
    assert close(refs["forward"][0], y64.detach()) and close(refs["forward +="][0], y64.detach() + y0.double())
    assert close(refs["dgrad"][0], dx64) and close(refs["dgrad +="][0], dx64 + dx0.double()) and close(refs["wgrad"][0], dw64)
    # a float32 evaluation of the same operations -- the data gradient as the entry computes it: a forward convolution of dy with the
    # rotated, transposed weights (wflip_kernel) at padding 2 dil - pad

    def emu(fault=None):
        d = 1 if fault == "spacing" else dil
        shift = dil - d                                        # spacing 1: the padding moves with the taps, the centre tap stays
        ww = w
        if fault == "mirror":
            ww = w.clone()
            ww[:, :, 0, 1], ww[:, :, 2, 1] = w[:, :, 2, 1], w[:, :, 0, 1]
        wt = ww.flip(2, 3).transpose(0, 1).contiguous()
        y = F.conv2d(x, ww, b, padding=pad - shift, dilation=d)
        q = 2 * dil - pad
        if fault == "dgrad_pad":                               # the window starts at iy - pad, not at iy - (2 dil - pad)
            dx = F.conv2d(F.pad(dy, (pad, 2 * q - pad, pad, 2 * q - pad)), wt, dilation=d)
        else:
            dx = F.conv2d(dy, wt, padding=q - shift, dilation=d)
        dw = NR._cw(dy, x, 3, 1, pad - shift, d)
        if fault == "mirror":
            dw = dw.clone()
            dw[:, :, 0, 1], dw[:, :, 2, 1] = dw[:, :, 2, 1].clone(), dw[:, :, 0, 1].clone()
        return {"forward": y, "forward +=": y + y0, "dgrad": dx, "dgrad +=": dx + dx0, "wgrad": dw}
    good = emu()
    for k, (r, a) in refs.items():
        rep = _ok(good[k], r, a)
        assert rep["n_bad"] == 0 and 0 < rep["worst"] <= 1, (k, rep)
    faults = {"spacing": ("forward", "dgrad", "wgrad"), "mirror": ("forward", "dgrad", "wgrad")}
    if 2 * dil - pad != pad:
        faults["dgrad_pad"] = ("dgrad",)
    else:
        assert torch.equal(emu("dgrad_pad")["dgrad"], good["dgrad"])          # invisible here by construction, not by tolerance
    missed = [(f, k) for f, ks in faults.items() for k in ks if _ok(emu(f)[k], *refs[k])["n_bad"] == 0]
    assert not missed, missed
    assert any(2 * s[5] - s[6] != s[6] for s in DIL)
