"""A2J training on the GPU: the dilated convolutions (csrc/train.hip), pn_a2j_loss and pn_adam (csrc/train_a2j.hip), the train-mode module
(network/a2j.py + network/_autograd.py), popnet_amd.train_a2j.A2JTrainEngine and scripts/train_a2j_mpaug.py -- against CPU torch in fp64
(tests/a2j_train_reference.py) and against the reference's own training step (tests/golden/a2j_train.npz, written by
tests/golden/make_golden_a2j_train.py).  The bars of the other training tests apply (tests/test_gpu_train.py: mask flips, the accuracy
class of torch fp32 against fp64)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import a2j_cases as AC
import a2j_train_reference as R
from test_gpu_train import _accuracy_class, _assert_same_class, _floor

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(GOLDEN, "a2j_train.npz"))
G0 = np.load(os.path.join(GOLDEN, "a2j.npz"))
U = 2.0 ** -24


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _lib_ctx(gpu):
    from popnet_amd import _lib
    return _lib, _lib.lib(), _lib.Context.for_device(gpu.index), _lib.current_stream_ptr(gpu)


# ---- dilated convolutions ----------------------------------------------------------------------------------------------------------
DIL_SHAPES = [
    # N, Cin, H, W, Cout, dil, pad
    (3, 512, 5, 6, 512, 2, 2),      # layer4.1 / layer4.2 conv2 on the SMALL case
    (2, 512, 2, 2, 512, 2, 2),      # every non-centre tap in the padding
    (2, 16, 1, 1, 16, 2, 2),
    (2, 5, 7, 9, 7, 2, 2),          # ragged
    (1, 20, 9, 13, 70, 3, 3),
    (2, 8, 6, 5, 8, 2, 1),
]


def _dil_case(shape, integer):
    N, Cin, H, W, Cout, dil, pad = shape
    Ho, Wo = H + 2 * pad - 2 * dil, W + 2 * pad - 2 * dil
    g = torch.Generator().manual_seed(N * 1000 + Cin + 7 * dil + pad)
    if integer:     # small integers: every product and every partial sum is exact in fp32, whatever the order
        mk = lambda *s: torch.randint(-2, 3, s, generator=g).float()
    else:
        mk = lambda *s: torch.randn(s, generator=g)
    x, w, b, dy = mk(N, Cin, H, W), mk(Cout, Cin, 3, 3) * (1.0 if integer else 0.1), mk(Cout), mk(N, Cout, Ho, Wo)
    return x, w, b, dy, mk(N, Cout, Ho, Wo), mk(N, Cin, H, W)


def _conv_abs(x, w, pad, dil):
    """per output element: the number of products and the sum of their absolute values"""
    n = F.conv2d(torch.ones_like(x, dtype=torch.float64), torch.ones_like(w, dtype=torch.float64), padding=pad, dilation=dil)
    return n, F.conv2d(x.double().abs(), w.double().abs(), padding=pad, dilation=dil)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("shape", DIL_SHAPES)
def test_dilated_conv_entries_vs_fp64(gpu, shape, integer, accumulate):
    """tests/layer_reference.py's allowance: n 2^-24 S per element, S = the sum of |every product (and addend)|, n = the chain's length.
    On integer probes every sum is exact in fp32: bit for bit."""
    _lib, L, ctx, s = _lib_ctx(gpu)
    N, Cin, H, W, Cout, dil, pad = shape
    x, w, b, dy, y0, dx0 = _dil_case(shape, integer)
    Ho, Wo = dy.shape[2:]
    xd, wd, bd, dyd = (t.to(gpu) for t in (x, w, b, dy))

    def check(got, ref, n, S, what):
        err = (got.cpu().double() - ref).abs()
        if integer:
            assert float(err.max()) == 0.0, (what, float(err.max()))
        else:
            allow = n * U * S
            assert bool((err <= allow + 1e-30).all()), (what, float((err - allow).max()))

    # forward
    ref = R.dilated_conv(x, w, b, pad, dil) + (y0.double() if accumulate else 0)
    n, S = _conv_abs(x, w, pad, dil)
    n, S = n + 1 + accumulate, S + b.double().abs()[None, :, None, None] + (y0.double().abs() if accumulate else 0)
    run = []
    for _ in range(2):
        y = y0.clone().to(gpu) if accumulate else torch.full((N, Cout, Ho, Wo), float("nan"), device=gpu)
        ctx.check(L.pn_conv2d_forward_dil(ctx.handle, _p(xd), _p(wd), _p(bd), _p(y), N, Cin, H, W, Cout, 3, 1, pad, dil, accumulate, s), "forward_dil")
        run.append(y)
    check(run[0], ref, n, S, "forward")
    assert torch.equal(run[0], run[1])                                   # a repeated call gives the same bits
    # data gradient
    _, dxr, dwr, dbr = R.dilated_conv(x, w, None, pad, dil, dy)
    ref = dxr + (dx0.double() if accumulate else 0)
    xg = x.double().requires_grad_()
    n = torch.autograd.grad(F.conv2d(xg, torch.ones_like(w, dtype=torch.float64), padding=pad, dilation=dil), xg, torch.ones_like(dy, dtype=torch.float64))[0]
    S = torch.autograd.grad(F.conv2d(xg, w.double().abs(), padding=pad, dilation=dil), xg, dy.double().abs())[0]
    n, S = n + accumulate, S + (dx0.double().abs() if accumulate else 0)
    run = []
    for _ in range(2):
        dx = dx0.clone().to(gpu) if accumulate else torch.full((N, Cin, H, W), float("nan"), device=gpu)
        ctx.check(L.pn_conv2d_dgrad_dil(ctx.handle, _p(dyd), _p(wd), _p(dx), N, Cin, H, W, Cout, 3, pad, dil, accumulate, s), "dgrad_dil")
        run.append(dx)
    check(run[0], ref, n, S, "dgrad")
    assert torch.equal(run[0], run[1])
    if accumulate:
        return          # the weight gradient has no accumulate form
    # weight and bias gradient: chains of N Ho Wo products
    wg = w.double().requires_grad_()
    S = torch.autograd.grad(F.conv2d(x.double().abs(), wg, padding=pad, dilation=dil), wg, dy.double().abs())[0]
    run = []
    for _ in range(2):
        dw, db = torch.full((Cout, Cin, 3, 3), float("nan"), device=gpu), torch.full((Cout,), float("nan"), device=gpu)
        ctx.check(L.pn_conv2d_wgrad_dil(ctx.handle, _p(xd), _p(dyd), _p(dw), _p(db), N, Cin, H, W, Cout, 3, 1, pad, dil, s), "wgrad_dil")
        run.append((dw, db))
    check(run[0][0], dwr, N * Ho * Wo, S, "wgrad")
    check(run[0][1], dbr, N * Ho * Wo, dy.double().abs().sum((0, 2, 3)), "dbias")
    assert torch.equal(run[0][0], run[1][0]) and torch.equal(run[0][1], run[1][1])


def test_dilation_one_is_the_undilated_entry_bit_for_bit(gpu):
    _lib, L, ctx, s = _lib_ctx(gpu)
    N, Cin, H, W, Cout, pad = 2, 8, 6, 5, 8, 1
    x, w, b, dy, _, _ = _dil_case((N, Cin, H, W, Cout, 1, pad), False)
    xd, wd, bd, dyd = (t.to(gpu) for t in (x, w, b, dy))
    out = []
    for dil in (True, False):
        y, dx = torch.empty(dy.shape, device=gpu), torch.empty(x.shape, device=gpu)
        dw, db = torch.empty(w.shape, device=gpu), torch.empty(b.shape, device=gpu)
        if dil:
            ctx.check(L.pn_conv2d_forward_dil(ctx.handle, _p(xd), _p(wd), _p(bd), _p(y), N, Cin, H, W, Cout, 3, 1, pad, 1, 0, s), "forward_dil")
            ctx.check(L.pn_conv2d_dgrad_dil(ctx.handle, _p(dyd), _p(wd), _p(dx), N, Cin, H, W, Cout, 3, pad, 1, 0, s), "dgrad_dil")
            ctx.check(L.pn_conv2d_wgrad_dil(ctx.handle, _p(xd), _p(dyd), _p(dw), _p(db), N, Cin, H, W, Cout, 3, 1, pad, 1, s), "wgrad_dil")
        else:
            ctx.check(L.pn_conv2d_forward(ctx.handle, _p(xd), _p(wd), _p(bd), _p(y), N, Cin, H, W, Cout, 3, 1, pad, 0, s), "forward")
            ctx.check(L.pn_conv2d_dgrad(ctx.handle, _p(dyd), _p(wd), _p(dx), N, Cin, H, W, Cout, 3, pad, 0, s), "dgrad")
            ctx.check(L.pn_conv2d_wgrad(ctx.handle, _p(xd), _p(dyd), _p(dw), _p(db), N, Cin, H, W, Cout, 3, 1, pad, s), "wgrad")
        out.append((y, dx, dw, db))
    for a, b_ in zip(*out):
        assert torch.equal(a, b_)
    assert float((out[0][0].cpu().double() - R.dilated_conv(x, w, b, pad, 1)).abs().max()) < 1e-4


@pytest.mark.parametrize("bad", [dict(ks=1), dict(stride=2), dict(pad=5), dict(dil=0)])
def test_dilated_entries_refuse_before_any_launch(gpu, bad):
    _lib, L, ctx, s = _lib_ctx(gpu)
    a = dict(ks=3, stride=1, pad=2, dil=2)
    a.update(bad)
    N, Cin, H, W, Cout = 2, 8, 6, 5, 8
    x, w, dy = torch.zeros(N, Cin, H, W, device=gpu), torch.zeros(Cout, Cin, 3, 3, device=gpu), torch.zeros(N, Cout, H, W, device=gpu)
    y, dx, dw = (torch.full(t.shape, float("nan"), device=gpu) for t in (dy, x, w))
    with pytest.raises(_lib.PopnetError):
        ctx.check(L.pn_conv2d_forward_dil(ctx.handle, _p(x), _p(w), None, _p(y), N, Cin, H, W, Cout, a["ks"], a["stride"], a["pad"], a["dil"], 0, s), "forward_dil")
    with pytest.raises(_lib.PopnetError):
        ctx.check(L.pn_conv2d_wgrad_dil(ctx.handle, _p(x), _p(dy), _p(dw), None, N, Cin, H, W, Cout, a["ks"], a["stride"], a["pad"], a["dil"], s), "wgrad_dil")
    if "stride" not in bad:
        with pytest.raises(_lib.PopnetError):
            ctx.check(L.pn_conv2d_dgrad_dil(ctx.handle, _p(dy), _p(w), _p(dx), N, Cin, H, W, Cout, a["ks"], a["pad"], a["dil"], 0, s), "dgrad_dil")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all() and torch.isnan(dx).all() and torch.isnan(dw).all())       # nothing was written
    # and the undilated entries accept nothing new: a dilated module never reaches them
    from popnet_amd.network import _autograd as ag
    m = torch.nn.Conv2d(8, 8, 3, padding=2, dilation=2, stride=2).to(gpu)
    with pytest.raises(_lib.PopnetError):
        ag.conv(x, m)


# ---- pn_a2j_loss ----------------------------------------------------------------------------------------------------------------------
def _anchors(h, w, A, K):
    from popnet_amd.network.a2j import generate_anchors, shift
    if h == 0:
        g = torch.Generator().manual_seed(K)
        return torch.rand(K, 2, generator=g) * 96
    assert A == 16
    return torch.from_numpy(shift([h, w], 16, generate_anchors())).float()


def _loss_hip(gpu, cls, reg, dep, geom, anchors, labels, sf, scale, grads=True):
    """-> terms [2], (dcls, dreg, ddep) or None: device tensors"""
    _lib, L, ctx, s = _lib_ctx(gpu)
    B, h, w, A, P = geom
    d = [t.contiguous().to(gpu) for t in (cls, reg, dep, anchors, labels)]
    sc = torch.tensor(scale, dtype=torch.float32, device=gpu)
    terms = torch.full((2,), float("nan"), device=gpu)
    out = [torch.full(t.shape, float("nan"), device=gpu) for t in d[:3]] if grads else [None] * 3
    ctx.check(L.pn_a2j_loss(ctx.handle, _p(d[0]), _p(d[1]), _p(d[2]), B, h, w, A, P, _p(d[3]), _p(d[4]), sf, _p(sc), _p(terms), _p(out[0]), _p(out[1]), _p(out[2]), s),
              "pn_a2j_loss")
    return terms, (out if grads else None)


_loss_fp64 = R.loss_fp64           # fp64 terms and gradients with their per-element bounds: shared with the replay of the engine's step


LOSS_SHAPES = [
    # B, h, w, A, P
    (1, 1, 1, 16, 15),      # K = 16: less than a wave
    (3, 5, 6, 16, 15),      # the SMALL case
    (2, 18, 18, 16, 15),    # the trainer's K = 5184
    (2, 3, 7, 16, 1),
    (2, 0, 480, 1, 15),     # the reference's flat layout
]


def _loss_inputs(geom):
    B, h, w, A, P = geom
    K = h * w * A if h else w
    g = torch.Generator().manual_seed(K + P)
    if h:
        cls, reg, dep = torch.randn(B, A * P, h, w, generator=g), torch.randn(B, A * P * 2, h, w, generator=g) * 3, torch.randn(B, A * P, h, w, generator=g)
    else:
        cls, reg, dep = torch.randn(B, K, P, generator=g), torch.randn(B, K, P, 2, generator=g) * 3, torch.randn(B, K, P, generator=g)
    anchors = _anchors(h, w, A, K)
    centre = anchors.mean(0)
    off = torch.from_numpy(np.resize(np.array([0.05, -0.3, 0.8, -1.5, 4.0, -9.0, 20.0, 0.4, -0.6]), B * P * 3).reshape(B, P, 3)).float()
    labels = torch.cat([centre.expand(B, P, 2), torch.zeros(B, P, 1)], 2) + off
    return cls, reg, dep, anchors, labels


@pytest.mark.parametrize("scale", [(1.0, 3.0), (0.0, 1.0)])
@pytest.mark.parametrize("geom", LOSS_SHAPES)
def test_a2j_loss_terms_and_gradients_vs_fp64(gpu, geom, scale):
    cls, reg, dep, anchors, labels = _loss_inputs(geom)
    sf = 0.5
    terms, grads = _loss_hip(gpu, cls, reg, dep, geom, anchors, labels, sf, scale)
    ref_t, ref_g, t_allow, g_allow = _loss_fp64(cls, reg, dep, geom, anchors, labels, sf, scale)
    err = (terms.cpu().double() - ref_t).abs()
    assert bool((err <= t_allow).all()), (err, t_allow)
    for got, ref, allow, name in zip(grads, ref_g, g_allow, ("dcls", "dreg", "ddep")):
        e = (got.cpu().double() - ref).abs()
        assert bool((e <= allow + 1e-30).all()), (name, float((e - allow).max()))
    # equal bits on a repeated call; NULL gradient pointers leave the terms as they are
    terms2, grads2 = _loss_hip(gpu, cls, reg, dep, geom, anchors, labels, sf, scale)
    assert torch.equal(terms, terms2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    terms3, _ = _loss_hip(gpu, cls, reg, dep, geom, anchors, labels, sf, scale, grads=False)
    assert torch.equal(terms, terms3)


def test_a2j_loss_null_gradients_write_nothing(gpu):
    """the three inputs lie in one buffer between NaN canaries: the term-only call changes no byte of it"""
    _lib, L, ctx, s = _lib_ctx(gpu)
    geom = B, h, w, A, P = 3, 5, 6, 16, 15
    cls, reg, dep, anchors, labels = _loss_inputs(geom)
    parts, pad = [], torch.full((64,), float("nan"))
    for t in (cls, reg, dep):
        parts += [pad, t.reshape(-1)]
    buf = torch.cat(parts + [pad]).to(gpu)
    before = buf.clone()
    off, views = 64, []
    for t in (cls, reg, dep):
        views.append(buf[off:off + t.numel()])
        off += t.numel() + 64
    an, lab, terms = anchors.to(gpu), labels.to(gpu), torch.zeros(2, device=gpu)
    ctx.check(L.pn_a2j_loss(ctx.handle, _p(views[0]), _p(views[1]), _p(views[2]), B, h, w, A, P, _p(an), _p(lab), 0.5, None, _p(terms), None, None, None, s), "pn_a2j_loss")
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))
    full, _ = _loss_hip(gpu, cls, reg, dep, geom, anchors, labels, 0.5, (1.0, 3.0))
    assert torch.equal(terms, full)
    with pytest.raises(_lib.PopnetError):       # all three gradient pointers or none
        ctx.check(L.pn_a2j_loss(ctx.handle, _p(views[0]), _p(views[1]), _p(views[2]), B, h, w, A, P, _p(an), _p(lab), 0.5, _p(terms), _p(terms), _p(an), None, None, s),
                  "pn_a2j_loss")


def test_a2j_loss_constructed_inputs(gpu):
    from popnet_amd.network.a2j import generate_anchors, shift
    # one logit at +90 among zeros: exp(90) overflows fp32 without the max subtraction; the softmax is one-hot
    geom = B, h, w, A, P = 1, 2, 2, 16, 3
    K = h * w * A
    anchors = torch.from_numpy(shift([h, w], 16, generate_anchors())).float()
    g = torch.Generator().manual_seed(5)
    cls = torch.zeros(B, A * P, h, w)
    reg, dep = torch.randn(B, A * P * 2, h, w, generator=g), torch.randn(B, A * P, h, w, generator=g)
    hot = (7, 1, 0)                                                           # anchor a = 7 of cell y = 1, x = 0, for every joint
    for p in range(P):
        cls[0, hot[0] * P + p, hot[1], hot[2]] = 90.0
    k = (hot[2] * h + hot[1]) * A + hot[0]
    labels = torch.tensor([[[30.0, 1.0, 0.5], [2.0, 40.0, -1.0], [10.0, 10.0, 3.0]]])
    terms, grads = _loss_hip(gpu, cls, reg, dep, geom, anchors, labels, 0.5, (1.0, 3.0))
    c64, r64 = R.a2j_loss((R.nchw_to_reference(cls.double(), A, P), R.nchw_to_reference(reg.double(), A, P, two=True), R.nchw_to_reference(dep.double(), A, P)),
                          labels.double(), anchors.double(), 0.5)
    t = terms.cpu().double()
    assert bool(torch.isfinite(t).all()) and abs(float(t[0]) - float(c64)) <= 1e-5 * float(c64) and abs(float(t[1]) - float(r64)) <= 1e-5 * float(r64)
    dcls, dreg, ddep = (x.cpu() for x in grads)
    assert bool(torch.isfinite(dcls).all() and torch.isfinite(dreg).all() and torch.isfinite(ddep).all())
    assert float(dcls.abs().max()) < 1e-30                                    # at the hot anchor v_k = V, elsewhere w_k = exp(-90)
    dreg_k = R.nchw_to_reference(dreg, A, P, two=True)[0]                     # [K, P, 2]
    ddep_k = R.nchw_to_reference(ddep, A, P)[0]
    others = torch.ones(K, dtype=torch.bool)
    others[k] = False
    assert float(dreg_k[others].abs().max()) < 1e-30 and float(ddep_k[others].abs().max()) < 1e-30
    # at the hot anchor: d Reg / d reg = 3 * 0.5 / (2 P B) * f'(d), d Reg / d dep = 3 / (P B) * -sign(d_z)
    pred = anchors[k][None, :] + R.nchw_to_reference(reg, A, P, two=True)[0, k]        # [P, 2]
    d = labels[0, :, :2] - pred
    want = 3 * 0.5 / (2 * P * B) * torch.where(d.abs() <= 1, -d, -torch.sign(d))
    assert torch.allclose(dreg_k[k], want, rtol=1e-5, atol=1e-7)
    dz = labels[0, :, 2] - R.nchw_to_reference(dep, A, P)[0, k]
    assert torch.allclose(ddep_k[k], 3.0 / (P * B) * -torch.sign(dz), rtol=1e-6, atol=0)

    # all logits equal, zero reg / dep, K = 64 a power of two, labels exactly on the mean anchor: the prediction IS the label in fp32
    z = lambda *s: torch.zeros(s)
    cls, reg, dep = torch.full((B, A * P, h, w), 0.25), z(B, A * P * 2, h, w), z(B, A * P, h, w)
    centre = anchors.double().mean(0)
    assert float(centre[0]) == 16.0 and float(centre[1]) == 16.0
    labels = torch.tensor([[[16.0, 16.0, 0.0]] * P])
    terms, grads = _loss_hip(gpu, cls, reg, dep, geom, anchors, labels, 0.5, (1.0, 3.0))
    assert float(terms.abs().max()) == 0.0 and all(float(x.abs().max()) == 0.0 for x in grads)
    # a difference of exactly 1 (the seam of the smooth L1: both branches give 0.5 and slope 1) and of exactly 0 on the depth term
    labels = torch.tensor([[[17.0, 15.0, 0.0]] * P])
    terms, grads = _loss_hip(gpu, cls, reg, dep, geom, anchors, labels, 0.5, (1.0, 3.0))
    assert terms.cpu().tolist() == [0.5, 0.25]
    assert float(grads[2].abs().max()) == 0.0                                 # d|x|/dx = 0 at 0, as torch.abs
    dreg_k = R.nchw_to_reference(grads[1].cpu(), A, P, two=True)              # w_k = 1 / 64 exactly
    want = torch.tensor([-1.0, 1.0]) * (3 * 0.5 / (2 * P * B)) / 64
    assert torch.allclose(dreg_k, want.expand_as(dreg_k), rtol=1e-6, atol=0)


# ---- pn_adam ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 1.0), (1e-4, 0.5)])
@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("n", [1, 3, 4, 1027])
def test_adam_vs_fp64_formula(gpu, n, t, wd, gs):
    """Elementwise |p - p64| <= 2^-22 (|p| + |update|).  The kernel evaluates the formula in double on the stored float state, so its own
    roundings are the three final conversions (p, m, v to float: half an ulp each); the bound leaves the rest to the float state itself."""
    _lib, L, ctx, s = _lib_ctx(gpu)
    rng = np.random.default_rng(n * 10 + t)
    p, g = rng.normal(0, 1, n).astype(np.float32), (rng.normal(0, 1, n) * 10.0 ** rng.integers(-4, 2, n)).astype(np.float32)
    m, v = (rng.normal(0, 0.1, n) * (t > 1)).astype(np.float32), (rng.uniform(0, 0.1, n) * (t > 1)).astype(np.float32)
    g[::3] = 0.0                                                               # g == 0 elements
    if n > 4:
        g[1] = 1e-30                                                           # v underflows to 0 in fp32: the update is lr m / eps-shaped
        m[1] = v[1] = 0.0
    lr, b1, b2, eps = 0.00035, 0.9, 0.999, 1e-8
    p64, m64, v64 = R.adam_step(p.astype(np.float64), g.astype(np.float64), m.astype(np.float64), v.astype(np.float64), t, lr, b1, b2, eps, wd, gs)
    # four slices of one allocation, each starting on a 16-byte boundary (shift_ 0: the vector path and its scalar tail) or one float
    # past it (shift_ 1: no 16-byte access anywhere)
    stride = (n + 3) // 4 * 4 + 4
    for shift_ in (0, 1):
        buf = torch.zeros(4 * stride + 1, device=gpu)
        assert buf.data_ptr() % 16 == 0
        d = [buf[shift_ + i * stride:shift_ + i * stride + n] for i in range(4)]
        for dst, src in zip(d, (p, g, m, v)):
            dst.copy_(torch.from_numpy(src))
        ctx.check(L.pn_adam(ctx.handle, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), n, lr, b1, b2, eps, wd, t, gs, s), "pn_adam")
        got_p, got_m, got_v = (x.cpu().numpy().astype(np.float64) for x in (d[0], d[2], d[3]))
        upd = np.abs(p64 - p.astype(np.float64))
        assert (np.abs(got_p - p64) <= 2.0 ** -22 * (np.abs(p64) + upd)).all()
        assert (np.abs(got_m - m64) <= 2.0 ** -22 * np.abs(m64) + 1e-45).all() and (np.abs(got_v - v64) <= 2.0 ** -22 * np.abs(v64) + 1e-45).all()
        assert np.array_equal(d[1].cpu().numpy(), g)                           # the gradient is read only
        if n > 4 and wd == 0.0:                                                # (with weight decay the effective gradient is wd p, not 1e-30)
            assert got_v[1] == 0.0                                          # 0.001 x 1e-60 is below the smallest float, as in torch fp32
    with pytest.raises(_lib.PopnetError):
        ctx.check(L.pn_adam(ctx.handle, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), n, lr, b1, b2, eps, wd, 0, gs, s), "pn_adam")


def test_adam_state_across_two_calls_vs_torch_optim(gpu):
    _lib, L, ctx, s = _lib_ctx(gpu)
    g = torch.Generator().manual_seed(11)
    n = 1027
    p0 = torch.randn(n, generator=g)
    pr = p0.clone().requires_grad_()
    opt = torch.optim.Adam([pr], lr=0.00035, weight_decay=1e-4)
    pd, md, vd = p0.to(gpu), torch.zeros(n, device=gpu), torch.zeros(n, device=gpu)
    for t in (1, 2):
        gr = torch.randn(n, generator=g)
        before = pr.detach().clone()
        m_old, v_old = (opt.state[pr][k].double().clone() for k in ("exp_avg", "exp_avg_sq")) if t > 1 else (torch.zeros(n, dtype=torch.float64),) * 2
        pr.grad = gr.clone()
        opt.step()
        ctx.check(L.pn_adam(ctx.handle, _p(pd), _p(gr.to(gpu)), _p(md), _p(vd), n, 0.00035, 0.9, 0.999, 1e-8, 1e-4, t, 1.0, s), "pn_adam")
        st = opt.state[pr]
        upd = (pr.detach() - before).abs().double()
        assert bool(((pd.cpu().double() - pr.detach().double()).abs() <= 2.0 ** -22 * (pr.detach().double().abs() + upd)).all())
        # the moments: b m + (1 - b) g (g g) evaluated twice, in torch's fp32 and in the kernel's double rounded once.  The two ADDENDS may
        # cancel, so the bound is on their absolute values.  Roundings of 2^-24 each on torch's side: g + wd p (1; it counts twice in g g), the
        # product g g (1), the constant 1 - b as a float (1), the product with it (1), the carried moment's own error from the step before
        # (the same count), the final sum (1): at most 8 -- 2^-21 of the addends; the kernel adds half an ulp of the result.  g and wd p may
        # cancel as well: the effective gradient enters by |g| + wd |p|.
        ge = gr.double().abs() + 1e-4 * before.double().abs()
        assert bool(((md.cpu().double() - st["exp_avg"].double()).abs() <= 2.0 ** -21 * (0.9 * m_old.abs() + 0.1 * ge) + 1e-45).all())
        assert bool(((vd.cpu().double() - st["exp_avg_sq"].double()).abs() <= 2.0 ** -21 * (0.999 * v_old + 0.001 * ge * ge) + 1e-45).all())


def test_adam_marks_the_weight_packs_stale(gpu):
    """with the pack cache on, a 3x3 convolution reads its cached pack; after pn_adam has moved the weights the next convolution rebuilds it"""
    from popnet_amd import _lib
    L, ctx, s = _lib.lib(), _lib.Context(gpu.index), _lib.current_stream_ptr(gpu)
    ctx.check(L.pn_train_pack_cache(ctx.handle, 1), "pack_cache")
    g = torch.Generator().manual_seed(2)
    N, Cc, H, W = 2, 16, 8, 8
    x, w = torch.randn(N, Cc, H, W, generator=g).to(gpu), torch.randn(Cc, Cc, 3, 3, generator=g).to(gpu)

    def conv():
        y = torch.empty(N, Cc, H, W, device=gpu)
        ctx.check(L.pn_conv2d_forward(ctx.handle, _p(x), _p(w), None, _p(y), N, Cc, H, W, Cc, 3, 1, 1, 0, s), "forward")
        return y
    y0 = conv()
    assert torch.equal(y0, conv())
    gr, m, v = torch.ones_like(w), torch.zeros_like(w), torch.zeros_like(w)
    ctx.check(L.pn_adam(ctx.handle, _p(w), _p(gr), _p(m), _p(v), w.numel(), 0.1, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, s), "pn_adam")
    y1 = conv()
    assert not torch.equal(y0, y1)
    assert float((y1.cpu().double() - F.conv2d(x.cpu().double(), w.cpu().double(), padding=1)).abs().max()) < 1e-3
    ctx.check(L.pn_train_pack_cache(ctx.handle, 0), "pack_cache")


# ---- the golden case: engine and train-mode module ------------------------------------------------------------------------------------
def _golden_sd():
    keys = [str(k) for k in G0["keys"]]
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(G0["shapes"], G0["ndim"])]
    return AC.state_dict_for_seed(AC.SEED, keys, shapes)


def _golden_batch():
    H, W, B = AC.SMALL
    return torch.from_numpy(AC.net_input(AC.SEED + H, B, H, W)), torch.from_numpy(G["labels"]).float()


@pytest.fixture(scope="module")
def cpu_ref():
    """torch on the CPU, once: the gradients of the golden step in fp64 and in fp32 (tests/a2j_train_reference.py)"""
    from popnet_amd.network.a2j import generate_anchors, shift
    H, W, B = AC.SMALL
    out = {}
    for dt in (torch.float64, torch.float32):
        sd = {k: (v.to(dt) if v.is_floating_point() else v.clone()) for k, v in _golden_sd().items()}
        names = [str(k) for k in G["grad_keys"]]
        for k in names:
            sd[k].requires_grad_(True)
        x, lab = _golden_batch()
        heads, _ = R.forward_train(sd, x.to(dt))
        c, r = R.a2j_loss(heads, lab.to(dt), torch.from_numpy(shift([H // 16, W // 16], 16, generate_anchors())).to(dt), float(G["spatial_factor"]))
        (c + float(G["reg_loss_factor"]) * r).backward()
        out[dt] = {k: sd[k].grad.detach() for k in names}
    return out


@pytest.fixture(scope="module")
def engine_step(gpu):
    """one engine on the golden case: after forward_backward (no update yet)"""
    from popnet_amd.train_a2j import A2JTrainEngine
    eng = A2JTrainEngine(_golden_sd(), device=gpu)
    x, lab = _golden_batch()
    terms = eng.forward_backward(x.to(gpu), lab.to(gpu)).cpu().numpy().astype(np.float64)
    return eng, terms


def test_engine_step_equals_the_reference_golden(gpu, engine_step, cpu_ref):
    """One engine step on the golden case against the reference's own step (tests/golden/a2j_train.npz) and torch's two CPU runs.
    Measured on an MI355X: loss terms 4.645572 / 5.809124 against 4.645573 / 5.809125 (tolerance 5e-6); head gradients at 0.11 / 0.18 / 0.19 of
    their tolerances; error of the parameter gradients against fp64 (median over tensors / maximum / whole vector) 5.7e-3 / 1.7e-2 / 5.6e-3
    for the engine next to 1.4e-3 / 2.7e-2 / 1.9e-3 for torch fp32 on the CPU -- the median passes through the `4 x torch fp32` arm of
    test_gpu_train._assert_same_class, not through its 5e-3 cap: the case is flip-heavy (BatchNorm over 90 values per channel in layer4), and
    the engine's convolutions sum their K = 512 .. 4608 products in one serial fp32 chain where torch's GEMM sums in blocks.
    That this distance is rounding and not a wrong operand is checked launch by launch in tests/test_gpu_train_a2j_layers.py: every one of the
    step's launches stays inside the fp64 allowance of its own definition on the operands it read (forward and data-gradient chains at <= 0.11 of it, weight gradients at <= 0.42, with
    no BatchNorm mask disagreement), and references with one wrong tap spacing, residual or accumulated gradient are rejected there."""
    eng, terms = engine_step
    H, W, B = AC.SMALL
    h, w = H // 16, W // 16
    tol = np.maximum(G["terms_tol"], 16 * U * np.abs(G["terms"]))
    print("loss terms", terms, "golden", G["terms"], "tol", tol)
    assert bool((np.abs(terms - G["terms"]) <= tol).all()), (terms, G["terms"], tol)
    for name, d, two in zip(("dcls", "dreg", "ddep"), eng.head_grads, (False, True, False)):
        got = R.nchw_to_reference(d.cpu().double(), 16, 15, two=two).numpy()
        err = np.abs(got - G[name]).max()
        print(name, err, float(G[name + "_tol"]))
        assert err <= float(G[name + "_tol"]), (name, err)
    # parameter gradients: torch fp32's accuracy class against fp64
    g32, g64 = cpu_ref[torch.float32], cpu_ref[torch.float64]
    assert set(eng.g) == set(g32) and not any(k.startswith("Backbone.model.fc.") for k in eng.g)
    floor = _floor(g32)
    excluded = sorted(k for k, v in g64.items() if not float(v.norm()) > 100 * floor * np.sqrt(v.numel()))
    assert excluded == sorted("%s.conv%d.bias" % (hd, i) for hd in ("classificationModel", "regressionModel", "DepthRegressionModel") for i in (1, 2, 3, 4)), excluded
    hip, t32 = _accuracy_class(eng, g32, g64)
    print("accuracy class: hip", hip, "torch fp32", t32)
    _assert_same_class(hip, t32)
    # the reference's own stored norms and samples: nearly all close, none wild
    gkeys = [str(k) for k in G["grad_keys"]]
    norms = np.array([float(eng.g[k].double().norm()) for k in gkeys])
    rel = np.abs(norms - G["grad_norms"]) / np.maximum(G["grad_norms"], 1e-30)
    big = np.array([k not in excluded for k in gkeys])
    assert rel[big].max() <= 3e-2 and (rel[big] <= 5e-3).mean() >= 0.95, (rel[big].max(), (rel[big] <= 5e-3).mean())
    flat = torch.cat([eng.g[k].reshape(-1) for k in gkeys]).cpu().double().numpy()[::int(G["sample_every"])]
    d = np.abs(flat - G["grad_samples"])
    rms = np.sqrt((G["grad_samples"] ** 2).mean())
    assert d.max() <= rms and (d <= 2e-2 * rms + float(G["grad_samples_tol"])).mean() >= 0.98, (d.max(), rms)
    # conv1: the three input slices see the same input
    g1 = eng.g["Backbone.model.conv1.weight"]
    assert torch.equal(g1[:, 0], g1[:, 1]) and torch.equal(g1[:, 0], g1[:, 2]) and float(g1.abs().max()) > 0
    # BatchNorm running statistics after the step
    new = eng.state_dict()
    for k in G.files:
        if k.startswith("stat_") and not k.endswith("_tol"):
            kind, layer = k.split(".", 1)
            got = new[layer + (".running_mean" if kind == "stat_mean" else ".running_var")].cpu().double().numpy()
            assert np.abs(got - G[k]).max() <= float(G[k + "_tol"]), (k, np.abs(got - G[k]).max(), float(G[k + "_tol"]))
    assert int(new["Backbone.model.bn1.num_batches_tracked"]) == 1


def test_engine_adam_steps_and_carried_fc(gpu, engine_step):
    """After step(): the parameters equal the fp64 Adam formula applied on the host to the ENGINE's own gradient (not the reference's
    post-step parameters: Adam's first step is sign-like, and elements whose gradient is rounding noise move by +-lr either way)."""
    eng, _ = engine_step
    sd0 = _golden_sd()
    p0, g1 = eng.flat_p.cpu().numpy().astype(np.float64), eng.flat_g.cpu().numpy().astype(np.float64)
    eng.apply()
    lr, wd = 0.00035, 1e-4
    p1, m1, v1 = R.adam_step(p0, g1, np.zeros_like(p0), np.zeros_like(p0), 1, lr, wd=wd)
    got = eng.flat_p.cpu().numpy().astype(np.float64)
    assert (np.abs(got - p1) <= 2.0 ** -22 * (np.abs(p1) + np.abs(p1 - p0))).all()
    # a second step runs; its Adam state matches torch.optim.Adam fed the engine's two gradients
    x, lab = _golden_batch()
    terms2 = eng.forward_backward(x.to(gpu), lab.to(gpu)).cpu().numpy()
    assert np.isfinite(terms2).all()
    g2 = eng.flat_g.cpu().clone()
    eng.apply()
    pr = torch.from_numpy(p0.astype(np.float32)).requires_grad_()
    opt = torch.optim.Adam([pr], lr=lr, weight_decay=wd)
    for gr in (torch.from_numpy(g1.astype(np.float32)), g2):
        pr.grad = gr.clone()
        opt.step()
    st = opt.state[pr]
    # bounds on the ADDENDS of b m + (1 - b) g (they may cancel), from the fp64 formula on the same two gradients: 2^-21, the count of
    # roundings written out in test_adam_state_across_two_calls_vs_torch_optim (g and wd p may cancel too: |g| + wd |p|; among 27 million
    # elements some do)
    ge1, ge2 = np.abs(g1) + wd * np.abs(p0), np.abs(g2.numpy().astype(np.float64)) + wd * np.abs(p1)
    m_allow = 2.0 ** -21 * (0.9 * 0.1 * ge1 + 0.1 * ge2) + 1e-45              # the carried first moments by their own absolute addends
    v_allow = 2.0 ** -21 * (0.999 * 0.001 * ge1 * ge1 + 0.001 * ge2 * ge2) + 1e-45
    assert (np.abs(eng.flat_m.cpu().numpy().astype(np.float64) - st["exp_avg"].numpy().astype(np.float64)) <= m_allow).all()
    assert (np.abs(eng.flat_v.cpu().numpy().astype(np.float64) - st["exp_avg_sq"].numpy().astype(np.float64)) <= v_allow).all()
    assert eng.steps == 2
    new = eng.state_dict()
    assert set(new) == set(sd0)
    for k in ("Backbone.model.fc.weight", "Backbone.model.fc.bias"):
        assert torch.equal(new[k].cpu(), sd0[k])                               # carried, never touched (no weight decay either)
    assert int(new["Backbone.model.bn1.num_batches_tracked"]) == 2


def test_engine_and_loss_refusals(gpu):
    from popnet_amd import _lib
    from popnet_amd.network.a2j import A2J_loss
    from popnet_amd.train_a2j import A2JTrainEngine
    eng = A2JTrainEngine(_golden_sd(), device=gpu)
    with pytest.raises(_lib.PopnetError, match="31"):
        eng.forward_backward(torch.zeros(32, 1, 32, 32, device=gpu), torch.zeros(32, 15, 3, device=gpu))
    with pytest.raises(_lib.PopnetError, match="multiple of 16"):
        eng.forward_backward(torch.zeros(2, 1, 72, 80, device=gpu), torch.zeros(2, 15, 3, device=gpu))
    with pytest.raises(_lib.PopnetError, match="one value per channel"):
        eng.forward_backward(torch.zeros(1, 1, 16, 16, device=gpu), torch.zeros(1, 15, 3, device=gpu))
    with pytest.raises(_lib.PopnetError):
        A2J_loss(shape=[5, 6], stride=16, P_h=None, P_w=None, is_3D=False)


def test_train_mode_module_equals_the_engine(gpu, engine_step):
    """The reference's loop with the imports swapped: heads = net(img); Cls, Reg = criterion(heads, label); (Cls + 3 Reg).backward();
    torch.optim.Adam(net.parameters()).step().  Same kernels in the same order as the engine, with two differences of order.
    (1) A2J_loss goes through pn_a2j_loss's flat-layout entry on the re-laid-out heads, the engine through the NCHW entry: the items of a
    (crop, joint) are dealt to the lanes in another order, so the sums round differently -- the terms agree to 16 ulp, the head gradients
    to rounding.  (2) Where a tensor feeds two consumers (x3: layer4 and the classification head; x4: two heads; a block's input: conv1
    and the identity) the engine accumulates the second data gradient inside the convolution's epilogue, autograd adds finished tensors:
    three addends may be summed in another order (a + b + c against a + c + b).  The backward pass is linear in the head gradients once the
    forward (identical in both) has fixed masks and statistics, so every gradient is compared at 1e-5 of its tensor's norm -- two orders of
    magnitude under torch fp32's own distance from fp64 on this case -- not bit for bit."""
    from popnet_amd.network.a2j import A2J_loss, A2J_model
    from popnet_amd.train_a2j import A2JTrainEngine
    H, W, B = AC.SMALL
    eng = A2JTrainEngine(_golden_sd(), device=gpu)
    x, lab = _golden_batch()
    xd, labd = x.to(gpu), lab.to(gpu)
    terms = eng.forward_backward(xd, labd).clone()
    net = A2J_model(15)
    net.load_state_dict(_golden_sd())
    net = net.to(gpu).train()
    criterion = A2J_loss(shape=[H // 16, W // 16], thres=[16.0, 32.0], stride=16, spatialFactor=0.5, img_shape=[W, H], P_h=None, P_w=None)
    optimizer = torch.optim.Adam(net.parameters(), lr=0.00035, weight_decay=1e-4)
    heads = net(xd)
    optimizer.zero_grad()
    cls_loss, reg_loss = criterion(heads, labd)
    assert tuple(cls_loss.shape) == (1,) and tuple(reg_loss.shape) == (1,) and heads[0].grad_fn is not None
    loss = 1 * cls_loss + reg_loss * 3
    loss.backward()
    got_terms = torch.cat([cls_loss, reg_loss]).detach()
    assert bool(((got_terms - terms).abs() <= 16 * U * terms.abs()).all()), (got_terms, terms)
    named = dict(net.named_parameters())
    assert named["Backbone.model.fc.weight"].grad is None
    floor = 1e-6 * max(float(g.double().norm()) / np.sqrt(g.numel()) for g in eng.g.values())      # test_gpu_train._floor's rule: the zero-gradient biases
    for k, g in eng.g.items():
        err, ref = float((named[k].grad - g).double().norm()), float(g.double().norm())
        assert err <= 1e-5 * ref + floor * np.sqrt(g.numel()), (k, err, ref)
    p_before = {k: p.detach().clone() for k, p in eng.p.items()}
    optimizer.step()
    eng.apply()
    lr, eps = 0.00035, 1e-8
    for k, p in eng.p.items():
        # the pn_adam bound between the two fp32 evaluations, plus the first-order effect of the two gradients' difference on Adam's first,
        # sign-like step  lr g / (|g| + eps):  |d update| <= lr |dg| / (|g| + eps)
        q, g = named[k].detach().double(), eng.g[k].double() + 1e-4 * p_before[k].double()
        dg = (named[k].grad - eng.g[k]).abs().double()
        allow = 2.0 ** -22 * (p.abs().double() + (p - p_before[k]).abs().double()) + 2 * lr * dg / (g.abs() + eps)
        assert bool(((q - p.double()).abs() <= allow).all()), k
    # eval afterwards reproduces the eval forward of a fresh module loaded from the module's own state
    sd_after = {k: v.detach().clone() for k, v in net.state_dict().items()}
    assert int(sd_after["Backbone.model.bn1.num_batches_tracked"]) == 1
    net.eval()
    with torch.no_grad():
        out_a = net(xd)
    fresh = A2J_model(15)
    fresh.load_state_dict(sd_after)
    fresh = fresh.to(gpu).eval()
    with torch.no_grad():
        out_b = fresh(xd)
    for a, b in zip(out_a, out_b):
        assert torch.equal(a, b)
    # ... and of one loaded from engine.state_dict(): the two states agree within the Adam bound, the heads to 1e-3 of their range
    fresh.load_state_dict(eng.state_dict())
    with torch.no_grad():
        out_c = fresh.to(gpu).eval()(xd)
    for a, c in zip(out_a, out_c):
        assert float((a - c).abs().max()) <= 1e-3 * float(a.abs().max())


# ---- the trainer script ------------------------------------------------------------------------------------------------------------------
def _fake_mpaug_tree(d, frames_per_set=8):
    """the synthetic MP-3DHP split of tests/test_gpu_train_yolo.py::test_train_script_on_a_fake_mpaug_dataset, with more frames per set"""
    import json
    from popnet_amd import synth
    for sub in ("img", "seg", "bg"):
        os.makedirs(os.path.join(d, sub))
    rng = np.random.default_rng(8)
    H, W = 320, 240
    ann_files = []
    for ii in range(5):
        ann = {"intrinsics": {"fx": 504.1, "fy": 504.0, "cx": 120.0, "cy": 160.0}}
        for f in range(frames_per_set):
            name = "s%d_%d.npy" % (ii, f)
            joints, depths = synth.planted_persons(rng, 1, size=224)
            j2 = joints[0] * [W / 224.0, H / 224.0]
            bbox = [float(j2[:, 0].min()) - 8, float(j2[:, 1].min()) - 8, float(j2[:, 0].max()) + 8, float(j2[:, 1].max()) + 8]
            ann[name] = [{"2d_joints": j2.tolist(), "3d_joints": np.concatenate([j2, np.full((15, 1), depths[0])], 1).tolist(), "bbox": bbox,
                          "pose_weight": float(rng.uniform(0.5, 2.0))}]
            mask = np.zeros((H, W), dtype=np.uint8)
            mask[max(int(bbox[1]), 0):int(bbox[3]), max(int(bbox[0]), 0):int(bbox[2])] = 1
            np.save(os.path.join(d, "img", name), np.clip(rng.normal(depths[0], 0.1, (H, W)), 0.3, 5.9).astype(np.float16))
            np.save(os.path.join(d, "seg", name), mask)
        path = os.path.join(d, "ann%d.json" % ii)
        json.dump(ann, open(path, "w"))
        ann_files.append(path)
    bgs = {}
    for f in range(2):
        np.save(os.path.join(d, "bg", "bg%d.npy" % f), np.clip(rng.normal(4.5, 0.3, (H, W)), 0, 6).astype(np.float16))
        bgs[str(f)] = {"file_name": "bg%d.npy" % f}
    json.dump(bgs, open(os.path.join(d, "bg.json"), "w"))
    return ann_files


def test_train_script_on_a_fake_mpaug_dataset(gpu, tmp_path, capsys):
    """scripts/train_a2j_mpaug.py end to end: composed and augmented frames, one box crop and label per frame, Adam steps, a finite
    validation loss, a falling training loss, one `.pth` per epoch with the reference's keys, loaded by the inference path (pn_a2j_predict)."""
    import importlib.util
    import random
    from popnet_amd.pipeline import A2JEngine
    d = str(tmp_path)
    ann_files = _fake_mpaug_tree(d)
    spec = importlib.util.spec_from_file_location("train_a2j_mpaug", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "train_a2j_mpaug.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    random.seed(2)
    out_dir = os.path.join(d, "out")
    mod.main(["--train-annotations"] + ann_files + ["--val-annotations"] + ann_files[:2] + ["--image-dir", os.path.join(d, "img"), "--bg-file", os.path.join(d, "bg.json"),
             "--bg-dir", os.path.join(d, "bg"), "--seg-dir", os.path.join(d, "seg"), "--output-dir", out_dir, "--batch-size", "4", "--lr", "0.001",
             "--epochs", "2", "--print-freq", "1", "--seed", "2", "--frame-size", "256", "--crop", "64"])
    out = capsys.readouterr().out
    train = [float(line.split(":")[1].split(",")[0]) for line in out.splitlines() if line.startswith("mean train_loss_add")]
    val = [float(line.split(":")[1].split(",")[0]) for line in out.splitlines() if line.startswith("mean val_loss")]
    assert len(train) == 2 and len(val) == 2, out
    assert np.isfinite(val).all() and np.isfinite(train).all(), out
    assert train[1] < train[0], out
    files = sorted(os.listdir(out_dir))
    assert len(files) == 2 and all(f.startswith("net_") and f.endswith(".pth") for f in files), files
    sd = torch.load(os.path.join(out_dir, files[-1]), map_location="cpu")
    assert sorted(sd) == sorted(str(k) for k in G0["keys"])                   # the reference's 410 keys: A2J_model.load_state_dict(strict) below
    eng = A2JEngine(precision="fp32", state_dict=sd, device=gpu, max_batch=2, crop=64)
    frames = torch.from_numpy(np.random.default_rng(1).uniform(1, 5, (1, 320, 240)).astype(np.float16)).to(gpu)
    recs = eng.predict_host(frames, np.array([[0, 40, 60, 160, 280, 0.9], [0, 10, 20, 100, 200, 0.8]], np.float32))
    assert recs.shape == (2,) and np.isfinite(recs["joint"]).all()
