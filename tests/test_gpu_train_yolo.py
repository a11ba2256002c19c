"""YoloPoseNet training on the GPU: the kernels of csrc/train_yolo.hip (strided data gradient, max pooling, prior targets, the cast +
loss + gradient of the head), the train-mode module (network/yolo_posenet.py + network/_autograd.py), popnet_amd.train_yolo.YoloTrainEngine
and scripts/train_yolo_mpaug.py -- against CPU torch in fp64 (tests/yolo_reference.py) and against the reference's own outputs
(tests/golden/yolo_train_step.npz, tests/golden/yolo_targets.npz, written by tests/golden/make_golden_yolo.py).
The bars of the rtpose training tests apply (tests/test_gpu_train.py: mask flips, the accuracy class of torch fp32 against fp64)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yolo_reference as yr
from helpers import YOLO_ANCHORS, sample_indices, state_dict_from_keys, train_case_inputs
from test_gpu_train import _accuracy_class, _f64, _rel

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(GOLDEN, "yolo_train_step.npz"))
T = np.load(os.path.join(GOLDEN, "yolo_targets.npz"))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _lib_ctx(gpu):
    from popnet_amd import _lib
    return _lib, _lib.lib(), _lib.Context.for_device(gpu.index), _lib.current_stream_ptr(gpu)


# ---- strided data gradient -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [
    # N, Cin, H, W, Cout, ks, stride, pad
    (3, 64, 24, 32, 128, 3, 2, 1),      # layer2.0.conv1 at the golden batch shape
    (3, 64, 24, 32, 128, 1, 2, 0),      # layer2.0.downsample.0
    (2, 64, 56, 56, 128, 3, 2, 1),      # layer2.0.conv1 at 224 x 224
    (2, 5, 13, 9, 7, 3, 2, 1),          # ragged, odd sizes
    (2, 6, 11, 7, 5, 1, 2, 0),
])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_strided_dgrad_vs_fp64(gpu, shape, accumulate):
    _lib, L, ctx, s = _lib_ctx(gpu)
    N, Cin, H, W, Cout, ks, st, pad = shape
    Ho, Wo = (H + 2 * pad - ks) // st + 1, (W + 2 * pad - ks) // st + 1
    g = torch.Generator().manual_seed(N * 1000 + Cin + ks)
    dy = torch.randn((N, Cout, Ho, Wo), generator=g)
    w = torch.randn((Cout, Cin, ks, ks), generator=g) * 0.1
    d0 = torch.randn((N, Cin, H, W), generator=g)
    dx = d0.clone().to(gpu) if accumulate else torch.full((N, Cin, H, W), float("nan"), device=gpu)
    dyd, wd = dy.to(gpu), w.to(gpu)                                      # held: the kernel runs after this line
    ctx.check(L.pn_conv2d_dgrad_strided(ctx.handle, _p(dyd), _p(wd), _p(dx), N, Cin, H, W, Cout, ks, st, pad, accumulate, s), "dgrad_strided")
    ref = torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), dy.double(), stride=st, padding=pad)
    bound = torch.nn.grad.conv2d_input((N, Cin, H, W), w.double().abs(), dy.double().abs(), stride=st, padding=pad)
    if accumulate:
        ref = ref + d0.double()
    # tests/layer_reference.py's allowance: n 2^-24 S per element, S = sum of |every product (and addend)|, n = the chain's length
    n = torch.nn.grad.conv2d_input((N, Cin, H, W), torch.ones_like(w, dtype=torch.float64), torch.ones_like(dy, dtype=torch.float64), stride=st, padding=pad)
    err = (dx.cpu().double() - ref).abs()
    allow = (n + accumulate) * 2.0 ** -24 * (bound + (d0.double().abs() if accumulate else 0)) + (2.0 ** -24 * ref.abs() if accumulate else 0)
    assert bool((err <= allow + 1e-30).all()), float((err - allow).max())
    # a repeated call gives the same bits
    dx2 = d0.clone().to(gpu) if accumulate else torch.empty((N, Cin, H, W), device=gpu)
    ctx.check(L.pn_conv2d_dgrad_strided(ctx.handle, _p(dyd), _p(wd), _p(dx2), N, Cin, H, W, Cout, ks, st, pad, accumulate, s), "dgrad_strided")
    assert torch.equal(dx, dx2)


# ---- max pooling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", [(3, 2, 1), (2, 2, 0)])
@pytest.mark.parametrize("shape", [(3, 64, 48, 64), (3, 256, 12, 16), (2, 3, 13, 9), (1, 2, 7, 12)])
def test_maxpool_forward_indices_and_backward_bit_exact(gpu, pool, shape):
    _lib, L, ctx, s = _lib_ctx(gpu)
    k, st, pad = pool
    N, Cc, H, W = shape
    g = torch.Generator().manual_seed(H * 100 + W + k)
    x = torch.randint(-3, 4, shape, generator=g).float() * 0.5          # coarse values: ties in most windows
    x.view(-1)[torch.randperm(x.numel(), generator=g)[:max(3, x.numel() // 97)]] = float("nan")
    x[0, 0, :2, :] = -float("inf")                                       # windows of -inf only: the index stays at the window's first pixel
    y_ref, i_ref = F.max_pool2d(x, k, st, pad, return_indices=True)
    Ho, Wo = y_ref.shape[2:]
    xd = x.to(gpu)
    y = torch.empty((N, Cc, Ho, Wo), device=gpu)
    idx = torch.empty((N, Cc, Ho, Wo), device=gpu, dtype=torch.int32)
    ctx.check(L.pn_maxpool_forward(ctx.handle, _p(xd), _p(y), _p(idx), N * Cc, H, W, k, st, pad, s), "maxpool_forward")
    assert torch.equal(idx.cpu().long(), i_ref)
    assert torch.equal(torch.isnan(y.cpu()), torch.isnan(y_ref)) and torch.equal(y.cpu().nan_to_num(), y_ref.nan_to_num())
    # backward against CPU autograd of the same pool
    xr = x.clone().requires_grad_(True)
    dy = torch.randn((N, Cc, Ho, Wo), generator=g)
    F.max_pool2d(xr, k, st, pad).backward(dy)
    dx = torch.full(shape, float("nan"), device=gpu)
    dyd = dy.to(gpu)
    ctx.check(L.pn_maxpool_backward(ctx.handle, _p(dyd), _p(idx), _p(dx), N * Cc, H, W, k, st, pad, s), "maxpool_backward")
    assert torch.equal(dx.cpu(), xr.grad)


# ---- prior targets ---------------------------------------------------------------------------------------------------------------
def test_prior_targets_bit_exact_vs_reference_golden(gpu):
    from popnet_amd import targets
    n = int(T["n_cases"])
    P = max(T["c%d_boxes" % c].shape[0] for c in range(n))
    boxes = np.zeros((n, P, 4))
    kp2d = np.zeros((n, P, 15, 2), np.float32)
    kpz = np.zeros((n, P, 15))
    pw = np.zeros((n, P))
    npers = np.zeros(n, np.int32)
    for c in range(n):
        m = T["c%d_boxes" % c].shape[0]
        boxes[c, :m], kp2d[c, :m], kpz[c, :m], pw[c, :m], npers[c] = T["c%d_boxes" % c], T["c%d_kp2d" % c], T["c%d_kpz" % c], T["c%d_pw" % c], m
    # the whole batch in one call (padded person slots), and every case on its own
    got = targets.prior_targets(*[torch.from_numpy(a).to(gpu) for a in (boxes, kp2d, kpz, pw, npers)])
    for c in range(n):
        alone = targets.prior_targets(*[torch.from_numpy(a[c:c + 1]).to(gpu) for a in (boxes, kp2d, kpz, pw, npers)])
        for i, name in enumerate(("prior", "conf", "coord", "weight")):
            ref = T["c%d_%s" % (c, name)]
            assert np.array_equal(got[i][c].cpu().numpy(), ref), (str(T["names"][c]), name)
            assert np.array_equal(alone[i][0].cpu().numpy(), ref), (str(T["names"][c]), name)
    empty = [i for i in range(n) if str(T["names"][i]) == "empty"][0]
    assert float(got[1][empty].min()) == float(got[1][empty].max()) == np.float32(0.1) and float(got[3][empty].min()) == 1.0


# ---- head casts + loss -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("B,h,w", [(3, 6, 8), (2, 14, 14), (1, 5, 7)])
def test_yolo_loss_terms_and_gradient_vs_fp64(gpu, weighted, B, h, w):
    _lib, L, ctx, s = _lib_ctx(gpu)
    prior, conf, coord, weight = [torch.from_numpy(a) for a in yr.yolo_case_targets(seed=B * 7 + h, B=B, H=16 * h, W=16 * w)]
    v = torch.from_numpy(np.random.default_rng(h * w).normal(0, 2, prior.shape).astype(np.float32))
    vd = v.to(gpu)
    out, dv = torch.empty_like(vd), torch.empty_like(vd)
    terms = torch.empty(4, device=gpu)
    dev = [t.to(gpu) for t in (prior, conf, coord, weight)]
    ctx.check(L.pn_yolo_loss(ctx.handle, _p(vd), _p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]) if weighted else None, B, 2, 15, h, w,
                             _p(out), _p(terms), _p(dv), s), "pn_yolo_loss")
    v64 = v.double().requires_grad_(True)
    sg = v64.view(B, 2, 50, h, w).sigmoid()
    o64 = torch.cat([(sg[:, :, :2] - 0.5) * 2, sg[:, :, 2:4] * 2, sg[:, :, 4:5], (sg[:, :, 5:] - 0.5) * 4], 2).view(v.shape)
    t64 = yr.loss_terms(o64, prior.double(), conf.double(), coord.double(), weight.double() if weighted else None)
    t64[0].backward()
    assert np.allclose(terms.cpu().numpy(), t64.detach().numpy(), rtol=1e-6, atol=0), (terms.cpu().numpy(), t64.detach().numpy())
    assert _rel(dv, v64.grad) < 1e-5
    assert float((out.cpu().double() - o64.detach()).abs().max()) < 1e-6
    # the torch glue of network/losses.py on the kernel's output gives the same terms
    from popnet_amd.network.losses import yolo_loss_fgweight, yolo_loss_fgweight_poseweight
    if weighted:
        tot, log = yolo_loss_fgweight_poseweight(out, *dev, 15, 2)
        assert np.allclose([log[k] for k in ("loss_prior", "loss_bbox", "loss_obj", "loss_selfpose")], terms.cpu().numpy(), rtol=2e-6)
    else:
        tot = yolo_loss_fgweight(out, *dev[:3], 15, 2)
    assert abs(float(tot) - float(terms[0])) <= 2e-6 * abs(float(terms[0]))


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def _engine(golden, gpu, **kw):
    from popnet_amd.train_yolo import YoloTrainEngine
    return YoloTrainEngine(state_dict_from_keys(golden.keys["yolo_posenet"], seed=0), device=gpu, **kw)


def _batch(seed=21, B=3, H=96, W=128, tseed=41):
    img = train_case_inputs(seed=seed, B=B, H=H, W=W)[0]
    return [torch.from_numpy(a) for a in (img,) + yr.yolo_case_targets(seed=tseed, B=B, H=H, W=W)]


def _assert_yolo_class(hip, t32):
    """_assert_same_class with the flip budget of YoloPoseNet's golden shape: its last layers are 6 x 8 and 12 x 16 maps, so one LeakyReLU
    sign or max-pool argmax that lands differently (luck on either side, see test_gpu_train.py) moves every upstream gradient by ~1 / sqrt(3 x 128
    x 48) ~ 7e-3.  Measured at step 0: median 4e-3 / 5e-3 (pose-weighted / plain), whole vector 4e-3 / 5e-3, while the loss terms, the forward and
    the BatchNorm statistics agree with fp32 autograd to 1e-7.  That these are flips is proven, not assumed: at this shape the engine's step
    differs from an unforced fp64 evaluation in ONE mask element (model1.4's LeakyReLU), and against fp64 forced onto the engine's own masks
    and argmaxes every gradient tensor meets the strict 1e-4 bar (test_engine_gradients_strict_against_mask_forced_fp64)."""
    for h, t, what, cap in zip(hip, t32, ("median", "max", "whole vector"), (1e-2, 3e-2, 1e-2)):
        assert h <= max(4 * t + 1e-4, cap), (what, hip, t32)


class _Grads:
    def __init__(self, g):
        self.g = g


def test_engine_two_steps_equal_reference_goldens(gpu, golden):
    """The golden case (B = 3, 96 x 128, O(1)-scale seeded weights, seeded prior targets): what the reference's own module,
    yolo_loss_fgweight_poseweight, backward() and torch.optim.SGD produced for two consecutive steps -- with the bars of
    test_gpu_train.py::test_training_step_equals_reference_goldens_and_oracle."""
    eng = _engine(golden, gpu)
    sd0 = state_dict_from_keys(golden.keys["yolo_posenet"], seed=0)
    sd = dict(sd0)
    batch = _batch()
    dbatch = [b.to(gpu) for b in batch]
    for step in range(2):
        r = yr.train_step(sd, *batch)
        r64 = yr.train_step(_f64(sd), *[b.double() for b in batch], dtype=torch.float64)
        terms = eng.forward_backward(*dbatch).cpu().numpy()
        tol = 2e-5 if step == 0 else 5e-4
        assert np.allclose(terms, G["s%d_terms" % step], rtol=tol, atol=0), (terms, G["s%d_terms" % step])
        assert np.allclose(terms, r["terms"], rtol=2e-5, atol=0)
        _assert_yolo_class(*_accuracy_class(eng, r["grads"], r64["grads"]))
        close = total = 0
        for name in eng.g:
            gs = eng.g[name].cpu().numpy().ravel()
            rms = float(G["s%d_g_norm/%s" % (step, name)]) / np.sqrt(gs.size)
            fl = 1e-6 * float(G["s%d_g_norm/model2_4.0.weight" % step])
            d = np.abs(gs[sample_indices(name, gs.size)] - G["s%d_g_samp/%s" % (step, name)])
            assert d.max() <= (1 + 2 * step) * rms + fl, name
            close += int((d <= (2e-2 if step == 0 else 0.2) * rms + fl).sum())
            total += d.size
        assert close >= (0.98 if step == 0 else 0.8) * total, (close, total)
        p_old, m_old, g_now = eng.flat_p.clone(), eng.flat_m.clone(), eng.flat_g.clone()
        eng.apply()
        b = g_now if step == 0 else 0.9 * m_old + g_now
        assert _rel(eng.flat_p, p_old - 1.0 * (g_now + 0.9 * b)) < 1e-6 and _rel(eng.flat_m, b) < 1e-6
        new = eng.state_dict()
        for name in eng.p:
            v = new[name].cpu().numpy().ravel()
            ref = G["s%d_p_samp/%s" % (step, name)]
            rms = float(G["s%d_g_norm/%s" % (step, name)]) / np.sqrt(v.size)
            assert np.abs(v[sample_indices(name, v.size)] - ref).max() <= (1 + 9 * step) * (4 * rms + 1e-5 * max(1.0, float(np.abs(ref).max()))), (step, name)
        for k in G.files:
            if k.startswith("s%d_stat/" % step):
                # step 1 starts lr = 1 x (step-0 gradient differences) away from the reference's trajectory: measured 1.7e-2 of the largest entry
                # (model1.4.running_mean); against the reference restarted from the engine's own state the statistics agree to 1e-7
                n = k.split("/", 1)[1]
                if step == 0:
                    assert np.allclose(new[n].cpu().numpy(), G[k], rtol=2e-5, atol=2e-6), k
                else:
                    assert np.abs(new[n].cpu().numpy() - G[k]).max() <= 5e-2 * np.abs(G[k]).max(), k
                assert np.allclose(new[n].cpu().numpy(), r["stats"][n].numpy(), rtol=2e-5, atol=2e-6), k
        sd = {k: v.cpu() for k, v in new.items()}
    assert int(new["model0.bn1.num_batches_tracked"]) == 2 and int(new["model0.layer3.0.bn1.num_batches_tracked"]) == int(sd0["model0.layer3.0.bn1.num_batches_tracked"])
    for k, v in sd0.items():
        if k.startswith("model0.layer3"):
            assert new[k].dtype == v.dtype and torch.equal(new[k].cpu(), v), k            # built, never run, never trained
    assert set(new) == {k for k, _ in golden.keys["yolo_posenet"]}


def _engine_masks(eng):
    """The branch every ReLU / LeakyReLU and max pool of the engine's last step took, keyed like yolo_reference.forward's `forced`.
    An activation's mask is what pn_bn_train_backward multiplies by: out > 0 of the stored output where a residual went in, otherwise the
    sign of the forward's own expression recomputed from the conv output (t_bn_affine = fma(fp32((x - mean) invstd), gamma, beta), whose
    sign is that of the exact fp64 value of b gamma + beta); the two readings must agree."""
    from popnet_amd.train import ACT_NONE
    masks = {}
    for key, val in eng.A.items():
        if key.startswith("mp:"):
            masks[key] = val[1].cpu().long()
        elif key.startswith("bn:") and val[4] != ACT_NONE:
            x, y, mean, invstd, _ = val
            name = key[3:]
            out = eng._bufs[("a:" + name, tuple(x.shape))].cpu()
            if y is None:                                                      # no residual: the backward recomputes the sign
                c = (1, -1, 1, 1)
                b = (x.cpu() - mean.cpu().view(c)) * invstd.cpu().view(c)         # fp32 like the kernel: two roundings
                z = b.double() * eng.p[name + ".weight"].cpu().double().view(c) + eng.p[name + ".bias"].cpu().double().view(c)
                assert torch.equal(out > 0, z > 0), (name, int(((out > 0) != (z > 0)).sum()))
            masks[key] = out > 0
    return masks


def _mask_differences(masks, own):
    """-> {key: elements where the engine's branch differs from an unforced fp64 evaluation's}"""
    assert set(masks) == set(own), sorted(set(masks) ^ set(own))
    return {k: int((masks[k] != own[k].to(masks[k].dtype)).sum()) for k in masks}


@pytest.mark.parametrize("B,H,W", [(3, 96, 128), (2, 224, 224)])
def test_engine_gradients_strict_against_mask_forced_fp64(gpu, golden, B, H, W):
    """Settles what _assert_yolo_class's bars stand for.  The fp64 step re-run with every ReLU / LeakyReLU mask and max-pool argmax
    of the engine's own step (yolo_reference.forward(forced=...)) computes exactly the function that run differentiated; against it
    the engine's step-0 gradients meet the strict bar of the rtpose training (test_gpu_train.py: 1e-4 per tensor plus _floor; in fact 5e-5),
    the loss terms agree to 1e-5 and the BatchNorm running statistics to 2e-5.  So the 4-5e-3 between the engine and unforced fp64 autograd is
    the mask elements that land differently (counted and printed here: a nonzero count wherever the unforced gap exceeds the strict bar),
    not an arithmetic defect of any kernel.  Measured (gradient error per tensor, median / worst): 3 x 96 x 128 forced 1.2e-5 / 1.7e-5,
    unforced 4.1e-3 / 7.0e-3 from 1 differing element of 3 041 280 (model1.4); 2 x 224 x 224 forced 1.4e-5 / 1.9e-5, unforced 5.8e-3 /
    7.7e-3 from 12 of 8 279 040 (9 activation signs, 3 argmaxes of model2_1's pool)."""
    from test_gpu_train import REL, _floor
    eng = _engine(golden, gpu)
    sd = state_dict_from_keys(golden.keys["yolo_posenet"], seed=0)
    batch = _batch(B=B, H=H, W=W)
    terms = eng.forward_backward(*[b.to(gpu) for b in batch]).cpu().numpy()
    masks = _engine_masks(eng)
    assert len(masks) == 1 + 2 + 2 * 7 + 4 + 3                              # stem ReLU, 2 pools, 7 blocks x 2 ReLU, model1, model2_x
    own = {}
    r64 = yr.train_step(_f64(sd), *[b.double() for b in batch], dtype=torch.float64, record=own)
    f64 = yr.train_step(_f64(sd), *[b.double() for b in batch], dtype=torch.float64, forced=masks)
    flips = _mask_differences(masks, own)
    assert np.allclose(terms, f64["terms"], rtol=1e-5, atol=0), (terms, f64["terms"])
    new = eng.state_dict()
    for k, v in f64["stats"].items():
        assert np.allclose(new[k].cpu().numpy(), v.numpy(), rtol=2e-5, atol=2e-6), k
    floor = _floor(f64["grads"])
    forced_err, free_err = {}, {}
    for name, g in f64["grads"].items():
        e = eng.g[name].double().cpu()
        ref = float(g.norm())
        err = float((e - g).norm())
        assert err <= REL * ref + floor * np.sqrt(g.numel()), (name, err, ref)
        if ref > 100 * floor * np.sqrt(g.numel()):
            forced_err[name] = err / ref
            free_err[name] = float((e - r64["grads"][name]).norm()) / float(r64["grads"][name].norm())
    worst = max(forced_err, key=forced_err.get)
    print("\nyolo %dx%dx%d: mask-forced fp64 median %.2e, worst %.2e (%s); unforced fp64 median %.2e, worst %.2e; mask elements "
          "differing from unforced fp64: %d of %d (%s)" % (B, H, W, np.median(list(forced_err.values())), forced_err[worst], worst,
                                                         np.median(list(free_err.values())), max(free_err.values()), sum(flips.values()),
                                                         sum(m.numel() for m in masks.values()), {k: v for k, v in flips.items() if v}))
    assert forced_err[worst] < 5e-5, (worst, forced_err[worst])
    if max(free_err.values()) > REL:
        assert sum(flips.values()) > 0, "the unforced gap exceeds the strict bar with every mask equal: not flips"


def test_engine_plain_loss_terms_equal_reference_golden(gpu, golden):
    eng = _engine(golden, gpu, rarity_weight=False)
    img, prior, conf, coord, _ = [b.to(gpu) for b in _batch()]
    terms = eng.forward_backward(img, prior, conf, coord).cpu().numpy()
    assert np.allclose(terms, G["s0_plain_terms"], rtol=2e-5, atol=0), (terms, G["s0_plain_terms"])
    sd = state_dict_from_keys(golden.keys["yolo_posenet"], seed=0)
    batch = _batch()
    r = yr.train_step(sd, *batch[:4])
    r64 = yr.train_step(_f64(sd), *[b.double() for b in batch[:4]], dtype=torch.float64)
    _assert_yolo_class(*_accuracy_class(eng, r["grads"], r64["grads"]))


def test_engine_refuses_other_precisions(gpu, golden):
    with pytest.raises(ValueError):
        _engine(golden, gpu, precision="bf16x3")


def test_reference_trainer_body_runs_with_import_swaps_only(gpu, golden):
    """The per-batch body of the reference trainer (train_yolo_posenet_kdh3d_mpaug.py:157-192 (CR)): DataParallel(model).cuda(),
    model.train(), pred = model(img), yolo_loss_fgweight_poseweight, optimizer.zero_grad(), total_loss.backward(),
    torch.optim.SGD(lr 1, momentum 0.9, nesterov).step() -- with only the imports swapped to popnet_amd.  autograd orders the HIP
    primitives (network/_autograd.py).  Two steps against the reference's stored loss terms and BatchNorm statistics, step 0's gradients
    against the engine's (same kernels) and fp64 autograd."""
    from popnet_amd.network.yolo_posenet import YoloPoseNet                        # was: from lib.network.yolo_posenet import ...
    from popnet_amd.network.losses import yolo_loss_fgweight_poseweight            # was: from lib.network.losses import ...
    anchors = np.array(YOLO_ANCHORS)
    sd = state_dict_from_keys(golden.keys["yolo_posenet"], seed=0)
    model = YoloPoseNet(num_parts=15, input_dim=1, anchors=anchors)
    model.load_state_dict(sd)
    model = torch.nn.DataParallel(model, device_ids=[gpu.index]).cuda(gpu)
    params = [p for p in model.parameters() if p.requires_grad]
    optimizer = torch.optim.SGD(params, lr=1.0, momentum=0.9, weight_decay=0.0, nesterov=True)
    eng = _engine(golden, gpu)
    img, prior_map, prior_mask_conf, prior_mask_coord, prior_weight_map = [b.cuda(gpu) for b in _batch()]
    model.train()
    for step in range(2):
        pred = model(img)
        total_loss, saved_for_log = yolo_loss_fgweight_poseweight(pred, prior_map, prior_mask_conf, prior_mask_coord, prior_weight_map,
                                                                  model.module.num_parts, len(anchors))
        optimizer.zero_grad()
        total_loss.backward()
        terms = np.array([saved_for_log[n] for n in ("loss_prior", "loss_bbox", "loss_obj", "loss_selfpose")])
        assert np.allclose(terms, G["s%d_terms" % step], rtol=2e-5 if step == 0 else 5e-4, atol=0), (terms, G["s%d_terms" % step])
        if step == 0:
            eterms = eng.forward_backward(img, prior_map, prior_mask_conf, prior_mask_coord, prior_weight_map).cpu().numpy()
            assert np.allclose(terms, eterms, rtol=1e-5, atol=0)
            named = dict(model.module.named_parameters())
            assert set(eng.g) == {k for k in named if not k.startswith("model0.layer3")}
            assert all(named[k].grad is None for k in named if k.startswith("model0.layer3"))
            grads = {k: named[k].grad.detach().cpu() for k in eng.g}
            batch = _batch()
            r = yr.train_step(sd, *batch)
            r64 = yr.train_step(_f64(sd), *[b.double() for b in batch], dtype=torch.float64)
            _assert_yolo_class(*_accuracy_class(_Grads(grads), r["grads"], r64["grads"]))
            num = sum(float((grads[k].double() - eng.g[k].double().cpu()).norm()) ** 2 for k in grads)
            den = sum(float(eng.g[k].double().norm()) ** 2 for k in grads)
            assert (num / den) ** 0.5 < 1e-2, (num / den) ** 0.5             # same kernels; room for one mask flip of the head glue's rounding
        optimizer.step()
        for k in G.files:
            if k.startswith("s%d_stat/" % step):
                got = model.module.state_dict()[k.split("/", 1)[1]].cpu().numpy()
                assert (np.allclose(got, G[k], rtol=2e-5, atol=2e-6) if step == 0 else np.abs(got - G[k]).max() <= 5e-2 * np.abs(G[k]).max()), k
    assert int(model.module.model0.bn1.num_batches_tracked) == 2
    model.eval()                                                               # .eval() re-folds the trained weights into the inference net
    assert model(torch.zeros((1, 1, 224, 224), device=gpu)).shape == (1, 100, 14, 14)


def test_two_replicas_average_like_dataparallel(gpu, golden):
    """Per-replica BatchNorm statistics, averaged gradients: two engines on the halves of a batch against yolo_reference run the same way."""
    batch = _batch(seed=33, B=4, tseed=43)
    sd = state_dict_from_keys(golden.keys["yolo_posenet"], seed=0)
    halves = [[b[:2].contiguous() for b in batch], [b[2:].contiguous() for b in batch]]
    refs = [yr.train_step(sd, *hb)["grads"] for hb in halves]
    ref64 = [yr.train_step(_f64(sd), *[b.double() for b in hb], dtype=torch.float64)["grads"] for hb in halves]
    engs = [_engine(golden, gpu), _engine(golden, gpu)]
    for e, hb in zip(engs, halves):
        e.forward_backward(*[t.to(gpu) for t in hb])
    engs[0].flat_g.add_(engs[1].flat_g)          # the all-reduce (sum)
    engs[0].world = 2                            # -> grad_scale 1/2 inside pn_sgd_nesterov
    before = engs[0].flat_p.clone()
    engs[0]._check(engs[0].L.pn_sgd_nesterov(engs[0].ctx.handle, _p(engs[0].flat_p), _p(engs[0].flat_g), _p(engs[0].flat_m), engs[0].flat_p.numel(), 1.0, 0.9, 0.0, 1, 0.5,
                                             None), "sgd")
    engs[0].flat_g.mul_(0.5)
    _assert_yolo_class(*_accuracy_class(engs[0], {k: (refs[0][k] + refs[1][k]) / 2 for k in refs[0]}, {k: (ref64[0][k] + ref64[1][k]) / 2 for k in ref64[0]}))
    assert _rel(engs[0].flat_p, before - 1.9 * engs[0].flat_g) < 1e-6


def test_checkpoint_round_trip_into_inference_and_decode(gpu, golden):
    from popnet_amd.network.yolo_posenet import YoloPoseNet
    from popnet_amd.utils.prior_pose_align import parse_prior_pose
    eng = _engine(golden, gpu)
    img, prior, conf, coord, weight = [b.to(gpu) for b in _batch(H=224, W=224)]
    for _ in range(2):
        eng.step(img, prior, conf, coord, weight)
    model = YoloPoseNet(15, input_dim=1).to(gpu)
    model.load_state_dict(eng.state_dict(prefix="module."))
    model.eval()
    model.precision = "fp32"
    out = model(img)
    assert out.shape == (3, 100, 14, 14) and bool(torch.isfinite(out).all())
    boxes, humans, vis = parse_prior_pose(out, YOLO_ANCHORS, 15, 224, 224, 3, 2, 0.35, 0.5)
    assert len(boxes) == len(humans) == 3


def test_train_script_on_a_fake_mpaug_dataset(gpu, tmp_path, capsys):
    """scripts/train_yolo_mpaug.py end to end on a fake MP-3DHP tree whose labels carry `bbox` and `pose_weight`: composed batches,
    prior targets, training steps, validation loss, `best_pose.pth` with the `module.` prefix, loaded by the inference module."""
    import importlib.util
    import json
    import random
    from popnet_amd import synth
    from popnet_amd.network.yolo_posenet import YoloPoseNet
    d = str(tmp_path)
    for sub in ("img", "seg", "bg"):
        os.makedirs(os.path.join(d, sub))
    rng = np.random.default_rng(8)
    H, W = 320, 240
    ann_files = []
    for ii in range(5):
        ann = {"intrinsics": {"fx": 504.1, "fy": 504.0, "cx": 231.7, "cy": 320.6}}
        for f in range(4):
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
    spec = importlib.util.spec_from_file_location("train_yolo_mpaug", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "train_yolo_mpaug.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    random.seed(2)
    best = mod.main(["--train-annotations"] + ann_files + ["--val-annotations"] + ann_files[:2] + ["--image-dir", os.path.join(d, "img"), "--bg-file", os.path.join(d, "bg.json"),
                    "--bg-dir", os.path.join(d, "bg"), "--seg-dir", os.path.join(d, "seg"), "--output-dir", os.path.join(d, "out"), "--batch-size", "2", "--lr", "0.01",
                    "--epochs", "1", "--print-freq", "1", "--seed", "2"])
    out = capsys.readouterr().out
    assert "val loss" in out and np.isfinite(best), out
    sd = torch.load(os.path.join(d, "out", "best_pose.pth"), map_location="cpu")
    assert all(k.startswith("module.") for k in sd) and len(sd) == 223
    model = YoloPoseNet(15, input_dim=1).to(gpu)
    model.load_state_dict(sd)
    model.eval()
    assert model(torch.zeros((1, 1, 224, 224), device=gpu)).shape == (1, 100, 14, 14)
    # the dataset path: boxes scaled like Resize, a missing key is a clear error
    from popnet_amd import targets
    ts = targets.MPAugTrainSet(os.path.join(d, "img"), ann_files, os.path.join(d, "bg.json"), os.path.join(d, "bg"), os.path.join(d, "seg"), device=gpu, shuffle=False)
    *_, n_persons, boxes, pw = ts.batch([0], with_boxes=True)
    assert boxes.dtype == torch.float64 and pw.dtype == torch.float64 and boxes.shape[-1] == 4 and len(ts.batch([0])) == 7
    json.dump({"intrinsics": {}, "x.npy": [{"2d_joints": np.zeros((15, 2)).tolist(), "3d_joints": np.zeros((15, 3)).tolist()}]}, open(os.path.join(d, "nobox.json"), "w"))
    np.save(os.path.join(d, "img", "x.npy"), np.ones((H, W), np.float16))
    np.save(os.path.join(d, "seg", "x.npy"), np.zeros((H, W), np.uint8))
    bad = targets.MPAugTrainSet(os.path.join(d, "img"), [os.path.join(d, "nobox.json")], os.path.join(d, "bg.json"), os.path.join(d, "bg"), os.path.join(d, "seg"), device=gpu)
    with pytest.raises(KeyError, match="bbox"):
        bad.batch([0], with_boxes=True)
