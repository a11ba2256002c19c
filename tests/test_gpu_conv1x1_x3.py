"""pn_conv1x1_x3_forward / _dgrad / _wgrad (csrc/conv1x1_x3.hip: the split-bf16 1x1 convolutions of A2JTrainEngine(precision="bf16x3")) against
fp64 of their definition on the operands read, at the smallest shapes that still break things (tests/conv1x1_x3_cases.py GPU_CASES; the census
in tests/test_conv1x1_x3_plan.py shows they reach every plan class of the trainer's shapes).

Per case and role: forward with bias on / off and accumulate on / off, data gradient with accumulate on / off, weight gradient with and
without the bias gradient -- each output NaN-prefilled inside a sentinel-guarded buffer, each launch repeated once for identical bits.
Allowances: forward / data gradient NR.conv_fwd_ref / NR.conv_dgrad_ref (ks = 1, x3 = True: n U S, n = 3 K + bias + accumulate); weight
gradient conv1x1_x3_reference.wgrad_ref (depth 3 x per_slice + slices from pn_conv1x1_x3_plan_info).  Integer probes ([-3, 3]: every split
exact, every sum below 2^24) must equal fp64 bit for bit.  The allowance can reject: references without the `hi lo` term, without the `lo hi`
term and with a channel shifted are compared, with nothing launched, against the outputs the accuracy runs produced."""
import numpy as np
import pytest
import torch

import conv1x1_x3_cases as CC
import conv1x1_x3_reference as CR
import nchw_layer_reference as NR
from test_gpu_train_nchw_layers import SENT, _4d, _bad, _d, _Out, _p

pytestmark = pytest.mark.gpu

PN_ERR_INVALID = -1
IDS = ["%dx%dx%dx%d_to_%d" % (N, Cin, h, w, Cout) for N, Cin, (h, w), Cout in CC.GPU_CASES]
REJECT_CASES = [c for c in CC.GPU_CASES if c in ((2, 64, (8, 12), 256), (3, 40, (5, 7), 72))]     # K small enough that one lo term outweighs n U S
_RUNS = {}


def _ctx(gpu, cache=False):
    from popnet_amd import _lib
    L, ctx = _lib.lib(), _lib.Context(gpu.index)
    ctx.check(L.pn_train_pack_cache(ctx.handle, 1 if cache else 0), "pn_train_pack_cache")
    return L, ctx, _lib.current_stream_ptr(gpu)


def _operands(case, integer, seed):
    N, Cin, (h, w), Cout = case
    shapes = {"x": (N, Cin, h, w), "w": (Cout, Cin, 1, 1), "b": (Cout,), "dy": (N, Cout, h, w), "y0": (N, Cout, h, w), "dx0": (N, Cin, h, w)}
    g = torch.Generator().manual_seed(seed)
    if integer:
        return {k: NR.integer_operand(shp, seed * 10 + i).float() for i, (k, shp) in enumerate(shapes.items())}
    return {k: torch.randn(shp, generator=g) * (1.0 / np.sqrt(Cin) if k == "w" else 1.0) for k, shp in shapes.items()}


def _run(gpu, case, integer=False):
    """Every launch of one case, once per process: -> (reports [(entry, label, what, report)], kept outputs, operands in float64, plans)"""
    key = (case, integer)
    if key in _RUNS:
        return _RUNS[key]
    N, Cin, (h, w), Cout = case
    HW = h * w
    L, ctx, s = _ctx(gpu)
    o = _operands(case, integer, seed=N + Cin + HW + Cout + (1 if integer else 0))
    dev = {k: v.to(gpu) for k, v in o.items()}
    d64 = {k: v.double() for k, v in o.items()}
    plans = {role: CC.plan(NR.plan_context(True), role, N, Cin, HW, Cout) for role in CC.ROLES}
    res, kept = [], {}

    def check(entry, role, what, launch, shape, fill, r, a):
        out = _Out(shape, gpu, fill)
        ctx.check(launch(out.t), entry + " " + what)
        torch.cuda.synchronize(gpu)
        assert out.guards_intact(), "%s %s wrote outside its output" % (entry, what)
        again = _Out(shape, gpu, fill)
        ctx.check(launch(again.t), entry + " " + what + " (again)")
        torch.cuda.synchronize(gpu)
        assert torch.equal(out.t.view(torch.int32), again.t.view(torch.int32)), "%s %s: two calls differ" % (entry, what)
        if integer:
            assert float(r.abs().max()) < 2 ** 24
            a = torch.zeros_like(r)
        rep = NR.compare(_4d(_d(out.t)), _4d(r), _4d(a))
        res.append((entry, plans[role]["kernel"] if role else "", what, rep))
        kept[(entry, what)] = _d(out.t)

    x, wt, b, dy = _p(dev["x"]), _p(dev["w"]), _p(dev["b"]), _p(dev["dy"])
    for with_b in (1, 0):
        for acc in (0, 1):
            check("pn_conv1x1_x3_forward", "forward", "y %s conv%s" % ("+=" if acc else "=", " + bias" if with_b else ""),
                  lambda y, with_b=with_b, acc=acc: L.pn_conv1x1_x3_forward(ctx.handle, x, wt, b if with_b else None, _p(y), N, Cin, HW, Cout, acc, s),
                  o["y0"].shape, dev["y0"] if acc else float("nan"),
                  *NR.conv_fwd_ref(d64["x"], d64["w"], d64["b"] if with_b else None, d64["y0"] if acc else None, 1, 0, True))
    for acc in (0, 1):
        check("pn_conv1x1_x3_dgrad", "dgrad", "dx +=" if acc else "dx =",
              lambda dx, acc=acc: L.pn_conv1x1_x3_dgrad(ctx.handle, dy, wt, _p(dx), N, Cin, HW, Cout, acc, s),
              o["dx0"].shape, dev["dx0"] if acc else float("nan"),
              *NR.conv_dgrad_ref(d64["dy"], d64["w"], d64["dx0"] if acc else None, tuple(o["dx0"].shape), 1, 0, True))
    for with_b in (1, 0):
        db = _Out(o["b"].shape, gpu, float("nan") if with_b else SENT)
        check("pn_conv1x1_x3_wgrad", "wgrad", "dw" + (" (with dbias)" if with_b else ""),
              lambda dw, with_b=with_b: L.pn_conv1x1_x3_wgrad(ctx.handle, x, dy, _p(dw), _p(db.t) if with_b else None, N, Cin, HW, Cout, s),
              o["w"].shape, float("nan"), *CR.wgrad_ref(d64["x"], d64["dy"], plans["wgrad"]))
        assert db.guards_intact()
        if with_b:
            r, a = NR.conv_dbias_ref(d64["dy"])
            rep = NR.compare(_4d(_d(db.t)), _4d(r), _4d(torch.zeros_like(r) if integer else a))
            res.append(("pn_conv1x1_x3_wgrad", "", "dbias", rep))
        else:
            assert bool((db.t == SENT).all()), "dbias written although NULL was passed"
    _RUNS[key] = (res, kept, d64, plans)
    return _RUNS[key]


@pytest.mark.parametrize("case", CC.GPU_CASES, ids=IDS)
def test_within_fp64_allowance_inside_the_output_and_deterministic(gpu, case):
    res, _, _, plans = _run(gpu, case)
    print("\nCONV1X1 X3 %s: %s" % (case, "; ".join("%s %s %.3f" % (e[14:], what, rep["worst"]) for e, _, what, rep in res)))
    assert all(p["kernel"] in CC.SPLIT_KERNELS for p in plans.values())
    bad = _bad([r + (False,) for r in res])
    assert not bad, "\n".join(bad)
    assert len(res) == 9


@pytest.mark.parametrize("case", CC.GPU_CASES, ids=IDS)
def test_integer_probes_are_bit_exact(gpu, case):
    res, _, _, _ = _run(gpu, case, integer=True)
    bad = _bad([r + (True,) for r in res])
    assert not bad, "\n".join(bad)
    assert len(res) == 9


@pytest.mark.parametrize("case", REJECT_CASES, ids=["%dx%dx%dx%d_to_%d" % (N, Cin, h, w, Cout) for N, Cin, (h, w), Cout in REJECT_CASES])
def test_the_allowance_rejects_a_missing_term_and_a_shifted_channel(gpu, case):
    """Nothing is launched: the outputs of the accuracy run again, against the right reference (passes) and three wrong ones per role."""
    _, kept, d, plans = _run(gpu, case)
    n_bad = lambda got, r, a: NR.compare(_4d(got), _4d(r), _4d(a))["n_bad"]          # noqa: E731
    wrong = ({"drop": "hi lo"}, {"drop": "lo hi"}, {"shift": 1})
    y = kept[("pn_conv1x1_x3_forward", "y = conv + bias")]
    dx = kept[("pn_conv1x1_x3_dgrad", "dx =")]
    dw = kept[("pn_conv1x1_x3_wgrad", "dw")]
    assert n_bad(y, *CR.fwd_ref(d["x"], d["w"], d["b"], None)) == 0
    assert n_bad(dx, *CR.dgrad_ref(d["dy"], d["w"], None)) == 0
    assert n_bad(dw, *CR.wgrad_ref(d["x"], d["dy"], plans["wgrad"])) == 0
    counts = []
    for kw in wrong:
        counts.append((n_bad(y, *CR.fwd_ref(d["x"], d["w"], d["b"], None, **kw)), n_bad(dx, *CR.dgrad_ref(d["dy"], d["w"], None, **kw)),
                       n_bad(dw, *CR.wgrad_ref(d["x"], d["dy"], plans["wgrad"], **kw))))
    print("\nCONV1X1 X3 wrong references %s: elements over the allowance (forward, dgrad, wgrad) -- no hi lo: %s, no lo hi: %s, channel shifted: %s" % (
        (case,) + tuple(counts)))
    assert all(c > 0 for row in counts for c in row), counts


@pytest.mark.parametrize("mode", ["cache_off", "cache_stale", "cache_refreshed"])
def test_forward_and_dgrad_read_the_weights_pn_adam_left(gpu, mode):
    """cache_off: packed on every call.  cache_stale: pn_adam marks the cached packs stale and the next call repacks.  cache_refreshed: the
    engine's order -- pn_train_pack_refresh rebuilds every cached pack (the plain and the transposed one) in its one launch."""
    N, Cin, (h, w), Cout = case = (3, 40, (5, 7), 72)
    HW = h * w
    L, ctx, s = _ctx(gpu, cache=mode != "cache_off")
    o = _operands(case, False, seed=5)
    dev = {k: v.to(gpu) for k, v in o.items()}
    wt = dev["w"].clone()
    g, m, v = torch.randn_like(wt), torch.zeros_like(wt), torch.zeros_like(wt)

    def both():
        y, dx = _Out(o["y0"].shape, gpu, float("nan")), _Out(o["dx0"].shape, gpu, float("nan"))
        ctx.check(L.pn_conv1x1_x3_forward(ctx.handle, _p(dev["x"]), _p(wt), _p(dev["b"]), _p(y.t), N, Cin, HW, Cout, 0, s), "forward")
        ctx.check(L.pn_conv1x1_x3_dgrad(ctx.handle, _p(dev["dy"]), _p(wt), _p(dx.t), N, Cin, HW, Cout, 0, s), "dgrad")
        torch.cuda.synchronize(gpu)
        assert y.guards_intact() and dx.guards_intact()
        w64 = _d(wt)
        ry, ay = NR.conv_fwd_ref(o["x"].double(), w64, o["b"].double(), None, 1, 0, True)
        rx, ax = NR.conv_dgrad_ref(o["dy"].double(), w64, None, tuple(o["dx0"].shape), 1, 0, True)
        return NR.compare(_d(y.t), ry, ay), NR.compare(_d(dx.t), rx, ax), _d(y.t)

    a, b, y_old = both()
    assert a["n_bad"] == 0 and b["n_bad"] == 0
    w_old = wt.clone()
    ctx.check(L.pn_adam(ctx.handle, _p(wt), _p(g), _p(m), _p(v), wt.numel(), 0.05, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, s), "pn_adam")
    torch.cuda.synchronize(gpu)
    assert float((wt - w_old).abs().min()) > 0.01                     # Adam's first step moves every weight by lr
    if mode == "cache_refreshed":
        ctx.check(L.pn_train_pack_refresh(ctx.handle, s), "pn_train_pack_refresh")
    a, b, y_new = both()
    assert a["n_bad"] == 0 and b["n_bad"] == 0, (mode, a, b)
    assert float((y_new - y_old).abs().max()) > 0.01                  # (the old weights' output is far outside the allowance)
    if mode == "cache_refreshed":                                      # the refreshed packs are used as they are, and stay right on a second use
        a, b, _ = both()
        assert a["n_bad"] == 0 and b["n_bad"] == 0


def test_refusals_return_invalid_and_launch_nothing(gpu):
    L, ctx, s = _ctx(gpu)
    N, Cin, HW, Cout = 2, 8, 12, 8
    x, wt, dy = torch.randn(N, Cin, HW, device=gpu), torch.randn(Cout, Cin, device=gpu), torch.randn(N, Cout, HW, device=gpu)
    y, dx, dw = (_Out(shp, gpu, SENT) for shp in ((N, Cout, HW), (N, Cin, HW), (Cout, Cin)))
    h = ctx.handle
    dims = [(0, Cin, HW, Cout), (N, 0, HW, Cout), (N, Cin, 0, Cout), (N, Cin, HW, 0), (-1, Cin, HW, Cout), (N, Cin, -3, Cout)]
    calls = []
    for d in dims:
        calls.append(L.pn_conv1x1_x3_forward(h, _p(x), _p(wt), None, _p(y.t), *d, 0, s))
        calls.append(L.pn_conv1x1_x3_dgrad(h, _p(dy), _p(wt), _p(dx.t), *d, 0, s))
        calls.append(L.pn_conv1x1_x3_wgrad(h, _p(x), _p(dy), _p(dw.t), None, *d, s))
    d = (N, Cin, HW, Cout)
    for args in ((None, _p(wt), None, _p(y.t)), (_p(x), None, None, _p(y.t)), (_p(x), _p(wt), None, None)):
        calls.append(L.pn_conv1x1_x3_forward(h, *args, *d, 0, s))
    for args in ((None, _p(wt), _p(dx.t)), (_p(dy), None, _p(dx.t)), (_p(dy), _p(wt), None)):
        calls.append(L.pn_conv1x1_x3_dgrad(h, *args, *d, 0, s))
    for args in ((None, _p(dy), _p(dw.t), None), (_p(x), None, _p(dw.t), None), (_p(x), _p(dy), None, None)):
        calls.append(L.pn_conv1x1_x3_wgrad(h, *args, *d, s))
    assert calls == [PN_ERR_INVALID] * len(calls), calls
    assert L.pn_conv1x1_x3_forward(None, _p(x), _p(wt), None, _p(y.t), *d, 0, s) == PN_ERR_INVALID
    torch.cuda.synchronize(gpu)
    for out in (y, dx, dw):
        assert bool((out.buf == SENT).all()), "a refused call wrote"
    # and the same arguments, valid, are accepted
    ctx.check(L.pn_conv1x1_x3_forward(h, _p(x), _p(wt), None, _p(y.t), *d, 0, s), "forward")
    torch.cuda.synchronize(gpu)
    assert y.guards_intact() and bool(torch.isfinite(y.t).all()) and not bool((y.t == SENT).any())
