"""Every launch of the NCHW training engines (csrc/train.hip, csrc/train_yolo.hip; popnet_amd.train.TrainEngine in "fp32-nchw" / "bf16x3-nchw",
popnet_amd.train_yolo.YoloTrainEngine) against the fp64 references of tests/nchw_layer_reference.py, element by element.

(a) replays: test-only subclasses of the two engines override the primitive methods; each override copies what the call reads and what it
    accumulates into, pre-fills what it overwrites with NaN, calls the engine's own method, and compares every output element with the
    reference of that one launch on the operands the GPU actually read.  The calls forward_backward makes inline (pn_yolo_loss, pn_head_*,
    pn_slice_copy) are checked by a forwarding proxy around engine.L, which also records every pn_* entry the step called: a called entry
    without a check fails the test.  Exempt, with reasons: pn_train_ws_keep, pn_train_set_precision, pn_train_pack_cache (host-side switches:
    they launch nothing) and pn_train_pack_refresh (its packs have no readable output of their own; the second step, run after apply(),
    reads the refreshed packs in every tile convolution and data gradient, which are checked).
(b) a table of single primitives chosen with pn_train_conv_plan_info so that every kernel label the planner can return appears, on both sides
    of each threshold; outputs sit inside sentinel-filled buffers; every row asserts the labels it expects.
(c) small-integer operands: exact in fp32 and in bf16 hi planes, so the result must equal the integer reference bit for bit.
(d) coverage guard: the labels the engines' steps use at their training shapes (from the plan description alone) are among those checked.
The replay mixin also serves tests/test_gpu_train_a2j_layers.py (A2JTrainEngine): its _conv / _conv_bwd take the dilation that engine passes and
check pn_conv2d_*_dil under the literal labels FD / GD (the plan description does not cover the dilated entries); the table's last rows are ResNet-50's shapes.

The tall one- and three-column rows of (b) (106 x 1, 87 x 3) exceed the 56-row limit of the other rows on purpose: they are the only shapes at
which t_tile_geometry_x3 / t_tile_geometry_x3w refuse a map (their halo tile outgrows the LDS image); they hold ~300 pixels.  t_tile_geometry and
t_tile_geometry_wx3 cannot refuse any shape ((128 / TW + 2)(TW + 2) <= 390 <= 512 and HR HP <= 288 <= 344), so "generic because the geometry was
refused" does not exist for the fp32 tile kernels and the weight gradient; generic 3x3 launches come from Cin < 16, stride 2 and pad > 2."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import nchw_layer_reference as NR
import yolo_reference as yr
from helpers import G, SENT, _Out, state_dict_from_keys, train_case_inputs

pytestmark = pytest.mark.gpu

PN_ERR_INVALID = -1
EXEMPT = {"pn_train_ws_keep", "pn_train_set_precision", "pn_train_pack_cache", "pn_train_pack_refresh"}
CHECKED = {}                 # source ("replay <tag>" / "table <prec>") -> {kernel label}
CALLS = {}                   # replay tag -> {(which, Cin, Cout, ks, stride, pad, image rows // map rows, image columns // map columns)}
WORST = {}                   # (op kind, precision) -> worst |gpu - r| / allowance, for the report
TRAIN_SHAPES = {"yolo": (30, 224, 224), "rtpose": (32, 224, 224)}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _d(t):
    return None if t is None else t.detach().cpu().double()


def _4d(t):
    return t if t.dim() == 4 else t.reshape(1, 1, 1, -1)


def _exactly_stored(r):
    """Every element of the exact result is a float32 number: a correct kernel has no rounding to make, so worst == 0 is legitimate (the sum of a
    BatchNorm's input gradient over a channel, which is what the bias gradient of a convolution in front of a BatchNorm adds up, cancels to a few bits)."""
    return bool((r.to(torch.float32).to(torch.float64) == r).all())


def _note(kind, prec, rep, what=""):
    if "dbias" in what:
        kind += " (dbias)"
    WORST[(kind, prec)] = max(WORST.get((kind, prec), 0.0), rep["worst"])


# ---- (a) the replay ---------------------------------------------------------------------------------------------------------------
class _Proxy:
    """engine.L with every pn_* call recorded and the calls forward_backward makes inline checked."""
    def __init__(self, lib, eng):
        self._lib, self._eng = lib, eng

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("pn_"):
            return fn
        eng = self._eng
        inline = getattr(eng, "_inline_" + name, None)

        def call(*a):
            eng.called.add(name)
            if inline is None or eng.light:
                return fn(*a)
            return inline(fn, *a)
        return call


class _Checked:
    """Mixin in front of an engine class: see the module docstring, (a)."""
    def start_checks(self, tag, prec):
        self.tag, self.prec, self.x3 = tag, prec, prec == "bf16x3"
        self.hplan = NR.plan_context(self.x3)
        self.reports, self.called, self.checked, self.labels, self.calls = [], set(), set(), set(), set()
        self.flips, self.light, self.img_hw, self.kept = 0, False, None, {}
        self.L = _Proxy(self.L, self)

    # -- bookkeeping
    def _cmp(self, entry, label, what, gpu, r, a, exact=False):
        torch.cuda.synchronize(self.device)
        rep = NR.compare(_4d(_d(gpu)), _4d(r), _4d(a))
        self.reports.append((entry, label, what, rep, exact or _exactly_stored(r)))
        self.checked.add(entry)
        if label:
            self.labels.add(label)
        _note(entry, self.prec, rep, what)
        return rep

    def _keep(self, key, *operands):
        """The operands of one comparison, for a test that re-runs it against a deliberately wrong reference (self.want: the keys to keep)."""
        if key in getattr(self, "want", ()) and key not in self.kept:
            self.kept[key] = operands

    def _plan(self, which, x_shape, Cout, ks, stride, pad):
        N, Cin, H, W = x_shape
        p = NR.plan(self.hplan, which, N, Cin, H, W, Cout, ks, stride, pad)
        self.calls.add((which, Cin, Cout, ks, stride, pad, self.img_hw[0] // H, self.img_hw[1] // W))
        return p

    def _view(self, ptr, N, ld, Cc, HW):
        """The [N, Cc, HW] tensor a raw pointer argument with an image stride of ld channels addresses (a slice of one of the engine's tensors)."""
        addr = ptr.value if isinstance(ptr, C.c_void_p) else ptr
        more = list(getattr(self, "_anchors", {}).values()) + [t for t in (getattr(self, "_scale", None),) if t is not None]      # A2JTrainEngine's
        for t in list(self._bufs.values()) + list(self._batch) + [self.loss_terms] + more:
            off = addr - t.data_ptr()
            if t.dtype == torch.float32 and 0 <= off < t.numel() * 4:
                assert off % 4 == 0 and off // 4 + (N - 1) * ld * HW + Cc * HW <= t.numel()
                return torch.as_strided(t.view(-1), (N, Cc, HW), (ld * HW, HW, 1), off // 4)
        raise AssertionError("pointer outside the engine's tensors")

    # -- the primitive methods
    def _conv(self, name, x, ks, stride=1, pad=0, dil=1):
        """dil > 1 (A2JTrainEngine only): pn_conv2d_forward_dil, the same definition with the taps dil apart."""
        if self.img_hw is None:
            self.img_hw = tuple(x.shape[2:])
        w, b = self.p[name + ".weight"], self.p.get(name + ".bias")
        N, Cin, H, W = x.shape
        Ho, Wo = (H + 2 * pad - dil * (ks - 1) - 1) // stride + 1, (W + 2 * pad - dil * (ks - 1) - 1) // stride + 1
        self._buf("c:" + name, (N, w.shape[0], Ho, Wo)).fill_(float("nan"))
        if dil != 1:
            y = super()._conv(name, x, ks, stride, pad, dil=dil)
            r, a = NR.conv_fwd_ref(_d(x), _d(w), _d(b), None, stride, pad, False, dilation=dil)
            self._cmp("pn_conv2d_forward_dil", FD, name, y, r, a)
            self._keep(("forward", name), _d(y), _d(x), _d(w), _d(b), stride, pad, dil)
            return y
        y = super()._conv(name, x, ks, stride, pad)
        p = self._plan("forward", x.shape, w.shape[0], ks, stride, pad)
        r, a = NR.conv_fwd_ref(_d(x), _d(w), _d(b), None, stride, pad, NR.is_x3(p["kernel"]))
        self._cmp("pn_conv2d_forward", p["kernel"], name, y, r, a)
        return y

    def _conv_bwd(self, name, dy, ks, stride=1, pad=0, dx=None, accumulate=False, need_dx=True, dil=1):
        """dil > 1 (A2JTrainEngine only): pn_conv2d_wgrad_dil and pn_conv2d_dgrad_dil.  The weight gradient's depth is pixels per slice + slices
        with the slices of NR.dil_wgrad_plan (the launch code's own t_wgrad_pixel_slices, read through an undilated call of the same P, Kdim, Cout)."""
        x, w = self.A["x:" + name], self.p[name + ".weight"]
        kw = {"dil": dil} if dil != 1 else {}
        if self.light and not (need_dx and stride == 1 and ks == 3):
            return super()._conv_bwd(name, dy, ks, stride, pad, dx=dx, accumulate=accumulate, need_dx=need_dx, **kw)
        if need_dx and dx is None:
            dx = self._buf("dx:" + name, x.shape)
        prev = _d(dx) if (need_dx and accumulate) else None
        if need_dx and not accumulate:
            dx.fill_(float("nan"))
        self.g[name + ".weight"].fill_(float("nan"))
        if name + ".bias" in self.g:
            self.g[name + ".bias"].fill_(float("nan"))
        out = super()._conv_bwd(name, dy, ks, stride, pad, dx=dx, accumulate=accumulate, need_dx=need_dx, **kw)
        xd, dyd = _d(x), _d(dy)
        if not self.light:
            if dil != 1:
                p = NR.dil_wgrad_plan(self.hplan, x.shape[0], x.shape[1], dy.shape[2], dy.shape[3], w.shape[0])
                entry, label = "pn_conv2d_wgrad_dil", GD
            else:
                p = self._plan("wgrad", x.shape, w.shape[0], ks, stride, pad)
                entry, label = "pn_conv2d_wgrad", p["kernel"]
            r, a = NR.conv_wgrad_ref(xd, dyd, ks, stride, pad, p, dilation=dil)
            self._cmp(entry, label, name + " dw", self.g[name + ".weight"], r, a)
            if name + ".bias" in self.g:
                r, a = NR.conv_dbias_ref(dyd)
                self._cmp(entry, "", name + " dbias", self.g[name + ".bias"], r, a)
        if need_dx and dil != 1:
            r, a = NR.conv_dgrad_ref(dyd, _d(w), prev, tuple(x.shape), stride, pad, False, dilation=dil)
            self._cmp("pn_conv2d_dgrad_dil", FD, name + " dx", out, r, a)
        elif need_dx:
            which = "dgrad" if stride == 1 else "dgrad_strided"
            p = self._plan(which, x.shape, w.shape[0], ks, stride, pad)
            r, a = NR.conv_dgrad_ref(dyd, _d(w), prev, tuple(x.shape), stride, pad, NR.is_x3(p["kernel"]))
            self._cmp("pn_conv2d_" + which, p["kernel"], name + " dx", out, r, a)
            self._keep(("dgrad", name), _d(out), dyd, _d(w), prev, tuple(x.shape), stride, pad, NR.is_x3(p["kernel"]))
        return out

    def _bn(self, name, x, act, res=None):
        if self.light:
            return super()._bn(name, x, act, res)
        rm, rv = _d(self.stats[name + ".running_mean"]), _d(self.stats[name + ".running_var"])
        self._buf("a:" + name, x.shape).fill_(float("nan"))
        y = super()._bn(name, x, act, res)
        _, _, mean, invstd, _ = self.A["bn:" + name]
        ref = NR.bn_stats_ref(_d(x), rm, rv)
        got = {"mean": mean, "invstd": invstd, "running_mean": self.stats[name + ".running_mean"], "running_var": self.stats[name + ".running_var"]}
        for k, (r, a) in ref.items():
            self._cmp("pn_bn_train_forward", "", "%s %s" % (name, k), got[k], r, a)
        args = (_d(x), _d(mean), _d(invstd), _d(self.p[name + ".weight"]), _d(self.p[name + ".bias"]), _d(res), act)
        r, a = NR.bn_apply_ref(*args)
        self._cmp("pn_bn_train_forward", "", name + " y", y, r, a)
        self._keep(("bn", name), _d(y), *args)
        return y

    def _bn_bwd(self, name, dy, dres=None, dres_accumulate=False):
        if self.light:
            return super()._bn_bwd(name, dy, dres, dres_accumulate)
        x, _, mean, invstd, act = self.A["bn:" + name]
        mask = _d(self._bufs[("a:" + name, tuple(x.shape))]) > 0
        prev = _d(dres) if (dres is not None and dres_accumulate) else None
        if dres is not None and not dres_accumulate:
            dres.fill_(float("nan"))
        self._buf("dc:" + name, x.shape).fill_(float("nan"))
        dx = super()._bn_bwd(name, dy, dres, dres_accumulate)
        torch.cuda.synchronize(self.device)
        args = (_d(x), _d(dy), mask, _d(mean), _d(invstd), _d(self.p[name + ".weight"]), act, _d(self.g[name + ".bias"]))
        ref = NR.bn_bwd_ref(*args, dres_prev=prev)
        got = {"dbeta": self.g[name + ".bias"], "dgamma": self.g[name + ".weight"], "dx": dx, "dres": dres}
        for k, (r, a) in ref.items():
            if got[k] is not None:
                self._cmp("pn_bn_train_backward", "", "%s %s" % (name, k), got[k], r, a, exact=k == "dres")
        self.flips += NR.mask_disagreements(_d(dx), *args)
        return dx

    def _pool(self, name, x):
        if self.light:
            return super()._pool(name, x)
        y = super()._pool(name, x)
        self._cmp("pn_avgpool3s2_forward", "", "pool " + name, y, *NR.avgpool_fwd_ref(_d(x)))
        return y

    def _pool_bwd(self, name, dy):
        if self.light:
            return super()._pool_bwd(name, dy)
        dx = super()._pool_bwd(name, dy)
        self._cmp("pn_avgpool3s2_backward", "", "pool_bwd " + name, dx, *NR.avgpool_bwd_ref(_d(dy), *dx.shape[2:]))
        return dx

    def _maxpool(self, name, x, k, stride, pad):
        if self.light:
            return super()._maxpool(name, x, k, stride, pad)
        y = super()._maxpool(name, x, k, stride, pad)
        yr_, ir = NR.maxpool_fwd_ref(x.cpu(), k, stride, pad)
        idx = self.A["mp:" + name][1]
        z = torch.zeros(yr_.shape, dtype=torch.float64)
        self._cmp("pn_maxpool_forward", "", "maxpool %s y" % name, y, yr_.double(), z, exact=True)
        self._cmp("pn_maxpool_forward", "", "maxpool %s idx" % name, idx, ir.double(), z, exact=True)
        return y

    def _maxpool_bwd(self, name, dy):
        if self.light:
            return super()._maxpool_bwd(name, dy)
        shape, idx = self.A["mp:" + name][:2]
        dx = super()._maxpool_bwd(name, dy)
        self._cmp("pn_maxpool_backward", "", "maxpool_bwd " + name, dx, *NR.maxpool_bwd_ref(_d(dy), idx.cpu(), shape[2], shape[3]), exact=True)
        return dx

    def apply(self):
        p, g, m, first = _d(self.flat_p), _d(self.flat_g), _d(self.flat_m), self.steps == 0
        super().apply()
        ref = NR.sgd_ref(p, g, m, self.lr, self.momentum, self.weight_decay, first, 1.0 / self.world)
        self._cmp("pn_sgd_nesterov", "", "parameters", self.flat_p, *ref["p"])
        self._cmp("pn_sgd_nesterov", "", "momentum", self.flat_m, *ref["buf"], exact=first)

    # -- the calls forward_backward makes inline (through the proxy)
    def _inline_pn_head_forward(self, fn, ctx, v, target, fg, kind, N, Cc, HW, s, out, out_ld, loss, stream):
        vv, tt = self._view(v, N, Cc, Cc, HW), self._view(target, N, Cc, Cc, HW)
        ff = self._view(fg, N, Cc, Cc, HW) if fg else None
        ss, oo, ll = self._view(s, N, Cc, Cc, HW), self._view(out, N, out_ld, Cc, HW), self._view(loss, 1, 1, 1, 1)
        ss.fill_(float("nan"))
        oo.fill_(float("nan"))
        rc = fn(ctx, v, target, fg, kind, N, Cc, HW, s, out, out_ld, loss, stream)
        rs, as_, ro, ao = NR.head_fwd_ref(_d(vv), kind)
        self._cmp("pn_head_forward", "", "sigmoid", ss, rs, as_)
        self._cmp("pn_head_forward", "", "out", oo, ro, ao)
        self._cmp("pn_head_forward", "", "loss", ll, *NR.head_loss_ref(_d(oo), _d(tt), _d(ff)))
        return rc

    def _inline_pn_head_backward(self, fn, ctx, s, target, fg, dextra, dextra_ld, kind, N, Cc, HW, dv, stream):
        ss, tt = self._view(s, N, Cc, Cc, HW), self._view(target, N, Cc, Cc, HW)
        ff = self._view(fg, N, Cc, Cc, HW) if fg else None
        de = self._view(dextra, N, dextra_ld, Cc, HW) if dextra else None
        dd = self._view(dv, N, Cc, Cc, HW)
        dd.fill_(float("nan"))
        rc = fn(ctx, s, target, fg, dextra, dextra_ld, kind, N, Cc, HW, dv, stream)
        self._cmp("pn_head_backward", "", "dv", dd, *NR.heads_bwd_ref(_d(ss), _d(tt), _d(ff), _d(de), kind))
        return rc

    def _inline_pn_slice_copy(self, fn, ctx, src, src_ld, dst, dst_ld, N, Cc, HW, accumulate, stream):
        sv, dv = self._view(src, N, src_ld, Cc, HW), self._view(dst, N, dst_ld, Cc, HW)
        prev = _d(dv) if accumulate else None
        if not accumulate:
            dv.fill_(float("nan"))
        rc = fn(ctx, src, src_ld, dst, dst_ld, N, Cc, HW, accumulate, stream)
        self._cmp("pn_slice_copy", "", "copy", dv, *NR.slice_copy_ref(_d(sv), prev), exact=not accumulate)
        return rc

    def _inline_pn_yolo_loss(self, fn, ctx, v, prior, mconf, mcoord, wmap, N, A, J, h, w, out, terms, dv, stream):
        Fc = A * (5 + 3 * J)
        vv, pr = self._view(v, N, Fc, Fc, h * w), self._view(prior, N, Fc, Fc, h * w)
        mk = [self._view(m, N, A, A, h * w) if m else None for m in (mconf, mcoord, wmap)]
        oo, dd, tt = self._view(out, N, Fc, Fc, h * w), self._view(dv, N, Fc, Fc, h * w), self._view(terms, 1, 4, 4, 1)
        oo.fill_(float("nan"))
        dd.fill_(float("nan"))
        rc = fn(ctx, v, prior, mconf, mcoord, wmap, N, A, J, h, w, out, terms, dv, stream)
        sh = lambda t, c: None if t is None else _d(t).view(N, c, h, w)       # noqa: E731
        ref = NR.yolo_loss_ref(sh(vv, Fc), sh(pr, Fc), sh(mk[0], A), sh(mk[1], A), sh(mk[2], A), A, J)
        self._cmp("pn_yolo_loss", "", "out", oo.view(N, Fc, h, w), *ref["out"])
        self._cmp("pn_yolo_loss", "", "dv", dd.view(N, Fc, h, w), *ref["dv"])
        self._cmp("pn_yolo_loss", "", "terms", tt, *ref["terms"])
        return rc


def _engine_class(base, mixin=_Checked):
    return type("Checked" + base.__name__, (mixin, base), {})


def _replay(golden, gpu, net, prec, B, H, W, rarity=True):
    """Two steps (the second after apply(), reading the refreshed packs); returns the checked engine."""
    tag = "%s_%s_%dx%dx%d%s" % (net, prec, B, H, W, "" if rarity else "_plain")
    if net == "yolo":
        from popnet_amd.train_yolo import YoloTrainEngine
        eng = _engine_class(YoloTrainEngine)(state_dict_from_keys(golden.keys["yolo_posenet"], seed=0), device=gpu, rarity_weight=rarity)
        batch = [torch.from_numpy(a).to(gpu) for a in (train_case_inputs(seed=21, B=B, H=H, W=W)[0],) + yr.yolo_case_targets(seed=41, B=B, H=H, W=W)]
        if not rarity:
            batch = batch[:4]
    else:
        from popnet_amd.train import TrainEngine
        eng = _engine_class(TrainEngine)(state_dict_from_keys(golden.keys["rtpose_light3d"], seed=0), device=gpu, precision=prec + "-nchw")
        batch = [torch.from_numpy(a).to(gpu) for a in train_case_inputs(seed=21, B=B, H=H, W=W)]
    eng.start_checks(tag, prec)
    eng._batch = batch
    eng.forward_backward(*batch)
    eng.apply()
    eng.light = True                    # second step: the launches that read a pack (tile forward convolutions and data gradients)
    eng.forward_backward(*batch)
    torch.cuda.synchronize(gpu)
    CHECKED["replay " + tag] = set(eng.labels)
    CALLS[tag] = set(eng.calls)
    return eng


def _bad(reports):
    return ["%s %s %s: worst %.3g, %d elements over, at (frame, channel, row, col, ratio) %s" % (e, lab, what, rep["worst"], rep["n_bad"], rep["where"])
            for e, lab, what, rep, _ in reports if rep["n_bad"]]


def _summary(reports):
    by = {}
    for e, _, _, rep, _ in reports:
        by[e] = max(by.get(e, 0.0), rep["worst"])
    return ", ".join("%s %.3f" % kv for kv in sorted(by.items()))


REPLAYS = [("yolo", "fp32", 3, 96, 128, True), ("yolo", "fp32", 3, 96, 128, False), ("yolo", "fp32", 2, 80, 112, True),
           ("rtpose", "fp32", 3, 72, 40, True), ("rtpose", "bf16x3", 3, 72, 40, True), ("rtpose", "fp32", 1, 104, 136, True),
           ("rtpose", "bf16x3", 1, 104, 136, True)]


@pytest.mark.parametrize("cfg", REPLAYS, ids=["%s_%s_%dx%dx%d%s" % (c[0], c[1], c[2], c[3], c[4], "" if c[5] else "_plain") for c in REPLAYS])
def test_every_launch_of_the_nchw_step_within_fp64_allowance(gpu, golden, cfg):
    t0 = time.time()
    eng = _replay(golden, gpu, *cfg)
    bad = _bad(eng.reports)
    print("\nNCHW LAYERS %s: %d checks; worst |gpu - r| / allowance per entry: %s" % (eng.tag, len(eng.reports), _summary(eng.reports)))
    print("NCHW LAYERS %s: kernels %s; BatchNorm-backward mask disagreements with the stored forward output: %d; %.1f s" % (
        eng.tag, sorted(eng.labels), eng.flips, time.time() - t0))
    unchecked = eng.called - EXEMPT - eng.checked
    assert not unchecked, "launches without a check: %s" % sorted(unchecked)
    assert not bad, "\n".join(bad)
    assert eng.flips == 0
    vacuous = [(e, what) for e, _, what, rep, exact in eng.reports if rep["worst"] == 0 and not exact]
    assert not vacuous, vacuous


# ---- (b) the primitive table ----------------------------------------------------------------------------------------------------
# N, Cin, H, W, Cout, ks, stride, pad | env | expected labels: fp32 (forward, dgrad, wgrad), bf16x3 (forward, dgrad, wgrad) | ops
T, X, XW, WT, W3, WPP, WV = ("tconv3_tile_kernel", "tconv3_tile_x3_kernel", "tconv3_tile_x3w_kernel", "tconv3_wgrad_tile_kernel", "tconv3_wgrad_x3_kernel",
                            "tconv3_wgrad_x3pp_kernel", "tconv3_wgrad_x3v_kernel")
F1, F3, F7, G1, G3, G7, S1, S3 = ("tconv_fwd_kernel<1>", "tconv_fwd_kernel<3>", "tconv_fwd_kernel<7>", "tconv_wgrad_kernel<1>", "tconv_wgrad_kernel<3>",
                                  "tconv_wgrad_kernel<7>", "dgrad_strided_kernel<1>", "dgrad_strided_kernel<3>")
FD, GD = "tconv_fwd_kernel<3> dil", "tconv_wgrad_kernel<3> dil"      # the dilated entries' launches: tconv_fwd_kernel<3, 0, true>, tconv_wgrad_kernel<3, true>
ALL = "fdw"
ROWS = [
    # Cin 15 | 16 and 31 | 32 (the data gradient's K is Cout)
    ((2, 15, 9, 7, 15, 3, 1, 1), {}, (F3, F3, G3), (F3, F3, G3), ALL),            # odd map, ragged everything; Cout 15
    ((2, 16, 9, 7, 16, 3, 1, 1), {}, (T, T, WT), (T, T, WPP), ALL),               # (W % 4 != 0: no vectorised weight gradient)
    ((2, 31, 12, 16, 31, 3, 1, 1), {}, (T, T, WT), (T, T, WV), ALL),
    ((2, 32, 12, 16, 32, 3, 1, 1), {}, (T, T, WT), (X, X, WV), ALL),
    ((1, 16, 6, 8, 32, 3, 1, 1), {}, (T, T, WT), (T, X, W3), ALL),                # N = 1, one tile: nt / 2 < 1 -> the two-block-per-CU weight gradient; R capped by Ho
    # pad 0 | 1 | 2 on the tile kernels
    ((2, 32, 13, 18, 40, 3, 1, 0), {}, (T, T, WT), (X, X, WPP), ALL),
    ((2, 32, 11, 14, 40, 3, 1, 2), {}, (T, T, WT), (X, X, WPP), ALL),
    # Wo 127 | 128 | 130: the second tile of two columns
    ((1, 32, 5, 127, 64, 3, 1, 1), {}, (T, T, WT), (X, X, WPP), ALL),
    ((1, 32, 5, 128, 64, 3, 1, 1), {}, (T, T, WT), (X, X, WV), ALL),
    ((1, 32, 5, 130, 64, 3, 1, 1), {}, (T, T, WT), (X, X, WPP), ALL),
    # the head convolution: Cout 100, two ragged 64-cout groups
    ((3, 128, 6, 8, 100, 3, 1, 1), {}, (T, T, WT), (X, X, WV), ALL),
    # partial last row tile on a 56-row map, three images
    ((3, 64, 55, 56, 64, 3, 1, 1), {}, (T, T, WT), (X, X, WV), ALL),
    # the wide split kernel: switch, and the blocks >= 448 / slots >= 192 rule on both sides (blocks from Cout; the data gradient's from Cin)
    ((2, 64, 20, 112, 64, 3, 1, 1), {"POPNET_TRAIN_X3_WIDE": "1"}, (T, T, WT), (XW, XW, WV), ALL),
    ((1, 40, 11, 70, 72, 3, 1, 1), {"POPNET_TRAIN_X3_WIDE": "1"}, (T, T, WT), (XW, XW, WPP), ALL),
    ((2, 32, 32, 128, 896, 3, 1, 1), {}, (T, None, None), (XW, None, None), "f"),      # 2 x 16 tiles x 14 groups = 448 blocks
    ((2, 32, 32, 128, 832, 3, 1, 1), {}, (T, None, None), (X, None, None), "f"),       # 416 blocks
    ((2, 896, 32, 128, 32, 3, 1, 1), {}, (None, T, None), (None, XW, None), "d"),
    ((2, 832, 32, 128, 32, 3, 1, 1), {}, (None, T, None), (None, X, None), "d"),
    ((3, 32, 3, 128, 4800, 3, 1, 1), {}, (T, None, None), (XW, None, None), "f"),      # 450 blocks of 3 x 64 = 192 slots
    ((3, 32, 2, 128, 4800, 3, 1, 1), {}, (T, None, None), (X, None, None), "f"),       # 450 blocks of 2 x 64 = 128 slots
    # geometry refusals of the split kernels (see the module docstring): back to the fp32 tile kernel / the 128-slot split kernel
    ((1, 32, 106, 1, 16, 3, 1, 1), {}, (T, None, None), (T, None, None), "f"),
    ((1, 32, 87, 3, 16, 3, 1, 1), {"POPNET_TRAIN_X3_WIDE": "1"}, (T, None, None), (X, None, None), "f"),
    # the three weight-gradient variants
    ((3, 64, 24, 32, 64, 3, 1, 1), {"POPNET_TRAIN_WGRAD_NOVEC": "1"}, (None, None, WT), (None, None, WPP), "w"),
    # stride 2 with 3x3, 1x1 and 7x7 (YoloPoseNet's layer2.0 and the stems), and stride-1 1x1 / 7x7
    ((3, 64, 24, 32, 128, 3, 2, 1), {}, (F3, S3, G3), (F3, S3, G3), ALL),
    ((3, 64, 24, 32, 128, 1, 2, 0), {}, (F1, S1, G1), (F1, S1, G1), ALL),
    ((2, 64, 13, 9, 70, 3, 2, 1), {}, (F3, S3, G3), (F3, S3, G3), ALL),
    ((2, 1, 40, 56, 64, 7, 2, 3), {}, (F7, None, G7), (F7, None, G7), "fw"),
    ((2, 3, 9, 11, 20, 7, 1, 3), {}, (F7, F7, G7), (F7, F7, G7), ALL),
    ((2, 128, 12, 16, 28, 1, 1, 0), {}, (F1, F1, G1), (F1, F1, G1), ALL),
    # ResNet-50 (A2J): the longest 1x1 K (128 chunks of 16 channels) and the widest Cout (32 blocks of 64), on layer4's 2 x 3 map
    ((2, 2048, 2, 3, 512, 1, 1, 0), {}, (F1, F1, G1), (F1, F1, G1), ALL),
    ((2, 1024, 2, 3, 2048, 1, 1, 0), {}, (F1, F1, G1), (F1, F1, G1), ALL),
    ((2, 64, 8, 12, 256, 1, 1, 0), {}, (F1, F1, G1), (F1, F1, G1), ALL),
    # its downsample and conv2 at stride 2, with their strided data gradients at 256 .. 512 channels
    ((2, 256, 8, 12, 512, 1, 2, 0), {}, (F1, S1, G1), (F1, S1, G1), ALL),
    ((2, 128, 8, 12, 128, 3, 2, 1), {}, (F3, S3, G3), (F3, S3, G3), ALL),
    ((2, 256, 4, 6, 256, 3, 2, 1), {}, (F3, S3, G3), (F3, S3, G3), ALL),
    # the tile kernels on a map smaller than any tile; the heads' output convolution (Cout % 64 = 32)
    ((2, 512, 2, 3, 512, 3, 1, 1), {}, (T, T, WT), (X, X, WPP), ALL),
    ((2, 256, 2, 3, 480, 3, 1, 1), {}, (T, T, WT), (X, X, WPP), ALL),
    # its stem: the depth channel three times
    ((2, 3, 32, 48, 64, 7, 2, 3), {}, (F7, None, G7), (F7, None, G7), "fw"),
]
ROW_IDS = ["%dx%dx%dx%d_to_%d_k%ds%dp%d%s" % (r[0] + ("_" + "_".join(k[7:].lower() for k in r[1]) if r[1] else "",)) for r in ROWS]


def _row_labels(hplan, shape, ops):
    N, Cin, H, W, Cout, ks, stride, pad = shape
    out = {}
    if "f" in ops:
        out["forward"] = NR.plan(hplan, "forward", *shape)
    if "d" in ops:
        out["dgrad" if stride == 1 else "dgrad_strided"] = NR.plan(hplan, "dgrad" if stride == 1 else "dgrad_strided", *shape)
    if "w" in ops:
        out["wgrad"] = NR.plan(hplan, "wgrad", *shape)
    return out


def _operands(shape, integer, seed, impulse=None):
    """x, w, bias, dy, previous y, previous dx as float32 CPU tensors.  impulse: (which tensor, flat index)"""
    N, Cin, H, W, Cout, ks, stride, pad = shape
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    shapes = {"x": (N, Cin, H, W), "w": (Cout, Cin, ks, ks), "b": (Cout,), "dy": (N, Cout, Ho, Wo), "y0": (N, Cout, Ho, Wo), "dx0": (N, Cin, H, W)}
    g = torch.Generator().manual_seed(seed)
    out = {}
    for i, (k, shp) in enumerate(shapes.items()):
        if integer:
            out[k] = NR.integer_operand(shp, seed * 10 + i).float()
        else:
            out[k] = torch.randn(shp, generator=g) * (1.0 / np.sqrt(Cin * ks * ks) if k == "w" else 1.0)
    if impulse is not None:
        k, idx = impulse
        out[k] = torch.zeros(shapes[k])
        out[k].view(-1)[idx] = 1.0
    return out


def _run_row(gpu, ctx, L, s, hplan, shape, ops, prec, integer=False, seed=1, impulse=None):
    """Every primitive of one table row on the GPU against the reference.  -> [(entry, label, what, report)] (integer: report["n_bad"] counts
    elements that differ from the exact result)."""
    N, Cin, H, W, Cout, ks, stride, pad = shape
    o = _operands(shape, integer, seed, impulse)
    dev = {k: v.to(gpu) for k, v in o.items()}
    d64 = {k: v.double() for k, v in o.items()}
    plans = _row_labels(hplan, shape, ops)
    res = []

    def check(entry, label, what, out, r, a):
        torch.cuda.synchronize(gpu)
        assert out.guards_intact(), "%s %s wrote outside its output" % (entry, what)
        if integer:
            assert float(r.abs().max()) < 2 ** 24
            a = torch.zeros_like(r)
        rep = NR.compare(_4d(_d(out.t)), _4d(r), _4d(a))
        res.append((entry, label, what, rep))
        if not integer:
            _note(entry, prec, rep, what)

    if "forward" in plans:
        lab = plans["forward"]["kernel"]
        x3 = NR.is_x3(lab)
        y = _Out(o["y0"].shape, gpu, float("nan"))
        ctx.check(L.pn_conv2d_forward(ctx.handle, _p(dev["x"]), _p(dev["w"]), _p(dev["b"]), _p(y.t), N, Cin, H, W, Cout, ks, stride, pad, 0, s), "forward")
        check("pn_conv2d_forward", lab, "y = conv + bias", y, *NR.conv_fwd_ref(d64["x"], d64["w"], d64["b"], None, stride, pad, x3))
        y = _Out(o["y0"].shape, gpu, dev["y0"])
        ctx.check(L.pn_conv2d_forward(ctx.handle, _p(dev["x"]), _p(dev["w"]), None, _p(y.t), N, Cin, H, W, Cout, ks, stride, pad, 1, s), "forward +=")
        check("pn_conv2d_forward", lab, "y += conv", y, *NR.conv_fwd_ref(d64["x"], d64["w"], None, d64["y0"], stride, pad, x3))
        y = _Out(o["y0"].shape, gpu, dev["y0"])
        ctx.check(L.pn_conv2d_forward(ctx.handle, _p(dev["x"]), _p(dev["w"]), _p(dev["b"]), _p(y.t), N, Cin, H, W, Cout, ks, stride, pad, 1, s), "forward += bias")
        check("pn_conv2d_forward", lab, "y += conv + bias", y, *NR.conv_fwd_ref(d64["x"], d64["w"], d64["b"], d64["y0"], stride, pad, x3))
    for which in ("dgrad", "dgrad_strided"):
        if which not in plans:
            continue
        lab = plans[which]["kernel"]
        for acc in (0, 1):
            dx = _Out(o["dx0"].shape, gpu, dev["dx0"] if acc else float("nan"))
            if which == "dgrad":
                rc = L.pn_conv2d_dgrad(ctx.handle, _p(dev["dy"]), _p(dev["w"]), _p(dx.t), N, Cin, H, W, Cout, ks, pad, acc, s)
            else:
                rc = L.pn_conv2d_dgrad_strided(ctx.handle, _p(dev["dy"]), _p(dev["w"]), _p(dx.t), N, Cin, H, W, Cout, ks, stride, pad, acc, s)
            ctx.check(rc, which)
            check("pn_conv2d_" + which, lab, "dx +=" if acc else "dx =", dx,
                  *NR.conv_dgrad_ref(d64["dy"], d64["w"], d64["dx0"] if acc else None, tuple(o["dx0"].shape), stride, pad, NR.is_x3(lab)))
    if "wgrad" in plans:
        p = plans["wgrad"]
        for with_bias in (1, 0):
            dw, db = _Out(o["w"].shape, gpu, float("nan")), _Out(o["b"].shape, gpu, float("nan") if with_bias else SENT)
            ctx.check(L.pn_conv2d_wgrad(ctx.handle, _p(dev["x"]), _p(dev["dy"]), _p(dw.t), _p(db.t) if with_bias else None, N, Cin, H, W, Cout, ks, stride, pad, s), "wgrad")
            check("pn_conv2d_wgrad", p["kernel"], "dw" + (" (with dbias)" if with_bias else ""), dw, *NR.conv_wgrad_ref(d64["x"], d64["dy"], ks, stride, pad, p))
            if with_bias:
                check("pn_conv2d_wgrad", "", "dbias", db, *NR.conv_dbias_ref(d64["dy"]))
            else:
                assert bool((db.t == SENT).all()), "dbias written although NULL was passed"
    return res, plans


def _ctx(gpu, prec, monkeypatch, env):
    from popnet_amd import _lib
    L, ctx = _lib.lib(), _lib.Context(gpu.index)
    for k in ("POPNET_TRAIN_X3_WIDE", "POPNET_TRAIN_WGRAD_NOVEC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                # read at every call
    ctx.check(L.pn_train_set_precision(ctx.handle, _lib.PN_PREC_BF16X3 if prec == "bf16x3" else 0), "precision")
    return L, ctx, _lib.current_stream_ptr(gpu)


def _expected(row, prec):
    shape, env, fp32, x3, ops = row
    exp = dict(zip(("forward", "dgrad", "wgrad"), fp32 if prec == "fp32" else x3))
    if shape[6] != 1:
        exp["dgrad_strided"] = exp.pop("dgrad")
    return {k: v for k, v in exp.items() if v is not None}


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_primitive_table_within_fp64_allowance_and_on_the_expected_kernel(gpu, monkeypatch, row, prec):
    shape, env, _, _, ops = row
    L, ctx, s = _ctx(gpu, prec, monkeypatch, env)
    hplan = NR.plan_context(prec == "bf16x3")
    res, plans = _run_row(gpu, ctx, L, s, hplan, shape, ops, prec, seed=sum(shape))
    assert {k: p["kernel"] for k, p in plans.items()} == _expected(row, prec)
    bad = _bad([r + (False,) for r in res])
    print("\nNCHW TABLE %s %s: %s" % (prec, shape, "; ".join("%s %s %s %.3f" % (e[3:], lab, what, rep["worst"]) for e, lab, what, rep in res)))
    assert not bad, "\n".join(bad)
    assert all(rep["worst"] > 0 for _, _, _, rep in res), [(e, what) for e, _, what, rep in res if rep["worst"] == 0]
    CHECKED.setdefault("table " + prec, set()).update(p["kernel"] for p in plans.values())


# ---- (c) integer probes -----------------------------------------------------------------------------------------------------------
def _impulses(shape):
    """flat indices into dy / x of the four corners and one interior pixel of the last image's last channel"""
    N, Cin, H, W, Cout, ks, stride, pad = shape
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    spots = lambda h, w: sorted({(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)})       # noqa: E731
    return ([("x", ((N * Cin - 1) * H + yy) * W + xx) for yy, xx in spots(H, W)] + [("dy", ((N * Cout - 1) * Ho + yy) * Wo + xx) for yy, xx in spots(Ho, Wo)])


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_primitive_table_integer_probes_are_bit_exact(gpu, monkeypatch, row, prec):
    """Operands in [-3, 3]: every hi / lo split is exact (lo = 0) and every fp32 partial sum an integer below 2^24 (asserted on the reference), so
    any summation order gives the exact result; a missing pixel, tap, seam or slice shows.  Strided and padded rows also get single impulses."""
    shape, env, _, _, ops = row
    L, ctx, s = _ctx(gpu, prec, monkeypatch, env)
    hplan = NR.plan_context(prec == "bf16x3")
    res, _ = _run_row(gpu, ctx, L, s, hplan, shape, ops, prec, integer=True, seed=sum(shape) + 1)
    n = len(res)
    if (shape[6] != 1 or shape[7] != 1) and shape[4] * shape[1] <= 128 * 128:
        for imp in _impulses(shape):
            res += _run_row(gpu, ctx, L, s, hplan, shape, ops, prec, integer=True, seed=7, impulse=imp)[0]
    bad = _bad([r + (True,) for r in res])
    print("\nNCHW INTEGER %s %s: %d results, %d impulse results, %d differ" % (prec, shape, n, len(res) - n, len(bad)))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("net,prec,B,H,W", [("yolo", "fp32", 3, 96, 128), ("yolo", "fp32", 2, 80, 112), ("rtpose", "fp32", 3, 72, 40),
                                            ("rtpose", "bf16x3", 3, 72, 40), ("rtpose", "fp32", 1, 104, 136), ("rtpose", "bf16x3", 1, 104, 136)])
def test_integer_probes_of_every_convolution_of_the_steps_are_bit_exact(gpu, golden, monkeypatch, net, prec, B, H, W):
    """Every distinct convolution / data gradient / weight gradient call of the replayed steps, as single primitives on integer operands."""
    tag = "%s_%s_%dx%dx%d" % (net, prec, B, H, W)
    if tag not in CALLS:
        _replay(golden, gpu, net, prec, B, H, W)
    L, ctx, s = _ctx(gpu, prec, monkeypatch, {})
    hplan = NR.plan_context(prec == "bf16x3")
    shapes = {}
    for which, Cin, Cout, ks, stride, pad, rh, rw in CALLS[tag]:
        shapes.setdefault((B, Cin, H // rh, W // rw, Cout, ks, stride, pad), set()).add({"forward": "f", "wgrad": "w"}.get(which, "d"))
    bad, n = [], 0
    for i, (shape, ops) in enumerate(sorted(shapes.items())):
        res, _ = _run_row(gpu, ctx, L, s, hplan, shape, "".join(sorted(ops)), prec, integer=True, seed=100 + i)
        n += len(res)
        bad += ["%s: %s" % (shape, b) for b in _bad([r + (True,) for r in res])]
    print("\nNCHW INTEGER %s: %d convolution shapes, %d results, %d differ" % (tag, len(shapes), n, len(bad)))
    assert len(shapes) >= 8
    assert not bad, "\n".join(bad)


# ---- element-wise primitives the table above does not hold -------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cc,H,W", [(3, 70, 13, 9), (3, 70, 12, 8), (3, 64, 48, 64), (1, 5, 1, 2), (31, 2048, 1, 2), (2, 2048, 2, 3)])
@pytest.mark.parametrize("act,with_res", [(0, False), (1, False), (1, True), (2, False), (2, True)])
def test_batchnorm_forward_backward_within_fp64_allowance(gpu, N, Cc, H, W, act, with_res):
    """Odd H W (the scalar kernels), H W a multiple of 4 (the 16-byte ones), several reduction slices (3 x 48 x 64 over 64 channels), the smallest
    count (2); with and without a residual; the mask from `out` and recomputed from x; dres overwritten and accumulated.  31 x 2048 planes
    (grid.y = 63488, next to the 65535 the entries refuse above) and 2 x 2048 x 2 x 3: ResNet-50's layer4 at the A2J trainer's largest batch
    and on the replayed maps."""
    from popnet_amd import _lib
    L, ctx, s = _lib.lib(), _lib.Context.for_device(gpu.index), _lib.current_stream_ptr(gpu)
    g = torch.Generator().manual_seed(N + Cc + H + act)
    shape = (N, Cc, H, W)
    x = torch.randn(shape, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)
    res = torch.randn(shape, generator=g) if with_res else None
    rm, rv = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    dy, d0 = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    dev = lambda t: None if t is None else t.to(gpu)           # noqa: E731
    xd, gd, bd, rd, dyd = dev(x), dev(gamma), dev(beta), dev(res), dev(dy)
    y, mean, invstd = _Out(shape, gpu, float("nan")), _Out((Cc,), gpu, float("nan")), _Out((Cc,), gpu, float("nan"))
    rmd, rvd = _Out((Cc,), gpu, rm), _Out((Cc,), gpu, rv)
    ctx.check(L.pn_bn_train_forward(ctx.handle, _p(xd), _p(gd), _p(bd), _p(rd), _p(y.t), _p(mean.t), _p(invstd.t), _p(rmd.t), _p(rvd.t), 0.1, 1e-5, act, N, Cc, H * W, s), "bn")
    torch.cuda.synchronize(gpu)
    reps = []

    def check(what, out, r, a, exact=False):
        assert out.guards_intact(), what
        rep = NR.compare(_4d(_d(out.t)), _4d(r), _4d(a))
        reps.append(("pn_bn_train_" + ("backward" if what.startswith("d") else "forward"), "", what, rep, exact or _exactly_stored(r)))
        _note(reps[-1][0], "fp32", rep)
    st = NR.bn_stats_ref(x.double(), rm.double(), rv.double())
    for k, o in (("mean", mean), ("invstd", invstd), ("running_mean", rmd), ("running_var", rvd)):
        check(k, o, *st[k])
    check("y", y, *NR.bn_apply_ref(x.double(), _d(mean.t), _d(invstd.t), gamma.double(), beta.double(), None if res is None else res.double(), act))
    mask = _d(y.t) > 0
    for out_given, accumulate in ((True, 0), (True, 1)) + (((False, 0),) if not with_res else ()):
        dx, dg, db = _Out(shape, gpu, float("nan")), _Out((Cc,), gpu, float("nan")), _Out((Cc,), gpu, float("nan"))
        dres = _Out(shape, gpu, dev(d0) if accumulate else float("nan"))
        ctx.check(L.pn_bn_train_backward(ctx.handle, _p(xd), _p(dyd), _p(y.t) if out_given else None, _p(gd), _p(bd), _p(mean.t), _p(invstd.t), act, N, Cc, H * W,
                                         _p(dx.t), _p(dg.t), _p(db.t), _p(dres.t), accumulate, s), "bn bwd")
        torch.cuda.synchronize(gpu)
        args = (x.double(), dy.double(), mask, _d(mean.t), _d(invstd.t), gamma.double(), act, _d(db.t))
        ref = NR.bn_bwd_ref(*args, dres_prev=d0.double() if accumulate else None)
        tagx = " (out %s, dres %s)" % ("given" if out_given else "NULL", "+=" if accumulate else "=")
        for k, o in (("dbeta", db), ("dgamma", dg), ("dx", dx), ("dres", dres)):
            check(k + tagx, o, *ref[k], exact=(k == "dres" and not accumulate and act != 2))
        assert NR.mask_disagreements(_d(dx.t), *args) == 0
    bad = _bad(reps)
    print("\nNCHW BN %s act %d res %s: %s" % (shape, act, with_res, _summary(reps)))
    assert not bad, "\n".join(bad)
    assert not [(w) for _, _, w, rep, exact in reps if rep["worst"] == 0 and not exact]


def test_batchnorm_refuses_too_many_planes_before_any_launch(gpu):
    """N * C > 65535 (the apply kernels' grid.y) is an argument error: PN_ERR_INVALID from the checks in front of every launch, outputs untouched."""
    from popnet_amd import _lib
    L, ctx, s = _lib.lib(), _lib.Context(gpu.index), _lib.current_stream_ptr(gpu)
    N, Cc, HW = 2, 32768, 2
    x = torch.zeros((N, Cc, 1, HW), device=gpu)
    v = [_Out((Cc,), gpu, SENT) for _ in range(6)]
    y = _Out(x.shape, gpu, SENT)
    rc = L.pn_bn_train_forward(ctx.handle, _p(x), _p(v[0].t), _p(v[1].t), None, _p(y.t), _p(v[2].t), _p(v[3].t), _p(v[4].t), _p(v[5].t), 0.1, 1e-5, 1, N, Cc, HW, s)
    assert rc == PN_ERR_INVALID and "N * C out of range" in ctx.last_error()
    rc = L.pn_bn_train_backward(ctx.handle, _p(x), _p(x), None, _p(v[0].t), _p(v[1].t), _p(v[2].t), _p(v[3].t), 1, N, Cc, HW, _p(y.t), _p(v[4].t), _p(v[5].t), None, 0, s)
    assert rc == PN_ERR_INVALID and "N * C out of range" in ctx.last_error()
    torch.cuda.synchronize(gpu)
    assert bool((y.buf == SENT).all()) and all(bool((o.buf == SENT).all()) for o in v)
    # the largest plane count the entries take still runs
    N, Cc = 1, 65535
    x = torch.randn((N, Cc, 1, HW), device=gpu)
    ones = torch.ones(Cc, device=gpu)
    y, mean, invstd = torch.empty_like(x), torch.empty(Cc, device=gpu), torch.empty(Cc, device=gpu)
    ctx.check(L.pn_bn_train_forward(ctx.handle, _p(x), _p(ones), _p(ones), None, _p(y), _p(mean), _p(invstd), None, None, 0.1, 1e-5, 0, N, Cc, HW, s), "bn")
    r, a = NR.bn_apply_ref(_d(x), _d(mean), _d(invstd), _d(ones), _d(ones), None, 0)
    assert NR.compare(_d(y), r, a)["n_bad"] == 0


def test_pools_heads_copies_and_sgd_within_fp64_allowance(gpu):
    from popnet_amd import _lib
    L, ctx, s = _lib.lib(), _lib.Context.for_device(gpu.index), _lib.current_stream_ptr(gpu)
    g = torch.Generator().manual_seed(9)
    reps = []

    def check(entry, what, out, r, a, exact=False):
        torch.cuda.synchronize(gpu)
        assert out.guards_intact(), what
        rep = NR.compare(_4d(_d(out.t)), _4d(r), _4d(a))
        reps.append((entry, "", what, rep, exact))
        _note(entry, "fp32", rep)
    for (N, Cc, H, W) in ((2, 5, 14, 10), (2, 5, 13, 9), (1, 3, 1, 1)):
        x = torch.randn((N, Cc, H, W), generator=g)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        dy = torch.randn((N, Cc, Ho, Wo), generator=g)
        y, dx = _Out(dy.shape, gpu, float("nan")), _Out(x.shape, gpu, float("nan"))
        xd, dyd = x.to(gpu), dy.to(gpu)
        ctx.check(L.pn_avgpool3s2_forward(ctx.handle, _p(xd), _p(y.t), N * Cc, H, W, s), "pool")
        ctx.check(L.pn_avgpool3s2_backward(ctx.handle, _p(dyd), _p(dx.t), N * Cc, H, W, s), "pool bwd")
        check("pn_avgpool3s2_forward", "avgpool %dx%d" % (H, W), y, *NR.avgpool_fwd_ref(x.double()))
        check("pn_avgpool3s2_backward", "avgpool_bwd %dx%d" % (H, W), dx, *NR.avgpool_bwd_ref(dy.double(), H, W))
        for k, st, pad in ((3, 2, 1), (2, 2, 0)):
            if H < k:
                continue
            xm = (torch.randint(-3, 4, x.shape, generator=g).float() * 0.5)          # coarse values: ties in most windows
            xm.view(-1)[::97] = float("nan")
            yr_, ir = NR.maxpool_fwd_ref(xm, k, st, pad)
            ym, im = _Out(yr_.shape, gpu, float("nan")), torch.empty(yr_.shape, device=gpu, dtype=torch.int32)
            xmd = xm.to(gpu)
            ctx.check(L.pn_maxpool_forward(ctx.handle, _p(xmd), _p(ym.t), _p(im), N * Cc, H, W, k, st, pad, s), "maxpool")
            torch.cuda.synchronize(gpu)
            assert ym.guards_intact() and torch.equal(im.cpu().long(), ir)
            assert torch.equal(torch.isnan(ym.t.cpu()), torch.isnan(yr_)) and torch.equal(ym.t.cpu().nan_to_num(), yr_.nan_to_num())
            dym = torch.randn(yr_.shape, generator=g)
            dxm, dymd = _Out(x.shape, gpu, float("nan")), dym.to(gpu)
            ctx.check(L.pn_maxpool_backward(ctx.handle, _p(dymd), _p(im), _p(dxm.t), N * Cc, H, W, k, st, pad, s), "maxpool bwd")
            check("pn_maxpool_backward", "maxpool_bwd k%d %dx%d" % (k, H, W), dxm, *NR.maxpool_bwd_ref(dym.double(), ir, H, W), exact=True)
    # heads into / out of a channel slice, both kinds, with and without fg weights and an upstream gradient
    N, Cc, h, w, LD = 2, 15, 6, 5, 40
    for kind, weighted, extra in ((1, True, True), (0, False, False), (1, False, True)):
        v, t = torch.randn((N, Cc, h, w), generator=g) * 2, torch.randn((N, Cc, h, w), generator=g)
        fg = (torch.rand((N, Cc, h, w), generator=g) < 0.3).float() if weighted else None
        ex = torch.randn((N, LD, h, w), generator=g)
        vd, td, fgd, exd = v.to(gpu), t.to(gpu), None if fg is None else fg.to(gpu), ex.to(gpu)
        sg, cat, loss, dv = _Out(v.shape, gpu, float("nan")), _Out((N, LD, h, w), gpu, SENT), _Out((1,), gpu, float("nan")), _Out(v.shape, gpu, float("nan"))
        ctx.check(L.pn_head_forward(ctx.handle, _p(vd), _p(td), _p(fgd), kind, N, Cc, h * w, _p(sg.t), C.c_void_p(cat.t.data_ptr() + 7 * h * w * 4), LD, _p(loss.t), s), "head")
        rs, as_, ro, ao = NR.head_fwd_ref(v.double(), kind)
        check("pn_head_forward", "sigmoid", sg, rs, as_)
        torch.cuda.synchronize(gpu)
        got = _d(cat.t)
        assert bool((got[:, :7] == SENT).all()) and bool((got[:, 7 + Cc:] == SENT).all()) and cat.guards_intact()        # the other channels of the slice's tensor
        rep = NR.compare(got[:, 7:7 + Cc], ro, ao)
        reps.append(("pn_head_forward", "", "out slice", rep, False))
        check("pn_head_forward", "loss", loss, *NR.head_loss_ref(got[:, 7:7 + Cc], t.double(), None if fg is None else fg.double()))
        ctx.check(L.pn_head_backward(ctx.handle, _p(sg.t), _p(td), _p(fgd), C.c_void_p(exd.data_ptr() + 7 * h * w * 4) if extra else None, LD, kind, N, Cc, h * w, _p(dv.t), s),
                  "head bwd")
        check("pn_head_backward", "dv", dv, *NR.heads_bwd_ref(_d(sg.t), t.double(), None if fg is None else fg.double(), ex[:, 7:7 + Cc].double() if extra else None, kind))
    # slice copies
    src, d0 = torch.randn((2, 9, 3, 5), generator=g), torch.randn((2, 12, 3, 5), generator=g)
    srcd = src.to(gpu)
    for acc in (0, 1):
        dst = _Out(d0.shape, gpu, d0.to(gpu))
        ctx.check(L.pn_slice_copy(ctx.handle, C.c_void_p(srcd.data_ptr() + 2 * 15 * 4), 9, C.c_void_p(dst.t.data_ptr() + 4 * 15 * 4), 12, 2, 6, 15, acc, s), "slice_copy")
        torch.cuda.synchronize(gpu)
        got = _d(dst.t)
        assert dst.guards_intact() and torch.equal(got[:, :4], d0[:, :4].double()) and torch.equal(got[:, 10:], d0[:, 10:].double())
        r, a = NR.slice_copy_ref(src[:, 2:8].double(), d0[:, 4:10].double() if acc else None)
        reps.append(("pn_slice_copy", "", "copy +=" if acc else "copy", NR.compare(got[:, 4:10], r, a), not acc))
    # Nesterov SGD: first and later steps, with and without weight decay and gradient scale
    for wd, gs in ((0.0, 1.0), (1e-2, 0.5)):
        n = 1003
        p, buf = torch.randn(n, generator=g), torch.zeros(n)
        pd, bufd = _Out((n,), gpu, p.to(gpu)), _Out((n,), gpu, buf.to(gpu))
        for k in range(3):
            gr = torch.randn(n, generator=g)
            p0, b0 = _d(pd.t), _d(bufd.t)
            grd = gr.to(gpu)
            ctx.check(L.pn_sgd_nesterov(ctx.handle, _p(pd.t), _p(grd), _p(bufd.t), n, 0.7, 0.9, wd, 1 if k == 0 else 0, gs, s), "sgd")
            ref = NR.sgd_ref(p0, gr.double(), b0, 0.7, 0.9, wd, k == 0, gs)
            check("pn_sgd_nesterov", "p step %d" % k, pd, *ref["p"])
            check("pn_sgd_nesterov", "buf step %d" % k, bufd, *ref["buf"], exact=(k == 0 and wd == 0 and gs == 1.0))
    bad = _bad(reps)
    print("\nNCHW ELEMENTWISE: %s" % _summary(reps))
    assert not bad, "\n".join(bad)
    assert not [w_ for _, _, w_, rep, exact in reps if rep["worst"] == 0 and not exact]


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("B,h,w", [(3, 6, 8), (2, 5, 7)])
def test_yolo_loss_within_fp64_allowance(gpu, weighted, B, h, w):
    from popnet_amd import _lib
    L, ctx, s = _lib.lib(), _lib.Context.for_device(gpu.index), _lib.current_stream_ptr(gpu)
    prior, conf, coord, weight = [torch.from_numpy(a) for a in yr.yolo_case_targets(seed=B * 7 + h, B=B, H=16 * h, W=16 * w)]
    v = torch.from_numpy(np.random.default_rng(h * w).normal(0, 2, prior.shape).astype(np.float32))
    dev = [t.to(gpu) for t in (v, prior, conf, coord, weight)]
    out, dv, terms = _Out(v.shape, gpu, float("nan")), _Out(v.shape, gpu, float("nan")), _Out((4,), gpu, float("nan"))
    ctx.check(L.pn_yolo_loss(ctx.handle, _p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]), _p(dev[4]) if weighted else None, B, 2, 15, h, w, _p(out.t), _p(terms.t), _p(dv.t), s),
              "pn_yolo_loss")
    torch.cuda.synchronize(gpu)
    ref = NR.yolo_loss_ref(v.double(), prior.double(), conf.double(), coord.double(), weight.double() if weighted else None, 2, 15)
    reps = []
    for k, o in (("out", out), ("dv", dv), ("terms", terms)):
        assert o.guards_intact()
        reps.append(("pn_yolo_loss", "", k, NR.compare(_4d(_d(o.t)), _4d(ref[k][0]), _4d(ref[k][1])), False))
        _note("pn_yolo_loss", "fp32", reps[-1][3])
    bad = _bad(reps)
    print("\nNCHW YOLO LOSS: %s" % ", ".join("%s %.3f" % (r[2], r[3]["worst"]) for r in reps))
    assert not bad, "\n".join(bad)
    assert all(r[3]["worst"] > 0 for r in reps)


def test_a_changed_parameter_reaches_the_next_convolution_through_the_pack_refresh(gpu):
    """pn_train_pack_refresh: with the pack cache on, a weight changed behind the cache's back is NOT seen by the next tile convolution, and is
    seen after the refresh -- for the fp32 pack (forward), the flipped one (data gradient) and both split packs."""
    from popnet_amd import _lib
    L, s = _lib.lib(), _lib.current_stream_ptr(gpu)
    N, Cin, H, W, Cout = 2, 32, 12, 16, 40
    for prec in ("fp32", "bf16x3"):
        ctx = _lib.Context(gpu.index)
        ctx.check(L.pn_train_set_precision(ctx.handle, _lib.PN_PREC_BF16X3 if prec == "bf16x3" else 0), "precision")
        ctx.check(L.pn_train_pack_cache(ctx.handle, 1), "cache")
        g = torch.Generator().manual_seed(3)
        x, w, dy = torch.randn((N, Cin, H, W), generator=g), torch.randn((Cout, Cin, 3, 3), generator=g) / 17, torch.randn((N, Cout, H, W), generator=g)
        xd, wd, dyd = x.to(gpu), w.to(gpu), dy.to(gpu)
        y, dx = torch.empty((N, Cout, H, W), device=gpu), torch.empty_like(xd)
        x3 = prec == "bf16x3"

        def run():
            ctx.check(L.pn_conv2d_forward(ctx.handle, _p(xd), _p(wd), None, _p(y), N, Cin, H, W, Cout, 3, 1, 1, 0, s), "forward")
            ctx.check(L.pn_conv2d_dgrad(ctx.handle, _p(dyd), _p(wd), _p(dx), N, Cin, H, W, Cout, 3, 1, 0, s), "dgrad")
            torch.cuda.synchronize(gpu)
            wn = _d(wd)
            return (NR.compare(_d(y), *NR.conv_fwd_ref(x.double(), wn, None, None, 1, 1, x3)),
                    NR.compare(_d(dx), *NR.conv_dgrad_ref(dy.double(), wn, None, tuple(x.shape), 1, 1, x3)))
        assert all(r["n_bad"] == 0 and r["worst"] > 0 for r in run())
        wd[3, 5, 1, 2] += 0.5
        assert all(r["n_bad"] > 0 for r in run())                   # the cached packs still hold the old weight
        ctx.check(L.pn_train_pack_refresh(ctx.handle, s), "refresh")
        assert all(r["n_bad"] == 0 and r["worst"] > 0 for r in run())
        ctx.check(L.pn_train_pack_cache(ctx.handle, 0), "cache off")


# ---- (d) coverage guard --------------------------------------------------------------------------------------------------------------
def test_coverage_guard_every_training_shape_kernel_is_checked(gpu, golden, monkeypatch):
    """The kernel labels the two engines' steps use at their training shapes (YoloPoseNet 30 x 224 x 224; rtpose_light3d 32 x 224 x 224 in both
    NCHW precisions), from pn_train_conv_plan_info alone -- nothing is launched at those sizes -- must be among the labels whose launches (a) and (b)
    compared.  A replay or a table precision that has not run in this process is run here."""
    for k in ("POPNET_TRAIN_X3_WIDE", "POPNET_TRAIN_WGRAD_NOVEC"):
        monkeypatch.delenv(k, raising=False)
    need = [("yolo", "fp32", 3, 96, 128), ("rtpose", "fp32", 3, 72, 40), ("rtpose", "bf16x3", 3, 72, 40)]
    for net, prec, B, H, W in need:
        if "%s_%s_%dx%dx%d" % (net, prec, B, H, W) not in CALLS:
            _replay(golden, gpu, net, prec, B, H, W)
    for prec in ("fp32", "bf16x3"):
        if "table " + prec not in CHECKED:
            L, ctx, s = _ctx(gpu, prec, monkeypatch, {})
            for row in ROWS:
                L, ctx, s = _ctx(gpu, prec, monkeypatch, row[1])
                res, plans = _run_row(gpu, ctx, L, s, NR.plan_context(prec == "bf16x3"), row[0], row[4], prec, seed=sum(row[0]))
                assert not _bad([r + (False,) for r in res])
                CHECKED.setdefault("table " + prec, set()).update(p["kernel"] for p in plans.values())
            for k in ("POPNET_TRAIN_X3_WIDE", "POPNET_TRAIN_WGRAD_NOVEC"):
                monkeypatch.delenv(k, raising=False)
    train = set()
    for net, prec, B, H, W in need:
        Bt, Ht, Wt = TRAIN_SHAPES[net]
        hplan = NR.plan_context(prec == "bf16x3")
        for which, Cin, Cout, ks, stride, pad, rh, rw in CALLS["%s_%s_%dx%dx%d" % (net, prec, B, H, W)]:
            train.add(NR.plan(hplan, which, Bt, Cin, Ht // rh, Wt // rw, Cout, ks, stride, pad)["kernel"])
    checked = set().union(*CHECKED.values())
    print("\nNCHW COVERAGE: training-shape kernels %s\nchecked kernels %s" % (sorted(train), sorted(checked)))
    print("NCHW WORST |gpu - r| / allowance per (entry, precision): %s" % ", ".join("%s %s %.3f" % (k[0][3:], k[1], v) for k, v in sorted(WORST.items())))
    assert {"tconv3_tile_x3w_kernel", "tconv3_wgrad_x3v_kernel", "tconv3_tile_kernel", "dgrad_strided_kernel<3>"} <= train
    assert train <= checked, sorted(train - checked)
    every = {T, X, XW, WT, W3, WPP, WV, F1, F3, F7, G1, G3, G7, S1, S3}
    assert every <= checked, sorted(every - checked)            # every label the plan description can return
