"""Every launch of the A2J training step (popnet_amd.train_a2j.A2JTrainEngine: csrc/train.hip with its dilated entries, csrc/train_yolo.hip,
csrc/train_a2j.hip) against the fp64 references of tests/nchw_layer_reference.py and tests/a2j_train_reference.py, element by element.

The replay is the one of tests/test_gpu_train_nchw_layers.py (its _Checked mixin in front of the engine class, its forwarding proxy around
engine.L): every primitive method copies what the call reads and what it accumulates into, pre-fills what it overwrites with NaN, calls the
engine's own method and compares every output element with the reference of that one launch on the operands the GPU read.  Added here:
  * pn_conv2d_forward_dil / _dgrad_dil / _wgrad_dil (the mixin's dil argument): the undilated definitions with the taps dil apart; the
    weight gradient's depth from the launch code's own slices (NR.dil_wgrad_plan);
  * pn_a2j_loss, called inline by forward_backward, through the proxy: loss terms and the three gradient maps against
    a2j_train_reference.loss_fp64 on the head maps, anchors, labels and scale the kernel read;
  * pn_adam on the whole flat buffer against a2j_train_reference.adam_step on the engine's own p, g, m, v, with the bound of
    test_gpu_train_a2j.test_adam_vs_fp64_formula; Backbone.model.fc.* stays as loaded, bit for bit.
Two steps per replay, the second after apply() in `light` mode (the launches that read a refreshed pack).  A called pn_* entry without a check
fails the test.  The replay must be able to fail: three comparisons of the first replay are repeated, with nothing launched, against a
deliberately wrong reference each.  The coverage guard takes the kernel of every replayed convolution call at the trainer's shapes (16 and 31
crops of 288 x 288) from pn_train_conv_plan_info alone.

Shapes: 2 x 32 x 48 (maps 16 x 24, 8 x 12, 4 x 6, 2 x 3: every BatchNorm of layer3 / layer4 over 12 values per channel, nearly every
non-centre tap of the dilated convolutions in the padding) and 3 x 48 x 80 (24 x 40 .. 3 x 5: odd maps at stride 16, N = 3).

Measured on an MI355X: 8.9 s for the 2 x 32 x 48 replay and 9.0 s for 3 x 48 x 80 (864 comparisons each; the fp64 host references and the Adam
check over the whole flat buffer dominate), so the larger one keeps N = 3.  Every launch passes; the worst |gpu - r| / allowance per entry is in
DESIGN.md (1.2, training)."""
import os
import time

import numpy as np
import pytest
import torch

import a2j_cases as AC
import a2j_train_reference as R
import nchw_layer_reference as NR
from test_gpu_train_nchw_layers import CALLS, CHECKED, EXEMPT, FD, GD, _bad, _Checked, _engine_class, _summary

pytestmark = pytest.mark.gpu

REPLAYS = [(2, 32, 48), (3, 48, 80)]
TRAIN_BATCHES, TRAIN_HW = (16, 31), (288, 288)          # scripts/train_a2j_mpaug.py's crops; popnet_amd.train_a2j.MAX_BATCH
DILATED, WITH_RESIDUAL, ACCUMULATED = "Backbone.model.layer4.1.conv2", "Backbone.model.layer2.1.bn3", "Backbone.model.layer2.1.conv1"
ENGINES = {}                                            # tag -> the checked engine after its replay
SECONDS = {}
_SD = {}                                                # the seeded state dict, built once


class _CheckedA2J(_Checked):
    """The mixin of test_gpu_train_nchw_layers.py with A2J's optimiser step and its inline loss call."""
    want = (("forward", DILATED), ("bn", WITH_RESIDUAL), ("dgrad", ACCUMULATED))

    def apply(self):
        n64 = lambda t: t.detach().cpu().numpy().astype(np.float64)          # noqa: E731
        p, g, m, v = (n64(t) for t in (self.flat_p, self.flat_g, self.flat_m, self.flat_v))
        super(_Checked, self).apply()                                        # A2JTrainEngine.apply: pn_adam at step counter self.steps + 1
        p1, m1, v1 = R.adam_step(p, g, m, v, self.steps, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, 1.0 / self.world)
        t = torch.from_numpy
        self._cmp("pn_adam", "", "parameters", self.flat_p, t(p1), t(2.0 ** -22 * (np.abs(p1) + np.abs(p1 - p))))
        self._cmp("pn_adam", "", "exp_avg", self.flat_m, t(m1), t(2.0 ** -22 * np.abs(m1) + 1e-45))
        self._cmp("pn_adam", "", "exp_avg_sq", self.flat_v, t(v1), t(2.0 ** -22 * np.abs(v1) + 1e-45))
        self._cmp("pn_adam", "", "gradient (read only)", self.flat_g, t(g), t(np.zeros_like(g)), exact=True)
        now = self.state_dict()
        carried = [k for k in self.loaded if k.startswith("Backbone.model.fc.")]
        assert len(carried) == 2 and not any(k in self.p for k in carried)
        for k in carried:
            assert now[k].dtype == self.loaded[k].dtype
            self._cmp("pn_adam", "", "carried " + k, now[k], self.loaded[k].double(), torch.zeros(self.loaded[k].shape, dtype=torch.float64), exact=True)

    def _inline_pn_a2j_loss(self, fn, ctx, cls, reg, dep, N, h, w, A, P, anchors, label, sf, scale, terms, dcls, dreg, ddep, stream):
        chans = (A * P, 2 * A * P, A * P)
        read = [self._view(p, N, c, c, h * w).detach().cpu().contiguous().view(N, c, h, w) for p, c in zip((cls, reg, dep), chans)]
        an = self._view(anchors, 1, 1, 1, h * w * A * 2).detach().cpu().reshape(h * w * A, 2)
        lab = self._view(label, 1, 1, 1, N * P * 3).detach().cpu().reshape(N, P, 3)
        sc = tuple(float(s) for s in self._view(scale, 1, 1, 1, 2).detach().cpu().reshape(2))
        tt = self._view(terms, 1, 1, 1, 2)
        outs = [self._view(p, N, c, c, h * w) for p, c in zip((dcls, dreg, ddep), chans)]
        for o in outs + [tt]:
            o.fill_(float("nan"))
        rc = fn(ctx, cls, reg, dep, N, h, w, A, P, anchors, label, sf, scale, terms, dcls, dreg, ddep, stream)
        ref_t, ref_g, t_allow, g_allow = R.loss_fp64(read[0], read[1], read[2], (N, h, w, A, P), an, lab, float(sf), sc)
        self._cmp("pn_a2j_loss", "", "terms", tt, ref_t, t_allow)
        for name, o, c, r, a in zip(("dcls", "dreg", "ddep"), outs, chans, ref_g, g_allow):
            self._cmp("pn_a2j_loss", "", name, o.view(N, c, h, w), r, a + 1e-30)
        return rc


def _golden_sd():
    if "sd" in _SD:
        return _SD["sd"]
    g0 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "a2j.npz"))
    keys = [str(k) for k in g0["keys"]]
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(g0["shapes"], g0["ndim"])]
    _SD["sd"] = AC.state_dict_for_seed(AC.SEED, keys, shapes)          # read only: the engine copies it
    return _SD["sd"]


def _tag(B, H, W):
    return "a2j_%dx%dx%d" % (B, H, W)


def _replay(gpu, B, H, W):
    """Two steps (the second after apply(), reading the refreshed packs); the checked engine, once per process and shape."""
    tag = _tag(B, H, W)
    if tag in ENGINES:
        return ENGINES[tag]
    from popnet_amd.train_a2j import A2JTrainEngine
    t0 = time.time()
    sd = _golden_sd()
    eng = _engine_class(A2JTrainEngine, _CheckedA2J)(sd, device=gpu)
    eng.loaded = sd
    rng = np.random.default_rng(B * 1000 + H + W)
    label = np.stack([rng.uniform(0, H, (B, 15)), rng.uniform(0, W, (B, 15)), rng.normal(0, 1, (B, 15))], 2).astype(np.float32)        # (y, x, z)
    batch = [torch.from_numpy(AC.net_input(AC.SEED + H, B, H, W)).to(gpu), torch.from_numpy(label).to(gpu)]
    eng.start_checks(tag, "fp32")
    eng._batch = batch
    eng.forward_backward(*batch)
    eng.apply()
    eng.light = True
    eng.forward_backward(*batch)
    torch.cuda.synchronize(gpu)
    CHECKED["replay " + tag] = set(eng.labels)
    CALLS[tag] = set(eng.calls)
    ENGINES[tag], SECONDS[tag] = eng, time.time() - t0
    return eng


def _worst_checks(reports):
    """entry -> the comparison with the largest |gpu - r| / allowance"""
    by = {}
    for e, _, what, rep, _ in reports:
        e += " (dbias)" if what.endswith("dbias") else ""
        if e not in by or rep["worst"] > by[e][1]:
            by[e] = (what, rep["worst"])
    return "; ".join("%s %s %.3f" % (e[3:], w, v) for e, (w, v) in sorted(by.items()))


@pytest.mark.parametrize("B,H,W", REPLAYS, ids=[_tag(*c) for c in REPLAYS])
def test_every_launch_of_the_a2j_step_within_fp64_allowance(gpu, B, H, W):
    eng = _replay(gpu, B, H, W)
    bad = _bad(eng.reports)
    print("\nA2J LAYERS %s: %d checks; worst |gpu - r| / allowance per entry: %s" % (eng.tag, len(eng.reports), _summary(eng.reports)))
    print("A2J LAYERS %s: kernels %s; BatchNorm-backward mask disagreements with the stored forward output: %d; %.1f s" % (
        eng.tag, sorted(eng.labels), eng.flips, SECONDS[eng.tag]))
    print("A2J LAYERS %s: the worst comparison of each entry: %s" % (eng.tag, _worst_checks(eng.reports)))
    unchecked = eng.called - EXEMPT - eng.checked
    assert not unchecked, "launches without a check: %s" % sorted(unchecked)
    assert {"pn_conv2d_forward_dil", "pn_conv2d_dgrad_dil", "pn_conv2d_wgrad_dil", "pn_a2j_loss", "pn_adam", "pn_conv2d_dgrad_strided", "pn_maxpool_backward"} <= eng.checked
    assert {FD, GD} <= eng.labels
    assert not bad, "\n".join(bad)
    assert eng.flips == 0
    vacuous = [(e, what) for e, _, what, rep, exact in eng.reports if rep["worst"] == 0 and not exact]
    assert not vacuous, vacuous


def test_the_replay_rejects_three_wrong_references(gpu):
    """Nothing is launched: three comparisons of the first replay again, on the tensors it captured, each against a reference with one fault --
    a dilated layer with the taps 1 apart (the padding moved with them, so the centre tap stays where it is), a bn3 without its residual, a
    block's conv1 data gradient without the identity gradient it accumulates into.  The right references pass on the same tensors."""
    eng = _replay(gpu, *REPLAYS[0])
    assert set(eng.kept) == set(eng.want)
    cmp4 = lambda got, r, a: NR.compare(got, r, a)["n_bad"]          # noqa: E731
    y, x, w, b, stride, pad, dil = eng.kept[("forward", DILATED)]
    assert dil == 2 and cmp4(y, *NR.conv_fwd_ref(x, w, b, None, stride, pad, False, dilation=dil)) == 0
    n_dil = cmp4(y, *NR.conv_fwd_ref(x, w, b, None, stride, pad - dil + 1, False, dilation=1))
    y, x, mean, invstd, gamma, beta, res, act = eng.kept[("bn", WITH_RESIDUAL)]
    assert res is not None and cmp4(y, *NR.bn_apply_ref(x, mean, invstd, gamma, beta, res, act)) == 0
    n_res = cmp4(y, *NR.bn_apply_ref(x, mean, invstd, gamma, beta, None, act))
    dx, dy, w, prev, shape, stride, pad, x3 = eng.kept[("dgrad", ACCUMULATED)]
    assert prev is not None and cmp4(dx, *NR.conv_dgrad_ref(dy, w, prev, shape, stride, pad, x3)) == 0
    n_prev = cmp4(dx, *NR.conv_dgrad_ref(dy, w, None, shape, stride, pad, x3))
    print("\nA2J LAYERS wrong references: elements over the allowance -- dilation 1: %d, no residual: %d, no prev: %d" % (n_dil, n_res, n_prev))
    assert n_dil > 0 and n_res > 0 and n_prev > 0


def test_coverage_guard_every_kernel_of_the_a2j_trainer_is_checked(gpu):
    """The kernel labels of every convolution call of the step at the trainer's shapes (16 and 31 crops of 288 x 288), from
    pn_train_conv_plan_info alone -- nothing is launched at those sizes --, are among the labels whose launches the two replays compared; the
    dilated entries, which the plan description does not cover, by their literal labels."""
    for cfg in REPLAYS:
        _replay(gpu, *cfg)
    hplan = NR.plan_context(False)
    checked = set().union(*(CHECKED["replay " + _tag(*c)] for c in REPLAYS))
    train = set()
    for cfg in REPLAYS:
        calls = CALLS[_tag(*cfg)]
        assert len(calls) >= 40
        for which, Cin, Cout, ks, stride, pad, rh, rw in calls:
            for Bt in TRAIN_BATCHES:
                train.add(NR.plan(hplan, which, Bt, Cin, TRAIN_HW[0] // rh, TRAIN_HW[1] // rw, Cout, ks, stride, pad)["kernel"])
    print("\nA2J COVERAGE: training-shape kernels %s\nchecked kernels %s" % (sorted(train), sorted(checked)))
    assert {"tconv3_tile_kernel", "tconv3_wgrad_tile_kernel", "tconv_fwd_kernel<1>", "tconv_fwd_kernel<7>", "dgrad_strided_kernel<1>", "dgrad_strided_kernel<3>"} <= train
    assert train | {FD, GD} <= checked, sorted((train | {FD, GD}) - checked)
