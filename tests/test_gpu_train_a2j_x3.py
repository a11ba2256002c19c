"""A2JTrainEngine(precision="bf16x3"): the step launch by launch against fp64, the unchanged default, the golden step and the trainer script.

(a) Replay, as tests/test_gpu_train_a2j_layers.py does for fp32 (its _CheckedA2J mixin, imported, with checks for the three new entries in a
    subclass): every primitive call copies what it reads, NaN-prefills what it overwrites, runs the engine's own method and compares each output
    element with the fp64 reference of that one launch on the operands the GPU read.  pn_conv1x1_x3_forward / _dgrad: NR.conv_fwd_ref /
    NR.conv_dgrad_ref with ks = 1, x3 = True; pn_conv1x1_x3_wgrad: conv1x1_x3_reference.wgrad_ref with the depth of pn_conv1x1_x3_plan_info.
    The other launches keep the mixin's checks at precision "bf16x3" (the 3x3 stride-1 layers on tconv3_tile_x3* / tconv3_wgrad_x3*).
(b) A2JTrainEngine(...) without a precision argument issues only the old entries.
(c) The golden step (tests/golden/a2j_train.npz, AC.SMALL).  MEASURED below holds what an MI355X gave; the bounds are
    max(golden tolerance, 4 x measured), the loss terms in no case above 1e-3 relative.
(d) scripts/train_a2j_mpaug.py --precision bf16x3 for one epoch on the fake tree of tests/test_gpu_train_a2j.py."""
import os
import time

import numpy as np
import pytest
import torch

import a2j_cases as AC
import conv1x1_x3_cases as CC
import conv1x1_x3_reference as CR
import nchw_layer_reference as NR
from test_gpu_train import _accuracy_class, _assert_same_class
from test_gpu_train_a2j import G, G0, _fake_mpaug_tree, _golden_batch, _golden_sd, cpu_ref  # noqa: F401  (cpu_ref: the fixture)
from test_gpu_train_a2j_layers import REPLAYS, _CheckedA2J, _tag, _worst_checks
from test_gpu_train_nchw_layers import EXEMPT, _bad, _d, _engine_class, _summary

pytestmark = pytest.mark.gpu

NEW = {"pn_conv1x1_x3_forward", "pn_conv1x1_x3_dgrad", "pn_conv1x1_x3_wgrad"}
ENGINES, SECONDS = {}, {}
# MEASURED on an MI355X, golden step in precision="bf16x3" (against the golden file and torch's fp64 CPU step, not against the engine's own fp32
# mode): |loss terms - golden| (Cls, Reg); the largest |running statistic - golden| in units of that statistic's golden tolerance; the error of
# the parameter gradients against fp64 autograd (median over tensors, maximum, whole vector).  See test_golden_step_in_bf16x3.
MEASURED = {"terms": (2.74e-6, 5.3e-7), "stats_over_tol": 2.617, "grad_class": (2.02e-2, 3.32e-2, 2.03e-2)}


class _CheckedA2JX3(_CheckedA2J):
    """_CheckedA2J with the stride-1 1x1 convolutions checked as the new entries define them."""

    def _is1x1(self, ks, stride, pad):
        return ks == 1 and stride == 1 and pad == 0

    def _plan1(self, role, x_shape, Cout):
        N, Cin, H, W = x_shape
        self.calls1x1.add((role, Cin, Cout, self.img_hw[0] // H, self.img_hw[1] // W))
        return CC.plan(self.hplan, role, N, Cin, H * W, Cout)

    def _conv(self, name, x, ks, stride=1, pad=0, dil=1):
        if not self._is1x1(ks, stride, pad):
            return super()._conv(name, x, ks, stride, pad, dil=dil) if dil != 1 else super()._conv(name, x, ks, stride, pad)
        w, b = self.p[name + ".weight"], self.p.get(name + ".bias")
        self._buf("c:" + name, (x.shape[0], w.shape[0]) + tuple(x.shape[2:])).fill_(float("nan"))
        y = super(_CheckedA2J.__mro__[1], self)._conv(name, x, ks, stride, pad)                 # A2JTrainEngine._conv: past the mixins
        p = self._plan1("forward", x.shape, w.shape[0])
        self._cmp("pn_conv1x1_x3_forward", p["kernel"], name, y, *NR.conv_fwd_ref(_d(x), _d(w), _d(b), None, 1, 0, True))
        return y

    def _conv_bwd(self, name, dy, ks, stride=1, pad=0, dx=None, accumulate=False, need_dx=True, dil=1):
        if not self._is1x1(ks, stride, pad):
            kw = {"dil": dil} if dil != 1 else {}
            return super()._conv_bwd(name, dy, ks, stride, pad, dx=dx, accumulate=accumulate, need_dx=need_dx, **kw)
        x, w = self.A["x:" + name], self.p[name + ".weight"]
        if need_dx and dx is None:
            dx = self._buf("dx:" + name, x.shape)
        prev = _d(dx) if (need_dx and accumulate) else None
        if need_dx and not accumulate:
            dx.fill_(float("nan"))
        self.g[name + ".weight"].fill_(float("nan"))
        assert name + ".bias" not in self.g                     # (no 1x1 convolution of A2J_model has a bias)
        out = super(_CheckedA2J.__mro__[1], self)._conv_bwd(name, dy, ks, stride, pad, dx=dx, accumulate=accumulate, need_dx=need_dx)
        xd, dyd = _d(x), _d(dy)
        if not self.light:
            p = self._plan1("wgrad", x.shape, w.shape[0])
            self._cmp("pn_conv1x1_x3_wgrad", p["kernel"], name + " dw", self.g[name + ".weight"], *CR.wgrad_ref(xd, dyd, p))
        if need_dx:
            p = self._plan1("dgrad", x.shape, w.shape[0])
            self._cmp("pn_conv1x1_x3_dgrad", p["kernel"], name + " dx", out, *NR.conv_dgrad_ref(dyd, _d(w), prev, tuple(x.shape), 1, 0, True))
        return out


def _replay(gpu, B, H, W):
    """Two steps (the second after apply(), in light mode: the launches that read a refreshed pack); once per process and shape."""
    tag = _tag(B, H, W) + "_x3"
    if tag in ENGINES:
        return ENGINES[tag]
    from popnet_amd.train_a2j import A2JTrainEngine
    t0 = time.time()
    sd = _golden_sd()
    eng = _engine_class(A2JTrainEngine, _CheckedA2JX3)(sd, device=gpu, precision="bf16x3")
    eng.loaded = sd
    eng.calls1x1 = set()
    rng = np.random.default_rng(B * 1000 + H + W)
    label = np.stack([rng.uniform(0, H, (B, 15)), rng.uniform(0, W, (B, 15)), rng.normal(0, 1, (B, 15))], 2).astype(np.float32)        # (y, x, z)
    batch = [torch.from_numpy(AC.net_input(AC.SEED + H, B, H, W)).to(gpu), torch.from_numpy(label).to(gpu)]
    eng.start_checks(tag, "bf16x3")
    eng._batch = batch
    eng.forward_backward(*batch)
    eng.apply()
    eng.light = True
    eng.forward_backward(*batch)
    torch.cuda.synchronize(gpu)
    ENGINES[tag], SECONDS[tag] = eng, time.time() - t0
    return eng


@pytest.mark.parametrize("B,H,W", REPLAYS, ids=[_tag(*c) + "_x3" for c in REPLAYS])
def test_every_launch_of_the_bf16x3_step_within_fp64_allowance(gpu, B, H, W):
    """Measured on an MI355X: see DESIGN.md 1.2 (training) for the worst |gpu - r| / allowance per entry."""
    eng = _replay(gpu, B, H, W)
    assert eng.precision == "bf16x3"
    bad = _bad(eng.reports)
    print("\nA2J X3 LAYERS %s: %d checks; worst |gpu - r| / allowance per entry: %s" % (eng.tag, len(eng.reports), _summary(eng.reports)))
    print("A2J X3 LAYERS %s: kernels %s; BatchNorm-backward mask disagreements: %d; %.1f s" % (eng.tag, sorted(eng.labels), eng.flips, SECONDS[eng.tag]))
    print("A2J X3 LAYERS %s: the worst comparison of each entry: %s" % (eng.tag, _worst_checks(eng.reports)))
    unchecked = eng.called - EXEMPT - eng.checked
    assert not unchecked, "launches without a check: %s" % sorted(unchecked)
    assert NEW | {"pn_conv2d_forward", "pn_conv2d_dgrad", "pn_conv2d_wgrad", "pn_conv2d_forward_dil", "pn_conv2d_dgrad_dil", "pn_conv2d_wgrad_dil", "pn_a2j_loss",
                  "pn_adam", "pn_conv2d_dgrad_strided", "pn_bn_train_forward", "pn_bn_train_backward"} <= eng.checked
    # the new kernels and the existing split 3x3 kernels actually ran
    assert "conv1x1_x3_kernel" in eng.labels and any(k.startswith("conv1x1_wgrad_x3_kernel<") for k in eng.labels)
    assert any(k.startswith("tconv3_tile_x3") for k in eng.labels) and any(k.startswith("tconv3_wgrad_x3") for k in eng.labels)
    # all 34 stride-1 1x1 layers went through the new entries in the three roles (every one of them has a data gradient)
    n1 = [sum(1 for e, _, what, _, _ in eng.reports if e == entry) for entry in sorted(NEW)]
    assert n1 == [34 + 34, 34 + 34, 34], n1           # dgrad and forward: both steps; wgrad: the first
    assert not any(e in ("pn_conv2d_forward", "pn_conv2d_dgrad", "pn_conv2d_wgrad") and lab.endswith("<1>") and ".downsample.0" not in what
                   for e, lab, what, _, _ in eng.reports)
    assert not bad, "\n".join(bad)
    assert eng.flips == 0
    vacuous = [(e, what) for e, _, what, rep, exact in eng.reports if rep["worst"] == 0 and not exact]
    assert not vacuous, vacuous


def test_default_precision_issues_only_the_old_entries(gpu):
    from popnet_amd.train_a2j import A2JTrainEngine

    class Recorder:
        def __init__(self, lib):
            self.lib, self.names = lib, set()

        def __getattr__(self, k):
            if k.startswith("pn_"):
                self.names.add(k)
            return getattr(self.lib, k)
    B, H, W = REPLAYS[0]
    label = torch.from_numpy(np.stack([np.full((B, 15), H / 2), np.full((B, 15), W / 2), np.ones((B, 15))], 2).astype(np.float32)).to(gpu)
    img = torch.from_numpy(AC.net_input(AC.SEED + H, B, H, W)).to(gpu)
    seen = {}
    for kw in ({}, {"precision": "fp32"}, {"precision": "bf16x3"}):
        eng = A2JTrainEngine(_golden_sd(), device=gpu, **kw)
        eng.L = rec = Recorder(eng.L)
        terms = eng.step(img, label)
        assert bool(torch.isfinite(terms).all())
        seen[kw.get("precision")] = (set(rec.names), eng.precision, eng.flat_g.clone())
    assert seen[None][1] == "fp32" and seen["bf16x3"][1] == "bf16x3"
    assert not any("conv1x1" in k for k in seen[None][0]) and seen[None][0] == seen["fp32"][0]
    assert torch.equal(seen[None][2], seen["fp32"][2])                                   # the same launches, the same bits
    assert seen["bf16x3"][0] == seen[None][0] | NEW
    assert not torch.equal(seen["bf16x3"][2], seen[None][2])
    with pytest.raises(ValueError):
        A2JTrainEngine(_golden_sd(), device=gpu, precision="bf16")
    from popnet_amd import _lib
    with pytest.raises(_lib.PopnetError):
        A2JTrainEngine(_golden_sd(), device=gpu, precision="bf16x3").capture()


@pytest.fixture(scope="module")
def x3_step(gpu):
    from popnet_amd.train_a2j import A2JTrainEngine
    eng = A2JTrainEngine(_golden_sd(), device=gpu, precision="bf16x3")
    x, lab = _golden_batch()
    terms = eng.forward_backward(x.to(gpu), lab.to(gpu)).cpu().numpy().astype(np.float64)
    return eng, terms


def test_golden_step_in_bf16x3(gpu, x3_step, cpu_ref):  # noqa: F811
    """The golden step of tests/test_gpu_train_a2j.py in precision="bf16x3".  MEASURED on an MI355X:
    * loss terms 4.6455698 / 5.8091245 against the golden 4.6455725 / 5.8091250: |difference| 2.74e-6 / 5.3e-7 (5.9e-7 / 9.1e-8 relative), inside the
      golden's own tolerance.  Asserted: max(G["terms_tol"], 4 x measured), in no case above 1e-3 relative.
    * running statistics: the worst |difference| is 2.617 x its golden tolerance (fp32 mode: inside it).  Asserted: max(1, 4 x 2.617) x the tolerance.
    * parameter gradients against fp64 autograd (median over tensors / maximum / whole vector): 2.02e-2 / 3.32e-2 / 2.03e-2, next to
      1.4e-3 / 2.7e-2 / 1.9e-3 for torch fp32 on the CPU and 5.7e-3 / 1.7e-2 / 5.6e-3 for the engine's fp32 mode.  The existing rule
      (test_gpu_train._assert_same_class) does NOT hold for the median (its bound here 5.7e-3) and the whole vector (1e-2); it holds for the maximum.
      Every launch of the bf16x3 step passes the fp64 allowance of its own definition (test_every_launch_of_the_bf16x3_step_within_fp64_allowance,
      the new entries at <= 0.024 of it, no BatchNorm mask disagreement with the stored outputs), so this is not a wrong operand: the case is
      flip-dominated (BatchNorm over 90 values per channel in layer4), and operands of 16 significant bits move ~2^8 times more pre-activations
      across zero than fp32 rounding does.  As the issue prescribes for that outcome nothing is widened silently: the median and the whole
      vector are asserted at twice the MEASURED value, marked as measured; the maximum keeps the existing rule."""
    eng, terms = x3_step
    dev = np.abs(terms - G["terms"])
    tol = np.minimum(np.maximum(G["terms_tol"], 4 * np.asarray(MEASURED["terms"])), 1e-3 * np.abs(G["terms"]))
    print("\nA2J X3 GOLDEN loss terms", terms, "golden", G["terms"], "|difference|", dev, "relative", dev / np.abs(G["terms"]), "tol", tol)
    # parameter gradients
    g32, g64 = cpu_ref[torch.float32], cpu_ref[torch.float64]
    hip, t32 = _accuracy_class(eng, g32, g64)
    print("A2J X3 GOLDEN accuracy class (median over tensors, max, whole vector): hip", hip, "torch fp32", t32)
    new = eng.state_dict()
    worst = 0.0
    stat_bad = []
    for k in G.files:
        if k.startswith("stat_") and not k.endswith("_tol"):
            kind, layer = k.split(".", 1)
            got = new[layer + (".running_mean" if kind == "stat_mean" else ".running_var")].cpu().double().numpy()
            ratio = float(np.abs(got - G[k]).max() / float(G[k + "_tol"]))
            worst = max(worst, ratio)
            if ratio > max(1.0, 4 * MEASURED["stats_over_tol"]):
                stat_bad.append((k, ratio))
    print("A2J X3 GOLDEN running statistics: worst |difference| / golden tolerance %.3f" % worst)
    assert bool((dev <= tol).all()), (terms, G["terms"], tol)
    _assert_same_class((0.0, hip[1], 0.0), t32)                                         # the maximum: the existing rule
    assert hip[0] <= 2 * MEASURED["grad_class"][0] and hip[2] <= 2 * MEASURED["grad_class"][2], (hip, MEASURED["grad_class"])      # MEASURED, x 2
    assert not stat_bad, stat_bad
    assert int(new["Backbone.model.bn1.num_batches_tracked"]) == 1
    assert all(int(v) == 1 for k, v in new.items() if k.endswith("num_batches_tracked"))
    sd0 = _golden_sd()
    for k in ("Backbone.model.fc.weight", "Backbone.model.fc.bias"):
        assert torch.equal(new[k].cpu(), sd0[k])                                         # carried bit for bit
    eng.apply()
    new = eng.state_dict()
    for k in ("Backbone.model.fc.weight", "Backbone.model.fc.bias"):
        assert torch.equal(new[k].cpu(), sd0[k])
    assert set(new) == set(sd0) and eng.steps == 1


def test_train_script_in_bf16x3_on_a_fake_mpaug_dataset(gpu, tmp_path, capsys):
    """scripts/train_a2j_mpaug.py --precision bf16x3, one epoch: a finite loss and a `.pth` that A2J_model.load_state_dict accepts."""
    import importlib.util
    import random
    from popnet_amd.network.a2j import A2J_model
    d = str(tmp_path)
    ann_files = _fake_mpaug_tree(d)
    spec = importlib.util.spec_from_file_location("train_a2j_mpaug", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "train_a2j_mpaug.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    random.seed(2)
    out_dir = os.path.join(d, "out")
    mod.main(["--train-annotations"] + ann_files + ["--val-annotations"] + ann_files[:2] + ["--image-dir", os.path.join(d, "img"), "--bg-file", os.path.join(d, "bg.json"),
             "--bg-dir", os.path.join(d, "bg"), "--seg-dir", os.path.join(d, "seg"), "--output-dir", out_dir, "--batch-size", "4", "--lr", "0.001",
             "--epochs", "1", "--print-freq", "1", "--seed", "2", "--frame-size", "256", "--crop", "64", "--precision", "bf16x3"])
    out = capsys.readouterr().out
    train = [float(line.split(":")[1].split(",")[0]) for line in out.splitlines() if line.startswith("mean train_loss_add")]
    assert len(train) == 1 and np.isfinite(train).all(), out
    files = sorted(os.listdir(out_dir))
    assert len(files) == 1 and files[0].endswith(".pth"), files
    sd = torch.load(os.path.join(out_dir, files[0]), map_location="cpu")
    assert sorted(sd) == sorted(str(k) for k in G0["keys"])
    A2J_model(15).load_state_dict(sd)                                                    # strict
    with pytest.raises(SystemExit):
        mod.main(["--precision", "bf16"])
