"""Yolo-A2J on the GPU: the crop kernel, every launch of the compiled A2J net, the anchor vote and the chain, against the
reference's own outputs (tests/golden/a2j.npz, a2j_crops.npz: made by tests/golden/make_golden_a2j.py) and fp64 host references.

The net is compiled once per (precision, shape, max_batch) for the whole module; the weights are rebuilt from the fixture's seed
(tests/a2j_cases.py), never stored.  Every net compiled here is a row of tests/a2j_plan_cases.py, which says which of its steps are
compared; tests/test_a2j_plan_cases.py shows without a GPU that those rows hold every kernel instance of the plans the engines deploy.

Wall time of the deployed-plan cases (section 2b: 288 x 288, two crops, every step; compile, 2 x 58 partial forwards and the fp64
reference on 16 host threads), measured on an MI355X machine: 2.9 to 3.2 s each (bf16 max_batch 32: 2.9, fp32 max_batch 32: 3.2, bf16
max_batch 16: 3.1, fp32 max_batch 16: 3.0, fp32 max_batch 2: 3.1); the census rows (section 2c) 0.15 to 0.5 s each.
"""
import ctypes as C
import functools
import importlib.util
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2j_cases as AC  # noqa: E402
import a2j_layer_reference as ALR  # noqa: E402
import a2j_plan_cases as APC  # noqa: E402
from a2j_vote_reference import vote_reference as _vote_reference  # noqa: E402
import layer_reference as LR  # noqa: E402
from popnet_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
_spec = importlib.util.spec_from_file_location("make_golden_net_steps", os.path.join(GOLDEN, "make_golden_net_steps.py"))
MK = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MK)


@pytest.fixture(scope="module")
def fx():
    g = np.load(os.path.join(GOLDEN, "a2j.npz"))
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(g["shapes"], g["ndim"])]
    sd = AC.state_dict_for_seed(int(g["seed"]), [str(k) for k in g["keys"]], shapes)
    return g, sd


class _Net:
    """One compiled A2J net with its input, run once in full."""
    def __init__(self, sd, gpu, prec, H, W, B, max_batch=None, monkeypatch=None):
        from popnet_amd.network.a2j import A2J_model
        max_batch = max_batch or B
        self.m = A2J_model(15).eval()
        self.m.load_state_dict(sd)
        self.m.precision = prec
        self.sd = ALR.stem_state_dict({k: v for k, v in sd.items()})
        self.gpu, self.B, self.H, self.W = gpu, B, H, W
        self.x = torch.from_numpy(AC.net_input(AC.SEED + H, B, H, W)).to(gpu)
        self.L, self.ctx = _lib.lib(), _lib.Context.for_device(0)
        if max_batch != B:                                # as network/_hipnet.py::_compile honours it
            monkeypatch.setenv("POPNET_MAX_BATCH", str(max_batch))
        self.heads = self.m(self.x)                       # compiles, one full forward; reference layout
        torch.cuda.synchronize()
        if max_batch != B:
            monkeypatch.delenv("POPNET_MAX_BATCH")
        self.h = self.m._net[0]
        self.info = self._info(-1)
        assert self.info["max_batch"] == max_batch and (self.info["in_h"], self.info["in_w"]) == (H, W)
        self.steps = [self._info(k) for k in range(self.L.pn_net_num_steps(self.h))]
        self.frames = list(range(B))

    def _info(self, k):
        buf = C.create_string_buffer(1 << 16)
        self.ctx.check(self.L.pn_net_step_info(self.h, k, buf, len(buf)), "pn_net_step_info")
        return json.loads(buf.value.decode())

    def forward(self, nsteps):
        self.ctx.check(self.L.pn_net_forward_partial(self.h, C.c_void_p(self.x.data_ptr()), self.B, nsteps, _lib.current_stream_ptr(self.gpu)), "pn_net_forward_partial")
        torch.cuda.synchronize()

    def reader(self):
        cache = {}

        def read(i):
            if i not in cache:
                H, W, Cc = self.info["bufs"][i]
                out = np.empty((self.B, Cc, H, W), np.float32)
                self.ctx.check(self.L.pn_net_read_activation(self.h, ("buf%d" % i).encode(), self.B, out.ctypes.data_as(C.c_void_p), out.size,
                                                             _lib.current_stream_ptr(self.gpu)), "pn_net_read_activation")
                cache[i] = LR.Act(torch.from_numpy(out).to(torch.float64))
            return cache[i]
        return read

    def check_steps(self, which=lambda st: True, dil_of=ALR.reported_dil):
        xf = self.x.cpu().to(torch.float64)
        results = []
        for k, st in enumerate(self.steps):
            if not which(st):
                continue
            self.forward(k)
            checks = ALR.step_reference(st, self.info, self.sd, self.reader(), xf, dil_of=dil_of)
            self.forward(k + 1)
            after = self.reader()
            for ch in checks:
                assert ch.where[0] == "buf"
                gpu = after(ch.where[1]).v[:, ch.where[2]:ch.where[2] + ch.r.shape[1]]
                results.append((k, st["kernel"], ch.name, LR.compare(gpu, ch.r, ch.allow, frames=self.frames)))
        return results

    def vote(self):
        """pn_a2j_vote on the head maps where the net left them -> [B, 15, 3] (y, x, z)."""
        from popnet_amd.network.a2j import generate_anchors, shift
        ptrs, (h, w), prec = self.m.run(self.x)
        anchors = torch.from_numpy(shift([h, w], 16, generate_anchors())).float().to(self.gpu)
        out = torch.empty((self.B, 15, 3), device=self.gpu)
        self.ctx.check(self.L.pn_a2j_vote(self.ctx.handle, ptrs[0], ptrs[1], ptrs[2], prec, self.B, h, w, 16, 15, C.c_void_p(anchors.data_ptr()),
                                          C.c_void_p(out.data_ptr()), None, None, None, _lib.current_stream_ptr(self.gpu)), "pn_a2j_vote")
        torch.cuda.synchronize()
        return out.cpu().numpy(), anchors.cpu().numpy()


_NETS = {}


@pytest.fixture(scope="module")
def nets(fx, gpu):
    def get(prec, size, max_batch=None, monkeypatch=None):
        """size: "s", "l" or (H, W, B).  Only rows of tests/a2j_plan_cases.py are compiled (find raises on anything else); net.case is the row."""
        H, W, B = AC.SMALL if size == "s" else AC.LARGE if size == "l" else size
        case = APC.find(prec, H, W, B, max_batch or B)
        if case[0] not in _NETS:
            _NETS[case[0]] = _Net(fx[1], gpu, prec, H, W, B, max_batch, monkeypatch)
            _NETS[case[0]].case = case
        return _NETS[case[0]]
    yield get
    _NETS.clear()


_is_dilated, _is_output = APC.is_dilated, APC.is_output


@functools.lru_cache(None)
def _no_device():
    return _lib.lib().pn_create(-1)


def _report(results):
    return ["step %d %s %s: worst %.3g, %d elements over, at (frame, channel, row, col, ratio) %s" % (k, kern, name, rep["worst"], rep["n_bad"], rep["where"])
            for k, kern, name, rep in results if rep["n_bad"]]


# ---- 1. crops ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(gpu):
    from popnet_amd.pipeline import A2JEngine
    return A2JEngine(precision="fp32", device=gpu, max_batch=2)      # the crops need no compiled net


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_crop_kernel_equals_reference_bit_for_bit(gpu, engine, dtype):
    g = np.load(os.path.join(GOLDEN, "a2j_crops.npz"))
    assert [str(n) for n in g["names"]] == [n for n, _ in AC.CROP_CASES] and np.array_equal(g["rows"], AC.crop_rows(0))
    frames = torch.from_numpy(AC.depth_frames(AC.SEED + 2, 1)).to(gpu).to(dtype)
    crops, flags = engine.crops(frames, g["rows"])
    torch.cuda.synchronize()
    got = crops.cpu().numpy()[:, 0]
    assert not flags.cpu().numpy().any()
    for i, name in enumerate(g["names"]):
        assert np.array_equal(got[i].view(np.uint32), g["crops"][i].view(np.uint32)), "%s: %d pixels differ" % (name, int((got[i] != g["crops"][i]).sum()))
    assert np.abs(g["crops"][0]).max() > 1.5          # depths past depth_max came through: no clamp


def test_crop_of_an_empty_region_is_zero_and_flagged(gpu, engine):
    """Where the reference raises (cv2.resize of an empty image) the crop is zeros and the row's flag is set."""
    frames = torch.from_numpy(AC.depth_frames(AC.SEED + 2, 1)).to(gpu)
    rows = np.array([[0, 100.0, 100.0, 100.5, 200.0, 0.9],       # no columns
                     [0, 100.0, 100.0, 200.0, 100.9, 0.9],       # no rows
                     [0, 500.0, 100.0, 560.0, 200.0, 0.9],       # right of the frame, pasted: 60 columns of zeros -> (0 - 3) / 2, not flagged
                     [0, 100.0, 100.0, 200.0, 200.0, 0.9]], np.float32)
    crops, flags = engine.crops(frames, rows)
    got, fl = crops.cpu().numpy()[:, 0], flags.cpu().numpy()
    assert fl.tolist() == [1, 1, 0, 0]
    assert not got[0].any() and not got[1].any() and np.all(got[2] == np.float32(-1.5)) and got[3].std() > 0


# ---- 2. every launch against fp64 ----------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_every_step_within_fp64_allowance_80x96(nets, prec):
    net = nets(prec, "s")
    dil = [st for st in net.steps if _is_dilated(st)]
    assert len(dil) == 2 and all(c["w"] in ("Backbone.model.layer4.1.conv2", "Backbone.model.layer4.2.conv2") for st in dil for c in st["convs"])
    assert all(c["dil"] == 2 and ", 2>" in st["kernel"] for st in dil for c in st["convs"])
    assert not any("dil" in c for st in net.steps if st["type"] == "conv" and not _is_dilated(st) for c in st["convs"])
    # fp32: every convolution on the blocked-accumulation instances, bf16: none
    assert all((c.get("blocked_acc", 0) == 1) == (prec == "fp32") for st in net.steps if st["type"] == "conv" for c in st["convs"])
    assert net.case[6] == APC.ALL
    results = net.check_steps(which=APC.selects(net.case[6]))
    assert len(results) >= len(net.steps)
    print("\nA2J LAYERS %s 80x96: %d steps, worst |gpu - r| / allowance = %.4f" % (prec, len(net.steps), max(r[3]["worst"] for r in results)))
    assert not _report(results), "\n".join(_report(results))
    assert all(r[3]["worst"] > 0 for r in results if "pool" not in r[2]), [(r[0], r[2]) for r in results if r[3]["worst"] == 0]


def test_dilated_and_output_steps_within_fp64_allowance_288(nets):
    net = nets("bf16", "l")
    assert net.case[6] == APC.DIL_OUT
    results = net.check_steps(which=APC.selects(net.case[6]))
    assert len({r[0] for r in results if ", 2>" in r[1]}) == 2 and sum(1 for r in results if r[2].endswith(".output")) == 3
    print("\nA2J LAYERS bf16 288: worst |gpu - r| / allowance = %.4f" % max(r[3]["worst"] for r in results))
    assert not _report(results), "\n".join(_report(results))


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("width,pitch", [(480, 64), (992, 120)])
def test_dilated_steps_at_the_wider_pitch_classes(nets, prec, width, pitch):
    """Input sizes are any multiple of 16: a 4 x 30 and a 4 x 62 layer4 map put the dilated halo (Wt + 4 columns) into the 64- and the
    120-pixel LDS pitch classes, which the two fixture shapes (pitch 16 and 32) never launch."""
    net = nets(prec, (64, width, 1))
    dil = [st for st in net.steps if _is_dilated(st)]
    assert len(dil) == 2 and all(st["convs"][0]["pitch"] == pitch for st in dil), [st["kernel"] for st in dil]
    assert APC.DIL_OUT in net.case[6]
    results = net.check_steps(which=APC.selects(APC.DIL_OUT))
    assert len(results) == 5 and not _report(results), "\n".join(_report(results))
    assert all(r[3]["worst"] > 0 for r in results)


# ---- 2b. the plans the engines deploy: 288 x 288 compiled for max_batch 32 / 16 / 2, every step ------------------------
@pytest.mark.parametrize("case", APC.DEPLOYED_CASES, ids=[c[0] for c in APC.DEPLOYED_CASES])
def test_every_step_of_the_deployed_plans_within_fp64_allowance(nets, monkeypatch, case):
    """conv_plan.h plans from max_batch as well as from H and W (8-row conv3 tiles from 1536 strip tiles on, 64-cout generic blocks below one
    block per CU, conv4 from 448 blocks on): the net A2JEngine, YoloA2JEngine and scripts/a2j_bench.py compile at max_batch 32 is another set
    of kernel instances than the max_batch 2 net of the fixture.  Compiled through POPNET_MAX_BATCH, two crops run, every step compared."""
    t0 = time.perf_counter()
    id_, prec, H, W, B, mb, which = case
    net = nets(prec, (H, W, B), mb, monkeypatch)
    assert net.info["max_batch"] == mb and net.B == B == 2 and which == APC.ALL
    results = net.check_steps(which=APC.selects(which))
    assert len(results) >= len(net.steps)
    print("\nA2J DEPLOYED %s: %d steps, worst |gpu - r| / allowance = %.4f, %.1f s" % (id_, len(net.steps), max(r[3]["worst"] for r in results), time.perf_counter() - t0))
    assert not _report(results), "\n".join(_report(results))
    assert all(r[3]["worst"] > 0 for r in results if "pool" not in r[2]), [(r[0], r[2]) for r in results if r[3]["worst"] == 0]
    # the plan compared is the plan a context without a device compiles (the one tests/test_a2j_plan_cases.py reads), label by label, and the
    # labels that were new with these rows are among the compared steps wherever this net's own list has them
    own = [st["kernel"] for st in MK.a2j_steps(_no_device(), prec, mb, H, W)]
    assert [st["kernel"] for st in net.steps] == own
    compared = {r[1] for r in results}
    new = set(APC.NEW_LABELS[prec]) & set(own)
    assert new <= compared and (mb != 32 or new == set(APC.NEW_LABELS[prec])), sorted(set(APC.NEW_LABELS[prec]) - compared)
    assert all((c.get("blocked_acc", 0) == 1) == (prec == "fp32") for st in net.steps if st["type"] == "conv" for c in st["convs"])


# ---- 2c. the census's additions: instance keys that only another crop size or max_batch reaches ----------------------------
_KEY_CASES = [c for c in APC.CASES if APC.key_part(c[6])]


@pytest.mark.parametrize("case", _KEY_CASES, ids=[c[0] for c in _KEY_CASES])
def test_steps_of_the_census_keys_within_fp64_allowance(nets, monkeypatch, case):
    """Only the steps that carry one of the row's instance keys (tests/test_a2j_plan_cases.py test b. has the census and why each row is there)."""
    id_, prec, H, W, B, mb, which = case
    keys = APC.key_part(which)
    net = nets(prec, (H, W, B), mb, monkeypatch)
    results = net.check_steps(which=APC.selects(tuple(keys)))
    seen = {APC.instance_key(c) for k in {r[0] for r in results} for c in net.steps[k]["convs"]}
    assert keys <= seen, sorted(keys - seen)
    print("\nA2J CENSUS %s: %d steps compared, worst |gpu - r| / allowance = %.4f" % (id_, len({r[0] for r in results}), max(r[3]["worst"] for r in results)))
    assert not _report(results), "\n".join(_report(results))
    assert all(r[3]["worst"] > 0 for r in results)


# ---- 3. the allowance rejects a wrong dilation -----------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_reference_with_wrong_dilation_fails(nets, prec):
    net = nets(prec, "s")
    layer4_conv2 = lambda st: st["type"] == "conv" and any(c["w"].startswith("Backbone.model.layer4.") and c["w"].endswith(".conv2") for c in st["convs"])
    plain = net.check_steps(which=layer4_conv2, dil_of=lambda c: 1)
    bad = {r[2] for r in plain if r[3]["n_bad"]}
    assert bad == {"Backbone.model.layer4.1.conv2", "Backbone.model.layer4.2.conv2"}, bad
    swapped = net.check_steps(which=layer4_conv2, dil_of=ALR.swapped_block_dil)
    bad = {r[2] for r in swapped if r[3]["n_bad"]}
    assert bad == {"Backbone.model.layer4.0.conv2", "Backbone.model.layer4.1.conv2"}, bad


# ---- 4. vote: one-hot probe --------------------------------------------------------------------------------
def test_vote_one_hot_probe_is_exact(gpu):
    from popnet_amd.network.a2j import post_process
    B, P, h, w = 32, 15, 5, 6
    K = h * w * 16
    assert K == B * P                                   # every anchor is hot exactly once
    rng = np.random.default_rng(7)
    cls = np.full((B, K, P), -1e4, np.float32)
    for b in range(B):
        for p in range(P):
            cls[b, 15 * b + p, p] = 0.0
    reg = rng.normal(0, 3, (B, K, P, 2)).astype(np.float32)
    dep = rng.normal(0, 1, (B, K, P)).astype(np.float32)
    pp = post_process(shape=[h, w], stride=16, P_h=None, P_w=None)
    out = pp((torch.from_numpy(cls).to(gpu), torch.from_numpy(reg).to(gpu), torch.from_numpy(dep).to(gpu))).cpu().numpy()
    anchors = pp.all_anchors_np.astype(np.float32)
    for b in range(B):
        for p in range(P):
            k = 15 * b + p
            want = np.array([anchors[k, 0] + reg[b, k, p, 0], anchors[k, 1] + reg[b, k, p, 1], dep[b, k, p]], np.float32)
            assert np.array_equal(out[b, p].view(np.uint32), want.view(np.uint32)), (b, p, out[b, p], want)


# ---- 5. vote: the net's own heads against fp64 --------------------------------------------------------------
def _check_vote(net, name, rows=(137,)):
    """rows: the anchor rows whose loss, and whose doubling, the allowance must reject."""
    cls, reg, dep = (t.cpu().numpy() for t in net.heads)
    got, anchors = net.vote()
    r, allow = _vote_reference(cls, reg, dep, anchors)
    ratio = np.abs(got - r) / allow
    print("\nA2J VOTE %s: worst |gpu - r| / allowance = %.4f" % (name, ratio.max()))
    assert ratio.max() <= 1, ratio.max()
    # the allowance rejects dropped or duplicated anchor rows
    rows = list(rows)
    keep = np.ones(cls.shape[1], bool)
    keep[rows] = False
    r_drop, a_drop = _vote_reference(cls[:, keep], reg[:, keep], dep[:, keep], anchors[keep])
    assert (np.abs(got - r_drop) > a_drop).any()
    dup = np.r_[np.arange(cls.shape[1]), rows]
    r_dup, a_dup = _vote_reference(cls[:, dup], reg[:, dup], dep[:, dup], anchors[dup])
    assert (np.abs(got - r_dup) > a_dup).any()


def test_vote_on_the_nets_heads_within_fp64_allowance(nets):
    _check_vote(nets("fp32", "s"), "80x96 fp32")


@pytest.mark.parametrize("size,max_batch", [("s", None), ("l", None), ("l", 32)], ids=["s", "l", "l_max_batch32"])
def test_vote_on_the_bf16_nets_heads_within_fp64_allowance(nets, monkeypatch, size, max_batch):
    """The vote reading bf16 head maps (its other load path).  A stored bf16 head is exact in float32, and the copy handed to the reference is
    that value, so the reference and its allowance are those of the fp32 vote: the products, sums and expf are fp32 in both."""
    net = nets("bf16", size, max_batch, monkeypatch)
    assert net.info["prec"] == "bf16" and all(bool((t == t.to(torch.bfloat16).float()).all()) for t in net.heads)
    # 80 x 96: one anchor row of 480, as on the fp32 net.  288 x 288: the allowance grows with the n = 5184 terms of a sum (any order: 2 n 2^-24 of
    # coordinates near 140, 0.09 px) past the share of one anchor (1 / 5184 of at most 140 px, 0.03 px), so what it must reject there is
    # the 16 anchors of one map cell, the corner cell (8, 8), 135 px from the voted joints: 16 / 5184 of that, 0.4 px
    _check_vote(net, "%s bf16%s" % ("80x96" if size == "s" else "288x288", " max_batch %d" % max_batch if max_batch else ""), rows=(137,) if size == "s" else range(16))


# ---- 6. end to end against the reference's fp64 run ----------------------------------------------------------
@pytest.mark.parametrize("size", ["s", "l"])
def test_fp32_heads_and_joints_within_reference_tolerance(nets, fx, size):
    """Heads and voted joints of the fp32 net within tol = 4 x max|reference fp32 - reference fp64| of the reference's fp64 run.
    Measured on an MI355X (error / tol): 80 x 96: cls 1.54e-6 / 6.36e-6, reg 1.99e-6 / 8.79e-6, dep 2.48e-6 / 1.03e-5, joints 5.63e-6 /
    1.49e-4; 288 x 288: 2.11e-6 / 1.73e-5, 3.78e-6 / 2.32e-5, 3.32e-6 / 2.47e-5, joints 3.31e-5 / 1.38e-3 -- the reference's own fp32
    error, a quarter of tol.  That is the blocked accumulation of the fp32 A2J net (conv_mfma_kernel<..., ACC = 1>): with one serial
    fp32 chain per output the same heads were 6.18e-6 / 7.59e-6 / 1.06e-5 from the fp64 run, the depth head 3 % over its tolerance."""
    g = fx[0]
    net = nets("fp32", size)
    joints, _ = net.vote()
    for name, t in zip(("cls", "reg", "dep"), net.heads):
        got = t.cpu().numpy().astype(np.float64)
        if size == "l":
            got = got.reshape(-1)[::AC.SUBSAMPLE]
        err, tol = np.abs(got - g["%s_%s" % (size, name)]).max(), float(g["%s_%s_tol" % (size, name)])
        print("\nA2J E2E fp32 %s %s: max error %.3g, tolerance %.3g" % (size, name, err, tol))
        assert err <= tol, (name, err, tol)
    err, tol = np.abs(joints - g["%s_joints" % size]).max(), float(g["%s_joints_tol" % size])
    print("A2J E2E fp32 %s joints: max error %.3g, tolerance %.3g" % (size, err, tol))
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("size", ["s", "l"])
def test_bf16_end_to_end_is_finite(nets, fx, size):
    """Finiteness; the deviation from the fp32 net (and, next to it, from the reference's fp64 run) is printed and recorded in
    profiles/a2j_notes.md.  The bound on the deviation from the fp64 run is the next test's."""
    net = nets("bf16", size)
    joints, _ = net.vote()
    assert np.isfinite(joints).all() and all(bool(torch.isfinite(t).all()) for t in net.heads)
    j32, _ = nets("fp32", size).vote()
    dev, d64 = np.abs(joints - j32), np.abs(joints - fx[0]["%s_joints" % size])
    print("\nA2J E2E bf16 %s joints: max deviation from fp32 %.3g px / %.3g (z); from the fp64 reference %.3g px / %.3g (z)" % (
        size, dev[..., :2].max(), dev[..., 2].max(), d64[..., :2].max(), d64[..., 2].max()))


# worst |bf16 joints - reference fp64 joints| over the crops and joints of the fixture, (pixels over y and x, z), measured on an MI355X
BF16_JOINTS_MEASURED = {"s": (0.0161971, 0.00186783), "l": (0.0992172, 0.00797895)}


@pytest.mark.parametrize("size", ["s", "l"])
def test_bf16_joints_within_twice_the_measured_deviation_from_the_reference(nets, fx, size):
    """The voted joints of the bf16 net against the reference's own fp64 run (tests/golden/a2j.npz, as the fp32 test above).  bf16 rounds every
    stored activation of 57 launches to 8 bits, so no bound follows from the formats; the bound is twice the deviation measured on an MI355X,
    the factor for other summation orders of the same plan.  Measured: 80 x 96 (3 crops): 0.0162 px, 0.00187 in z; 288 x 288 (2 crops):
    0.0992 px, 0.00798 in z (the fp32 net is 5.63e-6 and 3.31e-5 from the same run)."""
    joints, _ = nets("bf16", size).vote()
    d64 = np.abs(joints - fx[0]["%s_joints" % size])
    px, z = float(d64[..., :2].max()), float(d64[..., 2].max())
    print("\nA2J E2E bf16 %s joints against the fp64 reference: %.6g px, %.6g (z)" % (size, px, z))
    mpx, mz = BF16_JOINTS_MEASURED[size]
    assert np.isfinite(joints).all() and px <= 2 * mpx and z <= 2 * mz, (px, z, mpx, mz)
    assert px > 0 and z > 0          # the fixture's joints are those of this net's weights, and bf16 is not fp64


# ---- 7. the Python surface ---------------------------------------------------------------------------------
def test_forward_and_post_process_match_the_reference_layout(nets, fx):
    """Shapes and ordering of A2J_model.forward and post_process, by equality with the fixture under tol on the non-square crop."""
    from popnet_amd.network.a2j import post_process
    g = fx[0]
    net = nets("fp32", "s")
    H, W, B = AC.SMALL
    K = (H // 16) * (W // 16) * 16
    cls, reg, dep = net.heads
    assert tuple(cls.shape) == (B, K, 15) and tuple(reg.shape) == (B, K, 15, 2) and tuple(dep.shape) == (B, K, 15)
    for name, t in zip(("cls", "reg", "dep"), net.heads):
        assert np.abs(t.cpu().numpy() - g["s_" + name]).max() <= float(g["s_%s_tol" % name])
    out = post_process(shape=[H // 16, W // 16], stride=16, P_h=None, P_w=None)(net.heads)
    assert tuple(out.shape) == (B, 15, 3)
    assert np.abs(out.cpu().numpy() - g["s_joints"]).max() <= float(g["s_joints_tol"])


# ---- 8. the chain --------------------------------------------------------------------------------------------
def test_chain_predict_lists_equals_the_reference(gpu, fx):
    """Box rows -> crops -> net -> vote -> frame coordinates, three rows through max_batch = 2 (two chunks).  The votes are within
    chain_tol = 4 x the reference's own fp32 error of its fp64 run; a frame coordinate is vote x box size / 288 + corner, so it is within
    chain_tol x box size / 288, plus 4 float32 roundings of the map-back itself; X = (x - cx) Z / fx moves by (dx |Z| + |x - cx| dZ) / fx."""
    from popnet_amd.pipeline import A2JEngine
    g, sd = fx
    eng = A2JEngine(precision="fp32", state_dict=sd, device=gpu, max_batch=2)
    frames = torch.from_numpy(AC.depth_frames(AC.SEED + 1, 2)).to(gpu)
    p2, p3, pc = eng.predict_lists(frames, AC.CHAIN_ROWS)
    assert [len(f) for f in p2] == [1, 2] and [len(f) for f in p3] == [1, 2]
    assert pc[0] == [[0.0] * 15] and pc[1] == [[float(c)] * 15 for c in g["chain_conf"][1:]]          # confidences: exact
    recs = eng.predict_host(frames, AC.CHAIN_ROWS)
    assert eng.last_flags.cpu().tolist() == [0, 0, 0]                                                   # per row, across both chunks: no box the reference would raise on
    assert recs["frame"].tolist() == g["chain_frame"].tolist()
    tol = float(g["chain_tol"])
    got2 = np.array(p2[0] + p2[1]); got3 = np.array(p3[0] + p3[1])
    rows = AC.CHAIN_ROWS.astype(np.float64)
    size = np.stack([rows[:, 3] - rows[:, 1], rows[:, 4] - rows[:, 2]], -1)[:, None, :]                 # [3, 1, 2]
    want2, want3 = g["chain_xy"].astype(np.float64), g["chain_xyz"].astype(np.float64)
    tol2 = tol * size / 288.0 + 4 * 2.0 ** -23 * np.abs(want2)
    assert (np.abs(got2 - want2) <= tol2).all(), np.abs(got2 - want2).max()
    assert np.array_equal(got2[0], np.full((15, 2), -1.0))                                              # the no-detection person
    c = np.array([AC.INTRINSICS["cx"], AC.INTRINSICS["cy"]]); f = np.array([AC.INTRINSICS["fx"], AC.INTRINSICS["fy"]])
    z = np.abs(want3[..., 2:3])
    tol3 = (tol2 * (z + tol) + np.abs(want2 - c) * tol) / f + 4 * 2.0 ** -23 * np.abs(want3[..., :2])
    assert (np.abs(got3[..., :2] - want3[..., :2]) <= tol3).all() and (np.abs(got3[..., 2] - want3[..., 2]) <= tol).all()


# ---- 9. the evaluation script -------------------------------------------------------------------------------------
def test_evaluate_mpreal_a2j_script_writes_what_the_metrics_consume(gpu, golden, fx, tmp_path):
    """scripts/evaluate_mpreal_a2j.py on a fake two-frame dataset tree: YoloPoseNet boxes -> A2J joints -> eval_data.json, which
    popnet_amd.metrics.evaluate_mp_human_3d reads; every frame carries at least one person (a frame without a detection: the
    confidence-0 person at (-1, -1)), each with 15 joints and the box confidence repeated 15 times."""
    import importlib.util
    from helpers import state_dict_from_keys
    from popnet_amd import synth
    spec = importlib.util.spec_from_file_location("evaluate_mpreal_a2j", os.path.join(ROOT, "scripts", "evaluate_mpreal_a2j.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    s = golden.script_yolo
    ysd = state_dict_from_keys(golden.keys["yolo_posenet"], seed=s["weight_seed"])
    ysd["model2_4.0.weight"][[4, 54]] -= np.float32(s["conf_weight_shift"])
    torch.save({"module." + k: v for k, v in ysd.items()}, tmp_path / "yolo.pth")
    torch.save(fx[1], tmp_path / "a2j.pth")
    img_dir = tmp_path / "depth_maps"
    img_dir.mkdir()
    frames = synth.synth_depth(2, 640, 480, seed=s["depth_seed"])
    labels = {"intrinsics": dict(AC.INTRINSICS)}
    rng = np.random.default_rng(5)
    for i in range(2):
        np.save(img_dir / ("f%d.npy" % i), frames[i])
        j2 = rng.uniform(50, 400, (15, 2))
        labels["f%d.npy" % i] = [{"2d_joints": j2.tolist(), "3d_joints": np.c_[j2 / 200, np.full(15, 3.0)].tolist()}]
    json.dump(labels, open(tmp_path / "labels.json", "w"))
    out = mod.main(["--annotations", str(tmp_path / "labels.json"), "--image-dir", str(img_dir), "--batch-size", "2", "--weight", str(tmp_path / "yolo.pth"),
                    "--a2j-weight", str(tmp_path / "a2j.pth"), "--output-dir", str(tmp_path / "out")])
    data = json.load(open(tmp_path / "out" / "eval_data.json"))
    assert sorted(data) == ["human_gt_set_2d", "human_gt_set_3d", "human_pred_set_2d", "human_pred_set_3d", "human_pred_set_part_conf"]
    assert len(data["human_pred_set_2d"]) == 2 and data["human_gt_set_2d"][0] == [labels["f0.npy"][0]["2d_joints"]]
    n_ref = [len(f) for f in s["human_pred_set_2d"]]
    for b in range(2):
        p2, p3, pc = (np.array(data[k][b]) for k in ("human_pred_set_2d", "human_pred_set_3d", "human_pred_set_part_conf"))
        assert p2.shape == (max(n_ref[b], 1), 15, 2) and p3.shape == (max(n_ref[b], 1), 15, 3) and pc.shape == (max(n_ref[b], 1), 15)
        assert np.isfinite(p2).all() and np.isfinite(p3).all() and (pc == pc[:, :1]).all()
        if n_ref[b]:      # the boxes are YoloPoseNet's: the same confidences as its own evaluation
            assert np.abs(pc - np.array(s["human_pred_set_part_conf"][b])).max() < 1e-4
    assert out is not None and len(out["ap2d"]) == 16 and len(out["pck3d"]) == 15


def test_yolo_a2j_engine_chains_boxes_into_crops(gpu):
    """YoloA2JEngine: pn_yolo_frame.bbox_org + conf become the A2J rows (a frame without a detection: the confidence-0 row); one person
    list per frame, 15 joints each, the confidences those of the boxes.  A 96 x 96 crop keeps it quick and runs the crop kernel and
    the vote at another size than 288."""
    from popnet_amd import synth
    from popnet_amd.pipeline import YoloA2JEngine, yolo_box_rows
    eng = YoloA2JEngine(precision="bf16", device=gpu, max_batch=2, crop=96)
    depth = torch.from_numpy(synth.synth_depth(2, 640, 480, seed=7)).to(gpu)
    rows = yolo_box_rows(eng.yolo.predict_host(depth))
    p2, p3, pc = eng.predict_lists(depth)
    assert len(p2) == len(p3) == len(pc) == 2
    for f in range(2):
        mine = rows[rows[:, 0] == f]
        assert len(mine) >= 1 and np.array(p2[f]).shape == (len(mine), 15, 2) and np.array(p3[f]).shape == (len(mine), 15, 3)
        assert np.isfinite(np.array(p2[f])).all() and np.isfinite(np.array(p3[f])).all()
        assert np.array_equal(np.array(pc[f]), np.repeat(mine[:, 5:6].astype(np.float64), 15, axis=1))
        for k, r in enumerate(mine):
            if r[5] == 0:      # no detection: the person at (-1, -1)
                assert np.array_equal(np.array(p2[f][k]), np.full((15, 2), -1.0))
