"""Yolo-A2J in bf16x3 on the GPU: every launch of the compiled plane-pair net, the vote on [hi | lo] head rows, the end-to-end joints and the chain.

The nets are the rows of tests/a2j_x3_plan_cases.py (tests/test_a2j_x3_plan_cases.py shows without a GPU that they hold every kernel instance of the
bf16x3 plans the engines deploy); weights, inputs, the fp64 step reference and the vote reference are those of tests/test_gpu_a2j.py.  A bf16x3 net
has 58 steps: the 57 of the bf16 net with the stem and the max pool as two launches.

What a plane pair must satisfy, checked on every compared output: the lo plane is written (not all zero), and hi is a bf16 nearest to hi + lo.
The second reads `hi == RNE_bf16(hi + lo)` except at ties: lo = RNE_bf16(v - hi) rounds a remainder just under half an ulp of hi UP to exactly
half an ulp (one stored value in about a thousand), hi + lo is then the midpoint of two bf16 neighbours and round-to-nearest-even names the even one,
which is hi only half the time.  So: hi == RNE_bf16(hi + lo), or |lo| is exactly half an ulp of hi; the count of ties is printed.

End to end, the bound on |gpu joints - golden fp64 joints| is 2 x the emulated cost of the format (tests/a2j_x3_emulation.py::DEVIATION: fp64
sums, so the factor 2 is for the fp32 accumulators' other rounding path) + the golden's own fp32 joints tolerance (4 x the reference's fp32
error: any fp32 summation order); separately z <= 1e-3, the north-star tolerance of BASELINE.json.
"""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2j_cases as AC  # noqa: E402
import a2j_layer_reference as ALR  # noqa: E402
import a2j_plan_cases as APC  # noqa: E402
import a2j_x3_emulation as EMU  # noqa: E402
import a2j_x3_plan_cases as XPC  # noqa: E402
import layer_reference as LR  # noqa: E402
import test_gpu_a2j as TG  # noqa: E402
from popnet_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN, ROOT = TG.GOLDEN, TG.ROOT
NORTH_STAR_Z = 1e-3          # BASELINE.json: the tolerance on a 3D joint, metres


@pytest.fixture(scope="module")
def fx():
    g = np.load(os.path.join(GOLDEN, "a2j.npz"))
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(g["shapes"], g["ndim"])]
    return g, AC.state_dict_for_seed(int(g["seed"]), [str(k) for k in g["keys"]], shapes)


class _NetX3(TG._Net):
    """tests/test_gpu_a2j.py::_Net reading plane pairs: an activation is hi + lo with the hi plane the kernels read."""

    def plane(self, i, which):
        H, W, Cc = self.info["bufs"][i]
        out = np.empty((self.B, Cc, H, W), np.float32)
        self.ctx.check(self.L.pn_net_read_activation(self.h, ("buf%d.%s" % (i, which)).encode(), self.B, out.ctypes.data_as(C.c_void_p), out.size,
                                                     _lib.current_stream_ptr(self.gpu)), "pn_net_read_activation")
        return torch.from_numpy(out).to(torch.float64)

    def reader(self):
        cache = {}

        def read(i):
            if i not in cache:
                hi = self.plane(i, "hi")
                cache[i] = LR.Act(hi + self.plane(i, "lo"), hi)
            return cache[i]
        return read

    def check_steps(self, which=lambda st: True, dil_of=ALR.reported_dil):
        """-> ([(step, kernel, name, report)], [(step, name, lo plane written, stored values that are no valid pair, ties)])"""
        xf = self.x.cpu().to(torch.float64)
        results, pairs = [], []
        for k, st in enumerate(self.steps):
            if not which(st):
                continue
            self.forward(k)
            checks = ALR.step_reference(st, self.info, self.sd, self.reader(), xf, dil_of=dil_of)
            self.forward(k + 1)
            after = self.reader()
            for ch in checks:
                assert ch.where[0] == "buf"
                sl = slice(ch.where[2], ch.where[2] + ch.r.shape[1])
                act = after(ch.where[1])
                results.append((k, st["kernel"], ch.name, LR.compare(act.v[:, sl], ch.r, ch.allow, frames=self.frames)))
                hi, lo = act.hi[:, sl], (act.v - act.hi)[:, sl]
                _, e = torch.frexp(hi)
                tie = (lo.abs() == torch.ldexp(torch.ones_like(hi), e - 9)) & (hi != 0)
                ok = (hi == LR.rne_bf16(hi + lo)) | tie
                pairs.append((k, ch.name, bool((lo != 0).any()), int((~ok).sum()), int(tie.sum())))
        return results, pairs


_NETS = {}


@pytest.fixture(scope="module")
def nets(fx, gpu):
    def get(case, monkeypatch=None):
        """case: a row of tests/a2j_x3_plan_cases.py"""
        id_, prec, H, W, B, mb, which = XPC.BY_ID[case[0]]
        if id_ not in _NETS:
            _NETS[id_] = _NetX3(fx[1], gpu, prec, H, W, B, mb, monkeypatch)
            _NETS[id_].case = case
            assert _NETS[id_].info["prec"] == "bf16x3"
        return _NETS[id_]
    yield get
    _NETS.clear()


def _assert_steps(results, pairs):
    assert not TG._report(results), "\n".join(TG._report(results))
    assert all(r[3]["worst"] > 0 for r in results if "pool" not in r[2]), [(r[0], r[2]) for r in results if r[3]["worst"] == 0]
    assert all(p[2] for p in pairs), [p[:2] for p in pairs if not p[2]]                # both planes are written
    assert all(p[3] == 0 for p in pairs), [p for p in pairs if p[3]]                   # hi is the nearest bf16 of hi + lo (ties: module docstring)


# ---- 1. every launch against fp64 --------------------------------------------------------------------------------
def test_every_step_within_fp64_allowance_80x96(nets):
    net = nets(XPC.SMALL)
    assert len(net.steps) == 58 and [st["kernel"] for st in net.steps[:2]] == ["stem7x7_mfma_kernel<x3>", "pool_kernel<1, split>"]
    dil = [st for st in net.steps if APC.is_dilated(st)]
    assert len(dil) == 2 and all(c["dil"] == 2 and ", 2>" in st["kernel"] for st in dil for c in st["convs"])
    assert not any("blocked_acc" in c for st in net.steps if st["type"] == "conv" for c in st["convs"])
    results, pairs = net.check_steps(which=APC.selects(APC.ALL))
    assert len(results) >= len(net.steps)
    print("\nA2J X3 LAYERS 80x96: %d steps, worst |gpu - r| / allowance = %.4f, %d ties among the stored pairs" % (
        len(net.steps), max(r[3]["worst"] for r in results), sum(p[4] for p in pairs)))
    _assert_steps(results, pairs)


@pytest.mark.parametrize("case", [XPC.LARGE_32, XPC.LARGE_2], ids=[XPC.LARGE_32[0], XPC.LARGE_2[0]])
def test_steps_of_the_deployed_plans_keys_within_fp64_allowance_288(nets, monkeypatch, case):
    """288 x 288, two crops, compiled for max_batch 32 and 2: the steps that first launch the instance keys the 80 x 96 net does not."""
    id_, prec, H, W, B, mb, which = case
    net = nets(case, monkeypatch)
    assert net.info["max_batch"] == mb and net.B == 2
    keys = APC.key_part(which)
    results, pairs = net.check_steps(which=APC.selects(which))
    seen = {APC.instance_key(c) for k in {r[0] for r in results} for c in net.steps[k]["convs"]}
    assert keys <= seen, sorted(keys - seen)
    print("\nA2J X3 LAYERS %s: %d steps compared, worst |gpu - r| / allowance = %.4f" % (id_, len({r[0] for r in results}), max(r[3]["worst"] for r in results)))
    _assert_steps(results, pairs)


@pytest.mark.parametrize("case", XPC.WIDE, ids=[c[0] for c in XPC.WIDE])
def test_dilated_steps_at_the_wider_pitch_classes(nets, case):
    net = nets(case)
    dil = [st for st in net.steps if APC.is_dilated(st)]
    assert len(dil) == 2 and all(st["convs"][0]["pitch"] == XPC.WIDE_PITCH[case[3]] for st in dil), [st["kernel"] for st in dil]
    results, pairs = net.check_steps(which=APC.selects(APC.DIL_OUT))
    assert len(results) == 5
    _assert_steps(results, pairs)


def test_reference_with_wrong_dilation_fails(nets):
    net = nets(XPC.SMALL)
    layer4_conv2 = lambda st: st["type"] == "conv" and any(c["w"].startswith("Backbone.model.layer4.") and c["w"].endswith(".conv2") for c in st["convs"])
    plain, _ = net.check_steps(which=layer4_conv2, dil_of=lambda c: 1)
    bad = {r[2] for r in plain if r[3]["n_bad"]}
    assert bad == {"Backbone.model.layer4.1.conv2", "Backbone.model.layer4.2.conv2"}, bad


# ---- 2. the vote on [hi | lo] head rows -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", [XPC.SMALL, XPC.LARGE_32], ids=["80x96", "288x288_max_batch32"])
def test_vote_on_the_x3_nets_heads_within_fp64_allowance(nets, monkeypatch, case):
    """The heads handed to the reference are hi + lo as float32 (A2J_model.forward sums the planes, exactly), so the reference and its allowance
    are the fp32 vote's.  Dropped and doubled anchor rows are rejected as in the bf16 test: one row of 480 at 80 x 96, the 16 anchors of the
    corner cell at 288 x 288 (tests/test_gpu_a2j.py has the arithmetic)."""
    net = nets(case, monkeypatch)
    assert any(bool((t != t.to(torch.bfloat16).float()).any()) for t in net.heads)          # the lo plane carries something
    small = case is XPC.SMALL
    TG._check_vote(net, "%s bf16x3" % ("80x96" if small else "288x288 max_batch 32"), rows=(137,) if small else range(16))


def _pair(a):
    """float32 array -> (hi, lo) bf16 tensors and the float32 value hi + lo."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return hi, lo, (hi.float() + lo.float()).numpy()


def _nhwc_pairs(ref, B, h, w, A, tail):
    """[B, K, ...] in the reference's order (cells column by column) -> [B, h, w, 2 * A * tail] bf16: the [hi | lo] rows of the head maps."""
    hi, lo, val = _pair(ref)
    lay = lambda t: t.reshape(B, w, h, A * tail).permute(0, 2, 1, 3)
    return torch.cat([lay(hi), lay(lo)], -1).contiguous(), val


def _vote_x3(gpu, cls, reg, dep, anchors, B, h, w, prec=_lib.PN_PREC_BF16X3):
    L, ctx = _lib.lib(), _lib.Context.for_device(0)
    out = torch.empty((B, 15, 3), device=gpu)
    a = torch.from_numpy(anchors.astype(np.float32)).to(gpu)
    rc = L.pn_a2j_vote(ctx.handle, C.c_void_p(cls.data_ptr()), C.c_void_p(reg.data_ptr()), C.c_void_p(dep.data_ptr()), prec, B, h, w, 16 if h else 1, 15,
                       C.c_void_p(a.data_ptr()), C.c_void_p(out.data_ptr()), None, None, None, _lib.current_stream_ptr(gpu))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def test_vote_one_hot_probe_on_plane_pairs_is_exact(gpu):
    """Chosen hi and lo planes written directly: every (crop, joint) has one hot anchor, the vote is anchor + (hi + lo) bit for bit."""
    from popnet_amd.network.a2j import generate_anchors, shift
    B, P, h, w = 32, 15, 5, 6
    K = h * w * 16
    assert K == B * P
    rng = np.random.default_rng(11)
    cls = np.full((B, K, P), -1e4, np.float32)
    for b in range(B):
        for p in range(P):
            cls[b, 15 * b + p, p] = 0.3 + 0.01 * p          # not a bf16 value: the hot logit is hi + lo as well
    reg = rng.normal(0, 3, (B, K, P, 2)).astype(np.float32)
    dep = rng.normal(0, 1, (B, K, P)).astype(np.float32)
    c_dev, _ = _nhwc_pairs(cls, B, h, w, 16, P)
    r_dev, r_val = _nhwc_pairs(reg, B, h, w, 16, 2 * P)
    d_dev, d_val = _nhwc_pairs(dep, B, h, w, 16, P)
    assert (r_val != reg).any() and (r_val.astype(np.float32) != torch.from_numpy(reg).to(torch.bfloat16).float().numpy()).any()      # 16 bits: neither fp32 nor bf16
    anchors = shift([h, w], 16, generate_anchors()).astype(np.float32)
    rc, out = _vote_x3(gpu, c_dev.to(gpu), r_dev.to(gpu), d_dev.to(gpu), anchors, B, h, w)
    assert rc == 0
    for b in range(B):
        for p in range(P):
            k = 15 * b + p
            want = np.array([anchors[k, 0] + r_val[b, k, p, 0], anchors[k, 1] + r_val[b, k, p, 1], d_val[b, k, p]], np.float32)
            assert np.array_equal(out[b, p].view(np.uint32), want.view(np.uint32)), (b, p, out[b, p], want)


def test_vote_refusals_that_stay(gpu):
    B, h, w = 1, 2, 2
    z = torch.zeros((B, h, w, 4 * 16 * 15), device=gpu, dtype=torch.bfloat16)
    anchors = np.zeros((h * w * 16, 2), np.float32)
    ctx = _lib.Context.for_device(0)
    assert _vote_x3(gpu, z, z, z, anchors, B, h, w)[0] == 0
    assert _vote_x3(gpu, z, z, z, anchors, B, h, w, prec=7)[0] != 0 and "f32, bf16 or bf16x3" in ctx.last_error()
    # the [B, K, P] entry (h == 0, K passed as w) takes f32 tensors only
    assert _vote_x3(gpu, z, z, z, anchors, B, 0, h * w * 16)[0] != 0 and "takes f32 tensors" in ctx.last_error()
    assert _vote_x3(gpu, z, z, z, anchors, B, 0, h * w * 16, prec=_lib.PN_PREC_BF16)[0] != 0


# ---- 3. end to end against the reference's fp64 run -------------------------------------------------------------------
def _bound(size, tol):
    """(pixels, z): 2 x the emulated deviation + the golden's fp32 tolerance"""
    return 2 * EMU.DEVIATION[size][0] + tol, 2 * EMU.DEVIATION[size][1] + tol


@pytest.mark.parametrize("size", ["s", "l"])
def test_x3_joints_within_the_format_bound_of_the_reference(nets, fx, monkeypatch, size):
    """Measured on an MI355X (profiles/a2j_notes.md has the same lines): 80 x 96, 3 crops: 2.96e-5 px against a bound of 2.05e-4, 2.15e-6 in z against
    1.56e-4; 288 x 288, 2 crops, the max_batch 32 plan: 1.46e-4 px against 1.60e-3, 8.70e-6 in z against 1.39e-3 (and against the north star's 1e-3).
    The emulated format alone is 2.82e-5 / 3.48e-6 and 1.12e-4 / 7.20e-6; bf16 is 0.0992 px / 0.00798 from the same run."""
    g = fx[0]
    net = nets(XPC.SMALL if size == "s" else XPC.LARGE_32, monkeypatch)
    joints, _ = net.vote()
    d = np.abs(joints - g["%s_joints" % size])
    px, z = float(d[..., :2].max()), float(d[..., 2].max())
    bpx, bz = _bound(size, float(g["%s_joints_tol" % size]))
    print("\nA2J E2E bf16x3 %s joints against the fp64 reference: %.6g px (bound %.6g), %.6g in z (bound %.6g)" % (size, px, bpx, z, bz))
    assert np.isfinite(joints).all() and all(bool(torch.isfinite(t).all()) for t in net.heads)
    assert px <= bpx and z <= bz, (px, bpx, z, bz)
    assert z <= NORTH_STAR_Z
    assert px > 0 and z > 0


# ---- 4. the Python surface and the chain -----------------------------------------------------------------------------------
def test_forward_returns_the_reference_layout(nets):
    net = nets(XPC.SMALL)
    H, W, B = AC.SMALL
    K = (H // 16) * (W // 16) * 16
    cls, reg, dep = net.heads
    assert tuple(cls.shape) == (B, K, 15) and tuple(reg.shape) == (B, K, 15, 2) and tuple(dep.shape) == (B, K, 15)
    ptrs, (h, w), prec = net.m.run(net.x)
    assert (h, w) == (H // 16, W // 16) and prec == _lib.PN_PREC_BF16X3
    hh, ww, pp = C.c_int(), C.c_int(), C.c_int()
    net.ctx.check(net.L.pn_a2j_head_shape(net.h, C.byref(hh), C.byref(ww), C.byref(pp)), "pn_a2j_head_shape")
    assert (hh.value, ww.value, pp.value) == (h, w, _lib.PN_PREC_BF16X3)


def test_chain_predict_lists_within_the_format_bound(gpu, fx):
    """tests/test_gpu_a2j.py::test_chain_predict_lists_equals_the_reference in bf16x3: the same three box rows through max_batch = 2, the same golden,
    the same map-back arithmetic; chain_tol (the golden's fp32 tolerance of the chain's votes) becomes the end-to-end bound of the 288 x 288 shape."""
    from popnet_amd.pipeline import A2JEngine
    g, sd = fx
    eng = A2JEngine(precision="bf16x3", state_dict=sd, device=gpu, max_batch=2)
    frames = torch.from_numpy(AC.depth_frames(AC.SEED + 1, 2)).to(gpu)
    p2, p3, pc = eng.predict_lists(frames, AC.CHAIN_ROWS)
    assert [len(f) for f in p2] == [1, 2] and [len(f) for f in p3] == [1, 2]
    assert pc[0] == [[0.0] * 15] and pc[1] == [[float(c)] * 15 for c in g["chain_conf"][1:]]
    recs = eng.predict_host(frames, AC.CHAIN_ROWS)
    assert eng.last_flags.cpu().tolist() == [0, 0, 0] and recs["frame"].tolist() == g["chain_frame"].tolist()
    tol, tolz = _bound("l", float(g["chain_tol"]))
    got2 = np.array(p2[0] + p2[1]); got3 = np.array(p3[0] + p3[1])
    rows = AC.CHAIN_ROWS.astype(np.float64)
    size = np.stack([rows[:, 3] - rows[:, 1], rows[:, 4] - rows[:, 2]], -1)[:, None, :]
    want2, want3 = g["chain_xy"].astype(np.float64), g["chain_xyz"].astype(np.float64)
    tol2 = tol * size / 288.0 + 4 * 2.0 ** -23 * np.abs(want2)
    print("\nA2J CHAIN bf16x3: worst |xy - golden| %.4g px, |z - golden| %.4g (bounds on the votes: %.4g px, %.4g)" % (
        np.abs(got2 - want2)[1:].max(), np.abs(got3[..., 2] - want3[..., 2]).max(), tol, tolz))
    assert (np.abs(got2 - want2) <= tol2).all(), np.abs(got2 - want2).max()
    assert np.array_equal(got2[0], np.full((15, 2), -1.0))
    c = np.array([AC.INTRINSICS["cx"], AC.INTRINSICS["cy"]]); f = np.array([AC.INTRINSICS["fx"], AC.INTRINSICS["fy"]])
    z = np.abs(want3[..., 2:3])
    tol3 = (tol2 * (z + tolz) + np.abs(want2 - c) * tolz) / f + 4 * 2.0 ** -23 * np.abs(want3[..., :2])
    assert (np.abs(got3[..., :2] - want3[..., :2]) <= tol3).all() and (np.abs(got3[..., 2] - want3[..., 2]) <= tolz).all()
    # votes(): the same crops through pn_a2j_forward + pn_a2j_vote, against the golden's fp64 votes of the chain
    crops, _ = eng.crops(frames, AC.CHAIN_ROWS)
    votes = eng.votes(crops).cpu().numpy()
    dv = np.abs(votes - g["chain_votes"])
    assert dv[..., :2].max() <= tol and dv[..., 2].max() <= tolz, (dv[..., :2].max(), dv[..., 2].max())


def test_a2j_set_votes_runs_the_x3_engine(gpu, fx):
    """a2j_set_votes (the trainers' test loop): train_crops + votes in batches, here two boxes one at a time -- the votes of the same crops in one call."""
    from popnet_amd import a2j_crops
    from popnet_amd.pipeline import A2JEngine, a2j_set_votes
    eng = A2JEngine(precision="bf16x3", state_dict=fx[1], device=gpu, max_batch=2)
    frames = torch.from_numpy(AC.depth_frames(AC.SEED + 1, 2)).to(gpu)
    boxes = AC.CHAIN_ROWS[1:, 1:5]
    kp2, kp3 = np.zeros((2, 15, 2), np.float32), np.zeros((2, 15, 3), np.float32)

    def batch_fn(idx):
        items, labels = a2j_crops.box_items(idx, boxes, kp2, kp3, (AC.FRAME_H, AC.FRAME_W), frames=[1] * len(idx))
        return frames, items, labels
    one = a2j_set_votes(eng, batch_fn, 2, 1)
    crops, flags = eng.train_crops(frames, batch_fn([0, 1])[1])
    both = eng.votes(crops).cpu().numpy()
    assert flags.cpu().tolist() == [0, 0] and one.shape == (2, 15, 3) and np.isfinite(one).all()
    assert np.array_equal(one.view(np.uint32), both.view(np.uint32))


def test_yolo_a2j_engine_runs_both_stages_in_x3(gpu):
    from popnet_amd import synth
    from popnet_amd.pipeline import YoloA2JEngine, yolo_box_rows
    eng = YoloA2JEngine(precision="bf16x3", device=gpu, max_batch=2, crop=96)
    assert eng.yolo.model.precision == "bf16x3" and eng.a2j.model.precision == "bf16x3"
    depth = torch.from_numpy(synth.synth_depth(2, 640, 480, seed=7)).to(gpu)
    rows = yolo_box_rows(eng.yolo.predict_host(depth))
    p2, p3, pc = eng.predict_lists(depth)
    assert len(p2) == len(p3) == len(pc) == 2
    for f in range(2):
        mine = rows[rows[:, 0] == f]
        assert len(mine) >= 1 and np.array(p2[f]).shape == (len(mine), 15, 2) and np.array(p3[f]).shape == (len(mine), 15, 3)
        assert np.isfinite(np.array(p2[f])).all() and np.isfinite(np.array(p3[f])).all()
        assert np.array_equal(np.array(pc[f]), np.repeat(mine[:, 5:6].astype(np.float64), 15, axis=1))


def test_evaluate_mpreal_a2j_script_in_x3_writes_what_the_metrics_consume(gpu, golden, fx, tmp_path):
    """scripts/evaluate_mpreal_a2j.py --precision bf16x3 on the fake two-frame dataset tree of tests/test_gpu_a2j.py's script test."""
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
                    "--a2j-weight", str(tmp_path / "a2j.pth"), "--output-dir", str(tmp_path / "out"), "--precision", "bf16x3"])
    data = json.load(open(tmp_path / "out" / "eval_data.json"))
    assert sorted(data) == ["human_gt_set_2d", "human_gt_set_3d", "human_pred_set_2d", "human_pred_set_3d", "human_pred_set_part_conf"]
    n_ref = [len(f) for f in s["human_pred_set_2d"]]
    for b in range(2):
        p2, p3, pc = (np.array(data[k][b]) for k in ("human_pred_set_2d", "human_pred_set_3d", "human_pred_set_part_conf"))
        assert p2.shape == (max(n_ref[b], 1), 15, 2) and p3.shape == (max(n_ref[b], 1), 15, 3) and pc.shape == (max(n_ref[b], 1), 15)
        assert np.isfinite(p2).all() and np.isfinite(p3).all() and (pc == pc[:, :1]).all()
        if n_ref[b]:      # the boxes are YoloPoseNet's, here in bf16x3: the confidences of its fp32 evaluation within the mode's tolerance
            assert np.abs(pc - np.array(s["human_pred_set_part_conf"][b])).max() < 1e-4
    assert out is not None and len(out["ap2d"]) == 16 and len(out["pck3d"]) == 15
