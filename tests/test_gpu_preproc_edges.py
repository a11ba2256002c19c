"""The stand-alone pre-processing and the frames-in stems on edge-case depth frames (tests/preproc_cases.py; its census is in
tests/test_preproc_cases.py, without a GPU).

PoseEngine.predict, YoloEngine.predict and bench.py go through pn_rtpose_forward_frames / pn_yolo_forward_frames: the 7x7 stem reads
the raw frames and computes its input tile itself (popnet_amd/csrc/preproc_pixel.h).  The per-layer checks (test_gpu_layers.py,
test_gpu_layer_shapes.py) take a pre-processed x and so only ever launch the SRC = 0 stems.  Here:

  a  pn_preprocess == oracle.preproc.preprocess_frame on every case, bit for bit, written into the middle of a larger buffer whose
     rest must stay untouched, and a batch of three == three batches of one;
  b  the refusals (exact 2x decimation on both axes, a one-pixel side) of pn_preprocess, pn_*_forward_frames and
     pn_net_forward_frames_partial, and the partial entry's own checks;
  c  the stem by itself: pn_preprocess + pn_net_forward_partial(1) against pn_net_forward_frames_partial(1) on the raw frames, the
     stored stem (or fused stem + pool) output compared as int32, with a scrub in between so that a launch that writes nothing fails;
  d  the whole forward: pn_*_forward_frames (and the partial entry run to the last step) against pn_preprocess + pn_*_forward;
  e  the engines at input sizes 40 / 48 with the default and the ITOP profile.

No tolerance anywhere.  This chains the frames-in stems to fp64: the SRC = 0 stems are held to the fp64 allowance at small and ragged
sizes by test_gpu_layer_shapes.py, x is held to the oracle by (a), and (c) holds the frames-in stems to the SRC = 0 stems on that x.
bf16x3 is the sensitive arm of (c): its tile keeps 16 significant bits of every pixel.

Every comparison is one of int32 views, so that NaN positions count (and, as it turns out, the NaNs' sign and payload: Inf * 0 on
the device gives the pattern the host's oracle gives).
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import state_dict_from_keys  # noqa: E402
import preproc_cases as PC  # noqa: E402
from test_gpu_layers import _model, _step_info  # noqa: E402
from oracle import preproc as OP  # noqa: E402
from popnet_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

PN_ERR_INVALID, PN_ERR_STATE, PN_ERR_UNSUPPORTED = -1, -3, -4      # include/popnet_hip.h
B, MAX_BATCH = PC.B, 4
SENTINEL = 123.25
COUNTS = {"pixels": 0, "stem_elements": 0, "map_elements": 0, "nets": 0, "t0": time.time()}

# (kind, precision, S, environment read when the net is compiled)
NETS = [("rtpose", p, S, ()) for p in ("bf16", "bf16x3") for S in PC.RT_S]
NETS += [("yolo", "bf16", S, ()) for S in PC.YOLO_S if S != 48]
NETS += [("yolo", "bf16x3", 48, ()), ("yolo", "bf16", 112, (("POPNET_NO_STEMPOOL", "1"),))]


def _net_id(n):
    return "%s_%s_%d%s" % (n[0], n[1], n[2], "".join("_" + k[7:].lower() + v for k, v in n[3]))


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _dt(t):
    return _lib.PN_DEPTH_F16 if t.dtype == torch.float16 else _lib.PN_DEPTH_F32


def _i32(t):
    return t.contiguous().view(torch.int32)


def _preprocess(gpu, fr, out, S, consts):
    ctx, n = _lib.Context.for_device(0), fr.shape[0]
    ctx.check(_lib.lib().pn_preprocess(ctx.handle, _vp(fr), _dt(fr), n, fr.shape[1], fr.shape[2], _vp(out), S, *consts, _lib.current_stream_ptr(gpu)),
              "pn_preprocess")


# ---------------------------------------------------------------------------------------------
# a. pn_preprocess against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", PC.ALL_S)
def test_preprocess_equals_the_oracle_bit_for_bit(gpu, S):
    cs = PC.cases_for(S)
    assert len(cs) >= 4
    for c in cs:
        fr = torch.tensor(c.frames).to(gpu)
        buf = torch.full(((B + 2) * S * S,), float("nan"), device=gpu)
        fill = _i32(buf).clone()
        out = buf[S * S:(B + 1) * S * S]
        _preprocess(gpu, fr, out, S, c.consts)
        got = out.cpu().numpy().reshape(B, 1, S, S)
        ref = PC.reference(c)
        assert np.array_equal(got.view(np.int32), ref.view(np.int32)), (c.name, int((got.view(np.int32) != ref.view(np.int32)).sum()))
        assert torch.equal(_i32(buf)[:S * S], fill[:S * S]) and torch.equal(_i32(buf)[(B + 1) * S * S:], fill[(B + 1) * S * S:]), c.name
        single = torch.full((B, S * S), float("nan"), device=gpu)             # a frame must not depend on its neighbours in the batch
        for b in range(B):
            _preprocess(gpu, fr[b:b + 1], single[b], S, c.consts)
        assert torch.equal(_i32(single).view(-1), _i32(out)), c.name
        COUNTS["pixels"] += got.size


@pytest.mark.parametrize("S", PC.ALL_S)
def test_preprocess_refusals_leave_the_output_alone(gpu, S):
    ctx, L = _lib.Context.for_device(0), _lib.lib()
    out = torch.full((B, 1, S, S), SENTINEL, device=gpu)
    H2, W2 = PC.refused(S)
    for dtype in (torch.float16, torch.float32):
        fr = torch.ones((B, H2, W2), device=gpu, dtype=dtype)
        rc = L.pn_preprocess(ctx.handle, _vp(fr), _dt(fr), B, H2, W2, _vp(out), S, 6.0, 3.0, 2.0, _lib.current_stream_ptr(gpu))
        assert rc == PN_ERR_UNSUPPORTED and "%dx%d -> %d" % (W2, H2, S) in ctx.last_error(), (rc, ctx.last_error())
        for H, W in ((1, 5), (5, 1), (1, 1)):
            assert L.pn_preprocess(ctx.handle, _vp(fr), _dt(fr), B, H, W, _vp(out), S, 6.0, 3.0, 2.0, _lib.current_stream_ptr(gpu)) == PN_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------
# the compiled nets: one per (kind, precision, S, environment), shared by b, c and d
# ---------------------------------------------------------------------------------------------
class _FramesNet:
    def __init__(self, golden, gpu, spec):
        self.kind, self.prec, self.S, env = spec
        self.env = dict(env)
        self.gpu, S = gpu, self.S
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env:
                mp.setenv(k, v)
            self.m = _model(golden, self.kind, False)
            self.m.precision = self.prec
            self.h = self.m._compile(gpu, MAX_BATCH, S, S)
        self.ctx, self.L = _lib.Context.for_device(0), _lib.lib()
        if self.kind == "rtpose":
            chans = (self.m.num_limbs * 2, self.m.num_parts + 1, self.m.num_limbs + 1)
            self.outs = [torch.zeros((MAX_BATCH, c, S // 8, S // 8), device=gpu) for c in chans]
        else:
            self.outs = [torch.zeros((MAX_BATCH, len(self.m.anchors) * (5 + 3 * self.m.num_parts), S // 16, S // 16), device=gpu)]
        self.x = torch.zeros((MAX_BATCH, 1, S, S), device=gpu)
        self.forward()                                                   # the partial entries need one full forward
        self.info = _step_info(self.h, -1)
        self.nsteps = self.L.pn_net_num_steps(self.h)
        st = _step_info(self.h, 0)
        assert st["type"] == "stem" and st["cin"] == 1, st
        self.stem = st
        self.stem_buf = st["pool_buf"] if st["pool_buf"] >= 0 else st["out_buf"]
        COUNTS["nets"] += 1

    def _s(self):
        return _lib.current_stream_ptr(self.gpu)

    def forward(self):
        if self.kind == "rtpose":
            rc = self.L.pn_rtpose_forward(self.h, _vp(self.x), B, *(_vp(o) for o in self.outs), self._s())
        else:
            rc = self.L.pn_yolo_forward(self.h, _vp(self.x), B, _vp(self.outs[0]), self._s())
        self.ctx.check(rc, "pn_*_forward")

    def frames_rc(self, fr, H=None, W=None, consts=(6.0, 3.0, 2.0)):
        H, W = fr.shape[1] if H is None else H, fr.shape[2] if W is None else W
        if self.kind == "rtpose":
            return self.L.pn_rtpose_forward_frames(self.h, _vp(fr), _dt(fr), B, H, W, *consts, *(_vp(o) for o in self.outs), self._s())
        return self.L.pn_yolo_forward_frames(self.h, _vp(fr), _dt(fr), B, H, W, *consts, _vp(self.outs[0]), self._s())

    def frames_partial_rc(self, fr, nsteps, H=None, W=None, consts=(6.0, 3.0, 2.0)):
        H, W = fr.shape[1] if H is None else H, fr.shape[2] if W is None else W
        return self.L.pn_net_forward_frames_partial(self.h, _vp(fr), _dt(fr), B, H, W, *consts, nsteps, self._s())

    def partial(self, nsteps):
        self.ctx.check(self.L.pn_net_forward_partial(self.h, _vp(self.x), B, nsteps, self._s()), "pn_net_forward_partial")

    def read_stem(self):
        """the stored planes of the stem step's output, float32 [planes, B, C, H, W] (bf16 values, exact in float32)"""
        H, W, Cc = self.info["bufs"][self.stem_buf]
        names = ["buf%d.hi" % self.stem_buf, "buf%d.lo" % self.stem_buf] if self.prec == "bf16x3" else ["buf%d" % self.stem_buf]
        out = np.empty((len(names), B, Cc, H, W), np.float32)
        for i, name in enumerate(names):
            self.ctx.check(self.L.pn_net_read_activation(self.h, name.encode(), B, out[i].ctypes.data_as(C.c_void_p), out[i].size, self._s()),
                           "pn_net_read_activation")
        return out

    def fill_outs(self, v):
        for o in self.outs:
            o.fill_(v)

    def maps(self):
        torch.cuda.synchronize()
        return [_i32(o[:B]).clone() for o in self.outs]


@pytest.fixture(scope="module", params=NETS, ids=[_net_id(n) for n in NETS])
def net(request, golden, gpu):
    n = _FramesNet(golden, gpu, request.param)
    yield n
    n.m.invalidate()


def test_net_list(gpu):
    assert len(NETS) == 17 and len(set(NETS)) == 17
    assert {(n[1], n[2]) for n in NETS if n[0] == "rtpose"} == {(p, S) for p in ("bf16", "bf16x3") for S in (8, 32, 40, 136, 224)}
    assert {(n[1], n[2], n[3]) for n in NETS if n[0] == "yolo"} == {("bf16", S, ()) for S in (16, 32, 112, 224, 240)} | {
        ("bf16x3", 48, ()), ("bf16", 112, (("POPNET_NO_STEMPOOL", "1"),))}


# ---------------------------------------------------------------------------------------------
# c. the stem by itself
# ---------------------------------------------------------------------------------------------
def test_frames_in_stem_equals_the_stem_on_the_preprocessed_frames(net):
    fused = net.stem["pool_buf"] >= 0            # the yolo bf16 net's first step is the fused stem + pool launch unless POPNET_NO_STEMPOOL=1 was set
    assert fused == (net.kind == "yolo" and net.prec == "bf16" and not net.env), net.stem
    cs = PC.cases_for(net.S)
    assert {c.geom for c in cs} >= set(PC.GEOMETRY_NAMES) and {c.dtype for c in cs} == {np.float16, np.float32}
    print("\nSTEM %s %s S = %d: step 0 kernel %s, %s, %d cases" % (net.kind, net.prec, net.S, net.stem["kernel"],
                                                                 "fused stem + pool" if fused else "stem", len(cs)))
    for c in cs:
        fr = torch.tensor(c.frames).to(net.gpu)
        net.x.fill_(float("nan"))
        _preprocess(net.gpu, fr, net.x, net.S, c.consts)
        net.partial(1)
        want = net.read_stem()
        assert want.max() > 0, c.name
        net.x.zero_()                                                              # scrub: a frames-in launch that writes nothing must not pass
        net.partial(1)
        scrub = net.read_stem()
        assert not np.array_equal(scrub.view(np.int32), want.view(np.int32)), c.name
        net.x.fill_(float("nan"))                                                  # and one that reads x would show
        net.ctx.check(net.frames_partial_rc(fr, 1, consts=c.consts), "pn_net_forward_frames_partial")
        got = net.read_stem()
        diff = got.view(np.int32) != want.view(np.int32)
        assert not diff.any(), (c.name, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        COUNTS["stem_elements"] += got.size


# ---------------------------------------------------------------------------------------------
# d. the whole forward
# ---------------------------------------------------------------------------------------------
def test_frames_in_forward_equals_preprocess_plus_forward_on_edge_frames(net):
    cs = PC.cases_for(net.S, ("down", "up", "mixed2x"))
    assert {c.geom for c in cs} == {"down", "up", "mixed2x"} and {c.values for c in cs} == {"plain", "nonfinite"}
    for c in cs:
        fr = torch.tensor(c.frames).to(net.gpu)
        net.x.fill_(float("nan"))
        _preprocess(net.gpu, fr, net.x, net.S, c.consts)
        net.fill_outs(float("nan"))
        net.forward()
        two = net.maps()
        net.x.fill_(float("nan"))
        net.fill_outs(float("nan"))
        net.ctx.check(net.frames_rc(fr, consts=c.consts), "pn_*_forward_frames")
        one = net.maps()
        net.fill_outs(float("nan"))
        net.ctx.check(net.frames_partial_rc(fr, net.nsteps, consts=c.consts), "pn_net_forward_frames_partial")
        part = net.maps()
        for a, b, p in zip(two, one, part):
            assert torch.equal(a, b), c.name
            assert torch.equal(a, p), c.name
            COUNTS["map_elements"] += a.numel()


# ---------------------------------------------------------------------------------------------
# b. refusals of the net entries
# ---------------------------------------------------------------------------------------------
def test_net_entries_refuse_what_pn_preprocess_refuses(net):
    S = net.S
    H2, W2 = PC.refused(S)
    fr = torch.ones((B, H2, W2), device=net.gpu, dtype=torch.float16)
    net.fill_outs(SENTINEL)
    net.x.zero_()
    net.partial(1)
    before = net.read_stem()
    for call in (lambda **kw: net.frames_rc(fr, **kw), lambda **kw: net.frames_partial_rc(fr, 1, **kw), lambda **kw: net.frames_partial_rc(fr, net.nsteps, **kw)):
        rc = call()
        assert rc == PN_ERR_UNSUPPORTED and "%dx%d -> %d" % (W2, H2, S) in net.ctx.last_error(), (rc, net.ctx.last_error())
        for H, W in ((1, 5), (5, 1)):
            assert call(H=H, W=W) == PN_ERR_INVALID
    # the partial entry's own two checks come after those: nsteps in range (one full forward has run)
    ok = torch.ones((B, 5, 7), device=net.gpu, dtype=torch.float32)
    for nsteps in (-1, net.nsteps + 1):
        assert net.frames_partial_rc(ok, nsteps) == PN_ERR_INVALID and "nsteps" in net.ctx.last_error()
    assert net.frames_partial_rc(fr, -1) == PN_ERR_UNSUPPORTED                     # (the refusal of the sizes comes first)
    assert net.L.pn_net_forward_frames_partial(net.h, None, _lib.PN_DEPTH_F16, B, 5, 7, 6.0, 3.0, 2.0, 1, net._s()) == PN_ERR_INVALID
    assert net.L.pn_net_forward_frames_partial(net.h, _vp(ok), 7, B, 5, 7, 6.0, 3.0, 2.0, 1, net._s()) == PN_ERR_INVALID
    assert net.L.pn_net_forward_frames_partial(net.h, _vp(ok), _lib.PN_DEPTH_F32, MAX_BATCH + 1, 5, 7, 6.0, 3.0, 2.0, 1, net._s()) == PN_ERR_INVALID
    assert net.frames_partial_rc(ok, 0) == 0                                       # no step: nothing runs, nothing is written
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in net.outs)
    assert np.array_equal(net.read_stem().view(np.int32), before.view(np.int32))


def test_partial_frames_entry_state_and_precision_checks(gpu, golden):
    """Before the first full forward the partial entry answers PN_ERR_STATE; an fp32 net and a net that is not square are refused as
    pn_*_forward_frames refuses them; a null net is PN_ERR_INVALID."""
    L, ctx = _lib.lib(), _lib.Context.for_device(0)
    fr = torch.ones((B, 5, 7), device=gpu, dtype=torch.float16)
    args = (_vp(fr), _lib.PN_DEPTH_F16, B, 5, 7, 6.0, 3.0, 2.0, 1, _lib.current_stream_ptr(gpu))
    assert L.pn_net_forward_frames_partial(None, *args) == PN_ERR_INVALID
    for kind in ("rtpose", "yolo"):
        m = _model(golden, kind, False)
        m.precision = "bf16"
        h = m._compile(gpu, MAX_BATCH, 32, 32)
        assert L.pn_net_forward_frames_partial(h, *args) == PN_ERR_STATE and "full forward first" in ctx.last_error()
        m.invalidate()
    m = _model(golden, "rtpose", False)
    m.precision = "fp32"
    h = m._compile(gpu, MAX_BATCH, 32, 32)
    assert L.pn_net_forward_frames_partial(h, *args) == PN_ERR_UNSUPPORTED and "fp32" in ctx.last_error()
    m.precision = "bf16"
    h = m._compile(gpu, MAX_BATCH, 32, 48)
    assert L.pn_net_forward_frames_partial(h, *args) == PN_ERR_UNSUPPORTED and "square" in ctx.last_error()
    m.invalidate()


# ---------------------------------------------------------------------------------------------
# e. the engines
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", [None, "ITOP"])
@pytest.mark.parametrize("which,S", [("pose", 40), ("yolo", 48)])
def test_engines_frames_in_at_small_sizes_and_profiles(gpu, golden, which, S, profile):
    from popnet_amd.pipeline import PoseEngine, YoloEngine
    if which == "pose":
        eng = PoseEngine(precision="bf16", device=gpu, max_batch=B, input_size=S, profile=profile,
                         state_dict=state_dict_from_keys(golden.keys["rtpose_light3d"], seed=0))
        outs = lambda: (eng.paf, eng.heat, eng.z)
    else:
        eng = YoloEngine(precision="bf16", device=gpu, max_batch=B, input_size=S, profile=profile,
                         state_dict=state_dict_from_keys(golden.keys["yolo_posenet"], seed=1))
        outs = lambda: (eng.out,)
    p = eng.profile
    assert (p.depth_max, p.depth_mean, p.depth_std) == ((5, 3, 2) if profile else (6, 3, 2))
    for c in (c for c in PC.cases_for(S, ("up",)) if c.dtype == np.float16):
        assert c.H < S and c.W < S
        depth = torch.tensor(c.frames).to(gpu)
        eng.x.fill_(float("nan"))
        assert eng.preprocess(depth) == B
        with np.errstate(invalid="ignore", over="ignore"):
            want = OP.preprocess_batch(c.frames, input_size=S, depth_max=p.depth_max, depth_mean=p.depth_mean, depth_std=p.depth_std)
        assert np.array_equal(eng.x[:B].cpu().numpy().view(np.int32), want.view(np.int32)), c.name
        for o in outs():
            o.fill_(float("nan"))
        eng.forward(B)
        torch.cuda.synchronize()
        two = [_i32(o[:B]).clone() for o in outs()]
        for o in outs():
            o.fill_(float("nan"))
        eng.x.fill_(float("nan"))
        assert eng.forward_frames(depth) == B
        torch.cuda.synchronize()
        for a, o in zip(two, outs()):
            assert torch.equal(a, _i32(o[:B])), c.name
    eng.model.invalidate()


def test_zz_record(gpu):
    """Not a check: what the module compared, for the record."""
    print("\nPREPROC EDGES: %d cases, %d nets, %d pre-processed pixels, %d stem-output elements, %d map elements compared, %.1f s" % (
        len(PC.cases()), COUNTS["nets"], COUNTS["pixels"], COUNTS["stem_elements"], COUNTS["map_elements"], time.time() - COUNTS["t0"]))
