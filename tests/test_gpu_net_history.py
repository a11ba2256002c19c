"""A compiled net's forward must not depend on what the net ran before: forward(x, B) is a function of the pixels of x[0..B-1] alone.

Every other inference test compiles a net, runs one batch and compares.  A deployed net is compiled once and called thousands of times with other
batch sizes, frames and output buffers, and keeps device state between the calls: activation buffers zero-filled once (pad channels and the 2 KiB
zero page behind each buffer, which the kernels' halo padding reads), max_batch frame slots of which a smaller batch leaves the upper ones stale,
launch descriptors that run_forward rewrites when B or an output pointer changes, bb64_kernel's persistent tile tickets.  Here one HISTORY net per
row of tests/net_history_cases.py runs sequences of calls, and after each the probe batch X at B = b; its result -- every activation buffer (frame
slots < b, all channels, both planes of a bf16x3 buffer), the NCHW outputs, the three A2J head maps read through the pointers pn_a2j_forward
returns -- is compared ON BITS with a FRESH net of the same configuration whose only forward is that call.  The fresh net is tied to fp64 in the
same test by the per-step machinery of test_gpu_layers.py / test_gpu_a2j.py / test_gpu_a2j_x3.py over all frames of its batch: the probe's fresh
net always, the fresh nets of sequence 2 where the batch has at most 5 frames of at most 224 x 224 pixels (at the bench shape that leaves out the
32-frame net, which is tests/test_gpu_layers.py's rt_224_b32_bf16 / yolo_224_b32_bf16; the 512 x 288 row, the smallest frame at which max_batch 4
plans conv3_kernel<3, 2, 2, 1, 7, 4>, spends 3.5 s of host time on the fp64 reference of each frame).  No tolerance and no skip list: a difference
is a finding about a kernel or about run_forward.

Sequences, all on the one history net of a case, in this order:
  1  hostile history: max_batch frames holding NaN, +Inf, -Inf, +-3e38, 1e-40 and -0.0 (one value per frame at an eighth of the pixels and the four
     corners, the rest normal(0, 1)) and one frame mixing them all; then one normal frame at B = 1; then X.
  2  batch sizes max_batch -> 1 -> max_batch - 1 -> b (bench shape: 32 -> 5 -> 32 -> 2), other frames each time, every forward compared with the
     fresh net of that B (a batch size met twice: the frames in reversed order, against the fresh result reversed).
  3  forward(X[perm]) == forward(X)[perm] frame by frame, and forward(X[i:i+1], B = 1) == frame i of forward(X, b).  No kernel here splits K across
     frames or sums over them, so equality is asserted for every step; none is held to the fp64 allowance instead.
  4  output tensors A, then B, then A again (descriptors rewritten on pointers alone); every output tensor has max_batch frames inside a
     sentinel-guarded buffer, frames >= B and both guards keep the sentinel.  A2J has no caller-owned outputs: the head pointers must not move.
  5  (rtpose / yolo) a frames-in forward, refused calls (B = max_batch + 1, B = 0: PN_ERR_INVALID, nothing launched), a profiled forward -- X after
     each.  The frames-in forward is built for square bf16 / bf16x3 nets; on the other rows it is itself a refused call (PN_ERR_UNSUPPORTED).
After every compared forward the zeroed-once state is asserted directly: the channels of each buffer that no step writes (from pn_net_step_info)
are +0.0 bits in all max_batch slots, and the 2 KiB behind every buffer are zero bytes (pn_net_read_zero_page).

On a difference the history is replayed on a new net with every plain forward walked step by step (pn_net_forward_partial) beside a new fresh net:
the failure names the first call and step after which the zeroed-once state is broken or the step's output differs.
"""
import ctypes as C
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
import net_history_cases as NH  # noqa: E402
import test_gpu_a2j as TG  # noqa: E402
import test_gpu_a2j_x3 as TX  # noqa: E402
import test_gpu_layers as GL  # noqa: E402
from helpers import SENT, _Out  # noqa: E402
from popnet_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
PN_ERR_INVALID, PN_ERR_UNSUPPORTED = -1, -4
HOSTILE = (float("inf"), float("-inf"), 3e38, -3e38, 1e-40, -0.0, float("nan"))
TOTALS = {}          # net kind -> [cases, buffers (planes), pad channels, zero pages, compared forwards]


class _Raw:
    """Device memory by address, for torch.as_tensor."""
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2, "strides": None}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _step_name(st):
    if st["type"] in ("conv", "bblock"):
        return "%s [%s]" % (st["kernel"], ", ".join(c["w"] + (" + " + c["tail"]["w"] if c["tail"] else "") for c in st["convs"]))
    return st["kernel"]


def _compile(m, gpu, prec, mb, H, W, env, monkeypatch):
    """Compiles m for max_batch mb without running it."""
    m.precision = prec
    for k, v in dict(env, POPNET_MAX_BATCH=str(mb)).items():
        monkeypatch.setenv(k, v)
    h = m._compile(gpu, 1, H, W)
    for k in dict(env, POPNET_MAX_BATCH=""):
        monkeypatch.delenv(k)
    return h


class _Net:
    """One compiled net by handle: any call on it, its state as bits, and the log of its calls (replayed on another net when a comparison fails)."""
    def __init__(self, kind, m, gpu, out_shapes):
        self.kind, self.m, self.h, self.gpu, self.out_shapes = kind, m, m._net[0], gpu, out_shapes
        self.L, self.ctx = _lib.lib(), _lib.Context.for_device(0)
        self.info = GL._step_info(self.h, -1)
        self.steps = [GL._step_info(self.h, k) for k in range(self.L.pn_net_num_steps(self.h))]
        self.mb, self.x3 = self.info["max_batch"], self.info["prec"] == "bf16x3"
        self.names = [["buf%d.hi" % i, "buf%d.lo" % i] if self.x3 else ["buf%d" % i] for i in range(len(self.info["bufs"]))]
        self.outs, self.log, self.ptrs = {}, [], None
        self.written = NH.written_channels(self.info, self.steps)
        self.pad = [torch.from_numpy(np.flatnonzero(~w)).to(gpu) for w in self.written]
        if kind == "a2j":
            self.head_bufs = [next(c["out_buf"] for st in self.steps if st["type"] == "conv" for c in st["convs"] if c["w"] == p + ".output")
                              for p in ("classificationModel", "regressionModel", "DepthRegressionModel")]

    def stream(self):
        return _lib.current_stream_ptr(self.gpu)

    def step_outputs(self, k):
        """([(buffer plane name, first channel, end channel)] step k writes, whether it writes an NCHW output)"""
        st = self.steps[k]
        nchw = any(o and o.get("nchw_slot", -1) >= 0 for c in st.get("convs", ()) for o in (c, c["tail"]))
        return [(nm, c0, c1) for i, c0, c1 in NH.step_writes(st) for nm in self.names[i]], nchw

    def get_outs(self, key):
        """Sentinel-filled output tensors of max_batch frames, one set per key and net."""
        if key not in self.outs:
            self.outs[key] = [_Out((self.mb,) + s, self.gpu, SENT) for s in self.out_shapes]
        return self.outs[key]

    def forward(self, x, B, key):
        xp, o = C.c_void_p(x.data_ptr()), [C.c_void_p(t.t.data_ptr()) for t in self.get_outs(key)]
        if self.kind == "rtpose":
            rc = self.L.pn_rtpose_forward(self.h, xp, B, *o, self.stream())
        elif self.kind == "yolo":
            rc = self.L.pn_yolo_forward(self.h, xp, B, *o, self.stream())
        else:
            ptrs = [C.c_void_p() for _ in range(3)]
            rc = self.L.pn_a2j_forward(self.h, xp, B, *(C.byref(p) for p in ptrs), self.stream())
            if rc == 0:
                self.ptrs = [p.value for p in ptrs]
        torch.cuda.synchronize()
        return rc

    def partial(self, x, B, nsteps):
        self.ctx.check(self.L.pn_net_forward_partial(self.h, C.c_void_p(x.data_ptr()), B, nsteps, self.stream()), "pn_net_forward_partial")
        torch.cuda.synchronize()

    def forward_frames(self, depth, B, key):
        o = [C.c_void_p(t.t.data_ptr()) for t in self.get_outs(key)]
        fn = self.L.pn_rtpose_forward_frames if self.kind == "rtpose" else self.L.pn_yolo_forward_frames
        rc = fn(self.h, C.c_void_p(depth.data_ptr()), _lib.PN_DEPTH_F32, B, depth.shape[1], depth.shape[2], 6.0, 3.0, 2.0, *o, self.stream())
        torch.cuda.synchronize()
        return rc

    def do(self, op):
        """op: ("forward", x, B, outs key) | ("frames", depth, B, key) | ("profile_begin",) | ("profile_end",) -> return code; logged."""
        self.log.append(op)
        return self.run(op)

    def run(self, op):
        if op[0] == "forward":
            return self.forward(*op[1:])
        if op[0] == "frames":
            return self.forward_frames(*op[1:])
        if op[0] == "profile_begin":
            return self.L.pn_net_profile_begin(self.h)
        return self.L.pn_net_profile_end(self.h, None, None, None, None, None)

    def bufs(self):
        """{name: int32 [max_batch, C, H, W]}: every buffer (plane), all frame slots, all channels, widened exactly."""
        out = {}
        for i, (H, W, Cc) in enumerate(self.info["bufs"]):
            for nm in self.names[i]:
                t = torch.empty((self.mb, Cc, H, W), device=self.gpu, dtype=torch.float32)
                self.ctx.check(self.L.pn_net_copy_activation(self.h, nm.encode(), self.mb, C.c_void_p(t.data_ptr()), self.stream()), "pn_net_copy_activation")
                out[nm] = _bits(t)
        torch.cuda.synchronize()
        return out

    def result(self, B, key):
        r = {"bufs": self.bufs(), "outs": [_bits(o.t[:B].clone()) for o in self.get_outs(key)], "heads": []}
        if self.kind == "a2j":
            elt = (4 if self.info["prec"] == "fp32" else 2) * (2 if self.x3 else 1)
            for p, i in zip(self.ptrs, self.head_bufs):
                H, W, Cc = self.info["bufs"][i]
                r["heads"].append(torch.as_tensor(_Raw(p, B * H * W * Cc * elt), device=self.gpu).clone().view(B, -1))
        return r

    def broken_invariants(self, state=None):
        """Pad channels that are not +0.0 (one entry per buffer plane and frame slot), zero pages that are not zero."""
        bad, state = [], state or self.bufs()
        for i, names in enumerate(self.names):
            for nm in names:
                if len(self.pad[i]):
                    t = state[nm][:, self.pad[i]]
                    for slot in torch.nonzero(t.flatten(1).any(1)).flatten().tolist():
                        ch, y, x = torch.nonzero(t[slot])[0].tolist()
                        bad.append("%s, frame slot %d: pad channel %d is not +0.0 (first at row %d, column %d)" % (nm, slot, int(self.pad[i][ch]), y, x))
            page = (C.c_ubyte * 2048)()
            self.ctx.check(self.L.pn_net_read_zero_page(self.h, i, page, 2048), "pn_net_read_zero_page")
            if bytes(page).strip(b"\0"):
                bad.append("buf%d: byte %d of the zero page is not zero" % (i, next(j for j, v in enumerate(page) if v)))
        return bad

    def counts(self):
        return sum(len(n) for n in self.names), sum(len(n) * len(p) for n, p in zip(self.names, self.pad)), len(self.names)


def _differences(got, ref, frames, only=None):
    """Names of what differs on bits between frames [0, len(frames)) of `got` and frames `frames` of `ref`.  only: _Net.step_outputs of one step."""
    n, idx = len(frames), list(frames)
    if only is None:
        bad = [nm for nm in ref["bufs"] if not torch.equal(got["bufs"][nm][:n], ref["bufs"][nm][idx])]
    else:
        bad = ["%s[%d:%d]" % (nm, c0, c1) for nm, c0, c1 in only[0] if not torch.equal(got["bufs"][nm][:n, c0:c1], ref["bufs"][nm][idx][:, c0:c1])]
    if only is None or only[1]:
        bad += ["NCHW output %d" % i for i, (a, b) in enumerate(zip(got["outs"], ref["outs"])) if not torch.equal(a[:n], b[idx])]
        bad += ["head map %d" % i for i, (a, b) in enumerate(zip(got["heads"], ref["heads"])) if not torch.equal(a[:n], b[idx])]
    return bad


class _Case:
    """The nets of one row: how to compile one, the probe batch, the fresh results."""
    def __init__(self, gpu, monkeypatch, kind, prec, H, W, env, mb, b, make_model, out_shapes, frames_for, tie):
        self.gpu, self.mp, self.kind, self.prec, self.H, self.W, self.env, self.mb, self.b = gpu, monkeypatch, kind, prec, H, W, env, mb, b
        self.make_model, self.out_shapes, self.frames_for, self.tie = make_model, out_shapes, frames_for, tie
        self.fresh, self.compared, self.tied = {}, 0, []

    def new_net(self):
        m = self.make_model()
        _compile(m, self.gpu, self.prec, self.mb, self.H, self.W, self.env, self.mp)
        return _Net(self.kind, m, self.gpu, self.out_shapes)

    def frames(self, B, tag):
        return self.frames_for(B, tag).to(self.gpu)

    def fresh_result(self, B, tag):
        """(x, result) of a net whose only forward is x = frames(B, tag) at B; the net is then held to fp64 step by step and released."""
        if (B, tag) not in self.fresh:
            x, net = self.frames(B, tag), self.new_net()
            assert net.forward(x, B, "fresh") == 0
            res = net.result(B, "fresh")
            bad = net.broken_invariants(res["bufs"])
            if bad:
                pytest.fail("a net's first forward (B = %d) breaks the zeroed-once state: %s\n  -> %s" % (B, "; ".join(bad[:4]), self.diagnose([("forward", x, B, "fresh")])))
            assert all(bool((o.t[B:] == SENT).all()) and o.guards_intact() for o in net.get_outs("fresh"))
            if B <= 5 and (tag == "probe" or self.H * self.W <= 224 * 224):      # above the bench frame the fp64 reference of one frame takes seconds
                self.tied.append((B, tag, self.tie(net, x, B)))
            net.m.invalidate()
            self.fresh[(B, tag)] = (x, res)
        return self.fresh[(B, tag)]

    # ---- the diagnosis of a failed comparison ---------------------------------------------------------------------------------------
    def diagnose(self, log):
        """Replays the logged calls on a new net; every plain forward after the first is walked step by step (the last one beside a new fresh net
        run on the same input).  -> the first call / step after which the zeroed-once state is broken or the output differs."""
        net, fresh, key, known = self.new_net(), None, None, set()
        for j, op in enumerate(log):
            what = "call %d of the history (%s%s)" % (j, op[0], ", B = %d" % op[2] if len(op) > 2 else "")
            last = j == len(log) - 1
            if key is None and op[0] == "forward" and 2 <= op[2] <= net.mb:
                # the walk needs one full forward before it: the first frame alone, so that what a step does to the slots above shows in the walk
                assert net.forward(op[1][:1].contiguous(), 1, op[3]) == 0
                key, known = op[3], set(net.broken_invariants())
            if op[0] != "forward" or key is None or op[2] < 1 or op[2] > net.mb:
                net.run(op)
                if op[0] in ("forward", "frames"):
                    key = op[3]                          # the outputs a later partial forward writes (a refused call has set the pointers too)
                bad = [b for b in net.broken_invariants() if b not in known]
                if bad:
                    return "%s, not walked: %s" % (what, bad[0])
                continue
            if last:
                fresh = self.new_net()
                assert fresh.forward(op[1], op[2], "fresh") == 0
            for k in range(1, len(net.steps) + 1):
                net.partial(op[1], op[2], k)
                bad = [b for b in net.broken_invariants() if b not in known]
                if bad:
                    return "%s, step %d %s: %s" % (what, k - 1, _step_name(net.steps[k - 1]), bad[0])
                if last:
                    fresh.partial(op[1], op[2], k)
                    d = _differences(net.result(op[2], key), fresh.result(op[2], "fresh"), range(op[2]), only=net.step_outputs(k - 1))
                    if d:
                        return "%s, step %d %s: the first step whose output differs from a fresh net's (%s)" % (what, k - 1, _step_name(net.steps[k - 1]), ", ".join(d[:4]))
        return "the replay on a new net shows no difference: the failure does not repeat"

    def check(self, net, x, B, key, ref, frames, what):
        """One forward of x at B on the history net into the outputs `key`; compared with frames `frames` of the fresh result `ref`."""
        for o in net.get_outs(key):
            o.t.fill_(SENT)
        rc = net.do(("forward", x, B, key))
        assert rc == 0, (what, rc, net.ctx.last_error())
        self.compared += 1
        got = net.result(B, key)
        bad = _differences(got, ref, frames) + net.broken_invariants(got["bufs"])
        bad += ["output %d: frames >= B or a guard lost the sentinel" % i for i, o in enumerate(net.get_outs(key))
                if not (bool((o.t[B:] == SENT).all()) and o.guards_intact())]
        if bad:
            pytest.fail("%s: %s\n  -> %s" % (what, "; ".join(bad[:6]), self.diagnose(net.log)))

    def probe(self, net, what, key="probe"):
        x, ref = self.fresh_result(self.b, "probe")
        self.check(net, x, self.b, key, ref, range(self.b), what + ", then the probe batch at B = %d" % self.b)

    def refused(self, net, op, want, what):
        for o in net.get_outs("refused"):
            o.t.fill_(SENT)
        rc = net.do(op)
        assert rc == want, (what, rc, want, net.ctx.last_error())
        assert all(bool((o.buf == SENT).all()) for o in net.get_outs("refused")), what + ": a refused call wrote an output"

    # ---- the sequences ------------------------------------------------------------------------------------------------------------
    def seq1_hostile(self, net):
        rng = np.random.default_rng(1000 + self.H * 7 + self.W)
        like = self.frames(1, "shape")
        shape = tuple(like.shape[1:])
        frames = []
        for v in HOSTILE + ("mix",):
            f = rng.normal(0, 1, shape).astype(np.float32)
            m = rng.random(shape) < 0.125
            m[..., 0, 0] = m[..., 0, -1] = m[..., -1, 0] = m[..., -1, -1] = True
            f[m] = np.float32(v) if v != "mix" else np.asarray(HOSTILE, np.float32)[rng.integers(0, len(HOSTILE), int(m.sum()))]
            frames.append(f)
        for lo in ([0] if net.mb >= len(frames) else list(range(0, len(frames) - net.mb, net.mb)) + [len(frames) - net.mb]):
            x = torch.from_numpy(np.stack([frames[(lo + i) % len(frames)] for i in range(net.mb)])).to(self.gpu)      # the last batch ends in NaN and the mix
            assert net.do(("forward", x, net.mb, "junk")) == 0
        assert net.do(("forward", self.frames(1, "calm"), 1, "junk")) == 0
        stale = net.bufs()
        assert any(not bool(torch.isfinite(t[self.b:].view(torch.float32)).all()) for t in stale.values()), "the dead slots hold nothing hostile"
        self.probe(net, "hostile history (NaN, Inf, +-3e38, denormal, -0.0 in all %d slots), B = 1" % net.mb)

    def seq2_batch_sizes(self, net):
        walk, seen = NH.walk(self.mb, self.b), set()
        for B in walk[:-1]:
            x, ref = self.fresh_result(B, "walk")
            order = list(range(B)) if B not in seen else list(range(B))[::-1]
            seen.add(B)
            self.check(net, x[order].contiguous(), B, "walk", ref, order, "batch sizes %s: the forward at B = %d" % (" -> ".join(map(str, walk)), B))
        assert walk[-1] == self.b
        self.probe(net, "batch sizes %s" % " -> ".join(map(str, walk)))

    def seq3_permutation_and_split(self, net):
        x, ref = self.fresh_result(self.b, "probe")
        perm = list(range(1, self.b)) + [0]
        self.check(net, x[perm].contiguous(), self.b, "probe", ref, perm, "the probe batch permuted %s" % perm)
        for i in range(self.b):
            self.check(net, x[i:i + 1].contiguous(), 1, "probe", ref, [i], "frame %d of the probe batch alone at B = 1" % i)
        self.probe(net, "permutation and split")

    def seq4_output_buffers(self, net):
        if self.kind == "a2j":
            self.probe(net, "first of three forwards")
            p0 = list(net.ptrs)
            for i in (2, 3):
                self.probe(net, "forward %d of three" % i)
                assert net.ptrs == p0, "the head pointers moved"
            return
        self.probe(net, "outputs A", key="A")
        self.probe(net, "outputs A, then B", key="B")
        assert all(a.t.data_ptr() != b.t.data_ptr() for a, b in zip(net.get_outs("A"), net.get_outs("B")))
        self.probe(net, "outputs A, B, then A again", key="A")

    def seq5_call_state(self, net):
        S = self.H
        depth = torch.from_numpy(np.random.default_rng(5).uniform(0.5, 4.0, (self.b, S + 3, S + 5)).astype(np.float32)).to(self.gpu)
        if self.prec != "fp32" and self.H == self.W:
            assert net.do(("frames", depth, self.b, "junk")) == 0, net.ctx.last_error()
            self.probe(net, "a frames-in forward")
        else:
            self.refused(net, ("frames", depth, self.b, "refused"), PN_ERR_UNSUPPORTED, "frames-in forward on a net it is not built for")
            self.probe(net, "a refused frames-in forward")
        x = self.frames(self.b, "probe")
        self.refused(net, ("forward", x, net.mb + 1, "refused"), PN_ERR_INVALID, "B = max_batch + 1")
        self.probe(net, "a refused call (B = max_batch + 1)")
        self.refused(net, ("forward", x, 0, "refused"), PN_ERR_INVALID, "B = 0")
        self.probe(net, "a refused call (B = 0)")
        assert net.do(("profile_begin",)) == 0
        assert net.do(("forward", self.frames(self.b, "calm"), self.b, "junk")) == 0
        assert net.do(("profile_end",)) == 0
        self.probe(net, "a profiled forward")

    def run(self, id_, sequences, launched_must_hold=()):
        t0 = time.perf_counter()
        net = self.new_net()
        launched = NH.launched_as_planned(net.steps)
        assert set(launched_must_hold) <= launched, sorted(set(launched_must_hold) - launched)
        assert net.info["max_batch"] == self.mb and (net.info["in_h"], net.info["in_w"]) == (self.H, self.W) and net.info["prec"] == self.prec
        assert not net.broken_invariants()                      # as uploaded
        seqs = {1: self.seq1_hostile, 2: self.seq2_batch_sizes, 3: self.seq3_permutation_and_split, 4: self.seq4_output_buffers, 5: self.seq5_call_state}
        for s in sequences:
            seqs[s](net)
        nb, npad, nz = net.counts()
        if self.kind == "rtpose":      # not vacuous: the stage-1 concat buffer holds 187 written channels of 192
            cat = [i for i, b in enumerate(net.info["bufs"]) if b[2] == 192]
            assert cat and net.pad[cat[0]].tolist() == [187, 188, 189, 190, 191], [p.tolist() for p in net.pad]
        assert self.compared >= len(sequences) and self.tied and all(B <= 5 for B, _, _ in self.tied)
        t = TOTALS.setdefault(self.kind, [0, 0, 0, 0, 0])
        for i, v in enumerate((1, nb, npad, nz, self.compared)):
            t[i] += v
        print("\nNET HISTORY %s: sequences %s, %d forwards compared on bits, %d buffers (planes) / %d pad channels / %d zero pages asserted after each; "
              "fresh nets held to fp64: %s; %.1f s" % (id_, list(sequences), self.compared, nb, npad, nz,
                                                      ["B = %d: worst %.3f of the allowance" % (B, w) for B, _, w in self.tied], time.perf_counter() - t0))
        net.m.invalidate()


# ---- rtpose / yolo ----------------------------------------------------------------------------------------------------------------------
def _tie_layers(golden, kind, default=False):
    def tie(net, x, B):
        """tests/test_gpu_layers.py's per-step check on the fresh net as it stands, over all its frames."""
        chk = object.__new__(GL._Net)
        chk.kind, chk.m, chk.h, chk.gpu, chk.B, chk.x, chk.frames = kind, net.m, net.h, net.gpu, B, x, list(range(B))
        chk.sd = {k: v.detach().cpu().clone() for k, v in net.m.state_dict().items()}
        chk.ctx, chk.L, chk.info, chk.steps = net.ctx, net.L, net.info, net.steps
        chk.nchw = dict(zip((0, 1, 2) if kind == "rtpose" else (3,), (o.t[:B] for o in net.get_outs("fresh"))))
        chk.naf = 5 + 3 * net.m.num_parts
        results = chk.check_all()
        bad = ["step %d %s %s: worst %.3g, %d elements over, at (frame, channel, row, col, ratio) %s" % (k, kern, name, rep["worst"], rep["n_bad"], rep["where"])
               for k, kern, name, rep in results if rep["n_bad"]]
        assert len(results) >= len(net.steps) and not bad, "the fresh net itself misses fp64:\n" + "\n".join(bad)
        return max(r[3]["worst"] for r in results)
    return tie


def _pose_case(golden, gpu, monkeypatch, case):
    id_, kind, prec, H, W, env, mb, b, sequences = case
    m0 = GL._model(golden, kind, False)
    s = 8 if kind == "rtpose" else 16
    if kind == "rtpose":
        shapes = [(c, H // s, W // s) for c in (m0.num_limbs * 2, m0.num_parts + 1, m0.num_limbs + 1)]
    else:
        shapes = [(len(m0.anchors) * (5 + 3 * m0.num_parts), H // s, W // s)]
    cin = int(m0.input_dim)
    tags = {"probe": 0, "walk": 1, "calm": 2, "shape": 3}

    def frames_for(B, tag):
        return GL._frames(golden, B, cin, H, W, seed=H * 7 + W + B + 1000 * tags[tag])
    return _Case(gpu, monkeypatch, kind, prec, H, W, env, mb, b, lambda: GL._model(golden, kind, False), shapes, frames_for, _tie_layers(golden, kind))


@pytest.mark.parametrize("case", NH.CASES, ids=[c[0] for c in NH.CASES])
def test_forward_does_not_depend_on_history(gpu, golden, monkeypatch, case):
    _pose_case(golden, gpu, monkeypatch, case).run(case[0], case[8], launched_must_hold=NH.counted(case))


@pytest.mark.parametrize("case", NH.BENCH_CASES, ids=[c[0] for c in NH.BENCH_CASES])
def test_forward_does_not_depend_on_history_at_the_bench_shape(gpu, golden, monkeypatch, case):
    """224 x 224 bf16 compiled for max_batch 32: the only shape where bb64_kernel hands tiles out by persistent tickets (rtpose, POPNET_BB64_STRIP=0,
    B = 32: 1792 tiles; B = 5 and 2: static) and where the strip kernel is the default (rtpose, B = 32).  All 32 frame slots are compared wherever
    32 frames ran, and the pad channels of all 32 after every forward."""
    assert NH.bb64_launch(32, *NH.BENCH_LAYER1[case[1]], None, num_cus=torch.cuda.get_device_properties(gpu).multi_processor_count)[0] == (case[1] == "rtpose")
    _pose_case(golden, gpu, monkeypatch, case).run(case[0], case[8])


# ---- A2J ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def a2j_sd():
    g = np.load(os.path.join(TG.GOLDEN, "a2j.npz"))
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(g["shapes"], g["ndim"])]
    return AC.state_dict_for_seed(int(g["seed"]), [str(k) for k in g["keys"]], shapes)


@pytest.mark.parametrize("case", NH.A2J_CASES, ids=[c[0] for c in NH.A2J_CASES])
def test_a2j_forward_does_not_depend_on_history(gpu, a2j_sd, monkeypatch, case):
    from popnet_amd.network.a2j import A2J_model
    id_, prec, H, W, mb, b, sequences = case

    def make_model():
        m = A2J_model(15).eval()
        m.load_state_dict(a2j_sd)
        return m

    def frames_for(B, tag):
        return torch.from_numpy(AC.net_input(AC.SEED + H + {"probe": 0, "walk": 100 + B, "calm": 200, "shape": 300}[tag], B, H, W))

    def tie(net, x, B):
        """tests/test_gpu_a2j.py's (bf16x3: test_gpu_a2j_x3.py's) per-step check on the fresh net as it stands, every step, all frames."""
        chk = object.__new__(TX._NetX3 if prec == "bf16x3" else TG._Net)
        chk.m, chk.h, chk.gpu, chk.B, chk.H, chk.W, chk.x, chk.frames = net.m, net.h, net.gpu, B, H, W, x, list(range(B))
        chk.sd = ALR.stem_state_dict({k: v for k, v in a2j_sd.items()})
        chk.ctx, chk.L, chk.info, chk.steps = net.ctx, net.L, net.info, net.steps
        results = chk.check_steps(which=APC.selects(APC.ALL))
        if prec == "bf16x3":
            results, pairs = results
            assert all(p[2] and p[3] == 0 for p in pairs), [p for p in pairs if not p[2] or p[3]]
        assert len(results) >= len(net.steps) and not TG._report(results), "the fresh net itself misses fp64:\n" + "\n".join(TG._report(results))
        return max(r[3]["worst"] for r in results)
    _Case(gpu, monkeypatch, "a2j", prec, H, W, {}, mb, b, make_model, [], frames_for, tie).run(id_, sequences)


def test_zz_totals_of_what_was_asserted():
    """The sums for the record (printed; run with -s): cases, buffers, pad channels, zero pages and compared forwards per net kind."""
    for kind, (cases, nb, npad, nz, fw) in sorted(TOTALS.items()):
        print("\nNET HISTORY TOTAL %s: %d cases, %d buffers (planes), %d pad channels, %d zero pages; %d forwards compared on bits" % (kind, cases, nb, npad, nz, fw))
        assert nb and nz and fw
