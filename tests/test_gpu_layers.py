"""Every launch of the real bf16 / bf16x3 / fp32 forward against an fp64 host reference of the same operation.

For each configuration the net is compiled and run once in full; then for every step k of its compiled step list
the forward is run to k (pn_net_forward_partial), the buffers the step reads are read back, the forward is run to
k + 1 and the step's outputs are read back.  tests/layer_reference.py computes, on the first, a middle and the last
frame, the exact result of the kernel's operation on those operands and a per-element allowance (stored format's
half ulp + a bound on fp32 accumulation); every output element must be within it.  Unlike the end-to-end
tolerances, this does not depend on the kernels' summation order and catches a single wrong tap, halo row, bias or
channel of one layer.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import state_dict_from_keys  # noqa: E402
import layer_reference as LR  # noqa: E402
from popnet_amd import _lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu

# (id, network, precision, B, H, W, reference default topology, environment read when the net is compiled)
CONFIGS = []
for _p in ("bf16", "bf16x3"):
    CONFIGS += [
        ("rt_224_b32_" + _p, "rtpose", _p, 32, 224, 224, False, {}),     # the bench shape
        ("rt_224_b5_" + _p, "rtpose", _p, 5, 224, 224, False, {}),
        ("rt_200x232_" + _p, "rtpose", _p, 3, 200, 232, False, {}),
        ("rt_96x480_" + _p, "rtpose", _p, 3, 96, 480, False, {}),
        ("rt_256x192_" + _p, "rtpose", _p, 3, 256, 192, False, {}),
        ("yolo_224_b32_" + _p, "yolo", _p, 32, 224, 224, False, {}),
        ("yolo_224_b3_" + _p, "yolo", _p, 3, 224, 224, False, {}),
        ("yolo_240x336_" + _p, "yolo", _p, 2, 240, 336, False, {}),
        ("rt_default_" + _p, "rtpose", _p, 3, 224, 224, True, {}),
        ("yolo_default_" + _p, "yolo", _p, 3, 224, 224, True, {}),
    ]
CONFIGS += [
    ("rt_224_b5_bf16_no_conv3", "rtpose", "bf16", 5, 224, 224, False, {"POPNET_NO_CONV3": "1"}),
    ("yolo_224_b5_bf16_no_conv3", "yolo", "bf16", 5, 224, 224, False, {"POPNET_NO_CONV3": "1"}),
    ("rt_224_b5_bf16_conv4", "rtpose", "bf16", 5, 224, 224, False, {"POPNET_CONV4": "1"}),
    ("rt_224_b5_bf16x3_bblock_x3", "rtpose", "bf16x3", 5, 224, 224, False, {"POPNET_BBLOCK_X3": "1"}),
    ("rt_224_b3_fp32", "rtpose", "fp32", 3, 224, 224, False, {}),
    ("yolo_224_b3_fp32", "yolo", "fp32", 3, 224, 224, False, {}),
]
BENCH = [c for c in CONFIGS if c[0] in ("rt_224_b32_bf16", "rt_224_b32_bf16x3", "yolo_224_b32_bf16", "yolo_224_b32_bf16x3")]


def _model(golden, kind, default):
    from popnet_amd.network.rtpose_light3d import rtpose_light3d
    from popnet_amd.network.yolo_posenet import YoloPoseNet
    if kind == "rtpose":
        m = rtpose_light3d().eval() if default else rtpose_light3d(15, 14, 2, input_dim=1).eval()
    else:
        m = YoloPoseNet().eval() if default else YoloPoseNet(15, input_dim=1).eval()
    if default:
        synth.load_synth_weights(m, seed=8 if kind == "rtpose" else 9)
    else:
        m.load_state_dict(state_dict_from_keys(golden.keys["rtpose_light3d" if kind == "rtpose" else "yolo_posenet"], seed=0 if kind == "rtpose" else 1))
    return m


def _frames(golden, B, cin, H, W, seed):
    x = torch.from_numpy(np.random.default_rng(seed).normal(0, 1, (B, cin, H, W)).astype(np.float32))
    itop = torch.from_numpy(golden.forward["x"][:1])                      # the reference's ITOP frame, pre-processed
    x[0, :1] = F.interpolate(itop, size=(H, W), mode="bilinear", align_corners=False)[0] if (H, W) != (224, 224) else itop[0]
    return x


def _step_info(h, k):
    buf = C.create_string_buffer(1 << 16)
    ctx = _lib.Context.for_device(0)
    ctx.check(_lib.lib().pn_net_step_info(h, k, buf, len(buf)), "pn_net_step_info")
    return json.loads(buf.value.decode())


class _Net:
    def __init__(self, golden, cfg, gpu, monkeypatch):
        _, self.kind, prec, B, H, W, default, env = cfg
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.m = _model(golden, self.kind, default)
        self.m.precision = prec
        self.sd = {k: v.detach().cpu().clone() for k, v in self.m.state_dict().items()}
        cin = int(self.m.input_dim)
        self.x = _frames(golden, B, cin, H, W, seed=H * 7 + W + B).to(gpu)
        self.B, self.gpu = B, gpu
        self.frames = sorted({0, B // 2, B - 1})
        self.h = self.m._compile(gpu, B, H, W)
        for k in env:
            monkeypatch.delenv(k)
        self.ctx = _lib.Context.for_device(0)
        self.L = _lib.lib()
        h8 = H // (8 if self.kind == "rtpose" else 16)
        w8 = W // (8 if self.kind == "rtpose" else 16)
        if self.kind == "rtpose":
            np_, nh, nz = self.m.num_limbs * 2, self.m.num_parts + 1, self.m.num_limbs + 1
            self.nchw = {i: torch.zeros((B, c, h8, w8), device=gpu) for i, c in enumerate((np_, nh, nz))}
        else:
            self.nchw = {3: torch.zeros((B, len(self.m.anchors) * (5 + 3 * self.m.num_parts), h8, w8), device=gpu)}
        self.naf = 5 + 3 * self.m.num_parts
        self._forward(None)
        self.info = _step_info(self.h, -1)
        self.steps = [_step_info(self.h, k) for k in range(self.L.pn_net_num_steps(self.h))]

    def _forward(self, nsteps):
        s = _lib.current_stream_ptr(self.gpu)
        xp = C.c_void_p(self.x.data_ptr())
        if nsteps is not None:
            self.ctx.check(self.L.pn_net_forward_partial(self.h, xp, self.B, nsteps, s), "pn_net_forward_partial")
        elif self.kind == "rtpose":
            self.ctx.check(self.L.pn_rtpose_forward(self.h, xp, self.B, *(C.c_void_p(self.nchw[i].data_ptr()) for i in range(3)), s), "pn_rtpose_forward")
        else:
            self.ctx.check(self.L.pn_yolo_forward(self.h, xp, self.B, C.c_void_p(self.nchw[3].data_ptr()), s), "pn_yolo_forward")
        torch.cuda.synchronize()

    def _read(self, name, H, W, Cc):
        out = np.empty((self.B, Cc, H, W), np.float32)
        self.ctx.check(self.L.pn_net_read_activation(self.h, name.encode(), self.B, out.ctypes.data_as(C.c_void_p), out.size,
                                                     _lib.current_stream_ptr(self.gpu)), "pn_net_read_activation")
        return torch.from_numpy(out[self.frames]).to(torch.float64)

    def reader(self):
        cache = {}

        def read(i):
            if i not in cache:
                H, W, Cc = self.info["bufs"][i]
                if self.info["prec"] == "bf16x3":
                    hi = self._read("buf%d.hi" % i, H, W, Cc)
                    cache[i] = LR.Act(hi + self._read("buf%d.lo" % i, H, W, Cc), hi)
                else:
                    cache[i] = LR.Act(self._read("buf%d" % i, H, W, Cc))
            return cache[i]
        return read

    def check_all(self):
        """Per step: the reports of every output, and the kernel label."""
        xf = self.x[self.frames].cpu().to(torch.float64)
        results = []
        for k, st in enumerate(self.steps):
            self._forward(k)
            checks = LR.step_reference(st, self.info, self.sd, self.reader(), xf, naf=self.naf)
            self._forward(k + 1)
            after = self.reader()
            for ch in checks:
                if ch.where[0] == "buf":
                    gpu = after(ch.where[1]).v[:, ch.where[2]:ch.where[2] + ch.r.shape[1]]
                else:
                    gpu = self.nchw[ch.where[1]][self.frames].cpu().to(torch.float64)
                rep = LR.compare(gpu, ch.r, ch.allow, frames=self.frames)
                results.append((k, st["kernel"], ch.name, rep))
        return results


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_layer_within_fp64_allowance(gpu, golden, monkeypatch, cfg):
    net = _Net(golden, cfg, gpu, monkeypatch)
    results = net.check_all()
    assert len(results) >= len(net.steps)
    worst = max(r[3]["worst"] for r in results)
    print("\nLAYERS %s: %d steps, worst |gpu - r| / allowance = %.4f" % (cfg[0], len(net.steps), worst))
    bad = ["step %d %s %s: worst %.3g, %d elements over, at (frame, channel, row, col, ratio) %s" % (k, kern, name, rep["worst"], rep["n_bad"], rep["where"])
           for k, kern, name, rep in results if rep["n_bad"]]
    assert not bad, "\n".join(bad)
    # the allowance must not be vacuous: every checked output carries real data
    assert all(r[3]["worst"] > 0 for r in results if "pool1" not in r[2] and "pool2" not in r[2] and "maxpool" not in r[2]), \
        [(r[0], r[2]) for r in results if r[3]["worst"] == 0]


def test_coverage_guard_every_bench_kernel_is_checked(gpu, golden, monkeypatch):
    """The kernel labels of the bench-shape nets (both networks, bf16 and bf16x3, B = 32, 224 x 224) must each be
    run by at least one configuration above: a planner change that routes a level to a new instantiation fails here
    until that instantiation is checked too."""
    def labels(cfg):
        _, kind, prec, B, H, W, default, env = cfg
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = _model(golden, kind, default)
        m.precision = prec
        h = m._compile(gpu, B, H, W)
        for k in env:
            monkeypatch.delenv(k)
        out = {_step_info(h, k)["kernel"] for k in range(_lib.lib().pn_net_num_steps(h))}
        m.invalidate()
        return out
    bench = set().union(*(labels(c) for c in BENCH))
    checked = set().union(*(labels(c) for c in CONFIGS))
    print("\nbench kernel labels:", sorted(bench))
    assert any(l.startswith("conv4_kernel") for l in bench) and "bb64_kernel" in bench
    assert bench <= checked, sorted(bench - checked)
