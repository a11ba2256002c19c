#!/usr/bin/env python
"""Step time of A2JTrainEngine on one GPU: forward, A2J_loss, backward and the Adam update of A2J_model at 288 x 288 crops.

    python scripts/a2j_train_bench.py [--precisions fp32 bf16x3] [--batches 16 31] [--steps 10] [--reps 3] [--warmup 2] [--out profiles/a2j_train_bench.json]

Per precision and batch size (one result block each, both precisions in the same run so that the fp32 figures are the baseline of the
bf16x3 ones), all from HIP events around work that is already warm:
  ms_per_step          median over --reps windows of --steps eager steps each (the spread is kept), crops/s, and the algorithmic TFLOP/s of the
                       convolutions (A2JTrainEngine.flops_per_step: 2 x MAC of every forward, weight gradient and data gradient) -- a whole-step
                       rate, not a kernel's share of peak
  loss                 pn_a2j_loss alone (terms + the three gradients), next to the bytes it must move: the three head maps read once and their
                       gradients written once, and the rate that makes (the second and third pass over the heads are expected to hit L2)
  dilated              the six dilated launches' entries (forward, data and weight gradient of layer4.1.conv2 and layer4.2.conv2) timed one by one
                       in a pass of their own, and their share of the step
Then "layers_1x1": every distinct stride-1 1x1 shape of the step (A2JTrainEngine.conv1x1_shapes) at every batch size, in the three roles --
the split-bf16 entry (pn_conv1x1_x3_forward / _dgrad / _wgrad, packs cached and fresh as inside a step) next to the fp32 launch it replaces
(pn_conv2d_forward / _dgrad / _wgrad), each the median over --reps windows of 20 warm calls, with the plan's kernel label and the ratio.
"clocks_before" / "clocks_after": the device's shader clock and power draw as torch reports them; before = idle, after = right behind the last timed window (informational).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from popnet_amd import _lib  # noqa: E402
from popnet_amd.network.a2j import A2J_model  # noqa: E402
from popnet_amd.train_a2j import A2JTrainEngine  # noqa: E402


def _events(fn, n):
    """milliseconds per call of fn over n calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def bench(eng, B, crop, steps, reps, warmup):
    dev = eng.device
    rng = np.random.default_rng(B)
    img = torch.from_numpy(rng.normal(-1.0, 0.5, (B, 1, crop, crop)).astype(np.float32)).to(dev)
    label = torch.from_numpy(np.concatenate([rng.uniform(20, crop - 20, (B, 15, 2)), rng.uniform(1, 5, (B, 15, 1))], 2).astype(np.float32)).to(dev)
    for _ in range(warmup):
        eng.step(img, label)
    torch.cuda.synchronize()
    runs = [_events(lambda: eng.step(img, label), steps) for _ in range(reps)]
    ms = float(np.median(runs))
    flops = eng.flops_per_step(B, crop, crop)
    # pn_a2j_loss alone, on the head maps the last step left behind
    h = w = crop // 16
    A, P = eng.num_anchors, eng.num_classes
    cls, reg, dep = (eng._buf("c:%s.output" % n, (B, c, h, w)) for n, c in zip(("classificationModel", "regressionModel", "DepthRegressionModel"), (A * P, A * P * 2, A * P)))
    dcls, dreg, ddep = eng.head_grads
    terms = torch.zeros(2, device=dev)

    def loss():
        eng._check(eng.L.pn_a2j_loss(eng.ctx.handle, eng._ptr(cls), eng._ptr(reg), eng._ptr(dep), B, h, w, A, P, eng._ptr(eng.anchors(h, w)), eng._ptr(label),
                                     eng.spatial_factor, eng._ptr(eng._scale), eng._ptr(terms), eng._ptr(dcls), eng._ptr(dreg), eng._ptr(ddep), eng._s()), "pn_a2j_loss")
    loss()
    torch.cuda.synchronize()
    loss_runs = [_events(loss, 50) for _ in range(reps)]
    loss_ms = float(np.median(loss_runs))
    loss_bytes = 2 * 4 * (cls.numel() + reg.numel() + dep.numel())
    # the dilated entries, one by one: a pass of its own (an event pair per call serialises the host against the device)
    dil_ms = {"forward": 0.0, "dgrad": 0.0, "wgrad": 0.0}
    L = eng.L
    real = {k: getattr(L, k) for k in ("pn_conv2d_forward_dil", "pn_conv2d_dgrad_dil", "pn_conv2d_wgrad_dil")}
    pairs = []

    class Timed:
        def __init__(self, name, fn):
            self.name, self.fn = name, fn

        def __call__(self, *a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = self.fn(*a)
            e1.record()
            pairs.append((self.name, e0, e1))
            return rc

    class Proxy:
        def __getattr__(self, k):
            return Timed(k.split("_")[2], real[k]) if k in real else getattr(L, k)
    n_pass = 3
    eng.L = Proxy()
    try:
        for _ in range(n_pass):
            eng.forward_backward(img, label)
        torch.cuda.synchronize()
    finally:
        eng.L = L
    for name, e0, e1 in pairs:
        dil_ms[name] += e0.elapsed_time(e1) / n_pass
    dil_total = sum(dil_ms.values())
    return {"batch": B, "crop": [crop, crop], "ms_per_step": ms, "ms_per_step_runs": runs, "steps_per_window": steps, "crops_per_s": B / ms * 1e3,
            "conv_gflop_per_step": flops / 1e9, "conv_tflops_whole_step": flops / (ms * 1e-3) / 1e12,
            "loss": {"ms": loss_ms, "ms_runs": loss_runs, "bytes_min": loss_bytes, "gb_per_s_at_bytes_min": loss_bytes / (loss_ms * 1e-3) / 1e9,
                     "workgroups": B * P, "share_of_step": loss_ms / ms},
            "dilated": {"launches_per_step": len(pairs) // n_pass, "ms": dil_ms, "ms_total": dil_total, "share_of_step": dil_total / ms}}


def layer_table(eng, batches, crop, reps, calls=20):
    """The per-layer table: eng is a bf16x3 engine (its context caches the packs); every tensor is this function's own."""
    dev, L, h = eng.device, eng.L, eng.ctx.handle
    s = eng._s()
    p = eng._ptr
    shapes = {}
    for name, Cin, HW, Cout in eng.conv1x1_shapes(crop, crop):
        shapes.setdefault((Cin, HW, Cout), []).append(name)
    rows = []
    for B in batches:
        for (Cin, HW, Cout), names in sorted(shapes.items()):
            x, dy = torch.randn(B, Cin, HW, device=dev), torch.randn(B, Cout, HW, device=dev)
            y, dx = torch.empty(B, Cout, HW, device=dev), torch.empty(B, Cin, HW, device=dev)
            w, dw = torch.randn(Cout, Cin, device=dev) / np.sqrt(Cin), torch.empty(Cout, Cin, device=dev)
            side = int(round(np.sqrt(HW)))
            Hh, Ww = (side, side) if side * side == HW else (HW, 1)
            pairs = {
                "forward": (lambda: L.pn_conv1x1_x3_forward(h, p(x), p(w), None, p(y), B, Cin, HW, Cout, 0, s),
                            lambda: L.pn_conv2d_forward(h, p(x), p(w), None, p(y), B, Cin, Hh, Ww, Cout, 1, 1, 0, 0, s)),
                "dgrad": (lambda: L.pn_conv1x1_x3_dgrad(h, p(dy), p(w), p(dx), B, Cin, HW, Cout, 0, s),
                          lambda: L.pn_conv2d_dgrad(h, p(dy), p(w), p(dx), B, Cin, Hh, Ww, Cout, 1, 0, 0, s)),
                "wgrad": (lambda: L.pn_conv1x1_x3_wgrad(h, p(x), p(dy), p(dw), None, B, Cin, HW, Cout, s),
                          lambda: L.pn_conv2d_wgrad(h, p(x), p(dy), p(dw), None, B, Cin, Hh, Ww, Cout, 1, 1, 0, s)),
            }
            for role, (new, old) in pairs.items():
                ms = []
                for fn in (new, old):
                    for _ in range(3):
                        eng._check(fn(), role)
                    torch.cuda.synchronize()
                    ms.append(float(np.median([_events(fn, calls) for _ in range(reps)])))
                buf = C.create_string_buffer(1024)
                eng._check(L.pn_conv1x1_x3_plan_info(h, {"forward": 0, "dgrad": 1, "wgrad": 3}[role], B, Cin, HW, Cout, buf, 1024), "pn_conv1x1_x3_plan_info")
                rows.append({"batch": B, "Cin": Cin, "HW": HW, "Cout": Cout, "layers": len(names), "role": role, "kernel": json.loads(buf.value.decode())["kernel"],
                             "ms_bf16x3": ms[0], "ms_fp32": ms[1], "speedup": ms[1] / ms[0], "tflops_bf16x3": 2.0 * B * HW * Cin * Cout / (ms[0] * 1e-3) / 1e12})
            del x, dy, y, dx, w, dw
    return rows


def _clocks():
    try:
        return {"sclk_mhz": torch.cuda.clock_rate(), "power_draw": torch.cuda.power_draw()}          # as torch reports them (this build: watts)
    except Exception as e:              # informational only
        return {"unavailable": str(e)[:80]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", nargs="+", choices=("fp32", "bf16x3"), default=["fp32", "bf16x3"])
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 31])
    ap.add_argument("--crop", type=int, default=288)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "a2j_train_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise _lib.PopnetError("a2j_train_bench: no GPU -- nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(3)
    module = A2J_model(15)
    res = {"device": torch.cuda.get_device_name(0), "what": "A2JTrainEngine.step (eager, NCHW): forward, A2J_loss, backward, Adam", "clocks_before": _clocks(),
           "results": []}
    for prec in a.precisions:
        for B in a.batches:
            eng = A2JTrainEngine.from_module(module, device=dev, precision=prec)
            r = bench(eng, B, a.crop, a.steps, a.reps, a.warmup)
            r["precision"] = prec
            res["results"].append(r)
            del eng
            torch.cuda.empty_cache()
    if "bf16x3" in a.precisions:
        eng = A2JTrainEngine.from_module(module, device=dev, precision="bf16x3")
        res["layers_1x1"] = layer_table(eng, a.batches, a.crop, a.reps)
        del eng
    res["clocks_after"] = _clocks()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["results"]:
        print("%s B = %d: %.1f ms / step [%.1f .. %.1f over %d windows of %d], %.0f crops/s, %.1f TFLOP/s (convolutions, whole step); pn_a2j_loss %.3f ms for %.1f MB "
              "(%.0f GB/s, %.2f %% of the step); dilated launches %.2f ms = %.1f %% of the step" % (
                  r["precision"], r["batch"], r["ms_per_step"], min(r["ms_per_step_runs"]), max(r["ms_per_step_runs"]), a.reps, a.steps, r["crops_per_s"], r["conv_tflops_whole_step"],
                  r["loss"]["ms"], r["loss"]["bytes_min"] / 1e6, r["loss"]["gb_per_s_at_bytes_min"], 100 * r["loss"]["share_of_step"], r["dilated"]["ms_total"],
                  100 * r["dilated"]["share_of_step"]))
    for r in res.get("layers_1x1", []):
        print("1x1 B = %2d  %4d -> %4d on %4d px (x %d) %-7s %-32s bf16x3 %.3f ms  fp32 %.3f ms  x %.2f  %.0f TFLOP/s" % (
            r["batch"], r["Cin"], r["Cout"], r["HW"], r["layers"], r["role"], r["kernel"], r["ms_bf16x3"], r["ms_fp32"], r["speedup"], r["tflops_bf16x3"]))


if __name__ == "__main__":
    main()
