#!/usr/bin/env python
"""Throughput of the Yolo-A2J second stage on one GPU: crops/s of A2JEngine at B = 32, 288 x 288, bf16, bf16x3 and fp32.

    python scripts/a2j_bench.py [--batch 32] [--seconds 1.5] [--reps 5] [--warmup 5] [--out profiles/a2j_bench.json]

Reports, per precision: crops/s of the whole predict (crop kernel + net + vote) and of the net alone, the algorithmic FLOP per crop
counted from the compiled layer table (pn_net_flops_per_frame: 2 x MAC of every convolution; the stem counted as the single-channel
convolution it runs as), achieved TFLOP/s, the fraction of the matrix-core peak (bf16: 2500 TFLOP/s dense, fp32: 157.3 TFLOP/s -- the
MI355X data-sheet figures; bf16x3: a third of the bf16 figure, three bf16 products per algorithmic one), and a per-kernel table from HIP events around every launch (pn_net_profile_*), slowest first.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from popnet_amd import _lib  # noqa: E402
from popnet_amd.pipeline import A2JEngine  # noqa: E402

PEAK = {"bf16": 2500.0, "bf16x3": 2500.0 / 3, "fp32": 157.3}


def bench(prec, B, seconds, reps, warmup):
    eng = A2JEngine(precision=prec, max_batch=B)
    dev = eng.device
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.uniform(0.5, 5.0, (4, 640, 480)).astype(np.float16)).to(dev)
    rows = np.zeros((B, 6), np.float32)
    for i in range(B):
        x0, y0 = rng.uniform(0, 300), rng.uniform(0, 300)
        rows[i] = [i % 4, x0, y0, x0 + rng.uniform(60, 170), y0 + rng.uniform(150, 330), 0.9]
    L, net = eng.L, eng.net
    flops = L.pn_net_flops_per_frame(net)

    def timed(fn):
        """-> (median seconds per call, [seconds per call of every repetition]): `reps` windows of at least `seconds` / reps of work each,
        the call count sized from a first timed probe, so that a window is long against launch and scheduler noise."""
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls = max(5, int(seconds / reps / max((time.perf_counter() - t0) / 3, 1e-6)))
        runs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) / calls)
        return float(np.median(runs)), runs, calls

    t_all, runs_all, calls_all = timed(lambda: eng.predict(frames, rows))
    ptrs = [C.c_void_p() for _ in range(3)]
    fwd = lambda: eng.ctx.check(L.pn_a2j_forward(net, C.c_void_p(eng.x.data_ptr()), B, *(C.byref(p) for p in ptrs), _lib.current_stream_ptr(dev)), "pn_a2j_forward")
    t_net, runs_net, calls_net = timed(fwd)
    steps = 20                                    # forwards under the per-launch events
    L.pn_net_profile_begin(net)
    for _ in range(steps):
        fwd()
    cm, cl, cf, om, ol = C.c_double(), C.c_int64(), C.c_double(), C.c_double(), C.c_int64()
    eng.ctx.check(L.pn_net_profile_end(net, C.byref(cm), C.byref(cl), C.byref(cf), C.byref(om), C.byref(ol)), "pn_net_profile_end")
    kernels = []
    for rank in range(64):
        name, ms, n, fl = C.create_string_buffer(128), C.c_double(), C.c_int64(), C.c_double()
        if L.pn_net_profile_kernel(net, rank, name, 128, C.byref(ms), C.byref(n), C.byref(fl)) != 0:
            break
        kernels.append({"kernel": name.value.decode(), "ms_per_forward": ms.value / steps, "launches_per_forward": n.value / steps,
                        "tflops": fl.value / (ms.value * 1e-3) / 1e12 if ms.value > 0 else 0.0,
                        "fraction_of_peak": fl.value / (ms.value * 1e-3) / 1e12 / PEAK[prec] if ms.value > 0 else 0.0})
    tf = flops * B / t_net / 1e12
    return {"precision": prec, "batch": B, "crop": [eng.crop_h, eng.crop_w], "crops_per_s_predict": B / t_all, "crops_per_s_net": B / t_net,
            "timing": {"what": "median of %d windows" % reps, "calls_per_window_predict": calls_all, "calls_per_window_net": calls_net,
                       "crops_per_s_predict_runs": [B / t for t in runs_all], "crops_per_s_net_runs": [B / t for t in runs_net]},
            "gflop_per_crop": flops / 1e9, "tflops_net": tf, "peak_tflops": PEAK[prec], "fraction_of_peak": tf / PEAK[prec],
            "conv_ms_per_forward": cm.value / steps, "conv_launches_per_forward": cl.value / steps,
            "other_ms_per_forward": om.value / steps, "other_launches_per_forward": ol.value / steps, "kernels": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=1.5, help="timed work per measurement, split into --reps windows")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "a2j_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "results": [bench(p, a.batch, a.seconds, a.reps, a.warmup) for p in ("bf16", "bf16x3", "fp32")]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["results"]:
        print("%s: %.0f crops/s [%.0f .. %.0f over %d windows] (net alone %.0f), %.2f GFLOP/crop, %.1f TFLOP/s = %.1f %% of peak; conv %.2f ms in %d launches, other %.2f ms" % (
            r["precision"], r["crops_per_s_predict"], min(r["timing"]["crops_per_s_predict_runs"]), max(r["timing"]["crops_per_s_predict_runs"]), a.reps, r["crops_per_s_net"], r["gflop_per_crop"], r["tflops_net"], 100 * r["fraction_of_peak"],
            r["conv_ms_per_forward"], r["conv_launches_per_forward"], r["other_ms_per_forward"]))
        for k in r["kernels"][:8]:
            print("    %-44s %7.3f ms  %5.1f launches  %6.1f TFLOP/s" % (k["kernel"], k["ms_per_forward"], k["launches_per_forward"], k["tflops"]))


if __name__ == "__main__":
    main()
