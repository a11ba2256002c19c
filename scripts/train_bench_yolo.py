"""Times the HIP training step of YoloPoseNet (popnet_amd.train_yolo.YoloTrainEngine, fp32, pose-weighted loss) on synthetic data:
B frames of 224x224 (default 30, the trainer's batch), init-like weights (N(0, 0.01) convolutions, BatchNorm 1 / 0), seeded prior targets.
Prints one JSON line: train_step_ms_yolo_fp32 (device events around `steps` steps after a warm-up) and the step's algorithmic GFLOP
(forward + weight gradient of every convolution, data gradient of every convolution but the first; from the layer shapes).
usage: python scripts/train_bench_yolo.py [B] [steps] [warmup]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import popnet_amd  # noqa: E402,F401
from popnet_amd.network.yolo_posenet import YoloPoseNet  # noqa: E402
from popnet_amd.train_yolo import YoloTrainEngine  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 30
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 3
S = 224
dev = torch.device("cuda:0")
torch.manual_seed(3)
eng = YoloTrainEngine.from_module(YoloPoseNet(15, input_dim=1), device=dev, lr=0.01)
rng = np.random.default_rng(1)
g = S // 16
img = torch.from_numpy(rng.normal(0, 1, (B, 1, S, S)).astype(np.float32)).to(dev)
prior = torch.from_numpy(rng.uniform(-1, 1, (B, eng.n_out, g, g)).astype(np.float32)).to(dev)
coord = torch.from_numpy((rng.uniform(0, 1, (B, 2, g, g)) < 0.05).astype(np.float32)).to(dev)
conf = (0.1 + 0.9 * coord).contiguous()
weight = torch.from_numpy(rng.uniform(0.5, 2, (B, 2, g, g)).astype(np.float32)).to(dev)
for _ in range(warmup):
    eng.step(img, prior, conf, coord, weight)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(steps):
    t = eng.step(img, prior, conf, coord, weight)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / steps
gflop = eng.flops_per_step(B, S, S) / 1e9
print(json.dumps({"train_step_ms_yolo_fp32": round(ms, 3), "batch": B, "input": [S, S], "steps": steps, "warmup": warmup,
                  "gflop_per_step": round(gflop, 2), "gflop_per_frame": round(gflop / B, 3), "tflops": round(gflop / ms, 2),
                  "loss_terms": [round(float(v), 6) for v in t.cpu()]}))
