#!/usr/bin/env python
"""Times one pn_a2j_train_crop launch (A2JEngine.train_crops) with HIP events: n = 31 crops of 288 x 288 from 240 x 320 float16 frames,
the ITOP form with the warp on, every item with its own draws.  A warm-up, then --reps timed calls, each bracketed by events; the
median is what profiles/a2j_traincrop_timing.md records.  The call includes the upload of the 31 records; the host work that builds
them (popnet_amd.a2j_crops.itop_items) is timed separately with a host clock.  No throughput is claimed from this.

    python scripts/a2j_traincrop_timing.py [--reps 40] [--out timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=31)
    ap.add_argument("--crop", type=int, default=288)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import popnet_amd  # noqa: F401
    from popnet_amd import a2j_crops
    from popnet_amd.pipeline import A2JEngine

    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda", 0)
    n, H, W = args.n, 240, 320
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.uniform(1.5, 4.0, (n, H, W)).astype(np.float16)).to(dev)
    centres = np.stack([rng.uniform(100, 220, n), rng.uniform(80, 160, n), rng.uniform(2.5, 3.5, n)], -1).astype(np.float32).reshape(n, 1, 3)
    lefttop, rightbottom = centres.copy(), centres.copy()          # boxes of about 120 x 180 pixels around the centre
    lefttop[:, 0, 0] -= 60
    lefttop[:, 0, 1] -= 90
    rightbottom[:, 0, 0] += 60
    rightbottom[:, 0, 1] += 90
    kp = np.stack([rng.uniform(0, W, (n, 15)), rng.uniform(0, H, (n, 15)), rng.uniform(2.5, 3.5, (n, 15))], -1).astype(np.float32)
    np.random.seed(0)
    sampler = a2j_crops.A2JCropSampler("itop", args.crop, args.crop)
    eng = A2JEngine(precision="fp32", device=dev, max_batch=1, crop=args.crop)
    host_ms, ev_ms = [], []
    for rep in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        items, _ = a2j_crops.itop_items(list(range(n)), centres, lefttop, rightbottom, kp, (H, W), draws=sampler.draws(n), crop_w=args.crop, crop_h=args.crop)
        t1 = time.perf_counter()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        crops, flags = eng.train_crops(frames, items)
        b.record()
        torch.cuda.synchronize()
        if rep >= args.warmup:
            host_ms.append((t1 - t0) * 1e3)
            ev_ms.append(a.elapsed_time(b))
    assert not flags.cpu().numpy().any() and bool(torch.isfinite(crops).all())
    ev, host = np.sort(ev_ms), np.sort(host_ms)
    out = {"device": torch.cuda.get_device_name(0), "n": n, "crop": args.crop, "frames": [H, W, "float16"], "warmup": args.warmup, "reps": args.reps,
           "train_crop_ms": {"median": float(np.median(ev)), "min": float(ev[0]), "p90": float(ev[int(0.9 * (len(ev) - 1))]), "max": float(ev[-1])},
           "host_items_ms": {"median": float(np.median(host)), "min": float(host[0]), "max": float(host[-1])},
           "bytes_written": n * args.crop * args.crop * 4}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)
    return out


if __name__ == "__main__":
    main()
