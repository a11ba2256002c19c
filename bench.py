#!/usr/bin/env python
"""Headline benchmark: end-to-end depth-frames/s (480x640 f16 frames -> 3D joints) on N MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K-step region `--reps` times and prints the headline line (`value`, `ms_per_step`).
`--full` adds everything else the bench measures or checks: the hand-over regions from pinned host memory, the power /
sustained-MFMA probe, the per-kernel roofline pass, the multi-person and precision-mode legs, the CPU baseline, the
parity-mode / YoloPoseNet / RCCL child legs and the training step.  `--dump-outputs DIR` writes what the last timed step
returned to its caller (the pose records of its 32 frames; with `--workload train` the loss terms, parameters and gradient)
as DIR/<name>.npy; the inputs are seeded, so two builds can be compared output for output.

N > 1 from a bare shell: bench.py starts N fresh ranks itself (torch.distributed.run, one process per GPU, RCCL over
xGMI) BEFORE anything touches the GPU and relays rank 0's JSON line; started under torch.distributed.run it is a rank.

One step = one batch of 32 synthetic 480(w)x640(h) depth frames through the whole hot path on one GPU:
pn_preprocess -> rtpose_light3d forward (bf16 MFMA) -> pose parsing -> compact records copied to pinned host memory
(BASELINE.json configs[1]).  Every step takes a DIFFERENT batch: 18 distinct batches (354 MB, more than the 256 MB
Infinity Cache) rotate through the three in-flight slots.  The K-step timed region runs `--reps` (5) times per input
mode and the MEDIAN is reported, with min / max:
  * `value`               inputs already resident in HBM when the region starts (the bench contract);
  * `h2d_inclusive.value` every batch handed over from pinned host memory inside the region (19.7 MB per step over
                          PCIe on a copy stream, StreamingEngine.submit_host) -- SURVEY 8(d)'s "first H2D enqueue to
                          last record on host".
Weights are seeded random with the heat head calibrated to a realistic peak density (pipeline.calibrate_heads); data
is synthetic (no dataset / checkpoint ships with the reference).

Multi-GPU: weak scaling, every rank runs its own 32-frame batches (frames are independent, no collective on the data
path) and ONE all-gather of the pose records over RCCL/xGMI closes every timed region.  Prints exactly one JSON line
on rank 0.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

# The StreamingEngine keeps 3 compute streams + 1 copy stream busy; the HIP runtime multiplexes streams onto 4 hardware
# queues by default, so a fifth stream shares a queue with another and the PCIe hand-over of one batch serialises with the
# kernels of another (h2d_inclusive 45 k frames/s at 4 queues, 56-60 k at 8; `value` unchanged).  Must be set before the
# runtime initialises, i.e. before torch is imported; an explicit setting in the environment wins.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402


class GpuPowerSampler:
    """Package power and shader clock of the GPU this rank runs on, read from its hwmon files (plain sysfs reads, no privileges) every
    `period` seconds between start() and stop().  Context for `roofline.frac`: the 2.5 PFLOP/s peak assumes 2.4 GHz, and the conv stack
    holds the package at ~1.3 kW of its 1.4 kW limit at ~2.07 GHz (profiles/r05_power.txt).  Returns None where the files are absent.
    NEVER runs during a region that feeds `value` (its polling thread shares the GIL with the enqueue loop): bench.py samples
    one extra untimed region of >= 0.9 s and the pn_mfma_sustained probe."""

    def __init__(self, device_index, period=0.004):
        import glob
        import threading
        self.dir, self.period, self._stop, self._thr, self.samples = None, period, threading.Event(), None, []
        try:
            p = torch.cuda.get_device_properties(device_index)
            bdf = "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
            for h in glob.glob("/sys/bus/pci/devices/%s/hwmon/hwmon*" % bdf):
                if os.path.exists(os.path.join(h, "power1_input")) and os.path.exists(os.path.join(h, "freq1_input")):
                    self.dir, self.bdf = h, bdf
        except Exception:                                         # noqa: BLE001 -- no such attributes / no sysfs: the field stays null
            self.dir = None

    def _read(self, name):
        with open(os.path.join(self.dir, name)) as f:
            return int(f.read().strip())

    def start(self):
        import threading
        if self.dir is None:
            return self
        self._t0 = time.perf_counter()
        def loop():
            while not self._stop.is_set():
                try:
                    self.samples.append((time.perf_counter() - self._t0, self._read("power1_input") / 1e6, self._read("freq1_input") / 1e6))
                except (OSError, ValueError):
                    pass
                self._stop.wait(self.period)
        self._thr = threading.Thread(target=loop, daemon=True)
        self._thr.start()
        return self

    def stop(self, what=""):
        """-> {"package_w_median", "sclk_mhz_median", ...} over the SECOND half of the sampled interval (power1_input is the firmware's
        moving average: it needs ~0.3 s to rise), or None when the interval was shorter than 0.3 s / the files are absent."""
        if self.dir is None or self._thr is None:
            return None
        self._stop.set()
        self._thr.join()
        span = self.samples[-1][0] if self.samples else 0.0
        late = [(w, f) for t, w, f in self.samples if t >= 0.5 * span]
        if span < 0.3 or len(late) < 3:
            return None
        w = np.array([a for a, _ in late]); f = np.array([b for _, b in late])
        try:
            cap = self._read("power1_cap") / 1e6
        except (OSError, ValueError):
            cap = None
        return {"package_w_median": round(float(np.median(w)), 1), "package_w_max": round(float(w.max()), 1), "package_w_limit": cap,
                "sclk_mhz_median": round(float(np.median(f)), 0), "sclk_mhz_min": round(float(f.min()), 0), "samples": len(late), "sampled_s": round(span, 3),
                "what": "hwmon power1_input / freq1_input of %s every %.0f ms, second half of %s" % (self.bdf, self.period * 1e3, what)}

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BATCH = int(os.environ.get("POPNET_BENCH_BATCH", "32"))     # 32 = BASELINE configs[1]; the override is for experiments only
_PINNED = {}
PEAK_TFLOPS = {"bf16": 2500.0, "bf16x3": 2500.0, "fp32": 157.3}      # dense MFMA peaks, /opt/skills/guides/MI355X_MICROARCH.md


def cpu_baseline(engine, depth_host, frames_sample=32, reps=3):
    """The oracle (a port of the reference's CPU path: numpy/cv2-restatement pre-proc, torch fp32 CPU
    forward, NumPy parse) timed on a bounded sample of the same workload: ~15 s of CPU work.  torch's
    intra-op pool runs at min(32, host cores) threads -- these small convolutions do not scale to hundreds of
    threads (rounds 1-3 also tried every host core and always reported 32: on a 256-core host that trial alone
    cost 150 s of the bench's 240 s wall time, round 4 `leg_seconds`)."""
    from oracle import nets as onets, parse_paf as oparse, preproc as opre
    cores = os.cpu_count() or 1
    sd = {k: v.detach().cpu().clone() for k, v in engine.model.state_dict().items()}
    d = depth_host[:frames_sample]
    t0 = time.time()
    x = torch.from_numpy(opre.preprocess_batch(d))
    t_pre = time.time() - t0
    best = None
    for threads in (min(32, cores),):
        torch.set_num_threads(threads)
        onets.rtpose_light3d_forward(x[:1], sd)                      # warm the thread pool / allocator
        t1 = time.time()
        for _ in range(reps):
            paf, heat, z = onets.rtpose_light3d_forward(x, sd)
        t_fwd = (time.time() - t1) / reps
        if best is None or t_fwd < best[0]:
            best = (t_fwd, threads, paf, heat, z)
    t_fwd, threads, paf, heat, z = best
    t2 = time.time()
    paf, heat, z = (a.numpy().transpose(0, 2, 3, 1) for a in (paf, heat, z))
    for _ in range(reps):
        for b in range(len(d)):
            oparse.frame_to_records(heat[b].copy(), paf[b].copy(), z[b].copy())
    t_parse = (time.time() - t2) / reps
    total = t_pre + t_fwd + t_parse
    # SURVEY 8(d) asks for the reference's default batch as well: B = 15 (evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py:130), same
    # thread count, the batch-independent stages scaled to 15 frames
    torch.set_num_threads(threads)
    onets.rtpose_light3d_forward(x[:1], sd)
    t3 = time.time()
    for _ in range(reps):
        onets.rtpose_light3d_forward(x[:15], sd)
    t_fwd15 = (time.time() - t3) / reps
    n15 = min(15, len(d))
    total15 = (t_pre + t_parse) * n15 / len(d) + t_fwd15
    b15 = {"value": round(n15 / total15, 3), "unit": "frames/s", "cores": threads, "batch": n15,
           "sample": "the first %d of those frames as one batch (the reference's default batch size): torch-CPU forward %.2fs (%d threads) + the per-frame "
                     "preproc / parse times of the 32-frame sample" % (n15, t_fwd15, threads)}
    return {"value": round(len(d) / total, 3), "unit": "frames/s", "cores": threads, "kind": "port", "host_cores": cores, "batch": len(d), "b15": b15,
            "sample": "%d of the step's 32 frames (forward and parse repeated 3x, means reported), fp32: preproc %.2fs (1 thread) + torch-CPU forward %.2fs (%d threads of the host's %d cores) + "
                      "numpy parse %.2fs (1 thread)" % (len(d), t_pre, t_fwd, threads, cores, t_parse)}


def mpaug_parse_leg(engine, reps=20):
    """BASELINE configs[3] (multi-person stream, >= 4 persons per frame): the pose-assembly kernels on planted maps with
    4 / 6 / 8 overlapping persons per frame, 32 frames per launch; HIP-event time of pn_parse_paf."""
    from popnet_amd import synth
    out = {}
    dev = engine.device
    for persons in (2, 4, 6, 8):
        heat, paf, z = synth.planted_batch(4242 + persons, [persons] * engine.max_batch, noise=0.01)
        engine.heat.copy_(torch.from_numpy(heat).to(dev))
        engine.paf.copy_(torch.from_numpy(paf).to(dev))
        engine.z.copy_(torch.from_numpy(z).to(dev))
        for _ in range(3):
            engine.parse(engine.max_batch)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            engine.parse(engine.max_batch)
        b.record()
        torch.cuda.synchronize()
        from popnet_amd.pipeline import records_to_numpy
        recs = records_to_numpy(engine.frames)
        out["%d_persons" % persons] = {"parse_us_per_step": round(a.elapsed_time(b) * 1e3 / reps, 2),
                                       "mean_persons_found": round(float(recs["n_persons"].mean()), 2),
                                       "mean_peaks": round(float(recs["n_peaks"].mean()), 1),
                                       "overflow_frames": int((recs["status"] != 0).sum())}
    return out


def precision_modes_leg(dev, steps=30):
    """north_star's tolerance (1e-3 m, identical assignment) per precision mode, next to what each mode costs: every mode
    against the fp32 engine on 96 frames of this workload at both synthetic weight sets (popnet_amd.fidelity), and the
    single-engine, un-pipelined frames/s of the same eager loop in every mode (so the ratios compare like with like)."""
    from popnet_amd import synth
    from popnet_amd.fidelity import compare_engines
    from popnet_amd.pipeline import PoseEngine
    out = {}
    depth = torch.from_numpy(synth.synth_depth(BATCH, 640, 480, seed=77)).to(dev)
    ref = {g: PoseEngine(precision="fp32", device=dev, max_batch=BATCH, calib_gain=g) for g in (1.0, 6.0)}
    for prec in ("fp32", "bf16x3", "bf16"):
        eng = {g: (ref[g] if prec == "fp32" else PoseEngine(precision=prec, device=dev, max_batch=BATCH, calib_gain=g)) for g in (1.0, 6.0)}
        e = eng[1.0]
        for _ in range(3):
            e.predict(depth)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            e.predict(depth)
        torch.cuda.synchronize()
        rec = {"frames_per_s_one_engine_eager": round(steps * BATCH / (time.perf_counter() - t0), 1)}
        if prec != "fp32":
            rec["vs_fp32_threshold_calibrated_weights"] = compare_engines(ref[1.0], eng[1.0], 96)
            rec["vs_fp32_separated_weights"] = compare_engines(ref[6.0], eng[6.0], 96)
        out[prec] = rec
    return out


def synth_training_batch(dev, B, seed=0, persons=2):
    """A training batch the way the reference's dataset builds one (datasets_kdh3d_rtpose_mpaug.py:223-286 (CR)), on the GPU:
    `persons` single-person source frames per item composited over a background, resized, and the heat / PAF / z / fg targets
    rasterised from the planted skeletons (popnet_amd.targets.mpaug_batch).  Returns (batch tuple, seconds it took)."""
    from popnet_amd import synth, targets
    rng = np.random.default_rng(seed)
    H, W = 640, 480
    fd = torch.from_numpy(np.clip(rng.normal(2.5, 0.3, (B, persons, H, W)), 0.3, 5.9).astype(np.float16)).to(dev)
    fm = torch.zeros((B, persons, H, W), dtype=torch.uint8, device=dev)
    k2 = np.zeros((B, persons, 15, 2), dtype=np.float32)
    k3 = np.zeros((B, persons, 15, 3))
    for b in range(B):
        j, d = synth.planted_persons(rng, persons, size=224)
        k2[b] = j * np.array([W / 224.0, H / 224.0])               # annotations live in ORIGINAL pixel coordinates
        k3[b, :, :, 2] = d[:, None]
        for p in range(persons):
            x0, y0 = np.maximum(k2[b, p].min(0).astype(int) - 10, 0)
            x1, y1 = k2[b, p].max(0).astype(int) + 10
            fm[b, p, y0:y1, x0:x1] = 1
    bg = torch.from_numpy(np.clip(rng.normal(4.5, 0.3, (B, H, W)), 0, 6).astype(np.float16)).to(dev)
    n_src = torch.full((B,), persons, dtype=torch.int32, device=dev)
    npers = torch.full((B,), persons, dtype=torch.int32, device=dev)
    k2d, k3d = torch.from_numpy(k2).to(dev), torch.from_numpy(k3).to(dev)
    targets.mpaug_batch(fd, fm, n_src, bg, k2d, k3d, npers)           # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, heat, paf, z, fg = targets.mpaug_batch(fd, fm, n_src, bg, k2d, k3d, npers)
    torch.cuda.synchronize()
    return (x.contiguous(), heat, paf, z, fg), time.perf_counter() - t0


def train_step_cpu(batch, threads=32):
    """The oracle's training step (torch fp32 CPU autograd, oracle/train.py -- the checker, timed here as the CPU baseline of
    the training workload only) on the same batch and initial state, one warm-up + one timed step."""
    from oracle import train as otrain
    from popnet_amd import synth
    sd = synth.init_like_state_dict(seed=3)
    cpu = [b.cpu() for b in batch]
    old = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        otrain.train_step(sd, *cpu, lr=0.05)
        t0 = time.perf_counter()
        otrain.train_step(sd, *cpu, lr=0.05)
        dt = time.perf_counter() - t0
    finally:
        torch.set_num_threads(old)
    return {"ms_per_step": round(dt * 1e3, 1), "frames_per_s": round(len(cpu[0]) / dt, 2), "cores": threads, "kind": "port"}


def train_step_leg(dev, steps=8, warmup=2, world=1, group=None, lr=0.05, cpu=False, precision="fp32", batch_in=None, extras=True, last=None):
    """BASELINE configs[4]: one training step of rtpose_light3d (train-mode forward, rtpose_light3d_loss_fgweight, backward,
    Nesterov SGD; popnet_amd.train.TrainEngine, every kernel hand-written HIP) on BATCH frames of 224 x 224 per rank from the
    reference's initial state, targets built on the GPU; with world > 1 the flat 22 MB gradient is all-reduced every step.
    precision "fp32" = the parity mode (exact fp32 FMA chains), "bf16x3" = split-bf16; both on the round-6 planes engine (csrc/trainx.hip).
    extras=False skips the bf16x3 leg next to the fp32 one; a dict `last` receives the engine and the loss terms of the last timed step."""
    from popnet_amd import synth
    from popnet_amd.train import TrainEngine
    batch, t_targets = batch_in if batch_in is not None else synth_training_batch(dev, BATCH)
    eng = TrainEngine(synth.init_like_state_dict(seed=3), device=dev, lr=lr, world_size=world, process_group=group, precision=precision)
    first = float(eng.step(*batch).sum())
    eng.capture(*batch)                                              # the step as one hipGraph (two more eager steps inside)
    for k in range(warmup):
        t = eng.step(*batch)
    torch.cuda.synchronize()
    if world > 1:
        import torch.distributed as dist
        dist.barrier(group=group)
    t0 = time.perf_counter()
    for _ in range(steps):
        t = eng.step(*batch)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    if last is not None:
        last.update(engine=eng, terms=t)
    flops = 3 * 13.343e9 * BATCH                                     # forward + data gradient + weight gradient, SURVEY 8d's per-frame figure
    extra = {"cpu_baseline": train_step_cpu(batch)} if cpu else {}
    if extras and precision == "fp32" and batch_in is None and world == 1:      # the opt-in fast mode on the same batch, next to the parity mode
        fast = train_step_leg(dev, steps, warmup, world, group, lr, False, "bf16x3", (batch, t_targets))
        extra["bf16x3"] = {k: fast[k] for k in ("ms_per_step", "frames_per_s_per_gpu", "tflops", "loss_first_step", "loss_last_step", "launch_mode")}
        extra["bf16x3"]["physical_bf16_tflops"] = round(3 * fast["tflops"], 1)
        extra["bf16x3"]["frac_of_bf16_peak_physical"] = round(3 * fast["tflops"] / PEAK_TFLOPS["bf16"], 4)
        extra["bf16x3"]["what"] = ("TrainEngine(precision='bf16x3'), round 6: the whole step on NHWC [hi | lo] bf16 planes (csrc/trainx.hip) -- forward and data-gradient convolutions "
                                   "on the inference kernels (conv3 / conv4 / conv_mfma), pixel-K MFMA weight gradient (ds_read_b64_tr_b16), channel-minor BatchNorm / pool / head passes")
    return {**extra, "ms_per_step": round(dt * 1e3, 3), "frames_per_s_per_gpu": round(BATCH / dt, 1), "tflops": round(flops / dt / 1e12, 1), "dtype": "f32",
            "peak_tflops_f32_mfma": 157.0, "batch_per_gpu": BATCH, "input": "224x224", "parameters": int(eng.n_params),
            "loss_first_step": round(first, 5), "loss_last_step": round(float(t.sum()), 5), "targets_on_gpu_ms_per_batch": round(t_targets * 1e3, 3),
            "launch_mode": ("one C call per step, launches issued from C++ on two HIP streams (eager), update eager" if eng.planes else
                            "hipGraph replay of the step" if world == 1 else "hipGraph replay of forward + backward, all-reduce and update eager"),
            "engine": ("planes (csrc/trainx.hip): one fp32 plane per tensor, generic fp32 inference kernel for forward / data gradient, K = 4 row-streaming weight gradient" if eng.planes and precision == "fp32"
                       else "planes (csrc/trainx.hip)" if eng.planes else "NCHW (csrc/train.hip)"),
            "what": "TrainEngine.step: train-mode forward (batch-statistics BatchNorm), fg-weighted loss, backward (MFMA dgrad / wgrad), Nesterov SGD; %s"
                    % ("one all-reduce of the flat gradient per step over %d ranks" % world if world > 1 else "single GPU")}


def train_workload(args, dev, world, rank, dist):
    """`--workload train`: the training step as the timed workload (weak scaling: BATCH frames per rank per step)."""
    last = {}
    leg = train_step_leg(dev, steps=args.steps, warmup=max(2, min(args.warmup, 5)), world=world, group=None, extras=args.full, last=last)
    ms = torch.tensor([leg["ms_per_step"]], device=dev)
    if world > 1:
        dist.all_reduce(ms, op=dist.ReduceOp.MAX)
    if rank == 0 and args.dump_outputs:
        eng = last["engine"]
        dump_outputs(args.dump_outputs, {"loss_terms": last["terms"], "parameters": eng.flat_p, "gradient": eng.flat_g})
    if rank == 0:
        m = float(ms)
        print(json.dumps({"metric": "training frames/sec (rtpose_light3d_kdh3d_mpaug step, 224x224)", "value": round(world * BATCH / (m / 1e3), 1), "unit": "frames/s",
                          "n_gpus": world, "steps": args.steps, "warmup": max(2, min(args.warmup, 5)), "ms_per_step": round(m, 3),
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                          "config": {"workload": "BASELINE configs[4]: training step, batch %d per GPU, data parallel" % BATCH}, "train_step": leg}))


def dump_outputs(path, arrays):
    """--dump-outputs: every array as <path>/<name>.npy -- floating fields in their own precision (float32 / float64), integer fields
    as float64 (exact for these widths).  Structured record arrays are written one field per file (<name>_<field>.npy)."""
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        parts = {"%s_%s" % (name, f): a[f] for f in a.dtype.names} if a.dtype.names else {name: a}
        for n, v in parts.items():
            v = v if v.dtype in (np.float32, np.float64) else v.astype(np.float64)
            np.save(os.path.join(path, n + ".npy"), np.ascontiguousarray(v))


def bench_env():
    """Every environment variable that can change what the timed region runs, recorded in the JSON line.
    Timing-only ablation switches are refused outright: the shipped library has them compiled out (pn_build_experiments() == 0),
    a lab build that honours them is refused as well."""
    keep = ("GPU_MAX_HW_QUEUES", "HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "HSA_ENABLE_IPC_MODE_LEGACY", "OMP_NUM_THREADS")
    env = {k: v for k, v in sorted(os.environ.items()) if k.startswith("POPNET_") or k in keep}
    # (POPNET_TRAINX_*: scheduling / cross-check switches of the planes training engine -- the bench times the defaults only)
    forbidden = [k for k in env if k in ("POPNET_ABLATE_SKIP", "POPNET_X3_BF16_CONVS") or k.startswith("POPNET_TRAINX_")]
    if forbidden:
        raise SystemExit("bench.py: refusing to run with %s set (timing-only / result-changing experiment switches; unset them)" % ", ".join(forbidden))
    return env


def surface_in_parsed(out):
    """The driver's record keeps `config`, `roofline` and `cpu_baseline` of the line verbatim and lists every other key by name only
    (VERDICT r04 items 1, 4).  What a reader of that record must see next to `value` therefore goes INTO those objects: whether the
    headline dtype meets north_star's tolerance, the H2D-inclusive rate of the same region (SURVEY 8(d)'s literal metric), and the
    tolerance-meeting mode's own throughput / fidelity -- nested once and repeated as flat scalars."""
    cfg, rf = out["config"], out["roofline"]
    h2d = out.get("h2d_inclusive") or {}
    fid = out.get("fidelity") or {}
    if h2d:
        cfg["h2d_inclusive_value"] = h2d["value"]
        cfg["h2d_inclusive_fraction_of_value"] = h2d["fraction_of_value"]
        cfg["host_link_GBps"] = (h2d.get("host_link") or {}).get("GBps")
    if fid:
        cfg["value_meets_north_star_tolerance"] = fid["meets_north_star_tolerance"]
        cfg["value_same_assignment"] = fid["same_assignment"]
        cfg["value_d3_m_max"] = fid["d3_m_max"]
    pm = out.get("parity_mode") or {}
    if "value" in pm:
        f = pm["fidelity"]["threshold_calibrated_weights"]
        prf = pm["roofline"]
        block = {"dtype": pm["dtype"], "value": pm["value"], "unit": "frames/s", "ms_per_step": pm["ms_per_step"],
                 "h2d_inclusive": (pm.get("h2d_inclusive") or {}).get("value"),
                 "frac_physical": prf["frac"], "frac_algorithmic": round(prf["algorithmic_tflops"] / prf["peak"], 4),
                 "conv_stack_frac_physical": prf["conv_stack_physical_frac"],
                 "same_assignment": "%d/%d" % (f["same_assignment"], f["frames"]), "d3_m_max": f["d3_m_max"],
                 "meets_north_star_tolerance": bool(f["d3_m_max"] < 1e-3 and f["same_assignment"] >= f["frames"] - 2)}
        rf["parity_mode"] = block
        cfg["parity_mode"] = dict(block)
        for k in ("value", "ms_per_step", "h2d_inclusive", "frac_physical", "same_assignment", "d3_m_max", "meets_north_star_tolerance"):
            cfg["parity_mode_" + k] = block[k]
    tr = out.get("train_step") or {}
    if "ms_per_step" in tr:
        cfg["train_step_ms_fp32"] = tr["ms_per_step"]
        cfg["train_step_ms_bf16x3"] = (tr.get("bf16x3") or {}).get("ms_per_step")
    yl = out.get("yolo") or {}
    if "value" in yl:
        cfg["yolo_value"] = yl["value"]
        cfg["yolo_conv_stack_frac"] = (yl.get("conv_stack") or {}).get("frac")
    cs = rf.get("conv_stack") or {}
    rf["conv_stack_frac"] = cs.get("frac")
    pp = out.get("postproc") or {}
    if pp:
        rf["postproc_us_per_step"] = pp.get("us_per_step")


def plan_legs(world, rank, net, precision, no_extras, no_cpu_baseline):
    """Which secondary legs a rank runs besides the timed regions.  Everything here is rank-0-only AND world-1-only: an N-rank run
    (the driver's SCALE pass) times the headline region on every rank and nothing else -- no child processes, no CPU baseline, no
    extra engines that would oversubscribe the host or the GPUs next to the other ranks."""
    solo = rank == 0 and world == 1
    default_line = solo and net == "rtpose" and not no_extras
    return {"extras": default_line,                                                  # mpaug_parse, precision_modes, fidelity
            "cpu_baseline": solo and net == "rtpose" and not no_cpu_baseline,
            "children": default_line and precision == "bf16",                         # parity_mode, yolo, rccl_check (fresh child processes)
            "train_step": default_line and precision == "bf16"}


def launcher_dry_run(args):
    """CPU check of the self-launch path: every rank joins a gloo group, rank 0 prints one JSON line."""
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:
        dist.init_process_group(backend="gloo")
    t = torch.tensor([rank + 1], dtype=torch.int64)
    if world > 1:
        dist.all_reduce(t)
    # the same call main() makes after the timed region, on EVERY rank (a collective entered by rank 0 alone hangs the job)
    chk = dist_check(torch.device("cpu"), world, rank, dist) if world > 1 else None
    if rank == 0:
        print(json.dumps({"launcher_dry_run": True, "n_gpus": world, "rank_sum": int(t.item()), "local_rank": int(os.environ.get("LOCAL_RANK", "0")), "dist": chk}))
    if world > 1:
        dist.destroy_process_group()


def dist_check(dev, world, rank, dist):
    """RCCL on the hardware: with the process group initialised (backend "nccl" = RCCL; also at
    world_size 1 under --force-dist) run the two real exchanges of the repo on device tensors and compare with what
    they must return: pipeline.gather_records (the single all-gather of pose records) and
    TrainEngine.reduce_flat_gradient (the all-reduce of the 22 MB flat gradient)."""
    from popnet_amd import _lib
    from popnet_amd.pipeline import gather_records
    from popnet_amd.train import TrainEngine

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()
    item = _lib.POSE_WIRE_DTYPE.itemsize
    n_frames = 96 * world
    g = torch.Generator(device="cpu").manual_seed(11)
    allrec = torch.randint(0, 256, (n_frames, item), dtype=torch.uint8, generator=g)
    mine = allrec[rank::world].to(dev)
    # the first collective of a process group creates the communicator (178 ms at world 1 in round 4: that was what `gather_ms` timed);
    # one warm-up exchange first, then the median of 5 timed gathers
    ranks = torch.zeros(world, dtype=torch.int64, device=dev)
    ranks[rank] = 1
    dist.all_reduce(ranks)                                           # every rank adds its own 1: ranks_seen must equal world
    gather_records(mine, n_frames, rank, world)
    sync()
    tg = []
    for _ in range(5):
        t0 = time.perf_counter()
        got = gather_records(mine, n_frames, rank, world)
        sync()
        tg.append(time.perf_counter() - t0)
    t_gather = float(np.median(tg))
    gather_ok = bool(torch.equal(got.cpu(), allrec))
    flat = torch.randn(5525816, generator=g).to(dev)               # the trainer's flat gradient buffer: 22 MB
    ref = flat.clone()
    TrainEngine.reduce_flat_gradient(flat, world, None, force=True)
    sync()
    t1 = time.perf_counter()
    for _ in range(5):
        TrainEngine.reduce_flat_gradient(flat, world, None, force=True)
    sync()
    t_ar = (time.perf_counter() - t1) / 5
    # world replicas of the same buffer summed 6 times: flat == ref * world ** 6 -- exactly at world 1 and 2; a ring sums a, 2a, 3a, ...
    # sequentially and 3a is not always representable, so for world > 2 each all-reduce may round (world - 1) times: <= 2^-24 each
    # (found by the world-8 gloo dry run of round 4: the exact comparison would have reported False on the first real 8-GPU run)
    want = ref * float(world) ** 6
    allreduce_ok = bool(torch.equal(flat, want)) if world <= 2 else bool(torch.allclose(flat, want, rtol=6 * (world - 1) * 2.0 ** -23, atol=0.0))
    maps = open("/proc/self/maps").read()
    libs = sorted({ln.split("/")[-1] for ln in maps.splitlines() if "librccl" in ln or "libnccl" in ln})
    return {"backend": dist.get_backend(), "world_size": world, "gather_records_ok": gather_ok, "flat_gradient_allreduce_ok": allreduce_ok,
            "ranks_seen": int(ranks.sum().item()),
            "gather_ms": round(t_gather * 1e3, 3), "gather_ms_what": "median of 5 gathers after one warm-up exchange (communicator creation excluded)", "allreduce_22MB_ms": round(t_ar * 1e3, 3), "collective_library_loaded": libs,
            "what": "pipeline.gather_records on %d device-resident wire records and TrainEngine.reduce_flat_gradient on the 22 MB flat buffer over the initialised process group" % n_frames}


def pipelined_leg(args, dev, world, rank, dist, net, precision, want_h2d, dist_active):
    """The timed regions of one (network, precision): `--reps` repetitions of the K-step region with the inputs resident in HBM
    (-> value) and, with --full, the power / sustained-MFMA probe, the regions handed over from pinned host memory (want_h2d ->
    h2d_inclusive) and the eager roofline pass with HIP events around every conv launch.  Returns {"out": the JSON fields (rank 0; None
    elsewhere), "engine", "depth_host", "se", "last_records" / "last_seed": the last timed step's records and the seed of its input batch}."""
    from popnet_amd import _lib, synth
    from popnet_amd.pipeline import PoseEngine, StreamingEngine, YoloEngine
    Engine = PoseEngine if net == "rtpose" else YoloEngine
    REC = _lib.POSE_FRAME_DTYPE if net == "rtpose" else _lib.YOLO_FRAME_DTYPE
    WIRE = _lib.POSE_WIRE_DTYPE if net == "rtpose" else REC

    # popnet_amd.pipeline.StreamingEngine: PIPE batches in flight (per slot: engine = activations + private parse scratch,
    # POOL static input buffers, record buffers, a HIP stream, ONE hipGraph of the whole step per input buffer).  Batch k
    # runs on slot k % PIPE, so the latency-bound tail of one batch (head convs, pose parsing, the record D2H copy)
    # overlaps with the convolutions of the next.  Every batch still runs the whole path; only its latency is hidden.
    PIPE, POOL = max(1, args.pipeline), max(1, args.pool)
    NIN = PIPE * POOL
    se = StreamingEngine(Engine, depth=PIPE, pool=POOL, wire=True, graph=not args.no_graph, precision=precision, device=dev, max_batch=BATCH)
    engines, streams = se.engines, se.streams
    engine = engines[0]
    pinned = []                                                  # NIN distinct batches, pinned on the host ...
    for i in range(NIN):
        seed = 1234 + 1000 * rank + i
        if seed not in _PINNED:                                  # shared by the legs of one run (same frames in every mode)
            _PINNED[seed] = torch.from_numpy(synth.synth_depth(BATCH, 640, 480, seed=seed)).pin_memory()
        h = _PINNED[seed]
        pinned.append(h)
        se.input(i // POOL, i % POOL).copy_(h)                   # ... and resident in HBM (slot i // POOL, buffer i % POOL)
    depth_host = pinned[0].numpy()
    torch.cuda.synchronize()
    K, W = args.steps, args.warmup
    witem = WIRE.itemsize
    keep = torch.empty((K, BATCH, witem), device=dev, dtype=torch.uint8)       # every step's host-bound records (checks, gather)
    gathered = torch.empty((world * K * BATCH, witem), device=dev, dtype=torch.uint8) if dist_active else None

    batch_of = [0] * K                                           # which of the NIN batches step k of the LAST region ran

    keep_records = {"on": True}

    AHEAD = PIPE if POOL >= 2 else 0                             # hand-over regions: transfers posted this many batches ahead of their step

    def step(k, h2d):
        sl = se._tickets % PIPE                                  # the slot this submit will use
        if h2d:                                                  # PCIe-inclusive: 19.7 MB per batch, copied on the copy stream into the
            i = k % NIN                                          # slot's next input buffer (under the kernels of earlier batches)
            if AHEAD:
                t = se.submit_posted()                           # batch k: posted AHEAD steps ago (the first AHEAD before the region opened)
                se.post_host(pinned[(k + AHEAD) % NIN])          # ... and the transfer of batch k + AHEAD leaves now
            else:
                t = se.submit_host(pinned[i])
        else:                                                    # resident: buffer j of the slot holds batch sl * POOL + j
            j = (k // PIPE) % POOL
            i = sl * POOL + j
            t = se.submit(j)
        batch_of[k % K] = i
        if keep_records["on"]:                                   # bench bookkeeping (consistency check, the gather), not the product path
            with torch.cuda.stream(se.stream(t)):
                keep[k % K].copy_(se.wires[t % PIPE] if se.wire else se.records(t), non_blocking=True)

    host_enqueue_s = {}

    def region(h2d, steps=None):
        """K steps, barrier + device sync on both sides, max over ranks.  Returns seconds.
        Hand-over regions stream: the transfers of the first AHEAD batches are posted BEFORE the region opens and the region posts the
        transfers of the AHEAD batches after its last step (K transfers and K steps inside the window either way) -- a live stream's
        next frames are already on the link while the previous ones finish."""
        n = K if steps is None else steps
        if h2d and AHEAD:
            se.drop_posted()
            for a in range(AHEAD):
                se.post_host(pinned[a % NIN])
        if dist_active:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n):
            step(k, h2d)
        host_enqueue_s[h2d] = (time.perf_counter() - t0) * K / n  # how long the host needed to enqueue K steps
        if h2d and AHEAD and not dist_active:
            # "... to last record on host" -- the window closes when the last step's records have landed in pinned host memory
            # (every slot stream drained); the AHEAD transfers posted for the batches AFTER this window are drained untimed below
            for st in streams:
                st.synchronize()
            el = time.perf_counter() - t0
            torch.cuda.synchronize()
            return el
        se.join()
        if dist_active:
            dist.all_gather_into_tensor(gathered, keep.view(K * BATCH, witem))
        torch.cuda.synchronize()
        if dist_active:
            dist.barrier()
        el = time.perf_counter() - t0
        if dist_active:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el

    se.capture()
    # W untimed steps as asked -- and never fewer than 30: the first 20-step region of a fresh process ran 8-9 % under the median on clocks
    # that had not settled (r05 children, r06 main leg 62.9 k against 68.3 k); `warmup_steps_run` in the line says what ran
    WARM = max(W, 30)
    for i in range(WARM):
        step(i % K, False)
    se.join()
    if dist_active:
        dist.all_gather_into_tensor(gathered, keep.view(K * BATCH, witem))
    torch.cuda.synchronize()

    REPS = max(1, args.reps)
    runs = {"resident": [region(False) for _ in range(REPS)]}       # nothing else runs in this process while these are timed (no sampler thread: ADVICE r05)
    keep_res, batch_res = keep.cpu(), list(batch_of)
    # power / clock of the SAME resident region, sampled through one extra UNTIMED repetition long enough for the firmware's moving
    # average (>= 0.9 s), and the box's sustained matrix-core ceiling (pn_mfma_sustained: nothing but MFMAs on random bf16, 1.5 s)
    power, sustained = None, None
    if args.full and rank == 0 and world == 1 and not args.no_power:
        per_step = float(np.median(runs["resident"])) / K
        nlong = max(K, int(0.9 / max(per_step, 1e-6)) + 1)
        keep_records["on"] = False
        smp = GpuPowerSampler(dev.index if dev.index is not None else 0).start()
        t_long = region(False, steps=nlong)
        power = smp.stop("one untimed %d-step repetition of the resident region (%.2f s, %.1f frames/s)" % (nlong, t_long, nlong * BATCH / t_long))
        keep_records["on"] = True
        region(False)                                            # restores keep / batch_of to a K-step region's (the checks below read them)
        keep_res, batch_res = keep.cpu(), list(batch_of)
        tf, ghz = C.c_double(), C.c_double()
        smp = GpuPowerSampler(dev.index if dev.index is not None else 0).start()
        rc_ = _lib.lib().pn_mfma_sustained(engine.ctx.handle, 1.5, 4, C.byref(tf), C.byref(ghz), _lib.current_stream_ptr(dev))
        torch.cuda.synchronize()
        sp = smp.stop("the pn_mfma_sustained probe")
        if rc_ == 0:
            sustained = {"tflops": round(tf.value, 1), "in_kernel_ghz": round(ghz.value, 3), "power": sp,
                         "what": "pn_mfma_sustained: v_mfma_f32_16x16x32_bf16 only, random bf16 operands, 4 waves per SIMD on every CU, back to back for 1.5 s; the last 20 launches' rate"}
    link = None
    tail_h2d = []
    if want_h2d:
        region(True)                                             # one untimed pass: first touch of the pinned pool; ITS records feed the consistency check
        keep_h2d, batch_h2d = keep.cpu(), list(batch_of)
        # The per-step device copy into `keep` is bench bookkeeping; next to the PCIe transfers it costs the region 4-8 % on boxes with a
        # fast link (scripts/r04/h2d_experiments.py: h2d 68.2 k, with the keep copy 62.6-65.5 k, resident with / without 69.4 / 69.8 k) --
        # the product path is submit_host + the record copy to pinned host memory, and that is what the timed hand-over regions run.
        # A multi-rank run keeps it: the all-gather that closes the region needs every step's records on the device.
        keep_records["on"] = bool(dist_active)
        runs["h2d"] = [region(True) for _ in range(REPS)]
        keep_records["on"] = True
        se.drop_posted()
        # ... so the records of the TIMED hand-over regions are checked too: what the last PIPE steps of the last timed region
        # left in the slots' pinned host buffers must equal what the same batches gave in the resident regions
        if not dist_active:
            nt = min(PIPE, K)
            tail_h2d = [(batch_of[K - nt + i], se.host_records(se._tickets - nt + i).clone()) for i in range(nt)]
        if dist_active:
            keep_h2d, batch_h2d = keep.cpu(), list(batch_of)
        # what the box's link gives: one batch, pinned host -> device, on an idle GPU (the hand-over cannot beat frames / this time)
        tl = []
        for _ in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            se.input(0, 0).copy_(pinned[0], non_blocking=True)
            torch.cuda.synchronize()
            tl.append(time.perf_counter() - t0)
        tcopy = float(np.median(tl[1:]))
        link = {"GBps": round(pinned[0].numel() * pinned[0].element_size() / tcopy / 1e9, 1), "copy_ms_per_batch": round(tcopy * 1e3, 4),
                "frames_per_s_if_link_bound": round(BATCH / tcopy, 1)}
        torch.cuda.synchronize()
        for i in range(NIN):                                     # the hand-over cycled through every input buffer: restore the resident batches
            se.input(i // POOL, i % POOL).copy_(pinned[i])
        torch.cuda.synchronize()
    med = {m: float(np.median(v)) for m, v in runs.items()}
    elapsed = med["resident"]
    # what the last step of the last timed resident region handed to its caller: that step's records
    last_records = keep_res[(K - 1) % K].numpy().view(WIRE).reshape(BATCH)
    last_seed = 1234 + 1000 * rank + batch_res[(K - 1) % K]        # its input batch: synth.synth_depth(BATCH, 640, 480, seed=last_seed)

    def rate(sec):
        return round(world * K * BATCH / sec, 2)
    out = None
    if rank == 0:
        out = {
            "metric": "depth-frames/sec end-to-end (480x640)", "value": rate(elapsed),
            "unit": "frames/s", "n_gpus": world, "steps": K, "warmup": W, "warmup_steps_run": WARM,
            "ms_per_step": round(elapsed / K * 1e3, 4),
            "value_stat": {"what": "median of %d repetitions of the %d-step timed region" % (REPS, K), "min": rate(max(runs["resident"])), "max": rate(min(runs["resident"])),
                           "runs": [rate(v) for v in runs["resident"]]},
            "launch_mode": ("eager" if args.no_graph else "hipGraph replay (one graph per step)") + ", %d batches in flight on separate HIP streams" % PIPE, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": precision,
            "data": "synthetic, %d distinct batches (%.0f MB) resident in HBM, a different batch every step" % (NIN, NIN * BATCH * 640 * 480 * 2 / 1e6),
            "config": {"workload": "BASELINE configs[1]: batch=32 synthetic 480x640 f16 depth frames per GPU per step, "
                                   "resize->224^2, " + ("rtpose_light3d forward + PAF pose parsing" if net == "rtpose" else
                                                        "YoloPoseNet forward + box decode / NMS / skeleton read-out (secondary network of the path)") + ", records D2H",
                       "frames_per_step_per_gpu": BATCH, "input": "480x640 f16", "network_input": "224x224",
                       "weights": "seeded random, " + ("heat head calibrated (pipeline.calibrate_heads)" if net == "rtpose" else "confidence filters calibrated (pipeline.calibrate_yolo_conf)"),
                       "records": "pn_pose_wire (%d B per frame) to pinned host memory every step" % witem if se.wire else "pn_yolo_frame to pinned host memory every step",
                       "parallelism": "frames sharded x%d, one all-gather of records" % world},
        }
    if not args.full:
        return {"out": out, "engine": engine, "depth_host": depth_host, "se": se, "last_records": last_records, "last_seed": last_seed}

    # ---- roofline pass: K steps again, eager, every conv launch bracketed by HIP events on the launch stream (event
    # records inside the throughput pass would perturb it) ----
    L = _lib.lib()
    torch.cuda.synchronize()
    # the pass follows host-side copies and a synchronize: EAGER_WARM untimed eager steps first (a 20-step pass measured 39.2 us per conv4 launch
    # where the 200-step pass of the same box and minute measured 37.4: its first steps ran on clocks that had dropped during the pause)
    EAGER_WARM = 30
    with torch.cuda.stream(streams[0]):
        for k in range(EAGER_WARM):
            nb = engine.forward_frames(se.input(0, k % POOL))
            engine.parse(nb, se.records(0), se.wires[0]) if se.wire else engine.parse(nb, se.records(0))
    torch.cuda.synchronize()
    L.pn_net_profile_begin(engine.net)                           # only slot 0's net records events: its launches alone
    t1 = time.perf_counter()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(K)]
    with torch.cuda.stream(streams[0]):
        for k in range(K):
            nb = engine.forward_frames(se.input(0, k % POOL))  # the product path: pre-processing inside the stem launch (bf16 / bf16x3)
            ev[k][0].record()
            if se.wire:
                engine.parse(nb, se.records(0), se.wires[0])     # post-processing kernels of this step, bracketed on their stream
            else:
                engine.parse(nb, se.records(0))
            ev[k][1].record()
            ev[k][2].record()
            se.host_records(0).copy_(se.wires[0] if se.wire else se.records(0), non_blocking=True)
            ev[k][3].record()
    torch.cuda.synchronize()
    elapsed_profiled = time.perf_counter() - t1
    post_ms = sum(ev[k][0].elapsed_time(ev[k][1]) for k in range(K)) / K
    pack_ms = sum(ev[k][1].elapsed_time(ev[k][2]) for k in range(K)) / K
    d2h_ms = sum(ev[k][2].elapsed_time(ev[k][3]) for k in range(K)) / K
    conv_ms, other_ms, conv_flops = C.c_double(), C.c_double(), C.c_double()
    conv_n, other_n = C.c_int64(), C.c_int64()
    engine.ctx.check(L.pn_net_profile_end(engine.net, C.byref(conv_ms), C.byref(conv_n), C.byref(conv_flops),
                                          C.byref(other_ms), C.byref(other_n)), "pn_net_profile_end")
    kernels = []                                                # per instantiation, dominant first
    for r in range(16):
        name = C.create_string_buffer(96)
        kms, kfl, kn = C.c_double(), C.c_double(), C.c_int64()
        if L.pn_net_profile_kernel(engine.net, r, name, 96, C.byref(kms), C.byref(kn), C.byref(kfl)) != 0:
            break
        kernels.append({"kernel": name.value.decode(), "launches_per_step": kn.value / K, "us_per_step": round(kms.value * 1e3 / K, 2),
                        "avg_launch_us": round(kms.value * 1e3 / max(kn.value, 1), 3),
                        "tflops": round(kfl.value / (kms.value * 1e-3) / 1e12, 2) if kms.value > 0 else 0.0,
                        "flops_per_launch": round(kfl.value / max(kn.value, 1), 1)})
    frames_full = torch.stack([se.records(s) for s in range(PIPE)]).cpu()

    if rank == 0:
        first = {}                                               # the same input batch must give the same records, whatever step / slot / input mode ran it

        def consistent(kept, batches):
            raw = kept.numpy().reshape(K, -1)
            ok = True
            for k in range(K):
                ref = first.setdefault(batches[k], raw[k])
                ok = ok and np.array_equal(ref, raw[k])
            return ok
        same = consistent(keep_res, batch_res)
        if "h2d" in runs:
            same = consistent(keep_h2d, batch_h2d) and same
            for bt, rec in tail_h2d:                             # timed hand-over regions (no bookkeeping copy): the slots' host records
                same = same and bt in first and np.array_equal(first[bt], rec.numpy().reshape(-1)[:first[bt].size])
        wire = keep_res.numpy().view(WIRE).reshape(K, BATCH)
        recs = frames_full.numpy().view(REC).reshape(PIPE, BATCH)
        achieved = conv_flops.value / (conv_ms.value * 1e-3) / 1e12 if conv_ms.value > 0 else 0.0
        peak = PEAK_TFLOPS[precision]
        # network outputs read + records written per frame
        post_bytes = BATCH * ((185024 if net == "rtpose" else 100 * 14 * 14 * 4) + witem)
        dom = kernels[0] if kernels else {"kernel": "none", "us_per_step": 0.0, "avg_launch_us": 0.0, "tflops": 0.0, "flops_per_launch": 0.0, "launches_per_step": 0}
        # HBM bytes per launch of the dominant kernel.  PMC counters cannot be read from inside an un-profiled run: the figure
        # comes from separate `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes (scripts/r05/profiles.sh ->
        # scripts/make_traffic_json.py) and is labelled with where and when it was measured -- `traffic_source` -- so nobody
        # reads a stored constant as part of this run (VERDICT r03 item 3 ii)
        traffic, traffic_source = None, None
        pmc = os.path.join(ROOT, "profiles", "conv_hbm_traffic.json")
        if os.path.exists(pmc):
            try:
                tj = json.load(open(pmc))
                traffic = tj.get("by_kernel", {}).get(dom["kernel"], {}).get("hbm_bytes_per_launch")
                traffic_source = {"file": "profiles/conv_hbm_traffic.json", "measured_in_this_run": False, "commit": tj.get("commit"), "measured_at": tj.get("measured_at"),
                                  "method": tj.get("source"), "correction": tj.get("correction")}
            except Exception:
                traffic = None

        out.update({
            "roofline": {"bound": "mfma", "kernel": dom["kernel"] + " (dominant convolution instantiation: %.0f of %.0f conv us/step)" % (dom["us_per_step"], conv_ms.value * 1e3 / K),
                         "achieved": dom["tflops"], "peak": peak, "unit": "TFLOP/s", "frac": round(dom["tflops"] / peak, 4),
                         "traffic": traffic, "traffic_source": traffic_source, "avg_launch_us": dom["avg_launch_us"], "flops_per_launch": dom["flops_per_launch"],
                         "launches_per_step": dom["launches_per_step"],
                         # flat scalars (the driver's record keeps scalars of this object): the spec-peak `frac` above stays what it was; next to it
                         # the ceiling THIS box sustains on nothing but MFMAs and the package power / clock of the timed region
                         "peak_sustained_tflops": sustained["tflops"] if sustained else None,
                         "frac_of_sustained": round(dom["tflops"] / sustained["tflops"], 4) if sustained and sustained["tflops"] > 0 else None,
                         "peak_sustained_ghz": sustained["in_kernel_ghz"] if sustained else None,
                         "peak_sustained_power_w": (sustained.get("power") or {}).get("package_w_median") if sustained else None,
                         "power_w_median": power["package_w_median"] if power else None, "power_w_limit": power["package_w_limit"] if power else None,
                         "sclk_mhz_median": power["sclk_mhz_median"] if power else None,
                         "traffic_commit": (traffic_source or {}).get("commit"), "traffic_measured_at": (traffic_source or {}).get("measured_at"),
                         "power": power, "sustained": sustained,
                         "conv_stack": {"achieved": round(achieved, 2), "frac": round(achieved / peak, 4), "launches_per_step": conv_n.value // max(K, 1),
                                        "ms_per_step": round(conv_ms.value / K, 4), "tflops_inside_timed_region": round(conv_flops.value / elapsed / 1e12 / world, 2),
                                        "stem_pool_ms_per_step": round(other_ms.value / K, 4), "by_kernel": kernels},
                         "measured": "HIP events around every conv launch on the launch stream, the same %d steps re-run eagerly on one engine right after the timed regions and %d untimed eager steps (%.4f ms/step with events)" % (K, EAGER_WARM, elapsed_profiled / K * 1e3)},
            "postproc": {"bound": "hbm", "kernels": "pose parsing (NMS + refine, limb scoring + matching, assembly + read-out)" if net == "rtpose" else "box decode + NMS + skeleton read-out",
                         "algorithmic_bytes_per_step": post_bytes, "us_per_step": round(post_ms * 1e3, 2),
                         "achieved": round(post_bytes / (post_ms * 1e-3) / 1e9, 2), "peak": 8000.0, "unit": "GB/s",
                         "frac": round(post_bytes / (post_ms * 1e-3) / 8e12, 5), "pack_us_per_step": round(pack_ms * 1e3, 2), "record_d2h_us_per_step": round(d2h_ms * 1e3, 2),
                         "note": "latency-bound: 32 small frames per step; hidden behind the next batch by the StreamingEngine"},
            "host_enqueue_ms_per_step": {("h2d" if m else "resident"): round(v / K * 1e3, 4) for m, v in host_enqueue_s.items()},
            "frame_stats": {"mean_peaks": round(float(recs['n_peaks' if net == "rtpose" else 'n_candidates'].mean()), 2),
                            "mean_persons": round(float(wire['n_persons' if net == "rtpose" else 'n_det'].mean()), 3),
                            "overflow_frames": int((wire['status'] != 0).sum()),
                            "same_batch_same_records_across_steps_slots_and_input_modes": same},
        })
        if "h2d" in runs:
            out["h2d_inclusive"] = {"value": rate(med["h2d"]), "unit": "frames/s", "ms_per_step": round(med["h2d"] / K * 1e3, 4),
                                    "min": rate(max(runs["h2d"])), "max": rate(min(runs["h2d"])), "runs": [rate(v) for v in runs["h2d"]],
                                    "fraction_of_value": round(elapsed / med["h2d"], 4), "host_link": link,
                                    "posted_ahead": AHEAD,
                                    "what": "same region, every batch handed over from pinned host memory (StreamingEngine.post_host / submit_posted: %.1f MB per step over PCIe on the copy stream into the slot's next input buffer). "
                                            "Streaming form: a batch's transfer is posted %d steps ahead of its step, so the first %d transfers leave before the region opens and the region posts the %d that follow its last step "
                                            "-- K transfers posted and K steps run inside the window, which closes when the last step's records are in pinned host memory; median of %d" % (BATCH * 640 * 480 * 2 / 1e6, AHEAD, AHEAD, AHEAD, REPS)}
    return {"out": out, "engine": engine, "depth_host": depth_host, "se": se, "last_records": last_records, "last_seed": last_seed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "bf16x3"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying one hipGraph per step")
    ap.add_argument("--net", default="rtpose", choices=["rtpose", "yolo"],
                    help="rtpose = rtpose_light3d + PAF parsing (the headline workload); yolo = YoloPoseNet + box decode (SURVEY 8a rows 7, 12)")
    ap.add_argument("--no-h2d", action="store_true", help="skip the PCIe-inclusive passes (inputs handed over from pinned host memory)")
    ap.add_argument("--no-extras", action="store_true", help="skip the fidelity / multi-person legs (profiling runs)")
    ap.add_argument("--no-power", action="store_true", help="skip the untimed power-sampled repetition and the sustained-MFMA probe (child legs, profiling runs)")
    ap.add_argument("--pipeline", type=int, default=3, help="batches in flight per GPU (engines on separate HIP streams)")
    ap.add_argument("--pool", type=int, default=6, help="distinct input batches per slot (pipeline x pool x 19.7 MB should exceed the 256 MB Infinity Cache)")
    ap.add_argument("--reps", type=int, default=5, help="repetitions of the K-step timed region per input mode; the median is reported")
    ap.add_argument("--launcher-dry-run", action="store_true", help="CPU check of the --gpus N self-launch (gloo, no GPU work)")
    ap.add_argument("--force-dist", action="store_true", help="initialise the RCCL process group and run every exchange even at world_size 1 (in a fresh child rank started before any GPU call)")
    ap.add_argument("--workload", default="infer", choices=["infer", "train"], help="infer = the headline path (BASELINE configs[1]); train = the training step (configs[4])")
    ap.add_argument("--full", action="store_true", help="besides the headline region, run every secondary measurement and check: hand-over regions, power / "
                    "sustained-MFMA probe, roofline pass, multi-person and precision-mode legs, CPU baseline, child legs, training step, collective check")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step returned to its caller as DIR/<name>.npy (float32 / float64)")
    args = ap.parse_args()

    env_seen = bench_env()                                          # refuses ablation switches before anything else runs
    from popnet_amd import launch                                   # touches no GPU
    if (args.gpus > 1 or args.force_dist) and not launch.under_torchrun():
        # started from a bare shell: become the parent of N fresh ranks (nothing below this line has run, no HIP call yet)
        sys.exit(launch.relaunch(os.path.abspath(__file__), sys.argv[1:], args.gpus))
    if args.launcher_dry_run:
        return launcher_dry_run(args)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    dist_active = world > 1 or args.force_dist
    if dist_active:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group(backend="nccl", device_id=dev)

    import popnet_amd  # noqa: F401
    from popnet_amd import _lib as _pl
    lab_build = int(_pl.lib().pn_build_experiments())
    if lab_build and not os.environ.get("POPNET_BENCH_ALLOW_LAB_BUILD"):
        raise SystemExit("bench.py: %s is a lab build (-DPN_EXPERIMENTS: environment switches can skip launches); rebuild with python popnet_amd/build.py --force" % _pl.LIB_PATH)
    if args.workload == "train":
        train_workload(args, dev, world, rank, dist)
        if dist is not None:
            dist.destroy_process_group()
        return
    leg_s = {}
    _t = time.perf_counter()
    legs = pipelined_leg(args, dev, world, rank, dist, args.net, args.precision, want_h2d=args.full and not args.no_h2d, dist_active=dist_active)
    leg_s["timed_regions_and_roofline_pass"] = round(time.perf_counter() - _t, 1)
    # collectives: EVERY rank takes part (rank 0 alone would wait for the others forever)
    dist_res = dist_check(dev, world, rank, dist) if dist_active and args.full else None
    plan = plan_legs(world, rank, args.net, args.precision, args.no_extras, args.no_cpu_baseline)
    if not args.full:                                               # a plain run: the headline region and nothing else
        plan = dict.fromkeys(plan, False)
    if rank == 0:
        out = legs["out"]
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {"records": legs["last_records"]})
            out["dump_outputs"] = {"dir": args.dump_outputs, "input_seed": legs["last_seed"],
                                   "what": "records_<field>.npy: the %s records of the last timed step's %d frames" % ("pn_pose_wire" if args.net == "rtpose" else "pn_yolo_frame", BATCH)}
        engine = legs["engine"]
        out["process_group"] = {"initialised": bool(dist_active), "note": "a plain `python bench.py --gpus 1` (how the driver runs N = 1) initialises no process group: same code "
                                "path and value as the default line; under torch.distributed.run (N > 1, or --force-dist) the all-gather of the records closes every region"}
        if dist_res is not None:
            out["dist"] = dist_res
        if plan["extras"]:
            _t = time.perf_counter()
            out["mpaug_parse"] = mpaug_parse_leg(engine)
            out["precision_modes"] = precision_modes_leg(dev)
            leg_s["mpaug_parse_and_precision_modes"] = round(time.perf_counter() - _t, 1)
            # the headline dtype's own fidelity next to `value`: no reader can take the bf16 figure as a within-tolerance one
            fid = out["precision_modes"].get(args.precision, {}).get("vs_fp32_threshold_calibrated_weights")
            sep = out["precision_modes"].get(args.precision, {}).get("vs_fp32_separated_weights")
            if fid is not None:
                out["fidelity"] = {"dtype": args.precision, "vs": "the fp32 engine (the mode that equals the reference's CPU path), 96 frames",
                                   "same_assignment": "%d/%d" % (fid["same_assignment"], fid["frames"]), "d3_m_max": fid["d3_m_max"],
                                   "separated_weights": {"same_assignment": "%d/%d" % (sep["same_assignment"], sep["frames"]), "d3_m_max": sep["d3_m_max"]},
                                   "meets_north_star_tolerance": bool(fid["d3_m_max"] < 1e-3 and fid["same_assignment"] >= fid["frames"] - 2),
                                   "note": "north_star: joints within 1e-3 m, identical person assignment. The mode that meets it at matrix-core rate is `parity_mode` below."}
        cpu_eng_depth = (engine, legs["depth_host"])
        if plan["cpu_baseline"]:
            _t = time.perf_counter()
            out["cpu_baseline"] = cpu_baseline(*cpu_eng_depth)
            leg_s["cpu_baseline"] = round(time.perf_counter() - _t, 1)
    legs = None
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    if plan["children"]:
        # the tolerance-meeting fast mode through the SAME region code, then the secondary network: each
        # as a fresh CHILD process (started, not exec'ed; this process keeps its GPU context and idles) -- in-process a third
        # StreamingEngine's streams share hardware queues with the first one's and its batches stop overlapping
        # (YoloPoseNet: 54 k frames/s as the third in-process leg, 94 k on its own)
        def child_leg(extra, timeout=900):
            # its own session: on a timeout the whole process GROUP goes (under --force-dist the direct child is the
            # torch.distributed.run launcher; its rank must not survive and keep the GPU), and the headline line is printed regardless
            import signal
            import subprocess
            # a freshly started child's first region ran on clocks that had not settled (r05: runs[0] 9 % under the median): >= 30 untimed steps first
            cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(max(args.warmup, 30)), "--reps", str(args.reps),
                   "--pipeline", str(args.pipeline), "--pool", str(args.pool), "--no-extras", "--no-cpu-baseline", "--no-power", "--full"] + extra
            try:
                p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
            except OSError as e:
                return {"error": "child leg could not start: %s" % e}
            try:
                so, se_ = p.communicate(timeout=timeout)
            except subprocess.TimeoutExpired:
                try:
                    os.killpg(p.pid, signal.SIGKILL)
                except OSError:
                    pass
                try:
                    p.communicate(timeout=30)
                except Exception:
                    pass
                return {"error": "child leg timed out after %d s: %s" % (timeout, " ".join(extra))}
            lines = [ln for ln in so.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not lines:
                return {"error": "child leg failed (rc %d): %s" % (p.returncode, se_[-400:])}
            try:
                return json.loads(lines[-1])
            except ValueError as e:
                return {"error": "child leg printed no JSON line: %s" % e}
        _t = time.perf_counter()
        pm = child_leg(["--precision", "bf16x3"] + (["--no-h2d"] if args.no_h2d else []))
        leg_s["parity_mode_child"] = round(time.perf_counter() - _t, 1)
        x3 = out["precision_modes"]["bf16x3"]
        if "error" in pm:
            out["parity_mode"] = pm
        else:
            rf = pm["roofline"]
            out["parity_mode"] = {
                "dtype": "bf16x3", "value": pm["value"], "unit": "frames/s", "ms_per_step": pm["ms_per_step"], "value_stat": pm["value_stat"],
                "h2d_inclusive": pm.get("h2d_inclusive"),
                "roofline": {"bound": "mfma", "kernel": rf["kernel"], "achieved": round(3 * rf["achieved"], 2), "peak": rf["peak"], "unit": "TFLOP/s",
                             "frac": round(3 * rf["achieved"] / rf["peak"], 4), "algorithmic_tflops": rf["achieved"], "avg_launch_us": rf["avg_launch_us"],
                             "what": "physical bf16 MFMA FLOPs = 3 x algorithmic (x_hi W_hi + x_lo W_hi + x_hi W_lo)",
                             "conv_stack_algorithmic_tflops": rf["conv_stack"]["achieved"], "conv_stack_physical_frac": round(3 * rf["conv_stack"]["frac"], 4)},
                "fidelity": {"threshold_calibrated_weights": x3["vs_fp32_threshold_calibrated_weights"], "separated_weights": x3["vs_fp32_separated_weights"]},
                "what": "the same pipelined timed region (hipGraph replay, %d batches in flight, median of %d; its own process) with precision='bf16x3': every tensor as three bf16 planes, fp32-class results" % (args.pipeline, args.reps)}
        _t = time.perf_counter()
        yl = child_leg(["--net", "yolo", "--no-h2d"])
        leg_s["yolo_child"] = round(time.perf_counter() - _t, 1)
        if "error" in yl:
            out["yolo"] = yl
        else:
            out["yolo"] = {"value": yl["value"], "unit": "frames/s", "ms_per_step": yl["ms_per_step"], "value_stat": yl["value_stat"], "dtype": "bf16",
                           "roofline": {k: yl["roofline"][k] for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "avg_launch_us", "launches_per_step")},
                           "conv_stack": {k: yl["roofline"]["conv_stack"][k] for k in ("achieved", "frac", "launches_per_step", "ms_per_step", "by_kernel")},
                           "frame_stats": yl["frame_stats"],
                           "what": "YoloPoseNet forward + box decode / NMS / skeleton read-out (SURVEY 8a rows 7, 12) through the same pipelined region (its own process)"}
        # RCCL on this box: one fresh rank under torch.distributed.run with the process group initialised on
        # backend "nccl" at world_size 1: the region's all-gather plus gather_records / the 22 MB gradient all-reduce on device tensors
        _t = time.perf_counter()
        rc = child_leg(["--force-dist", "--no-h2d", "--steps", "100", "--warmup", "5", "--reps", "2", "--pool", "2"])
        leg_s["rccl_check_child"] = round(time.perf_counter() - _t, 1)
        out["rccl_check"] = rc if "error" in rc else dict(rc.get("dist", {"error": "no dist block in the child's line"}), value_with_process_group=rc["value"])
        if plan["train_step"]:
            _t = time.perf_counter()
            out["train_step"] = train_step_leg(dev, cpu=not args.no_cpu_baseline)
            leg_s["train_step"] = round(time.perf_counter() - _t, 1)
    if rank == 0:
        if args.full:
            surface_in_parsed(out)
        out["leg_seconds"] = leg_s
        out["env"] = dict(env_seen, library="popnet_amd/" + os.path.basename(_pl.LIB_PATH), lab_build=bool(lab_build),
                          GPU_MAX_HW_QUEUES=os.environ.get("GPU_MAX_HW_QUEUES"))
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
