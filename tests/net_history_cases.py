"""The nets whose forward tests/test_gpu_net_history.py runs after a history of other calls, as one table (names and numbers only, no GPU).

A compiled net keeps device state between calls: activation buffers zero-filled once (pad channels, the 2 KiB zero page behind every buffer),
max_batch frame slots of which a smaller batch leaves the upper ones stale, launch descriptors rewritten when the batch size or an output pointer
changes, bb64_kernel's persistent tile tickets.  The GPU file runs sequences of calls on one net per row and compares the last forward, on bits,
with a net that has run nothing else.  This file says which nets; tests/test_net_history_cases.py holds the census that fixes the rows.

  LABEL_ROWS   kernel label -> (network, H, W, precision, environment): for every kernel label that the launch planner gives, at max_batch 4, to a
               convolution launched as planned over the frame grid 8..512 (test_plan_cases.grid_pass((), (4,)); plan_cases.LARGE_BATCH_ONLY
               exempt), the smallest frame that reaches it with the net compiled for max_batch 4 and run at B = 2.  Candidates in three tiers, the
               first that reaches the label decides: plan_cases.SWEEP entries without switches, SWEEP entries with switches, the whole grid.
               Smallest: by H * W, then (H, W), then the order of plan_cases.ALL.
  SWITCH_ROWS  the SWEEP's switch entries, once per switch, with the kernel labels the switch selects at max_batch 4 (labels the same frame does
               not launch without it).
  CASES        the rtpose / yolo rows: every frame of LABEL_ROWS in all the precisions its SWEEP entry lists (a frame from the grid tier: in the
               precision that reaches the label), then SWITCH_ROWS.  (id, network, precision, H, W, environment, max_batch, b, sequences)
  BENCH_CASES  the bench shape, 224 x 224 bf16 compiled for max_batch 32: sequences 1 and 2, as planned and with POPNET_BB64_STRIP set against the
               default of net_run.hip at B = 32 (bb64_launch restates the rule; the census checks which way each net goes).
  A2J_CASES    (id, precision, H, W, max_batch, b, sequences)
"""
import numpy as np

import plan_cases as PC

MAX_BATCH, PROBE_B = 4, 2
ALL_SEQ = (1, 2, 3, 4, 5)

LABEL_ROWS = {
    "conv3_kernel<3, 2, 1, 1, 7, 4>": ("rtpose", 8, 264, "bf16x3", {}),
    "conv3_kernel<3, 2, 2, 1, 7, 4>": ("rtpose", 512, 288, "bf16x3", {}),            # grid tier: no SWEEP frame has 1536 strip tiles at max_batch 4
    "conv3_kernel<3, 4, 1, 1, 7, 4>": ("rtpose", 40, 104, "bf16", {}),
    "conv4_kernel": ("rtpose", 24, 240, "bf16", {"POPNET_CONV4": "1"}),             # by block count first at 448 x 184
    "conv_mfma_kernel<0, 1, 1, 120, 0>": ("rtpose", 8, 264, "fp32", {}),
    "conv_mfma_kernel<0, 1, 1, 32, 0>": ("rtpose", 8, 8, "fp32", {}),
    "conv_mfma_kernel<0, 1, 1, 32, 2>": ("rtpose", 8, 8, "fp32", {}),
    "conv_mfma_kernel<0, 1, 1, 64, 0>": ("rtpose", 8, 264, "fp32", {}),
    "conv_mfma_kernel<0, 1, 1, 64, 2>": ("rtpose", 8, 264, "fp32", {}),
    "conv_mfma_kernel<0, 1, 2, 120, 0>": ("yolo", 48, 272, "fp32", {}),
    "conv_mfma_kernel<0, 1, 2, 64, 0>": ("yolo", 16, 16, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 120, 0>": ("rtpose", 8, 264, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 120, 1>": ("rtpose", 8, 264, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 120, 3>": ("rtpose", 8, 512, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 120, 4>": ("rtpose", 72, 128, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 16, 0>": ("rtpose", 8, 8, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 16, 1>": ("rtpose", 8, 8, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 16, 3>": ("rtpose", 8, 8, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 32, 0>": ("rtpose", 40, 64, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 32, 1>": ("yolo", 32, 96, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 32, 3>": ("rtpose", 24, 232, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 64, 0>": ("rtpose", 8, 264, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 64, 1>": ("rtpose", 8, 264, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 64, 3>": ("rtpose", 8, 264, "fp32", {}),
    "conv_mfma_kernel<0, 3, 1, 64, 4>": ("rtpose", 40, 248, "fp32", {}),
    "conv_mfma_kernel<0, 3, 2, 120, 0>": ("yolo", 48, 256, "fp32", {}),
    "conv_mfma_kernel<0, 3, 2, 64, 0>": ("yolo", 16, 16, "fp32", {}),
    "conv_mfma_kernel<1, 1, 1, 120, 1>": ("rtpose", 8, 264, "bf16", {}),
    "conv_mfma_kernel<1, 1, 1, 32, 1>": ("rtpose", 8, 8, "bf16", {}),
    "conv_mfma_kernel<1, 1, 1, 32, 2>": ("rtpose", 8, 8, "bf16x3", {}),
    "conv_mfma_kernel<1, 1, 1, 64, 1>": ("rtpose", 8, 264, "bf16", {}),
    "conv_mfma_kernel<1, 1, 1, 64, 2>": ("rtpose", 8, 264, "bf16x3", {}),
    "conv_mfma_kernel<1, 3, 1, 120, 1>": ("rtpose", 8, 264, "bf16", {}),
    "conv_mfma_kernel<1, 3, 1, 120, 3>": ("rtpose", 8, 512, "bf16", {}),
    "conv_mfma_kernel<1, 3, 1, 16, 1>": ("rtpose", 8, 8, "bf16", {}),
    "conv_mfma_kernel<1, 3, 1, 16, 3>": ("rtpose", 8, 8, "bf16", {}),
    "conv_mfma_kernel<1, 3, 1, 32, 1>": ("rtpose", 40, 64, "bf16", {}),
    "conv_mfma_kernel<1, 3, 1, 32, 3>": ("rtpose", 24, 232, "bf16", {}),
    "conv_mfma_kernel<1, 3, 1, 64, 1>": ("rtpose", 8, 264, "bf16", {}),
    "conv_mfma_kernel<1, 3, 1, 64, 3>": ("rtpose", 8, 264, "bf16", {}),
    "conv_mfma_kernel<1, 3, 1, 64, 4>": ("rtpose", 136, 248, "bf16", {}),            # grid tier
    "conv_mfma_kernel<1, 3, 2, 120, 0>": ("yolo", 48, 256, "bf16", {}),
    "conv_mfma_kernel<1, 3, 2, 64, 0>": ("yolo", 16, 16, "bf16", {}),
}

# (network, H, W, environment, precisions, labels the switch selects at max_batch 4).  POPNET_CONV3_PT14=1 acts on plans with WP = 2 only, which
# max_batch 4 does not make at 96 x 240: that entry is here for POPNET_NO_BBLOCK=1, which keeps the four layer1 launches of the bf16 net apart.
SWITCH_ROWS = [
    ("rtpose", 32, 88, {"POPNET_CONV3_PT14": "2"}, ("bf16", "bf16x3"), ("conv3_kernel<3, 4, 1, 1, 14, 8>",)),
    ("rtpose", 16, 88, {"POPNET_CONV3_NBUF2": "1"}, ("bf16", "bf16x3"), ("conv3_kernel<3, 4, 1, 2, 7, 4>",)),
    ("rtpose", 24, 56, {"POPNET_CONV3_RPG8": "1"}, ("bf16", "bf16x3"), ("conv3_kernel<3, 4, 1, 1, 7, 8>",)),
    ("rtpose", 24, 240, {"POPNET_CONV4": "1"}, ("bf16", "bf16x3"), ("conv4_kernel",)),
    ("rtpose", 96, 240, {"POPNET_CONV3_PT14": "1", "POPNET_NO_BBLOCK": "1"}, ("bf16",), ("conv3_kernel<3, 2, 1, 1, 7, 4>",)),
]
SWITCHES = ("POPNET_CONV3_PT14", "POPNET_CONV3_NBUF2", "POPNET_CONV3_RPG8", "POPNET_CONV4", "POPNET_NO_BBLOCK")


def _env_id(env):
    return "".join("_" + k[7:].lower() + v for k, v in sorted(env.items()))


def case_id(kind, H, W, prec, env, max_batch=MAX_BATCH, b=PROBE_B):
    return "%s_%dx%d_b%dof%d%s_%s" % ("rt" if kind == "rtpose" else "yolo", H, W, b, max_batch, _env_id(env), prec)


def sweep_entry(kind, H, W, env):
    """The plan_cases.SWEEP entry of a frame under an environment, or None (a frame of the grid tier)."""
    for e in PC.SWEEP:
        if (e[0], e[1], e[2], e[5]) == (kind, H, W, env):
            return e
    return None


def _cases():
    out, seen = [], set()

    def add(kind, H, W, env, precs):
        for p in precs:
            id_ = case_id(kind, H, W, p, env)
            if id_ not in seen:
                seen.add(id_)
                out.append((id_, kind, p, H, W, dict(env), MAX_BATCH, PROBE_B, ALL_SEQ))
    for kind, H, W, prec, env in sorted(LABEL_ROWS.values(), key=lambda r: (r[0], r[1] * r[2], r[1], r[2], sorted(r[4].items()), r[3])):
        e = sweep_entry(kind, H, W, env)
        add(kind, H, W, env, [p for p in PC.ALL if p in e[6]] if e and not env else (prec,))
    for kind, H, W, env, precs, _ in SWITCH_ROWS:
        add(kind, H, W, env, precs)
    return out


CASES = _cases()


def counted(case):
    """The labels the census counts for a row: those LABEL_ROWS sends to it and, for a switch row, the labels the switch selects."""
    _, kind, prec, H, W, env = case[:6]
    out = {l for l, r in LABEL_ROWS.items() if r == (kind, H, W, prec, env)}
    for k, h, w, e, precs, labels in SWITCH_ROWS:
        if (k, h, w, e) == (kind, H, W, env) and prec in precs:
            out |= set(labels)
    return out


# ---- the bench shape -----------------------------------------------------------------------------------------------------------------
BENCH_MAX_BATCH, BENCH_WALK = 32, (32, 5, 32, 2)
NUM_CUS = 256


def bb64_launch(B, H, W, strip_switch, num_cus=NUM_CUS):
    """(strip kernel?, tickets?) of a bf16 BasicBlock(64) step on an H x W map at batch B: net_run.hip::run_forward's rule restated (strip_switch:
    None unset, 0, 1)."""
    segs = (W + 27) // 28
    wt = (W + segs - 1) // segs
    tiles_x = (W + wt - 1) // wt
    T, ncols = (H + 7) // 8, B * tiles_x
    S = max(1, min((num_cus + ncols - 1) // ncols, T // 2))
    strip = T >= 2 and (strip_switch == 1 or (strip_switch is None and T >= 4 * S))
    if strip:
        return True, ncols * S > num_cus
    return False, B * T * tiles_x >= 4 * num_cus


# (id, network, precision, H, W, environment, max_batch, b, sequences); layer1 map: 112 x 112 (rtpose), 56 x 56 (yolo).
# rtpose runs the strip kernel at B = 32 by default, so its second row sets POPNET_BB64_STRIP=0: there bb64_kernel hands tiles out by ticket at
# B = 32 (1792 tiles) and statically at B = 5 and 2.  yolo runs bb64_kernel by default (7 row tiles per column), so its second row sets =1.
BENCH_CASES = [
    ("rt_224_b2of32_bf16", "rtpose", "bf16", 224, 224, {}, BENCH_MAX_BATCH, PROBE_B, (1, 2)),
    ("rt_224_b2of32_bb64_strip0_bf16", "rtpose", "bf16", 224, 224, {"POPNET_BB64_STRIP": "0"}, BENCH_MAX_BATCH, PROBE_B, (1, 2)),
    ("yolo_224_b2of32_bf16", "yolo", "bf16", 224, 224, {}, BENCH_MAX_BATCH, PROBE_B, (1, 2)),
    ("yolo_224_b2of32_bb64_strip1_bf16", "yolo", "bf16", 224, 224, {"POPNET_BB64_STRIP": "1"}, BENCH_MAX_BATCH, PROBE_B, (1, 2)),
]
BENCH_LAYER1 = {"rtpose": (112, 112), "yolo": (56, 56)}

# ---- A2J: (id, precision, H, W, max_batch, b, sequences) --------------------------------------------------------------------------------
A2J_CASES = [
    ("a2j_80x96_b2of3_bf16", "bf16", 80, 96, 3, 2, (1, 2, 3, 4)),
    ("a2j_80x96_b2of3_fp32", "fp32", 80, 96, 3, 2, (1, 2, 3, 4)),
    ("a2j_80x96_b2of3_bf16x3", "bf16x3", 80, 96, 3, 2, (1, 2, 3, 4)),      # a2j_x3_plan_cases.SMALL's shape: the smallest plane-pair row with the dilated steps
    ("a2j_288x288_b2of32_bf16", "bf16", 288, 288, 32, 2, (1,)),           # a2j_plan_cases.DEPLOYED_CASES[0]: the plan the engines deploy
]


def walk(max_batch, b):
    """Sequence 2's batch sizes; the last forward is the probe."""
    return BENCH_WALK if max_batch == BENCH_MAX_BATCH else (max_batch, 1, max_batch - 1, b)


# ---- what the steps of a compiled net (pn_net_step_info) write --------------------------------------------------------------------------
def step_writes(st):
    """[(buffer, first channel, end channel)] one step writes: the stem's 64 channels, a pool's slice, a convolution's [out_coff, out_coff + cout) --
    of its fused tail or fused pool where it has one, since the convolution's own tile then never leaves the CU, as the first convolution's of a
    BasicBlock step."""
    if st["type"] == "stem":
        return [(st["pool_buf"] if st["pool_buf"] >= 0 else st["out_buf"], 0, 64)]
    if st["type"] == "pool":
        return [(st["out_buf"], st["out_coff"], st["out_coff"] + st["C"])]
    out = []
    for c in (st["convs"][1:] if st["type"] == "bblock" else st["convs"]):
        o = c["tail"] if c["tail"] else dict(c["pool"], cout=c["cout"]) if c["pool"] else c
        if o["out_buf"] >= 0:
            out.append((o["out_buf"], o["out_coff"], o["out_coff"] + o["cout"]))
    return out


def written_channels(info, steps):
    """Per activation buffer, which channels some step writes (one plane of a bf16x3 buffer: both planes take the same channels).  The other
    channels are pad channels: zero-filled once."""
    written = [np.zeros(b[2], bool) for b in info["bufs"]]
    for st in steps:
        for buf, c0, c1 in step_writes(st):
            written[buf][c0:c1] = True
    return written


def launched_as_planned(steps):
    """Labels of the plain convolution steps: no fused tail, no fused pool, not a BasicBlock step (test_gpu_layer_shapes._plan_view_matches)."""
    return {st["kernel"] for st in steps if st["type"] == "conv" and not any(c["tail"] or c["pool"] for c in st["convs"])}
