"""The A2J inference nets whose launches the suite compares with fp64, as one table (arrays and numbers only, no GPU).

popnet_amd/csrc/conv_plan.h chooses kernel, cout block and tile of every convolution from max_batch as well as from the map's height and
width, so a (precision, H, W) net is a different set of kernel instances at max_batch 2, 16 and 32.  tests/test_gpu_a2j.py compiles and
compares exactly the rows of CASES; tests/test_a2j_plan_cases.py compiles the same rows without a device and asserts that every convolution
of the nets the engines and scripts compile (DEPLOYED), and every instance the census sizes reach (CENSUS_*), is one that a row compares;
tests/golden/make_golden_net_steps.py records the step list of every row.

  CASES        (id, precision, H, W, B run, max_batch compiled, which steps).  B < max_batch: compiled with POPNET_MAX_BATCH, as
               network/_hipnet.py::_compile honours it.  which: ALL, DIL_OUT (the two dilated steps and the step of the three output
               convolutions) or a tuple of instance keys, DIL_OUT possibly among them: the steps with a convolution of one of those keys.
  instance_key one convolution of pn_net_step_info -> (kernel label, cfg, pitch, wc, wp, nbuf, pt, rpg, lds_two, dil, blocked_acc): the
               kernel instantiation and the launch geometry class it runs in.
"""
KEY_FIELDS = ("kernel", "cfg", "pitch", "wc", "wp", "nbuf", "pt", "rpg", "lds_two")
ALL, DIL_OUT = "all", "dilated+output"


def instance_key(conv):
    return tuple(conv[f] for f in KEY_FIELDS) + (int(conv.get("dil", 1)), int(conv.get("blocked_acc", 0)))


def is_dilated(st):
    return st["type"] == "conv" and any(c.get("dil", 1) != 1 for c in st["convs"])


def is_output(st):
    return st["type"] == "conv" and any(c["w"].endswith(".output") for c in st["convs"])


def selects(which):
    """which -> predicate over one step of pn_net_step_info."""
    if which == ALL:
        return lambda st: True
    parts = (which,) if which == DIL_OUT else tuple(which)
    keys = key_part(which)
    dil_out = DIL_OUT in parts
    return lambda st: (dil_out and (is_dilated(st) or is_output(st))) or (st["type"] == "conv" and any(instance_key(c) in keys for c in st["convs"]))


def key_part(which):
    """The instance keys a row names (none for ALL and DIL_OUT alone)."""
    return set() if which in (ALL, DIL_OUT) else {p for p in which if p != DIL_OUT}


def compared_keys(steps, which):
    """Instance keys of the convolutions in the steps a row compares (check_steps compares every convolution of a selected step)."""
    sel = selects(which)
    return {instance_key(c) for st in steps if st["type"] == "conv" and sel(st) for c in st["convs"]}


def case_id(prec, H, W, B, max_batch):
    return "a2j_%dx%d_b%d%s_%s" % (H, W, B, "of%d" % max_batch if max_batch != B else "", prec)


def _case(prec, H, W, B, max_batch, which):
    return (case_id(prec, H, W, B, max_batch), prec, H, W, B, max_batch, which)


# ---- the configurations tests/test_gpu_a2j.py compared before the deployed plans were added (80 x 96: tests/a2j_cases.py SMALL; 288 x 288: LARGE)
CASES = [
    _case("bf16", 80, 96, 3, 3, ALL),
    _case("fp32", 80, 96, 3, 3, ALL),
    _case("bf16", 288, 288, 2, 2, DIL_OUT),
    # the three keys beside DIL_OUT: the census's additions (below) whose smallest net is one of these
    _case("bf16", 64, 480, 1, 1, (DIL_OUT, ("conv3_kernel<3, 4, 1, 1, 7, 4>", 0, 32, 4, 1, 1, 7, 4, 1, 1, 0))),
    _case("fp32", 64, 480, 1, 1, (DIL_OUT, ("conv_mfma_kernel<0, 1, 2, 120, 0>", 0, 120, 0, 0, 0, 7, 4, 1, 1, 1))),
    _case("bf16", 64, 992, 1, 1, (DIL_OUT, ("conv_mfma_kernel<1, 3, 2, 120, 0>", 0, 120, 0, 0, 0, 7, 4, 1, 1, 0))),
    _case("fp32", 64, 992, 1, 1, DIL_OUT),
]
# ---- the deployed plans: A2JEngine, YoloA2JEngine and scripts/a2j_bench.py compile 288 x 288 at max_batch 32 (16: --batch 16); every step, two crops.
# 288 x 288 stays because the plan is the subject: at 64 x 288 the 8-row conv3 tiles of max_batch 32 are no longer chosen (tiles112 * cout blocks < 1536).
DEPLOYED_CASES = [
    _case("bf16", 288, 288, 2, 32, ALL),
    _case("fp32", 288, 288, 2, 32, ALL),
    _case("bf16", 288, 288, 2, 16, ALL),
    _case("fp32", 288, 288, 2, 16, ALL),
    _case("fp32", 288, 288, 2, 2, ALL),          # compiled and run end to end before; none of its steps was compared
]
CASES += DEPLOYED_CASES

# the nets the engines and scripts compile for themselves: (H, W, max_batch), both precisions (crop 96: YoloA2JEngine in tests/test_gpu_a2j.py)
DEPLOYED = [(288, 288, 32), (288, 288, 16), (288, 288, 2), (96, 96, 2)]
# the census: square crops 32 .. 384 in steps of 16 and the three non-square shapes of CASES, at max_batch 1, 2, 16, 32, both precisions
CENSUS_SIZES = [(s, s) for s in range(32, 385, 16)] + [(80, 96), (64, 480), (64, 992)]
CENSUS_MAX_BATCH = (1, 2, 16, 32)
PRECISIONS = ("bf16", "fp32")

# Kernel labels of the 288 x 288 plans that no test compared before DEPLOYED_CASES (bf16: run by no test of any net; fp32: the first two by no
# test, the rest only on nets without the blocked-accumulation instances).  Each must be among the compared steps of every 288 x 288 row whose
# own step list has it; the max_batch 32 rows have all of their precision's.
NEW_LABELS = {
    "bf16": ("conv3_kernel<1, 2, 2, 1, 7, 4>", "conv_mfma_kernel<1, 1, 2, 120, 0>", "conv_mfma_kernel<1, 1, 1, 64, 0>", "conv_mfma_kernel<1, 3, 1, 64, 0>",
             "conv_mfma_kernel<1, 1, 1, 32, 0>", "conv_mfma_kernel<1, 3, 1, 32, 0>", "conv_mfma_kernel<1, 3, 1, 32, 0, 2>"),
    "fp32": ("conv_mfma_kernel<0, 1, 1, 120, 1>", "conv_mfma_kernel<0, 3, 1, 32, 0, 2>"),
}

# ---- the census's additions (tests/test_a2j_plan_cases.py test b): for every instance key that the census sizes reach and no row above compares,
# the smallest crop and max_batch that produce it, comparing only the steps that carry it
CENSUS_CASES = [
    _case("bf16", 32, 32, 1, 1, (
        ("conv_mfma_kernel<1, 1, 1, 32, 1>", 1, 32, 0, 0, 0, 7, 4, 0, 1, 0),
        ("conv_mfma_kernel<1, 3, 1, 16, 1>", 1, 16, 0, 0, 0, 7, 4, 0, 1, 0),
        ("conv_mfma_kernel<1, 3, 2, 64, 0>", 0, 64, 0, 0, 0, 7, 4, 1, 1, 0))),
    _case("fp32", 32, 32, 1, 1, (
        ("conv_mfma_kernel<0, 1, 2, 64, 0>", 0, 64, 0, 0, 0, 7, 4, 1, 1, 1),
        ("conv_mfma_kernel<0, 3, 1, 16, 1>", 1, 16, 0, 0, 0, 7, 4, 0, 1, 1),
        ("conv_mfma_kernel<0, 3, 2, 64, 0>", 0, 64, 0, 0, 0, 7, 4, 1, 1, 1))),
    _case("bf16", 64, 64, 1, 1, (("conv_mfma_kernel<1, 3, 1, 32, 1>", 1, 32, 0, 0, 0, 7, 4, 0, 1, 0),)),
    _case("bf16", 80, 80, 2, 32, (("conv_mfma_kernel<1, 1, 1, 32, 0>", 0, 32, 0, 0, 0, 7, 4, 0, 1, 0),)),
    _case("bf16", 128, 128, 1, 1, (("conv_mfma_kernel<1, 3, 1, 64, 1>", 1, 64, 0, 0, 0, 7, 4, 0, 1, 0),)),
    _case("fp32", 128, 128, 1, 1, (("conv_mfma_kernel<0, 3, 1, 64, 1>", 1, 64, 0, 0, 0, 7, 4, 0, 1, 1),)),
    _case("bf16", 144, 144, 1, 1, (("conv_mfma_kernel<1, 1, 1, 64, 1>", 1, 64, 0, 0, 0, 7, 4, 0, 1, 0),)),
    _case("fp32", 144, 144, 1, 1, (
        ("conv_mfma_kernel<0, 1, 1, 64, 0>", 0, 64, 0, 0, 0, 7, 4, 0, 1, 1),
        ("conv_mfma_kernel<0, 1, 1, 64, 1>", 1, 64, 0, 0, 0, 7, 4, 0, 1, 1),
        ("conv_mfma_kernel<0, 1, 1, 64, 1>", 1, 64, 0, 0, 0, 7, 4, 1, 1, 1))),
    _case("bf16", 144, 144, 2, 16, (("conv_mfma_kernel<1, 1, 1, 64, 0>", 0, 64, 0, 0, 0, 7, 4, 0, 1, 0),)),
    _case("bf16", 64, 480, 2, 32, (("conv_mfma_kernel<1, 3, 1, 64, 0, 2>", 0, 64, 0, 0, 0, 7, 4, 1, 2, 0),)),
    _case("bf16", 176, 176, 2, 32, (
        ("conv_mfma_kernel<1, 3, 1, 16, 0, 2>", 0, 16, 0, 0, 0, 7, 4, 1, 2, 0),
        ("conv_mfma_kernel<1, 3, 1, 16, 0>", 0, 16, 0, 0, 0, 7, 4, 1, 1, 0))),
    _case("fp32", 192, 192, 1, 1, (("conv_mfma_kernel<0, 3, 1, 64, 4>", 4, 64, 0, 0, 0, 7, 4, 0, 1, 1),)),
    _case("fp32", 208, 208, 1, 1, (("conv_mfma_kernel<0, 3, 1, 32, 0, 2>", 0, 32, 0, 0, 0, 7, 4, 0, 2, 1),)),
    _case("bf16", 64, 992, 2, 32, (("conv_mfma_kernel<1, 3, 1, 120, 0, 2>", 0, 120, 0, 0, 0, 7, 4, 1, 2, 0),)),
]
CASES += CENSUS_CASES

BY_ID = {c[0]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def find(prec, H, W, B, max_batch):
    return BY_ID[case_id(prec, H, W, B, max_batch)]
