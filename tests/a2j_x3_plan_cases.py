"""The bf16x3 A2J inference nets whose launches tests/test_gpu_a2j_x3.py compares with fp64, as one table (arrays and numbers only, no GPU).

The shape of tests/a2j_plan_cases.py, whose instance_key, selects and compared_keys are used as they are: a row is (id, precision, H, W, B run,
max_batch compiled, which steps), a convolution is identified by its instance key.  A bf16x3 net plans like the bf16 net of the same shape except
that every K loop is three times as long (three plane pairs), which moves some convolutions to another cout block or LDS mode, and that the stem and
the max pool stay two launches: 58 steps where the bf16 net has 57.

  80 x 96, 3 crops                  every step
  288 x 288, 2 crops, max_batch 32  the steps with an instance key that the 80 x 96 net does not launch
  288 x 288, 2 crops, max_batch 2   the steps with an instance key that neither of the two above launches
  64 x 480 / 64 x 992, 1 crop       the two dilated steps (LDS pitch classes 64 and 120) and the step of the three output convolutions

tests/test_a2j_x3_plan_cases.py shows without a device that every convolution of the plans the engines deploy in bf16x3 (DEPLOYED) has the key of a
step that one of these rows compares -- the max_batch 16 plan through the rows beside it.
"""
import a2j_plan_cases as APC

PREC = "bf16x3"
ALL, DIL_OUT = APC.ALL, APC.DIL_OUT


def _case(H, W, B, max_batch, which):
    return (APC.case_id(PREC, H, W, B, max_batch), PREC, H, W, B, max_batch, which)


# instance key: (kernel label, cfg, pitch, wc, wp, nbuf, pt, rpg, lds_two, dil, blocked_acc)
KEYS_288_MAX_BATCH_32 = (
    ("conv3_kernel<1, 2, 2, 1, 7, 4>", 1, 32, 2, 2, 1, 7, 4, 1, 1, 0),
    ("conv3_kernel<3, 2, 2, 1, 7, 4>", 1, 32, 2, 2, 1, 7, 4, 1, 1, 0),
    ("conv_mfma_kernel<1, 1, 2, 120, 0>", 0, 120, 0, 0, 0, 7, 4, 1, 1, 0),
    ("conv_mfma_kernel<1, 3, 2, 120, 0>", 0, 120, 0, 0, 0, 7, 4, 0, 1, 0),
    ("conv_mfma_kernel<1, 1, 1, 64, 0>", 0, 64, 0, 0, 0, 7, 4, 1, 1, 0),
    ("conv_mfma_kernel<1, 3, 1, 64, 0>", 0, 64, 0, 0, 0, 7, 4, 1, 1, 0),
    ("conv_mfma_kernel<1, 1, 1, 32, 0>", 0, 32, 0, 0, 0, 7, 4, 1, 1, 0),
    ("conv_mfma_kernel<1, 3, 1, 32, 1>", 1, 32, 0, 0, 0, 7, 4, 1, 1, 0),
    ("conv_mfma_kernel<1, 3, 1, 32, 0>", 0, 32, 0, 0, 0, 7, 4, 1, 1, 0),
    ("conv_mfma_kernel<1, 3, 1, 32, 0, 2>", 0, 32, 0, 0, 0, 7, 4, 1, 2, 0),
)
KEYS_288_MAX_BATCH_2 = (
    ("conv_mfma_kernel<1, 1, 1, 64, 1>", 1, 64, 0, 0, 0, 7, 4, 1, 1, 0),
    ("conv_mfma_kernel<1, 3, 1, 64, 1>", 1, 64, 0, 0, 0, 7, 4, 1, 1, 0),
    ("conv_mfma_kernel<1, 3, 1, 32, 1, 2>", 1, 32, 0, 0, 0, 7, 4, 1, 2, 0),
)

SMALL = _case(80, 96, 3, 3, ALL)
LARGE_32 = _case(288, 288, 2, 32, KEYS_288_MAX_BATCH_32)
LARGE_2 = _case(288, 288, 2, 2, KEYS_288_MAX_BATCH_2)
WIDE = [_case(64, 480, 1, 1, DIL_OUT), _case(64, 992, 1, 1, DIL_OUT)]
WIDE_PITCH = {480: 64, 992: 120}                      # LDS pitch class of the dilated steps
CASES = [SMALL, LARGE_32, LARGE_2] + WIDE

# the bf16x3 nets the engines and scripts compile for themselves: (H, W, max_batch) -- as tests/a2j_plan_cases.py::DEPLOYED
DEPLOYED = list(APC.DEPLOYED)

BY_ID = {c[0]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def find(H, W, B, max_batch):
    return BY_ID[APC.case_id(PREC, H, W, B, max_batch)]
