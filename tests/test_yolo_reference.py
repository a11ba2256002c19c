"""The mask-forced form of tests/yolo_reference.py on the CPU (no GPU): forced with an evaluation's own masks and argmaxes it is that
evaluation, and one element forced the other way moves the gradients by more than the strict bar of the GPU comparison
(test_gpu_train_yolo.py::test_engine_gradients_strict_against_mask_forced_fp64) -- so the forcing is live and the bar sees a single flip."""
import numpy as np
import pytest
import torch

import yolo_reference as yr
from helpers import state_dict_from_keys, train_case_inputs

B, H, W = 2, 32, 48


def _case(golden):
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in state_dict_from_keys(golden.keys["yolo_posenet"], seed=0).items()}
    img = train_case_inputs(seed=5, B=B, H=H, W=W)[0]
    batch = [torch.from_numpy(a).double() for a in (img,) + yr.yolo_case_targets(seed=6, B=B, H=H, W=W)]
    return sd, batch


def _worst(a, b):
    return max(float((a[k] - b[k]).norm()) / float(b[k].norm()) for k in b if float(b[k].norm()) > 0)


def test_forced_with_own_masks_is_the_unforced_step(golden):
    sd, batch = _case(golden)
    own = {}
    free = yr.train_step(sd, *batch, dtype=torch.float64, record=own)
    assert len(own) == 1 + 2 + 2 * 7 + 4 + 3
    assert all(v.dtype == torch.bool for k, v in own.items() if k.startswith("bn:"))
    forced = yr.train_step(sd, *batch, dtype=torch.float64, forced=own)
    assert np.allclose(forced["terms"], free["terms"], rtol=1e-14, atol=0)
    assert _worst(forced["grads"], free["grads"]) < 1e-12
    assert _worst(forced["stats"], free["stats"]) < 1e-12


@pytest.mark.parametrize("key", ["bn:model2_3.1", "bn:model0.layer2.1.bn2", "bn:model0.bn1", "mp:stem", "mp:model2_1"])
def test_one_forced_element_moves_the_gradients_past_the_strict_bar(golden, key):
    sd, batch = _case(golden)
    own = {}
    free = yr.train_step(sd, *batch, dtype=torch.float64, record=own)
    forced = {k: v.clone() for k, v in own.items()}
    m = forced[key].view(-1)
    if key == "bn:model0.bn1":
        i = int(own["mp:stem"].view(-1)[0])                             # the stem pool's first window reads it: frame 0, channel 0
        m[i] = ~m[i]
    elif key.startswith("bn:"):
        i = int(torch.nonzero(m).view(-1)[0])                           # a passing element, forced to the other branch
        m[i] = False
    else:
        i = 0
        m[i] = m[i] + 1 if int(m[i]) % W != W - 1 else m[i] - 1      # the neighbouring pixel of the same window row
    got = yr.train_step(sd, *batch, dtype=torch.float64, forced=forced)
    moved = _worst(got["grads"], free["grads"])
    assert moved > 1e-4, (key, moved)
