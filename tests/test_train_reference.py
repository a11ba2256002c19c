"""tests/train_reference.py on the CPU (no GPU): unforced it is oracle/train.py's step; forced with an evaluation's own masks it is that
evaluation; one element forced the other way moves the gradients by more than the strict bar of the GPU comparison
(test_gpu_train.py::test_planes_engine_gradients_strict_against_mask_forced_fp64) -- so the forcing is live and the bar sees a single flip."""
import numpy as np
import pytest
import torch

import train_reference as tr
from helpers import init_like_state_dict, train_case_inputs

B, H, W = 2, 32, 48


def _case(golden):
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in init_like_state_dict(golden.keys["rtpose_light3d"], seed=3).items()}
    batch = [torch.from_numpy(a).double() for a in train_case_inputs(seed=5, B=B, H=H, W=W)]
    return sd, batch


def _worst(a, b):
    floor = 1e-6 * max(float(g.norm()) / np.sqrt(g.numel()) for g in b.values())          # test_gpu_train.py::_floor
    return max(float((a[k] - b[k]).norm()) / float(b[k].norm()) for k in b if float(b[k].norm()) > 100 * floor * np.sqrt(b[k].numel()))


def test_unforced_step_is_the_oracle_step(golden):
    from oracle import train as otrain
    sd, batch = _case(golden)
    mine = tr.train_step(sd, *batch, dtype=torch.float64)
    ref = otrain.train_step(sd, *batch, apply=False, dtype=torch.float64)
    assert np.allclose(mine["terms"], ref["terms"], rtol=1e-13, atol=0)
    assert set(mine["grads"]) == set(ref["grads"])
    assert _worst(mine["grads"], ref["grads"]) < 1e-11
    for k, v in mine["stats"].items():
        assert torch.allclose(v, ref["new_sd"][k], rtol=1e-13, atol=1e-15), k


def test_forced_with_own_masks_is_the_unforced_step(golden):
    sd, batch = _case(golden)
    own = {}
    free = tr.train_step(sd, *batch, dtype=torch.float64, record=own)
    assert list(own) == tr.mask_keys() and len(own) == 1 + 6 + 1 + 24
    assert all(v.dtype == torch.bool for v in own.values())
    forced = tr.train_step(sd, *batch, dtype=torch.float64, forced=own)
    assert np.allclose(forced["terms"], free["terms"], rtol=1e-14, atol=0)
    assert _worst(forced["grads"], free["grads"]) < 1e-12
    assert _worst(forced["stats"], free["stats"]) < 1e-12


@pytest.mark.parametrize("key", ["bn:model0.bn1", "bn:model0.layer1.1.bn2", "bn:model0.layer2.0.bn1", "bn:model0.bn2", "bn:model1_2.4", "bn:model2_1.10", "bn:model2_3.1"])
def test_one_forced_element_moves_the_gradients_past_the_strict_bar(golden, key):
    sd, batch = _case(golden)
    own = {}
    free = tr.train_step(sd, *batch, dtype=torch.float64, record=own)
    forced = {k: v.clone() for k, v in own.items()}
    m = forced[key].view(-1)
    i = int(torch.nonzero(m).view(-1)[m.sum() // 2])                   # a passing element, forced to the other branch
    m[i] = False
    got = tr.train_step(sd, *batch, dtype=torch.float64, forced=forced)
    moved = _worst(got["grads"], free["grads"])
    assert moved > 1e-4, (key, moved)
