"""GPU (-m gpu): bb64_kernel's tile paths against the unfused plan, bit for bit, at the smallest frames that reach each path.

conv2 of the fused BasicBlock hands its fourteen 16-pixel tiles out as three whole tiles per compute wave plus the two
leftover tiles (12, 13) split by cout-tile pairs, and the last two k-steps of each convolution run pixel tile outer so
that a finished tile's epilogue is issued among the next tile's MFMAs.  Which wave owns an accumulator and when its
epilogue is issued are all that may differ from four conv3_kernel launches (POPNET_NO_BBLOCK=1, read when the net is
compiled; those launches are checked against fp64 by tests/test_gpu_layer_shapes.py): same k order, same MFMA, so the
maps must be IDENTICAL.  layer1 maps are H/2 x W/2:

    16 x 16   ->  8 x 8    NOT fused: net.hip fuses a BasicBlock only where the planner gave its convolutions a strip kernel, which it does
                           from 24-column maps on; both plans are the same launches here.  Kept (it must stay equal), asserted to be unfused
    24 x 48   -> 12 x 24   the smallest fused map, in its place: one strip; first row tile nout = 192: both split tiles all padding; second
                           row tile R = 4, nout = 96: whole pixel tiles 6..11 padding too, every epilogue mask active
    56 x 56   -> 28 x 28   Wc = 28: 8-row tiles fill all 14 pixel tiles, both split tiles carry pixels; last row tile R = 4
    24 x 200  -> 12 x 100  four strips of Wc = 25: nout = 200, split tile 12 half valid, 13 all padding; second row tile nout = 100
    24 x 104  -> 12 x 52   Wc = 26: nout = 208, tile 12 full, tile 13 all padding

YoloPoseNet is checked next to the first and the last size.  It takes frames that are multiples of 16 only and its layer1 maps are
H/4 x W/4, so it runs at the frame that gives it the SAME layer1 map through the fused kernel: 48 x 96 (12 x 24) and 48 x 208 (12 x 52).
Every fused comparison asserts that the default plan has BasicBlock steps and the other plan has none, so that it cannot compare a plan
with itself.

The ticket schedule (>= 1 024 tiles) and the POPNET_BB64_HALVES / POPNET_BB64_STATIC switches stay with
tests/test_gpu_parity.py."""
import numpy as np
import pytest
import torch

from helpers import state_dict_from_keys
from popnet_amd import _lib
from test_gpu_layers import _step_info
from test_gpu_parity import _rtpose

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (24, 48), (56, 56), (24, 200), (24, 104)]
UNFUSED = {(16, 16)}                                          # below what net.hip fuses
YOLO_SIZE = {(24, 48): (48, 96), SIZES[-1]: (48, 208)}        # the YoloPoseNet frame with the layer1 map of the first fused and the last size


def _yolo(golden):
    from popnet_amd.network.yolo_posenet import YoloPoseNet
    m = YoloPoseNet(15, input_dim=1).eval()
    m.load_state_dict(state_dict_from_keys(golden.keys["yolo_posenet"], seed=1))
    m.precision = "bf16"
    return m


def _run(m, x):
    """-> (clones of the outputs, number of fused BasicBlock steps in the plan that computed them)"""
    out = m(x)
    out = [t.clone() for t in out[0]] if isinstance(out, tuple) else out.clone()
    h = m._compile(x.device, x.shape[0], x.shape[2], x.shape[3])       # the net the forward has just run
    steps = [_step_info(h, k) for k in range(_lib.lib().pn_net_num_steps(h))]
    return out, sum(st["type"] == "bblock" for st in steps)


@pytest.mark.parametrize("hw", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_bb64_tiles_equal_the_unfused_plan_bit_for_bit(gpu, golden, hw, monkeypatch):
    H, W = hw
    do_yolo = hw in YOLO_SIZE
    rng = np.random.default_rng(64)
    x = torch.from_numpy(rng.normal(0, 1, (2, 1, H, W)).astype(np.float32)).to(gpu)
    xy = torch.from_numpy(rng.normal(0, 1, (2, 1) + YOLO_SIZE[hw]).astype(np.float32)).to(gpu) if do_yolo else None
    got, nbb = _run(_rtpose(golden, "bf16"), x)
    got_y, nbb_y = _run(_yolo(golden), xy) if do_yolo else (None, 1)
    monkeypatch.setenv("POPNET_NO_BBLOCK", "1")          # read when the net is compiled
    ref, nbb_ref = _run(_rtpose(golden, "bf16"), x)
    ref_y, nbb_ref_y = _run(_yolo(golden), xy) if do_yolo else (None, 0)
    monkeypatch.delenv("POPNET_NO_BBLOCK")
    torch.cuda.synchronize()
    if hw in UNFUSED:
        assert nbb == 0 and nbb_ref == 0
    else:                                                # fused against unfused, not a plan against itself
        assert nbb > 0 and nbb_y > 0 and (nbb_ref, nbb_ref_y) == (0, 0), (nbb, nbb_y, nbb_ref, nbb_ref_y)
    for a, b, name in zip(got, ref, ("paf", "heat", "z")):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), name
    if do_yolo:
        assert torch.isfinite(got_y).all() and torch.equal(got_y, ref_y)
