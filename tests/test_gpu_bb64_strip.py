"""GPU (-m gpu): bb64s_strip_kernel (POPNET_BB64_STRIP=1) against bb64_kernel (POPNET_BB64_STRIP=0) and against the unfused plan
(POPNET_NO_BBLOCK=1), bit for bit, at the smallest frames that reach each of its paths.

The strip kernel cuts every column (frame x strip of <= 28 output columns) of T = ceil(H / 8) row tiles into S segments -- the
smallest S that gives every CU a segment, at most T / 2 -- and walks a segment top-down: its first tile evaluates conv1 on the whole
10-row intermediate halo as bb64_kernel does, every further tile keeps rows 8, 9 of the tile above as its rows 0, 1 and evaluates
rows 2..9 only.  A carried row is the same sum, in the same k order, from the same MFMA as the recomputed one, so the maps must be
IDENTICAL.  rtpose bf16 at B = 2; layer1 maps are H/2 x W/2:

    32 x 104  -> 16 x 52   two strips of 26; T = 2, S = 1: the shortest carry, one carried tile
    40 x 48   -> 20 x 24   T = 3, tiles of 8, 8, 4 rows: a ragged carried last tile
    80 x 56   -> 40 x 28   T = 5; the batch has 2 columns only, so S = T / 2 = 2: segments of 3 + 2 tiles, the second starts
                           mid-column with the full conv1 path (no zero row above it)
    48 x 200  -> 24 x 100  four strips of 25, every epilogue mask active
    16 x 16   ->  8 x 8    stays unfused

18 frames of 64 x 800 (32 x 400 maps: T = 4, 15 strips) are 270 columns, S = 1: more segments than the device has CUs, so further
segments come through the ticket counter (and, with POPNET_BB64_STRIP=0, 1 080 tiles: bb64_kernel's tile tickets).  That net runs
three times in a row and once as a captured and replayed graph: the counters must be back at zero after every launch.  The same frames
with POPNET_BB64_STRIP=2 (twice as many segments: S = 2, 540 segments of two tiles) give the same maps.

Every fused comparison asserts through pn_net_step_info that the plan has BasicBlock steps and the unfused plan has none, and takes
the segment counts from the step's input buffer rather than assuming them."""
import ctypes as C

import numpy as np
import pytest
import torch

from popnet_amd import _lib
from test_gpu_layers import _step_info
from test_gpu_parity import _rtpose

pytestmark = pytest.mark.gpu

#            frame      (T, columns, S) of the layer1 BasicBlocks at B = 2
CASES = [((32, 104), (2, 4, 1)),
         ((40, 48), (3, 2, 1)),
         ((80, 56), (5, 2, 2)),
         ((48, 200), (3, 8, 1)),
         ((16, 16), None)]


def _segments(h, B, cus, fine=False):
    """[(T, columns, S)] of every BasicBlock step of the compiled net h, by the rule of net_run.hip (fine: POPNET_BB64_STRIP=2, twice the segments)."""
    L = _lib.lib()
    bufs = _step_info(h, -1)["bufs"]
    out = []
    for k in range(L.pn_net_num_steps(h)):
        st = _step_info(h, k)
        if st["type"] != "bblock":
            continue
        H, W = bufs[st["convs"][0]["in_buf"]][:2]
        T, cols = (H + 7) // 8, B * ((W + 27) // 28)
        S = max(1, min((cus + cols - 1) // cols, T // 2))
        out.append((T, cols, max(1, min(2 * S, T // 2)) if fine else S))
    return out


def _run(golden, x, monkeypatch, switch):
    """-> (clones of paf, heat, z; the segments of the plan's BasicBlock steps) with the switch set while the net is compiled"""
    k, v = switch.split("=")
    monkeypatch.setenv(k, v)
    m = _rtpose(golden, "bf16")
    out = [t.clone() for t in m(x)[0]]
    monkeypatch.delenv(k)
    h = m._compile(x.device, x.shape[0], x.shape[2], x.shape[3])
    return out, _segments(h, x.shape[0], torch.cuda.get_device_properties(x.device).multi_processor_count, fine=switch == "POPNET_BB64_STRIP=2")


def _assert_equal(got, ref, what):
    for a, b, name in zip(got, ref, ("paf", "heat", "z")):
        assert torch.isfinite(a).all(), (what, name)
        assert torch.equal(a, b), (what, name)


@pytest.mark.parametrize("hw,segs", CASES, ids=["%dx%d" % c[0] for c in CASES])
def test_strip_kernel_equals_bb64_kernel_and_the_unfused_plan(gpu, golden, hw, segs, monkeypatch):
    x = torch.from_numpy(np.random.default_rng(65).normal(0, 1, (2, 1) + hw).astype(np.float32)).to(gpu)
    strip, seg_strip = _run(golden, x, monkeypatch, "POPNET_BB64_STRIP=1")
    tiles, seg_tiles = _run(golden, x, monkeypatch, "POPNET_BB64_STRIP=0")
    unfused, seg_unfused = _run(golden, x, monkeypatch, "POPNET_NO_BBLOCK=1")
    torch.cuda.synchronize()
    if segs is None:
        assert seg_strip == [] and seg_tiles == [] and seg_unfused == []
    else:                                                # fused against unfused, not a plan against itself
        assert seg_strip and seg_strip == seg_tiles and seg_unfused == []
        assert all(s == segs for s in seg_strip), seg_strip
    _assert_equal(strip, tiles, "POPNET_BB64_STRIP=0")
    _assert_equal(strip, unfused, "POPNET_NO_BBLOCK=1")


def test_strip_segment_tickets_are_left_at_zero_for_the_next_launch(gpu, golden, monkeypatch):
    B, hw = 18, (64, 800)
    x = torch.from_numpy(np.random.default_rng(66).normal(0, 1, (B, 1) + hw).astype(np.float32)).to(gpu)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    tiles, _ = _run(golden, x, monkeypatch, "POPNET_BB64_STRIP=0")
    unfused, seg_unfused = _run(golden, x, monkeypatch, "POPNET_NO_BBLOCK=1")
    monkeypatch.setenv("POPNET_BB64_STRIP", "1")
    m = _rtpose(golden, "bf16")
    first = [t.clone() for t in m(x)[0]]
    monkeypatch.delenv("POPNET_BB64_STRIP")
    h = m._compile(gpu, B, *hw)
    segs = _segments(h, B, cus)
    assert segs and seg_unfused == []
    for T, cols, S in segs:                              # more segments than workgroups: the ticket path
        assert T >= 2 and cols * S > cus, (segs, cus)
    _assert_equal(first, tiles, "POPNET_BB64_STRIP=0")
    _assert_equal(first, unfused, "POPNET_NO_BBLOCK=1")
    fine, seg_fine = _run(golden, x, monkeypatch, "POPNET_BB64_STRIP=2")
    assert [(T, cols, 2 * S) for T, cols, S in segs] == seg_fine, (segs, seg_fine)
    _assert_equal(fine, first, "POPNET_BB64_STRIP=2")
    for _ in range(2):                                   # three launches in a row
        _assert_equal([t.clone() for t in m(x)[0]], first, "eager again")
    # once as a graph, into buffers of its own (the descriptors are written by the eager launch before the capture)
    outs = [torch.zeros_like(t) for t in first]

    def body():
        m._ctx.check(_lib.lib().pn_rtpose_forward(h, C.c_void_p(x.data_ptr()), B, C.c_void_p(outs[0].data_ptr()), C.c_void_p(outs[1].data_ptr()),
                                                  C.c_void_p(outs[2].data_ptr()), _lib.current_stream_ptr(gpu)), "pn_rtpose_forward")

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    _assert_equal(outs, first, "eager into the graph's buffers")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        body()
    for _ in range(2):
        for t in outs:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        _assert_equal(outs, first, "graph replay")
    _assert_equal([t.clone() for t in m(x)[0]], first, "eager after the replays")
