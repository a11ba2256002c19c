"""GPU: parse_yolo_kernel (popnet_amd/csrc/parse_yolo.hip) on the hand-built edge cases of tests/yolo_cases.py against
oracle/parse_yolo.py.  Every comparison is an equality: bit-exact agreement is the contract stated at the top of parse_yolo.hip.

Per frame: n_det, n_candidates, status; bbox, human, visibility (and vis_pred with pred_vis) of the first 64 survivors ==
oracle.parse_yolo.parse_prior_pose; joints_2d, joints_3d, bbox_org == oracle.parse_yolo.frame_glue of those; every row past
n_det reads as zero.  Each group (one map shape) is parsed as one batch, frame by frame, and permuted, under both
configurations of yolo_cases.CONFIGS (vis_margin 0 without, vis_margin 2 with predicted visibilities); the input tensor is
compared with its copy after every call.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import popnet_amd  # noqa: F401
from popnet_amd import _lib
from popnet_amd.utils.paf_to_pose import make_parse_cfg
from popnet_amd.utils.prior_pose_align import parse_prior_pose, parse_yolo_batch

import yolo_cases as YC

pytestmark = pytest.mark.gpu

KEYS = [g.key for g in YC.groups()]
TALLY = {"frames": 0, "candidates": 0, "survivors": 0, "mismatches": 0}


def _cfg():
    return make_parse_cfg(None, input_size=YC.GLUE_INPUT, w_org=YC.W_ORG, h_org=YC.H_ORG, intrinsics=YC.INTRINSICS)


def _parse(g, maps, gpu, vis_margin, pred_vis):
    """maps: list of raw maps of the group -> (records, vis_pred [B, 64, J] or None); the device tensor must come back unchanged"""
    host = np.stack(maps)
    t = torch.from_numpy(host.copy()).to(gpu)
    vp = torch.full((len(maps), _lib.PN_YOLO_MAX_DET, YC.J), 7.0, device=gpu) if pred_vis else None
    recs = parse_yolo_batch(t, list(g.anchors), YC.J, g.w_out, g.h_out, YC.DEPTH_MEAN, YC.DEPTH_STD, g.conf_thr, g.nms_thr,
                            vis_margin, glue_cfg=_cfg(), vis_pred=vp)
    assert np.array_equal(t.cpu().numpy(), host), "%s: the input map was modified" % g.key
    return recs, (vp.cpu().numpy() if pred_vis else None)


def _check(g, c, fr, vp, vis_margin, pred_vis):
    ref = YC.reference(g, c, vis_margin, pred_vis)
    name = "%s/%s/m%d" % (g.key, c.name, vis_margin)
    n = ref["n_det"]
    assert (int(fr["n_det"]), int(fr["n_candidates"]), int(fr["status"])) == (n, ref["n_candidates"], ref["status"]), name
    for k in ("bbox", "human", "visibility"):
        assert np.array_equal(fr[k][:n], ref[k]), "%s: %s rows %s differ" % (name, k, np.nonzero((fr[k][:n] != ref[k]).reshape(n, -1).any(1))[0][:8])
    if pred_vis:
        assert np.array_equal(vp[:n], ref["vis_pred"]), "%s: vis_pred" % name
        assert not vp[n:].any(), "%s: vis_pred rows past n_det are not zero" % name
    if n:
        gl = YC.glue(ref, g)
        assert np.array_equal(fr["joints_2d"][:n], gl["humans_2d"]), "%s: joints_2d" % name
        assert np.array_equal(fr["joints_3d"][:n], gl["humans_3d"]), "%s: joints_3d" % name
        assert np.array_equal(fr["bbox_org"][:n], gl["bboxes"][:, :4]), "%s: bbox_org" % name
    for k in ("bbox", "human", "visibility", "joints_2d", "joints_3d", "bbox_org"):
        assert not fr[k][n:].any(), "%s: %s rows past n_det are not zero" % (name, k)
    TALLY["frames"] += 1
    TALLY["candidates"] += ref["n_candidates"]
    TALLY["survivors"] += n


@pytest.mark.parametrize("vis_margin,pred_vis", YC.CONFIGS, ids=["m0", "m2_predvis"])
@pytest.mark.parametrize("key", KEYS)
def test_batch_alone_and_permuted_equal_the_oracle(gpu, key, vis_margin, pred_vis):
    g = YC.group(key)
    maps = [YC.case_map(key, c.name, pred_vis) for c in g.cases]
    recs, vp = _parse(g, maps, gpu, vis_margin, pred_vis)
    for b, c in enumerate(g.cases):
        _check(g, c, recs[b], vp[b] if pred_vis else None, vis_margin, pred_vis)
    for b, c in enumerate(g.cases):                                   # every frame alone: the same record, byte for byte
        one, vp1 = _parse(g, [maps[b]], gpu, vis_margin, pred_vis)
        assert one[0].tobytes() == recs[b].tobytes(), "%s/%s: the record of the frame alone differs from its record in the batch" % (key, c.name)
        assert not pred_vis or np.array_equal(vp1[0], vp[b])
    perm = np.random.default_rng(5).permutation(len(maps))
    got, vpp = _parse(g, [maps[i] for i in perm], gpu, vis_margin, pred_vis)
    for k, i in enumerate(perm):
        assert got[k].tobytes() == recs[i].tobytes(), "%s/%s: record differs after a permutation of the batch" % (key, g.cases[i].name)
        assert not pred_vis or np.array_equal(vpp[k], vp[i])
    print("%s m%d: compared so far %d frames, %d candidates, %d survivors; mismatches: %d"
          % ((key, vis_margin) + tuple(TALLY[k] for k in ("frames", "candidates", "survivors", "mismatches"))))


def test_parse_prior_pose_raises_at_65_survivors_and_not_at_64(gpu):
    g = YC.group("2x14x14")
    args = (list(g.anchors), YC.J, g.w_out, g.h_out, YC.DEPTH_MEAN, YC.DEPTH_STD, g.conf_thr, g.nms_thr)
    t64 = torch.from_numpy(YC.case_map(g.key, "survivors64").copy()).to(gpu)
    b, h, v = parse_prior_pose(t64, *args)
    ref = YC.reference(g, next(c for c in g.cases if c.name == "survivors64"), 0, False)
    assert len(b[0]) == 64 and np.array_equal(np.array(b[0]), ref["bbox"]) and np.array_equal(np.array(h[0]), ref["human"])
    assert np.array_equal(np.array(v[0]).astype(np.int32), ref["visibility"])
    t65 = torch.from_numpy(YC.case_map(g.key, "survivors65").copy()).to(gpu)
    with pytest.raises(_lib.PopnetError, match="overflow"):
        parse_prior_pose(t65, *args)


def _raw_call(gpu, A, h, w, anchors, channels=None):
    """pn_parse_yolo / pn_parse_yolo_predvis called directly: (return codes, frames buffer, vis_pred buffer) with sentinels"""
    L = _lib.lib()
    ctx = _lib.Context.for_device(gpu.index)
    pm = torch.zeros((1, channels or A * (5 + 3 * YC.J), h, w), device=gpu)
    frames = torch.full((1, _lib.YOLO_FRAME_DTYPE.itemsize), 0x5a, device=gpu, dtype=torch.uint8)
    vp = torch.full((1, _lib.PN_YOLO_MAX_DET, YC.J), -7.0, device=gpu)
    flat = [float(v) for a in anchors for v in a]
    arr = (C.c_float * len(flat))(*flat)
    args = (ctx.handle, C.c_void_p(pm.data_ptr()), 1, h, w, arr, A, YC.J, 224, 224, 3.0, 2.0, 0.5, 0.5, 0, None, C.c_void_p(frames.data_ptr()))
    rc = (L.pn_parse_yolo(*args, _lib.current_stream_ptr(gpu)),
          L.pn_parse_yolo_predvis(*args, C.c_void_p(vp.data_ptr()), _lib.current_stream_ptr(gpu)))
    torch.cuda.synchronize()
    return rc, frames, vp, ctx


@pytest.mark.parametrize("A,h,w", [(1, 19, 27), (3, 9, 19), (4, 8, 8)], ids=["513_cells", "513_cells_3_anchors", "4_anchors"])
def test_refusals_are_host_checks_and_write_nothing(gpu, A, h, w):
    """A * h * w above 512 and more than three anchors: PN_ERR_UNSUPPORTED from both entry points before any launch, the output
    buffers keep their sentinel, and the Python wrapper raises without returning records"""
    PN_ERR_UNSUPPORTED = -4
    anchors = [(6., 3.), (12., 6.), (3., 9.), (5., 7.)][:A]
    rc, frames, vp, ctx = _raw_call(gpu, A, h, w, anchors)
    assert rc == (PN_ERR_UNSUPPORTED, PN_ERR_UNSUPPORTED)
    assert bool((frames == 0x5a).all()) and bool((vp == -7.0).all())
    assert ("anchors" if A > 3 else "exceed 512") in ctx.last_error()
    got = None
    with pytest.raises(_lib.PopnetError):
        got = parse_yolo_batch(torch.zeros((1, A * (5 + 3 * YC.J), h, w), device=gpu), anchors, YC.J, 224, 224, 3, 2, 0.5, 0.5)
    assert got is None


def test_a_channel_count_that_does_not_match_is_refused(gpu):
    g = YC.group("2x14x14")
    got = None
    for channels, pred_vis in ((2 * (5 + 3 * YC.J) - 1, False), (2 * (5 + 3 * YC.J), True), (2 * (5 + 4 * YC.J), False), (5 + 3 * YC.J, False)):
        pm = torch.zeros((1, channels, 14, 14), device=gpu)
        vp = torch.full((1, _lib.PN_YOLO_MAX_DET, YC.J), -7.0, device=gpu) if pred_vis else None
        with pytest.raises(_lib.PopnetError, match="channels"):
            got = parse_yolo_batch(pm, list(g.anchors), YC.J, 224, 224, 3, 2, 0.5, 0.5, vis_pred=vp)
        assert got is None and (vp is None or bool((vp == -7.0).all()))
