"""GPU: the part-affinity parse kernels (popnet_amd/csrc/parse_paf.hip, parse_unbounded.hip, parse_peaks.hip) on the hand-built edge cases of tests/parse_cases.py,
stage by stage against oracle/parse_paf.py.  Every comparison is an equality: bit-exact agreement is the contract stated at
the top of parse_device.h.

  peaks        peak_x / peak_y / peak_score / peak_type == O.nms row for row -- through peaks_refine_kernel's two instantiations: <MAXP> (batch)
               and the uncapped one (unbounded pass, pn_nms_peaks)
  connections  per limb the count, (i, j) and the float64 score == O.find_connected_joints, in order (limb_match_kernel, limb_unbounded_kernel)
  persons      person_joint / person_count / person_score / joints_2d / joints_3d / part_conf == O.frame_to_records
               (group_readout_kernel, big_group_kernel).  person_score is compared for equality too: the kernels add in the
               oracle's order, (a + b) + c for a new row and row + (b + c) for an extension.

Cases whose census (parse_cases.census) says they overflow a record capacity must carry exactly that overflow bit in the fixed-size
record and are compared in full through the unbounded pass.  The one-row and one-column maps run last, in a test of their own.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import popnet_amd  # noqa: F401
from popnet_amd import _lib
from popnet_amd.utils import paf_to_pose as P2P
from popnet_amd.utils.common import retrieve_depth_heat_weighted_many
from oracle import parse_paf as O

import parse_cases as PC

pytestmark = pytest.mark.gpu

SHAPES = [s for s, cs in PC.shapes().items() if cs[0].name not in PC.LINE_CASES]
TALLY = {"peaks": 0, "connections": 0, "persons": 0, "frames": 0}
_CACHE = {}


def _cfg():
    return P2P.make_parse_cfg(w_org=PC.W_ORG, h_org=PC.H_ORG)


def _dev(cs, gpu):
    """cases of one shape -> NCHW device tensors (heat, paf, z)"""
    return tuple(torch.from_numpy(np.ascontiguousarray(np.stack([getattr(c, k) for c in cs]).transpose(0, 3, 1, 2))).to(gpu)
                 for k in ("heat", "paf", "z"))


def _batch(shape, gpu):
    """the shape's cases as one batch: (records, connection lists per frame), parsed once"""
    if shape not in _CACHE:
        cs = PC.shapes()[shape]
        recs = P2P.parse_paf_batch(*_dev(cs, gpu), _cfg())
        _CACHE[shape] = (recs, [P2P.parse_connections(b, gpu) for b in range(len(cs))])
    return _CACHE[shape]


def _ref_joint_list(ref):
    return np.asarray(ref["rec"]["joint_list"], dtype=np.float64).reshape(-1, 5)


def _check_peaks(name, got, ref):
    want = _ref_joint_list(ref)
    got = np.asarray(got, dtype=np.float64).reshape(-1, 5)
    assert got.shape == want.shape, "%s: %d peaks, oracle %d" % (name, len(got), len(want))
    assert np.array_equal(got, want), "%s: peak rows %s differ" % (name, np.nonzero((got != want).any(axis=1))[0][:8])
    TALLY["peaks"] += len(want)


def _check_connections(name, got, ref):
    for limb in range(PC.L):
        want = np.asarray(ref["connected"][limb], dtype=np.float64).reshape(-1, 5)
        assert len(got[limb]) == len(want), "%s limb %d: %d connections, oracle %d" % (name, limb, len(got[limb]), len(want))
        assert np.array_equal(got[limb][:, :2], want[:, 3:5]), "%s limb %d: connection order / indices differ" % (name, limb)
        assert np.array_equal(got[limb][:, 2], want[:, 2]), "%s limb %d: limb scores differ" % (name, limb)
        TALLY["connections"] += len(want)


def _check_persons(name, assoc, j2, j3, conf, ref):
    want = np.asarray(ref["assoc"], dtype=np.float64).reshape(-1, PC.J + 2)
    assoc = np.asarray(assoc, dtype=np.float64).reshape(-1, PC.J + 2)
    n = len(want)
    assert len(assoc) == n, "%s: %d persons, oracle %d" % (name, len(assoc), n)
    assert np.array_equal(assoc[:, :PC.J], want[:, :PC.J]), "%s: person_joint differs" % name
    assert np.array_equal(assoc[:, -1], want[:, -1]), "%s: person_count differs" % name
    assert np.array_equal(assoc[:, -2], want[:, -2]), "%s: person_score differs by %g" % (name, np.abs(assoc[:, -2] - want[:, -2]).max())
    rec = ref["rec"]
    assert np.array_equal(np.asarray(j2)[:n].reshape(-1, PC.J, 2), np.array(rec["humans_2d"], dtype=np.float64).reshape(-1, PC.J, 2)), "%s: joints_2d" % name
    assert np.array_equal(np.asarray(j3)[:n].reshape(-1, PC.J, 3), np.array(rec["humans_3d"], dtype=np.float64).reshape(-1, PC.J, 3)), "%s: joints_3d" % name
    assert np.array_equal(np.asarray(conf)[:n].reshape(-1, PC.J), np.array(rec["conf"], dtype=np.float64).reshape(-1, PC.J)), "%s: part_conf" % name
    TALLY["persons"] += n


def _check_fixed(c, fr, conns):
    ref, cen = PC.reference(c), PC.census(c)
    want_status = PC.expected_status(cen)
    assert int(fr["status"]) == want_status, "%s: status %d, expected %d" % (c.name, int(fr["status"]), want_status)
    TALLY["frames"] += 1
    if want_status & _lib.PN_FRAME_OVERFLOW_PEAKS:
        # truncation is first-come in reference order: every joint type keeps the oracle's first 32 peaks
        got = P2P.frame_joint_list(fr)
        for j in range(PC.J):
            mine = got[got[:, 4] == j][:, :3]
            assert np.array_equal(mine, np.asarray(ref["peaks"][j])[:_lib.PN_MAX_PEAKS_PER_JOINT, :3]), (c.name, j)
        return
    _check_peaks(c.name, P2P.frame_joint_list(fr), ref)
    _check_connections(c.name, conns, ref)
    if want_status:
        return
    p = int(fr["n_persons"])
    _check_persons(c.name, P2P.frame_assoc(fr).reshape(-1, PC.J + 2), fr["joints_2d"][:p], fr["joints_3d"][:p], fr["part_conf"][:p], ref)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_batch_equals_oracle_stage_by_stage(gpu, shape):
    recs, conns = _batch(shape, gpu)
    for b, c in enumerate(PC.shapes()[shape]):
        _check_fixed(c, recs[b], conns[b])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_alone_in_batch_and_permuted_give_identical_records(gpu, shape):
    cs = PC.shapes()[shape]
    recs, conns = _batch(shape, gpu)
    cfg = _cfg()
    for b, c in enumerate(cs):
        one = P2P.parse_paf_batch(*_dev([c], gpu), cfg)
        assert one[0].tobytes() == recs[b].tobytes(), "%s: the record of the frame alone differs from its record in the batch" % c.name
        alone = P2P.parse_connections(0, gpu)
        for limb in range(PC.L):
            assert np.array_equal(alone[limb], conns[b][limb]), (c.name, limb)
    perm = np.random.default_rng(5).permutation(len(cs))
    got = P2P.parse_paf_batch(*_dev([cs[i] for i in perm], gpu), cfg)
    for k, i in enumerate(perm):
        assert got[k].tobytes() == recs[i].tobytes(), "%s: record differs after a permutation of the batch" % cs[i].name


def _check_unbounded(c, gpu):
    ref = PC.reference(c)
    heat, paf, z = (t[0] for t in _dev([c], gpu))
    r = P2P.parse_paf_unbounded(heat, paf, z, _cfg())
    _check_peaks(c.name + " (unbounded)", r["joint_list"], ref)
    _check_connections(c.name + " (unbounded)", P2P.unbounded_connections(len(_ref_joint_list(ref)), gpu), ref)
    _check_persons(c.name + " (unbounded)", r["person_to_joint_assoc"], r["joints_2d"], r["joints_3d"], r["part_conf"], ref)
    TALLY["frames"] += 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_unbounded_pass_equals_oracle_stage_by_stage(gpu, shape):
    for c in PC.shapes()[shape]:
        _check_unbounded(c, gpu)


def _check_nms(c):
    cfg = SimpleNamespace(MODEL=SimpleNamespace(DOWNSAMPLE=8, NUM_KEYPOINTS=PC.J), TEST=SimpleNamespace(THRESH_HEATMAP=0.1))
    got = P2P.NMS(c.heat.copy(), upsampFactor=8, config=cfg)
    want = PC.reference(c)["peaks"]
    for j in range(PC.J):
        assert got[j].shape == np.asarray(want[j]).shape and np.array_equal(got[j], want[j]), (c.name, j)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_nms_peaks_equals_oracle(gpu, shape):
    for c in PC.shapes()[shape]:
        _check_nms(c)


def test_wire_records_at_16_and_17_persons(gpu):
    """16 kept persons fill the wire record exactly; the 17th sets PN_FRAME_OVERFLOW_PERSONS in the wire record only.  The wire
    records pn_parse_paf_wire writes in the read-out launch equal what pn_pack_pose_frames derives from the frame records."""
    cs = [PC.case("persons16"), PC.case("persons17")]
    heat, paf, z = _dev(cs, gpu)
    cfg, L = _cfg(), _lib.lib()
    ctx = _lib.Context.for_device(gpu.index)
    frames = torch.empty((2, _lib.POSE_FRAME_DTYPE.itemsize), device=gpu, dtype=torch.uint8)
    wire = torch.full((2, _lib.POSE_WIRE_DTYPE.itemsize), 0x5a, device=gpu, dtype=torch.uint8)
    packed = torch.full((2, _lib.POSE_WIRE_DTYPE.itemsize), 0xa5, device=gpu, dtype=torch.uint8)
    vp = lambda t: C.c_void_p(t.data_ptr())
    ctx.check(L.pn_parse_paf_wire(ctx.handle, vp(heat), vp(paf), vp(z), 2, 28, 28, C.byref(cfg), vp(frames), vp(wire), _lib.current_stream_ptr(gpu)), "pn_parse_paf_wire")
    ctx.check(L.pn_pack_pose_frames(ctx.handle, vp(frames), 2, vp(packed), _lib.current_stream_ptr(gpu)), "pn_pack_pose_frames")
    torch.cuda.synchronize()
    assert torch.equal(wire, packed)
    fr = frames.cpu().numpy().view(_lib.POSE_FRAME_DTYPE).reshape(2)
    wr = wire.cpu().numpy().view(_lib.POSE_WIRE_DTYPE).reshape(2)
    assert [int(f["status"]) for f in fr] == [0, 0] and [int(f["n_persons"]) for f in fr] == [16, 17]
    assert [int(x["status"]) for x in wr] == [0, _lib.PN_FRAME_OVERFLOW_PERSONS] and [int(x["n_persons"]) for x in wr] == [16, 17]
    for f, x, c in zip(fr, wr, cs):
        rec = PC.reference(c)["rec"]
        n = _lib.PN_WIRE_MAX_PERSONS
        assert np.array_equal(x["person_joint"], f["person_joint"][:n].astype(np.int16))
        assert np.array_equal(x["vals"][:, :, 0:2], np.array(rec["humans_2d"], dtype=np.float64)[:n].astype(np.float32))
        assert np.array_equal(x["vals"][:, :, 2:5], np.array(rec["humans_3d"], dtype=np.float64)[:n].astype(np.float32))
        assert np.array_equal(x["vals"][:, :, 5], np.array(rec["conf"], dtype=np.float64)[:n].astype(np.float32))


@pytest.mark.parametrize("h,w", [(64, 65), (65, 64)])
def test_maps_above_4096_cells_are_refused_and_nothing_is_written(gpu, h, w):
    """a host check: PN_ERR_UNSUPPORTED from all three entry points, no launch, the output buffers keep their sentinel"""
    PN_ERR_UNSUPPORTED = -4
    L, cfg = _lib.lib(), _cfg()
    ctx = _lib.Context.for_device(gpu.index)
    heat, paf, z = (torch.zeros((1, n, h, w), device=gpu) for n in (16, 28, 15))
    vp = lambda t: C.c_void_p(t.data_ptr())
    frames = torch.full((1, _lib.POSE_FRAME_DTYPE.itemsize), 0x5a, device=gpu, dtype=torch.uint8)
    assert L.pn_parse_paf(ctx.handle, vp(heat), vp(paf), vp(z), 1, h, w, C.byref(cfg), vp(frames), _lib.current_stream_ptr(gpu)) == PN_ERR_UNSUPPORTED
    npk, npers = C.c_int(-7), C.c_int(-7)
    assert L.pn_parse_paf_unbounded(ctx.handle, vp(heat), vp(paf), vp(z), h, w, C.byref(cfg), C.byref(npk), C.byref(npers),
                                    _lib.current_stream_ptr(gpu)) == PN_ERR_UNSUPPORTED
    cnt = torch.full((15,), -7, device=gpu, dtype=torch.int32)
    xs, ys, sc = (torch.full((15, h * w), -7.0, device=gpu) for _ in range(3))
    assert L.pn_nms_peaks(ctx.handle, vp(heat), 15, h, w, 0.1, 8, vp(cnt), vp(xs), vp(ys), vp(sc), _lib.current_stream_ptr(gpu)) == PN_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((frames == 0x5a).all()) and (npk.value, npers.value) == (-7, -7)
    assert bool((cnt == -7).all()) and all(bool((t == -7.0).all()) for t in (xs, ys, sc))
    assert "exceeds 4096 cells" in ctx.last_error()


def test_connection_view_refuses_what_it_cannot_answer(gpu):
    PN_ERR_STATE = -3
    L = _lib.lib()
    buf = [np.zeros(14 * 32, t) for t in (np.int32, np.int32, np.int32, np.float64)]
    args = [a.ctypes.data_as(C.c_void_p) for a in buf]
    fresh = _lib.Context(gpu.index)                      # a private context: no parse has run on it
    assert L.pn_parse_debug_connections(fresh.handle, 0, *args) == PN_ERR_STATE
    assert L.pn_parse_paf_unbounded_connections(fresh.handle, 32, *args) == PN_ERR_STATE
    cs = PC.shapes()[(20, 36)]
    P2P.parse_paf_batch(*_dev(cs, gpu), _cfg())
    ctx = _lib.Context.for_device(gpu.index)
    assert L.pn_parse_debug_connections(ctx.handle, len(cs) - 1, *args) == _lib.PN_OK
    assert L.pn_parse_debug_connections(ctx.handle, len(cs), *args) == PN_ERR_STATE
    assert L.pn_parse_debug_connections(ctx.handle, -1, *args) == PN_ERR_STATE


def test_retrieve_depth_radius_1_to_5_at_corners_edges_and_interior(gpu):
    """windows of 4 .. 121 cells: numpy's sequential sum below 8 cells, its blocked pairwise sum with a tail above (25, 49, 81, 121
    cells in the interior, every clipped size at the borders); negative heat cells are clamped first.  Radius 6 (169 cells) is refused."""
    h, w = 20, 36
    rng = np.random.default_rng(41)
    heat = rng.uniform(-0.3, 1.0, (h, w)).astype(np.float32)
    depth = (rng.standard_normal((h, w)) * 2 + 3).astype(np.float32)
    assert (heat < 0).sum() > 50
    xs, ys = (0, 1, 2, 4, 17, w - 5, w - 3, w - 2, w - 1), (0, 1, 3, 9, h - 4, h - 2, h - 1)
    centres = [(x, y) for y in ys for x in xs]
    sizes = set()
    for radius in (1, 2, 3, 4, 5):
        got = retrieve_depth_heat_weighted_many(centres, depth, heat.copy(), radius=radius)
        want = np.array([O.retrieve_depth_heat_weighted(list(ctr), depth, heat.copy(), radius=radius) for ctr in centres], dtype=np.float32)
        assert got.dtype == np.float32 and np.array_equal(got, want), "radius %d: centres %s differ" % (radius, [centres[i] for i in np.nonzero(got != want)[0][:6]])
        sizes |= {(min(x + radius, w - 1) - max(x - radius, 0) + 1) * (min(y + radius, h - 1) - max(y - radius, 0) + 1) for x, y in centres}
    assert {4, 6, 9, 25, 49, 81, 121} <= sizes
    hm = heat.copy()
    retrieve_depth_heat_weighted_many(centres[:1], depth, hm, radius=1)
    assert hm.min() == 0.0 and np.array_equal(hm, np.maximum(heat, 0))          # clamped in place, like the reference
    with pytest.raises(_lib.PopnetError, match="too large"):
        retrieve_depth_heat_weighted_many(centres, depth, heat.copy(), radius=6)


def test_zz_one_row_and_one_column_maps(gpu):
    """h == 1 and w == 1 (runs after the others).  The index arithmetic of the six kernels was read for these shapes: every
    neighbour access is guarded by y > 0 / y < h - 1 / x > 0 / x < w - 1, patches and read-out windows are clipped to the map, and
    bicubic8 clamps every tap to [0, h - 1] x [0, w - 1]; nothing is read or written out of range."""
    for name in PC.LINE_CASES:
        c = PC.case(name)
        recs = P2P.parse_paf_batch(*_dev([c], gpu), _cfg())
        _check_fixed(c, recs[0], P2P.parse_connections(0, gpu))
        _check_unbounded(c, gpu)
        _check_nms(c)
    print("compared: %(frames)d frame parses, %(peaks)d peaks, %(connections)d connections, %(persons)d persons; mismatches: 0" % TALLY)
