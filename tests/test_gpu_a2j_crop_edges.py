"""The A2J crop and vote kernels on seeded sweeps of edge-case boxes (tests/a2j_crop_cases.py), against plain numpy restatements.

What is swept.  Two sets of three 16-value frames, 40 x 30 ("tall": the deployed relation to imgWidth x imgHeight = 30 x 32) and 24 x 34
("wide": the opposite in both axes), 736 + 732 rows: 300 seeded random boxes per set and every class below built on purpose (rows per class,
both sets together, counted by tests/test_a2j_crop_edges.py::test_class_census from the restatement's intermediate values): unpadded inside
228; crossing the left / top / right / bottom side alone 162 / 141 / 157 / 115, all four 33; an end past the image bound but not the frame
bound 65 (x) and 83 (y), past the frame bound but not the image bound 43 and 103; a negative slice end 105 (x) and 96 (y), 44 of them
unpadded and valid; a start past the frame 115 and 114; i == start and j == start met by the strict paste test 52 and 54; an edge exactly at
0, -0.0, img, nextafter(img), size - 1, size 16 to 27 each per axis; int() height or width 0 (the reference raises) and 1, padded and not,
22 to 66 each; float32 y1 - y0 / x1 - x0 truncating apart from float64 16 each; confidence 0.01, its float32 successor, 0 and NaN 16 each
(0: 32); a low confidence in front of NaN coordinates 16; the no-detection row 16; the last frame 478; a paste bounded by the crop's own
size, not by `end`, 53; 215 rows on which the reference raises.  On top, per set, 16 rows with NaN, +-Inf and 1e12 in each coordinate
position (zeros, flag 1 by the project's rule) between the others, and 10 rows whose frame index names no frame.

pn_a2j_crop is compared bit for bit with tests/a2j_crop_reference.py, which equals the reference's own dataPreprocess on every row
(tests/golden/a2j_crop_edges.npz, on the CPU); pn_a2j_train_crop with tests/a2j_traincrop_reference.py::train_crops, which is pinned by the
27 goldens of a2j_traincrop.npz and by tests/test_cv2_warp_kat.py; pn_a2j_vote with the fp64 reference and allowance of
tests/a2j_vote_reference.py, and its map back with a2j_cases.map_back in float32.

Wall time on an MI355X, host references included (each test prints its own, `A2J EDGES ...`): the crop sweep 0.02 to 0.36 s per case (the first
of a set computes the restatement), neighbour independence 0.02 and 0.36 s, the wrong references 0.1 s, the training-crop sweep 0.01 to 0.66 s (788
and 784 records; the first case of a form and set computes the reference), a vote case and a map-back case under 0.05 s; all 37 cases 4.6 s.
"""
import ctypes as C
import functools
import operator
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2j_cases as AC  # noqa: E402
import a2j_crop_cases as CC  # noqa: E402
import a2j_crop_reference as CR  # noqa: E402
import a2j_traincrop_cases as TC  # noqa: E402
import a2j_traincrop_reference as TR  # noqa: E402
from a2j_vote_reference import vote_reference  # noqa: E402
from popnet_amd import _lib, a2j_crops as AJ  # noqa: E402

pytestmark = pytest.mark.gpu
SENT, FLAG_SENT, GUARD = -77.25, 0x5A5A5A5A, 512
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
SETS = pytest.mark.parametrize("name", list(CC.SETS))
f32 = np.float32


def make_cfg(cwh, mean=3.0, std=2.0):
    from popnet_amd.network.a2j import A2JCfg
    cfg = A2JCfg()
    _lib.lib().pn_a2j_cfg_default(C.byref(cfg))
    cfg.img_w, cfg.img_h = CC.IMG_WH
    cfg.crop_w, cfg.crop_h = cwh
    cfg.mean, cfg.std = mean, std
    return cfg


def guarded(gpu, n, fill, dtype):
    """n elements between two guards of GUARD elements, everything filled with a sentinel -> (buffer, pointer to the inner part)"""
    buf = torch.full((GUARD + n + GUARD,), fill, device=gpu, dtype=dtype)
    return buf, C.c_void_p(buf.data_ptr() + GUARD * buf.element_size())


def check_guards(buf, n, fill, what):
    assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), "%s: written outside its %d elements" % (what, n)
    assert not bool((buf[GUARD:GUARD + n] == fill).any()), "%s: an element was never written" % what
    return buf[GUARD:GUARD + n].cpu().numpy()


def crop_call(gpu, frames, rows, cwh):
    """pn_a2j_crop through the C entry, output and flags inside sentinel-filled buffers -> (crops [n, ch, cw], flags [n])"""
    L, ctx = _lib.lib(), _lib.Context.for_device(0)
    n, (cw, ch) = len(rows), cwh
    out, out_p = guarded(gpu, n * ch * cw, SENT, torch.float32)
    fl, fl_p = guarded(gpu, n, FLAG_SENT, torch.int32)
    rows_dev = torch.from_numpy(np.array(rows, dtype=np.float32)).to(gpu)
    cfg = make_cfg(cwh)
    dt = _lib.PN_DEPTH_F16 if frames.dtype == torch.float16 else _lib.PN_DEPTH_F32
    ctx.check(L.pn_a2j_crop(ctx.handle, C.c_void_p(frames.data_ptr()), dt, frames.shape[0], frames.shape[1], frames.shape[2], C.c_void_p(rows_dev.data_ptr()), n,
                            C.byref(cfg), out_p, fl_p, _lib.current_stream_ptr(gpu)), "pn_a2j_crop")
    torch.cuda.synchronize()
    return check_guards(out, n * ch * cw, SENT, "crops").reshape(n, ch, cw), check_guards(fl, n, FLAG_SENT, "flags")


def differing(got, want):
    """rows whose bits differ; where the reference's pixel is NaN the result must be NaN (the payload is not compared)"""
    bad = []
    for k, (a, b) in enumerate(zip(got, want)):
        nan = np.isnan(b)
        if not (np.isnan(a[nan]).all() and np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan])):
            bad.append(k)
    return bad


@functools.lru_cache(None)
def restated(name, cwh, which):
    """The restatement's crops and flags, computed once per (set, crop size, row list) and left unchanged."""
    rows = {"all": lambda: CC.all_rows(name)[0], "large": lambda: CC.rows(name)[CC.large_index(name)], "bad_frame": lambda: CC.bad_frame_rows(name)}[which]()
    crops, flags, infos = CR.crops(CC.frames(name), rows, CC.IMG_WH, cwh)
    for a in (rows, crops, flags):
        a.setflags(write=False)
    return rows, crops, flags, infos


_ENGINES = {}


def engine(gpu, size):
    """One A2JEngine per crop size (its crops need no compiled net); mean / std are set per call."""
    from popnet_amd.pipeline import A2JEngine
    if size not in _ENGINES:
        _ENGINES[size] = A2JEngine(precision="fp32", device=gpu, max_batch=2, crop=(size[1], size[0]), img_wh=CC.IMG_WH)
    _ENGINES[size].cfg.mean, _ENGINES[size].cfg.std = 3.0, 2.0
    return _ENGINES[size]


def device_frames(gpu, name, dtype):
    return torch.from_numpy(CC.frames(name)).to(gpu).to(dtype)


# ---- 1. pn_a2j_crop on every row -----------------------------------------------------------------------------------------------------
@SETS
@DTYPES
def test_crop_kernel_equals_the_restatement_on_every_row(gpu, name, dtype):
    """One launch per crop size: 64 x 48 and the ragged 50 x 37 with every row, the hostile ones between them; 288 x 288 with six.  Crops and
    flags bit for bit, sentinels before and after intact.  Measured on an MI355X: 0.36 s for the first case of a set (the restatement runs), 0.02 to 0.09 s for the others."""
    t0 = time.perf_counter()
    frames = device_frames(gpu, name, dtype)
    _, ia, ib = CC.all_rows(name)
    for cwh, which in [(c, "all") for c in CC.CROPS] + [(CC.LARGE, "large")]:
        rows, want, wflags, _ = restated(name, cwh, which)
        got, flags = crop_call(gpu, frames, rows, cwh)
        bad = differing(got, want)
        assert not bad, "%s %dx%d: %d rows differ, the first: row %d %s, %d pixels" % (name, cwh[0], cwh[1], len(bad), bad[0], rows[bad[0]], int((got[bad[0]] != want[bad[0]]).sum()))
        assert np.array_equal(flags, wflags), (name, cwh, np.nonzero(flags != wflags)[0][:10])
        if which == "all":
            assert len(rows) == len(ia) + len(ib) and flags[ib].all() and not got[ib].any()          # NaN, +-Inf, 1e12: zeros, flag 1
            assert all(not got[k].any() for k in np.nonzero(flags)[0])
    if name == "tall":
        assert sum(1 for c in restated(name, CC.CROPS[0], "all")[1] if np.isnan(c).any()) >= 8 and np.isinf(restated(name, CC.CROPS[0], "all")[1]).any()
    print("\nA2J EDGES crop %s %s: %d rows x 2 sizes + %d at 288, %.2f s" % (name, dtype, len(ia) + len(ib), CC.N_LARGE, time.perf_counter() - t0))


@SETS
def test_a_frame_index_that_names_no_frame_is_a_zero_crop_with_flag_1(gpu, name):
    """The decision of include/popnet_hip.h: frame -1, F, NaN, 1e12 and -0.5, above and below the confidence threshold, give zeros and flag 1
    (the reference loads the frame before it reads the confidence, and has no such frame); the good rows around them keep their bits."""
    frames = device_frames(gpu, name, torch.float16)
    bad_rows = CC.bad_frame_rows(name)
    good, want, wflags, _ = restated(name, CC.CROPS[1], "all")
    pick = np.arange(0, 3 * len(bad_rows), 3)
    rows = np.concatenate([np.stack([good[k], b]) for k, b in zip(pick, bad_rows)] + [good[-1:]])
    got, flags = crop_call(gpu, frames, rows, CC.CROPS[1])
    assert flags[1::2].all() and not got[1::2].any()
    assert not differing(got[0::2], np.concatenate([want[pick], want[-1:]])) and np.array_equal(flags[0::2], np.r_[wflags[pick], wflags[-1:]])
    _, wb, fb, _ = restated(name, CC.CROPS[1], "bad_frame")
    assert fb.all() and not wb.any()                                                                 # the restatement says the same


# ---- 2. neighbour independence ----------------------------------------------------------------------------------------------------------
@SETS
def test_a_rows_crop_does_not_depend_on_its_neighbours(gpu, name):
    """The same rows shuffled, split over two launches, one alone, and a subset through A2JEngine.crops: each row the same bits."""
    t0 = time.perf_counter()
    cwh = CC.CROPS[1]
    frames = device_frames(gpu, name, torch.float16)
    rows, want, wflags, _ = restated(name, cwh, "all")
    base, bflags = crop_call(gpu, frames, rows, cwh)
    assert not differing(base, want)
    perm = np.random.default_rng(CC.SEED + 5).permutation(len(rows))
    got, flags = crop_call(gpu, frames, rows[perm], cwh)
    assert np.array_equal(got.view(np.int32), base[perm].view(np.int32)) and np.array_equal(flags, bflags[perm])
    cut = 301
    for lo, hi in ((0, cut), (cut, len(rows))):
        got, flags = crop_call(gpu, frames, rows[lo:hi], cwh)
        assert np.array_equal(got.view(np.int32), base[lo:hi].view(np.int32)) and np.array_equal(flags, bflags[lo:hi])
    for k in (0, CC.N_RANDOM + 5, len(rows) - 1):
        got, flags = crop_call(gpu, frames, rows[k:k + 1], cwh)
        assert np.array_equal(got.view(np.int32), base[k:k + 1].view(np.int32)) and flags[0] == bflags[k]
    eng = engine(gpu, cwh)
    sub = np.arange(3, len(rows), 7)
    crops, flags = eng.crops(frames, rows[sub])
    torch.cuda.synchronize()
    assert np.array_equal(crops.cpu().numpy()[:, 0].view(np.int32), base[sub].view(np.int32)) and np.array_equal(flags.cpu().numpy(), bflags[sub])
    print("\nA2J EDGES neighbours %s: %.2f s" % (name, time.perf_counter() - t0))


# ---- 3. the comparison can fail ---------------------------------------------------------------------------------------------------------
@SETS
def test_wrong_references_are_rejected(gpu, name):
    """The kernel's crops against two deliberately wrong restatements: `<=` in place of `<` in the paste test, and end = size in place of
    end = size + start (dropping the `end = ...` lines altogether changes no pixel: tests/test_a2j_crop_edges.py shows that the size test
    implies them).  Each reports differing pixels, and only on rows of its class."""
    cwh = CC.CROPS[0]
    frames = device_frames(gpu, name, torch.float16)
    rows, want, wflags, infos = restated(name, cwh, "all")
    got, flags = crop_call(gpu, frames, rows, cwh)
    assert not differing(got, want)
    iw, ih = CC.IMG_WH
    le = CR.crops(CC.frames(name), rows, CC.IMG_WH, cwh, paste=functools.partial(CR.paste_loop, less=operator.le))[0]
    bad = differing(got, le)
    assert len(bad) >= 100 and all(infos[k]["padded"] for k in bad)
    assert all(int((got[k] != le[k]).sum()) > 0 for k in bad)
    # i == start with a negative integer origin is such a row
    eq = [k for k, i in enumerate(infos) if i.get("padded") and not wflags[k] and i["pasted"] > 0 and i["start1"] > 0 and i["start1"] == int(i["start1"]) and i["start1"] < min(i["end1"], i["sh"])]
    assert len(eq) >= 8 and set(eq) <= set(bad)
    ns = CR.crops(CC.frames(name), rows, CC.IMG_WH, cwh, end_rule="no_start")[0]
    bad = differing(got, ns)
    assert len(bad) >= 8 and all((rows[k][1] < 0 and rows[k][3] > iw) or (rows[k][2] < 0 and rows[k][4] > ih) for k in bad)


# ---- 4. pn_a2j_train_crop on a seeded sweep -------------------------------------------------------------------------------------------------
ROT, SCALE_BOX, SCALE_ITOP = (-10, 0, 9), (0.7, 1.0, 1.699), (0.5, 1.0, float(np.nextafter(1.5, 0)))


def _sweep_rows(name):
    """The rows of section 1 that the host accepts: finite coordinates (a2j_crops._finite refuses the others).  Every class of the census
    that does not consist of NaN coordinates is among them: the confidence is not read by the trainers' forms."""
    rows = CC.rows(name)
    return rows[np.isfinite(rows[:, 1:5]).all(1)]


def _hand_draws(scales):
    return [dict(offsets=o, rotate=r, scale=s) for r in ROT for s in scales for o in ((-5, -5, -5, -5), (4, 4, 4, 4), (-5, 4, 4, -5))]


@functools.lru_cache(None)
def train_sweep(form, name, size):
    """-> (records, reference crops, reference flags, mean, std) for one launch: the accepted rows of the set, every second one for each of
    the two small sizes (so each row is used), the draws from the project's own sampler under a seeded np.random, then the hand-made
    extremes on the first rows of the list; 288 x 288: the six large rows with sampler draws."""
    rows = _sweep_rows(name)
    if size == CC.LARGE:
        rows = CC.rows(name)[CC.large_index(name)]
    else:
        rows = rows[CC.CROPS.index(size)::2]
    cw, ch = size
    hand = _hand_draws(SCALE_ITOP if form == "itop" else SCALE_BOX) if size != CC.LARGE else []
    state = np.random.get_state()
    np.random.seed(CC.SEED + len(name) + cw)
    draws = AJ.A2JCropSampler(form, cw, ch).draws(len(rows)) + hand
    np.random.set_state(state)
    extra = np.arange(len(hand)) % 40                       # inside, each side, all four, between the bounds ...: the first deliberate rows
    rows = np.concatenate([rows, CC.rows(name)[CC.N_RANDOM + extra]]) if hand else rows
    n, P = len(rows), 15
    fr = [int(r[0]) for r in rows]
    if form == "box":
        rec, _ = AJ.box_items(list(range(n)), rows[:, 1:5], np.zeros((n, P, 2), f32), np.zeros((n, P, 3), f32), CC.SETS[name], draws=draws, crop_w=cw, crop_h=ch,
                              img_wh=CC.IMG_WH, frames=fr)
        mean, std = 3.0, 2.0
    else:
        depth = np.where(np.arange(n) % 2 == 0, f32(TC.C_HI), f32(TC.C_LO)).astype(f32)
        centres = np.stack([(rows[:, 1] + rows[:, 3]) / 2, (rows[:, 2] + rows[:, 4]) / 2, depth], -1)[:, None, :].astype(f32)
        lt = np.stack([rows[:, 1], rows[:, 2], depth], -1)[:, None, :]
        rb = np.stack([rows[:, 3], rows[:, 4], depth], -1)[:, None, :]
        rec, _ = AJ.itop_items(list(range(n)), centres, lt, rb, np.ones((n, P, 3), f32), CC.SETS[name], draws=draws, crop_w=cw, crop_h=ch, frames=fr)
        mean, std = TC.ITOP_MEAN, TC.ITOP_STD
    want, wflags = TR.train_crops(CC.frames(name), rec, cw, ch, mean, std)
    want.setflags(write=False)
    return rec, want, wflags, mean, std, draws


@pytest.mark.parametrize("form", ["box", "itop"])
@SETS
@DTYPES
def test_train_crop_kernel_equals_its_restatement_on_a_seeded_sweep(gpu, form, name, dtype):
    """pn_a2j_train_crop against tests/a2j_traincrop_reference.py::train_crops (pinned by the 27 goldens of a2j_traincrop.npz and by
    tests/test_cv2_warp_kat.py), bit for bit under the same_bits rule of tests/test_gpu_a2j_traincrop.py, flags equal: per set and form about
    370 records at each small size and 6 at 288 x 288, one launch per crop size."""
    t0 = time.perf_counter()
    frames = device_frames(gpu, name, dtype)
    total = 0
    for size in CC.CROPS + [CC.LARGE]:
        rec, want, wflags, mean, std, draws = train_sweep(form, name, size)
        eng = engine(gpu, size)
        eng.cfg.mean, eng.cfg.std = mean, std
        crops, flags = eng.train_crops(frames, rec)
        torch.cuda.synchronize()
        got = crops.cpu().numpy()[:, 0]
        bad = differing(got, want)
        assert not bad, "%s %s %dx%d: %d records differ, the first: %d, %d pixels" % (form, name, size[0], size[1], len(bad), bad[0], int((got[bad[0]] != want[bad[0]]).sum()))
        assert np.array_equal(flags.cpu().numpy(), wflags)
        total += len(rec)
        if size != CC.LARGE:      # the extremes of every draw are there
            assert {d["rotate"] for d in draws} >= set(ROT) and {d["scale"] for d in draws} >= set(SCALE_ITOP if form == "itop" else SCALE_BOX)
            assert {o for d in draws for o in d["offsets"]} >= {-5, 4} and wflags.sum() >= 8 and (wflags == 0).sum() >= 200
    assert total >= 400
    if form == "itop":      # both window bounds are hit exactly: 3.0 and 2.0 are palette values present in every frame
        assert f32(TC.C_HI) + f32(0.4) == f32(3.0) and f32(TC.C_LO) - f32(0.4) == f32(2.0)
        assert all((CC.frames(name)[k] == 3.0).any() and (CC.frames(name)[k] == 2.0).any() for k in range(CC.N_FRAMES))
    print("\nA2J EDGES train crop %s %s %s: %d records, %.2f s" % (form, name, dtype, total, time.perf_counter() - t0))


# ---- 5. pn_a2j_vote on small maps ---------------------------------------------------------------------------------------------------------
A, P = 16, 15
MAPS = [(1, 1), (1, 2), (2, 3), (4, 4)]                      # K = 16, 32, 96, 256 anchors: K <= 256 threads; 1 .. 16 cells: fewer than the 17 groups
PRECS = [("f32", _lib.PN_PREC_F32), ("bf16", _lib.PN_PREC_BF16), ("bf16x3", _lib.PN_PREC_BF16X3)]


def _pair(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return hi, lo


def head_maps(ref, B, h, w, tail, prec):
    """[B, K, ...] float32 in the reference's order (cells column by column) -> (the NHWC head map pn_a2j_vote reads, the float32 values it
    holds in the reference's order): f32 as it is, bf16 rounded, bf16x3 the [hi | lo] rows, hi + lo exact in float32."""
    lay = lambda t: t.reshape(B, w, h, A * tail).permute(0, 2, 1, 3).contiguous()
    t = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32))
    if prec == _lib.PN_PREC_F32:
        return lay(t), ref.astype(np.float32)
    if prec == _lib.PN_PREC_BF16:
        hi = t.to(torch.bfloat16)
        return lay(hi), hi.float().numpy()
    hi, lo = _pair(ref.astype(np.float32))
    return torch.cat([lay(hi), lay(lo)], -1).contiguous(), (hi.float() + lo.float()).numpy()


def vote_call(gpu, cls, reg, dep, anchors, B, h, w, prec, rows=None, cwh=None):
    """-> votes [B, P, 3]; with rows also the records, both inside sentinel-filled buffers"""
    from popnet_amd.network.a2j import A2J_RECORD_DTYPE
    L, ctx = _lib.lib(), _lib.Context.for_device(0)
    out, out_p = guarded(gpu, B * P * 3, SENT, torch.float32)
    a = torch.from_numpy(anchors.astype(np.float32)).to(gpu)
    dev = [t.to(gpu) for t in (cls, reg, dep)]
    rec = rows_dev = cfg = None
    nrec = B * A2J_RECORD_DTYPE.itemsize // 4
    if rows is not None:
        rec, rec_p = guarded(gpu, nrec, FLAG_SENT, torch.int32)
        rows_dev = torch.from_numpy(np.array(rows, dtype=np.float32)).to(gpu)
        cfg = make_cfg(cwh)
    ctx.check(L.pn_a2j_vote(ctx.handle, *(C.c_void_p(t.data_ptr()) for t in dev), prec, B, h, w, A, P, C.c_void_p(a.data_ptr()), out_p,
                            C.c_void_p(rows_dev.data_ptr()) if rows is not None else None, C.byref(cfg) if rows is not None else None,
                            rec_p if rows is not None else None, _lib.current_stream_ptr(gpu)), "pn_a2j_vote")
    torch.cuda.synchronize()
    votes = check_guards(out, B * P * 3, SENT, "votes").reshape(B, P, 3)
    if rows is None:
        return votes
    return votes, check_guards(rec, nrec, FLAG_SENT, "records").view(A2J_RECORD_DTYPE).reshape(B)


def _anchors(h, w):
    from popnet_amd.network.a2j import generate_anchors, shift
    return shift([h, w], 16, generate_anchors()).astype(np.float32)


@pytest.mark.parametrize("h,w", MAPS, ids=["%dx%d" % m for m in MAPS])
@pytest.mark.parametrize("pname,prec", PRECS, ids=[p[0] for p in PRECS])
def test_vote_on_small_maps_within_fp64_allowance(gpu, pname, prec, h, w):
    """Fewer anchors than the 256 threads of a2j_vote_kernel, fewer cells than the 17 groups of a2j_vote_x3_kernel (idle threads and groups
    bring -inf maxima and empty sums to the reductions).  Crop 0 and 1: seeded heads; crop 2: the logits of joint 4 all equal; crop 3: one
    logit of joint 7 80 above the rest (the max subtraction: exp(80 + c) overflows no float32 only after it).  Reference and allowance:
    tests/a2j_vote_reference.py, on the float32 values the head maps hold."""
    B, K = 4, h * w * A
    assert K <= 256 and h * w < 512 // (A * P // 8)
    rng = np.random.default_rng(CC.SEED + K)
    cls = rng.normal(0, 0.7, (B, K, P)).astype(np.float32)
    cls[2, :, 4] = 0.37
    cls[3, :, 7] = rng.normal(0, 0.5, K)
    cls[3, K // 2, 7] = np.delete(cls[3, :, 7], K // 2).max() + 80
    reg = rng.normal(0, 3, (B, K, P, 2)).astype(np.float32)
    dep = rng.normal(0, 1, (B, K, P)).astype(np.float32)
    (c_dev, c_val), (r_dev, r_val), (d_dev, d_val) = head_maps(cls, B, h, w, P, prec), head_maps(reg, B, h, w, 2 * P, prec), head_maps(dep, B, h, w, P, prec)
    assert np.unique(c_val[2, :, 4]).size == 1 and abs(c_val[3, K // 2, 7] - np.delete(c_val[3, :, 7], K // 2).max() - 80) < 0.5          # bf16 rounds 81 to a quarter
    anchors = _anchors(h, w)
    got = vote_call(gpu, c_dev, r_dev, d_dev, anchors, B, h, w, prec)
    r, allow = vote_reference(c_val, r_val, d_val, anchors)
    ratio = np.abs(got - r) / allow
    print("\nA2J EDGES vote %s %dx%d: worst |gpu - r| / allowance = %.4f" % (pname, h, w, ratio.max()))
    assert np.isfinite(got).all() and ratio.max() <= 1, ratio.max()
    if K > 16:      # the allowance rejects a dropped and a doubled anchor row (crops 0 and 1: spread softmax)
        keep = np.ones(K, bool)
        keep[K // 3] = False
        r2, a2 = vote_reference(c_val[:2, keep], r_val[:2, keep], d_val[:2, keep], anchors[keep])
        assert (np.abs(got[:2] - r2) > a2).any()
        dup = np.r_[np.arange(K), K // 3]
        r2, a2 = vote_reference(c_val[:2, dup], r_val[:2, dup], d_val[:2, dup], anchors[dup])
        assert (np.abs(got[:2] - r2) > a2).any()


@pytest.mark.parametrize("pname,prec", PRECS, ids=[p[0] for p in PRECS])
def test_vote_one_hot_probe_at_a_1x1_map_is_exact(gpu, pname, prec):
    h = w = 1
    B, K = 16, 16
    rng = np.random.default_rng(CC.SEED + 17)
    cls = np.full((B, K, P), -1e4, np.float32)
    hot = lambda b, p: (b + 3 * p) % K
    for b in range(B):
        for p in range(P):
            cls[b, hot(b, p), p] = 0.3 + 0.01 * p
    reg = rng.normal(0, 3, (B, K, P, 2)).astype(np.float32)
    dep = rng.normal(0, 1, (B, K, P)).astype(np.float32)
    (c_dev, _), (r_dev, r_val), (d_dev, d_val) = head_maps(cls, B, h, w, P, prec), head_maps(reg, B, h, w, 2 * P, prec), head_maps(dep, B, h, w, P, prec)
    anchors = _anchors(h, w)
    got = vote_call(gpu, c_dev, r_dev, d_dev, anchors, B, h, w, prec)
    for b in range(B):
        for p in range(P):
            k = hot(b, p)
            want = np.array([anchors[k, 0] + r_val[b, k, p, 0], anchors[k, 1] + r_val[b, k, p, 1], d_val[b, k, p]], np.float32)
            assert np.array_equal(got[b, p].view(np.uint32), want.view(np.uint32)), (b, p, got[b, p], want)


# ---- 6. the map back to the frame ----------------------------------------------------------------------------------------------------------
@SETS
@pytest.mark.parametrize("pname,prec", [PRECS[0], PRECS[2]], ids=["f32", "bf16x3"])
def test_map_back_of_every_row_equals_the_float32_restatement(gpu, name, pname, prec):
    """pn_a2j_vote's records for every row (zero-width, negative-width, no-detection, NaN and infinite rows included) with seeded heads on a
    1 x 2 map: joints bit for bit a2j_cases.map_back of the votes the same launch wrote (NaN where that is NaN), conf and frame copied
    exactly.  f32 heads run vote_finish from a2j_vote_kernel, plane pairs from a2j_vote_x3_kernel."""
    t0 = time.perf_counter()
    h, w = 1, 2
    rows = CC.all_rows(name)[0]
    B, K = len(rows), h * w * A
    rng = np.random.default_rng(CC.SEED + B)
    cls = rng.normal(0, 0.7, (B, K, P)).astype(np.float32)
    reg = rng.normal(0, 20, (B, K, P, 2)).astype(np.float32)
    dep = rng.normal(2, 1, (B, K, P)).astype(np.float32)
    cwh = CC.CROPS[1]
    votes, recs = vote_call(gpu, head_maps(cls, B, h, w, P, prec)[0], head_maps(reg, B, h, w, 2 * P, prec)[0], head_maps(dep, B, h, w, P, prec)[0],
                            _anchors(h, w), B, h, w, prec, rows=rows, cwh=cwh)
    with np.errstate(all="ignore"):
        xy, xyz = AC.map_back(votes, rows, crop_w=cwh[0], crop_h=cwh[1])
    want = np.concatenate([xy, xyz], -1).astype(np.float32)
    bad = differing(recs["joint"], want)
    assert not bad, "%d rows differ, the first: %s" % (len(bad), rows[bad[0]])
    assert np.array_equal(recs["conf"].view(np.uint32), rows[:, 5].view(np.uint32)) and np.array_equal(recs["frame"], rows[:, 0].astype(np.int32))
    assert np.isfinite(votes).all() and np.isnan(want).any() and np.isfinite(want).all(-1).all(-1).sum() > 0.9 * B
    nodet = [k for k, r in enumerate(rows) if np.array_equal(r[1:], f32([-1, -1, -1, -1, 0]))]
    assert len(nodet) >= 8 and all(np.array_equal(recs["joint"][k][:, :2], np.full((P, 2), -1, f32)) for k in nodet)
    print("\nA2J EDGES map back %s %s: %d rows, %.2f s" % (name, pname, B, time.perf_counter() - t0))
