"""MP-3DHP ingest and the result schema: the data formats on either side of the hot path.

Upstream of the path -- what the reference's test-mode dataset does before the network sees a frame
(tpm/lib/datasets/datasets_kdh3d_rtpose_mpreal.py:181-246 (CR line endings), data_augmentation_2d3d.py:76-89,507-522):
    ``labels.json``   {"intrinsics": {fx, fy, cx, cy}, "<frame id>": [ {"2d_joints": [15][2], "3d_joints": [15][3], ...}, ... ]}
                      frame ids (dict order, "intrinsics" skipped) are file names under the image directory, ``.npy`` included;
    ``<id>.npy``      one depth frame [H, W] in metres (float16 on disk for MP-3DHP).
Here only the file read stays on the host: resize + clamp + normalise run in pn_preprocess on the raw frame.

Downstream -- the ``eval_data.json`` dictionary the evaluation scripts write and main_evaluate_mp_human_3D.py reads
(evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py:398-409, evaluation_yolo_posenet_kdh3d_mpreal.py:255-262):
parallel lists indexed by frame: human_pred_set_2d[f][p][15][2], _3d[f][p][15][3], _part_conf[f][p][15]
(+ _visibility, and the ground truth copied from the labels).

Sweeps shard frames over ranks as i -> rank i % world, keep global frame order and -- unlike the
reference's ``drop_last=True`` loader -- never drop the tail unless asked to.
"""
import json
import os

import numpy as np

from . import _lib, profiles
from .config import INTRINSICS, NUM_PARTS


class MP3DHPFrames:
    """Frame list + annotations of one MP-3DHP split (test-mode KDH3D_Keypoints, datasets_kdh3d_rtpose_mpreal.py:181-236)."""

    def __init__(self, img_dir, ann_file):
        self.img_dir = img_dir
        self.anno_dic = json.load(open(ann_file, "r"))
        self.ids = [k for k in self.anno_dic.keys() if k != "intrinsics"]
        self.intrinsics = dict(self.anno_dic.get("intrinsics", INTRINSICS))

    def __len__(self):
        return len(self.ids)

    def load(self, index):
        """Raw frame as stored: float16 / float32 kept (the device kernel widens exactly like the reference's
        ``astype(np.float)``), anything else (float64, integers) narrowed to float32 as Cvt2ndarray does."""
        a = np.load(os.path.join(self.img_dir, self.ids[index]))
        if a.ndim != 2:
            raise _lib.PopnetError("%s: expected one [H, W] depth frame, got shape %s" % (self.ids[index], a.shape))
        return a if a.dtype in (np.float16, np.float32) else a.astype(np.float32)

    def ground_truth(self):
        """(human_gt_set_2d, human_gt_set_3d) in frame order (main_evaluate_mp_human_3D.py:21-41)."""
        g2 = [[p["2d_joints"] for p in self.anno_dic[k]] for k in self.ids]
        g3 = [[p["3d_joints"] for p in self.anno_dic[k]] for k in self.ids]
        return g2, g3

    def batches(self, indices, batch_size, drop_last=False):
        """Yields (index list, host array [b, H, W]); every frame of a batch must have the same shape and dtype."""
        indices = list(indices)
        for s in range(0, len(indices), batch_size):
            chunk = indices[s:s + batch_size]
            if drop_last and len(chunk) < batch_size:
                return
            frames = [self.load(i) for i in chunk]
            if any(f.shape != frames[0].shape or f.dtype != frames[0].dtype for f in frames):
                raise _lib.PopnetError("frames %s..%s differ in shape or dtype" % (self.ids[chunk[0]], self.ids[chunk[-1]]))
            yield chunk, np.stack(frames)


ABLATION_KEYS = ("human_pred_set_3d_read_raw_depth", "human_pred_set_3d_perfect_2d", "human_pred_set_3d_perfect_2d_read_raw_depth",
                 "human_gt_set_2d_visible")


def pose_records_to_lists(recs, overflow=None, ablation=None, profile=None):
    """profile (popnet_amd.profiles, None = MP3DHP): a single-person profile (ITOP) names the lists as evaluation_rtpose_light3d_itop.py:294-298
    does -- human_pred_set_2d, human_pred_set_3d, visibility_pred_set (all parsed persons of a frame, as in that script) -- see
    _itop_pose_lists; the records themselves already carry the profile's read-out, rescale and back-projection (the engine's parse cfg).
    pn_pose_frame records -> the per-frame entries of human_pred_set_{2d,3d,visibility,part_conf} (float64 lists,
    [-1, -1] / Z = -1 for joints a person does not have, exactly what the evaluation script appends).
    overflow: {frame index: result of utils.paf_to_pose.parse_paf_unbounded} for the frames whose record carries an overflow
    status (PoseEngine.predict_lists fills it); without it such a frame raises -- it is never truncated silently.
    ablation: the depth-ablation arms of the same frames (PoseEngine.predict_ablation; evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py:
    197-313) -- {"pred_raw": float64 [F, PN_MAX_PERSONS, 15, 3], "perfect_map" / "perfect_raw": float64 [F, Gmax, 15, 3], "gt_2d": per
    frame the labels' [n_g][15][2], "overflow_raw": {frame index: [P, 15, 3]} for the frames in `overflow`} -- adds ABLATION_KEYS:
    the raw arm follows the predicted persons, the perfect_* arms and human_gt_set_2d_visible the ground-truth persons."""
    prof = profiles.get(profile)
    if prof.single_person:
        if ablation is not None:
            raise _lib.PopnetError("the depth-ablation arms are the MP-3DHP script's; the %s profile has none" % prof.name)
        full = pose_records_to_lists(recs, overflow)
        return {"human_pred_set_2d": full["human_pred_set_2d"], "human_pred_set_3d": full["human_pred_set_3d"],
                "visibility_pred_set": full["human_pred_set_visibility"]}
    out = {"human_pred_set_2d": [], "human_pred_set_3d": [], "human_pred_set_visibility": [], "human_pred_set_part_conf": []}
    if ablation is not None:
        if len(ablation["gt_2d"]) < len(recs) or any(len(ablation[k]) < len(recs) for k in ("pred_raw", "perfect_map", "perfect_raw")):
            raise _lib.PopnetError("ablation arms cover fewer frames than the %d records" % len(recs))
        out.update({k: [] for k in ABLATION_KEYS})
        for i, fr in enumerate(recs):
            g = ablation["gt_2d"][i]
            if len(g) > ablation["perfect_map"].shape[1]:
                raise _lib.PopnetError("frame %d has %d ground-truth persons, the ablation arms carry %d" % (i, len(g), ablation["perfect_map"].shape[1]))
            if int(fr["status"]):
                if i not in ablation.get("overflow_raw", {}):
                    raise _lib.PopnetError("pose record overflow (status=%d) in frame %d: its raw-depth arm needs the second pass -- use "
                                           "PoseEngine.ablation_lists" % (int(fr["status"]), i))
                raw = np.asarray(ablation["overflow_raw"][i], dtype=np.float64)
            else:
                raw = np.asarray(ablation["pred_raw"][i][:int(fr["n_persons"])], dtype=np.float64)
            out["human_pred_set_3d_read_raw_depth"].append(raw.tolist())
            out["human_pred_set_3d_perfect_2d"].append(np.asarray(ablation["perfect_map"][i][:len(g)], dtype=np.float64).tolist())
            out["human_pred_set_3d_perfect_2d_read_raw_depth"].append(np.asarray(ablation["perfect_raw"][i][:len(g)], dtype=np.float64).tolist())
            out["human_gt_set_2d_visible"].append([np.array(h).tolist() for h in g])      # copy.deepcopy(np.array(human_gt)).tolist() (:304-305)
    for i, fr in enumerate(recs):
        if int(fr["status"]):
            if overflow is None or i not in overflow:
                raise _lib.PopnetError("pose record overflow (status=%d): more than %d peaks per joint map or %d persons -- re-parse the frame "
                                       "with utils.paf_to_pose.parse_paf_unbounded / PoseEngine.predict_lists" % (int(fr["status"]), _lib.PN_MAX_PEAKS_PER_JOINT, _lib.PN_MAX_PERSONS))
            r = overflow[i]
            out["human_pred_set_2d"].append(r["joints_2d"].tolist())
            out["human_pred_set_3d"].append(r["joints_3d"].tolist())
            out["human_pred_set_visibility"].append((r["person_joint"] >= 0).astype(int).tolist())
            out["human_pred_set_part_conf"].append(r["part_conf"].tolist())
            continue
        n = int(fr["n_persons"])
        out["human_pred_set_2d"].append(np.asarray(fr["joints_2d"][:n], dtype=np.float64).tolist())
        out["human_pred_set_3d"].append(np.asarray(fr["joints_3d"][:n], dtype=np.float64).tolist())
        out["human_pred_set_visibility"].append((np.asarray(fr["person_joint"][:n]) >= 0).astype(int).tolist())
        out["human_pred_set_part_conf"].append(np.asarray(fr["part_conf"][:n], dtype=np.float64).tolist())
    return out


def yolo_records_to_lists(recs, profile=None):
    """pn_yolo_frame records -> human_pred_set_{2d,3d,part_conf} of evaluation_yolo_posenet_kdh3d_mpreal.py:182-247.
    A single-person profile (ITOP): human_pred_set_{2d,3d} of evaluation_yolo_posenet_itop.py:169-207 -- per frame ONE person, the first
    detection of the record (build the YoloEngine with conf_threshold=0.1 and the profile, as that script parses), or, without a detection,
    the script's placeholder: joints (-1, -1) and depth -1 as float64, rescaled and back-projected like any other value
    (x = -1 / input_size * w_org, X = (x - cx) / f * -1, Y negated)."""
    prof = profiles.get(profile)
    if prof.single_person:
        out = {"human_pred_set_2d": [], "human_pred_set_3d": []}
        for fr in recs:
            # bit 0 (more than PN_YOLO_MAX_DET survivors) truncates first-come in the reference's order: the first person, the only one
            # this script keeps, is exact all the same (an untrained net at conf_threshold 0.1 sets it on every frame)
            if int(fr["status"]) & ~1:
                raise _lib.PopnetError("yolo record overflow (status=%d)" % int(fr["status"]))
            if int(fr["n_det"]) > 0:
                out["human_pred_set_2d"].append([np.asarray(fr["joints_2d"][0]).tolist()])
                out["human_pred_set_3d"].append([np.asarray(fr["joints_3d"][0]).tolist()])
            else:
                j2, j3 = yolo_placeholder_person(prof)
                out["human_pred_set_2d"].append([j2.tolist()])
                out["human_pred_set_3d"].append([j3.tolist()])
        return out
    out = {"human_pred_set_2d": [], "human_pred_set_3d": [], "human_pred_set_part_conf": []}
    for fr in recs:
        if int(fr["status"]):
            raise _lib.PopnetError("yolo record overflow (status=%d)" % int(fr["status"]))
        n = int(fr["n_det"])
        out["human_pred_set_2d"].append(np.asarray(fr["joints_2d"][:n]).tolist())
        out["human_pred_set_3d"].append(np.asarray(fr["joints_3d"][:n]).tolist())
        out["human_pred_set_part_conf"].append(np.repeat(np.asarray(fr["bbox"][:n, 4:5], dtype=np.float64), NUM_PARTS, axis=1).tolist())
    return out


def kdh3d_pose_lists(lists, first_person=False):
    """pose_records_to_lists(...) of the MP-3DHP profile (with or without ablation=) -> the lists of the composed and single-person KDH3D
    scripts (evaluation_rtpose_light3d_kdh3d_mpaug_ablation.py:397-410, ..._kdh3d_ablation.py:400-410): the visibility list is named
    `visibility_pred_set` and there is no part confidence.  first_person: the single-person scripts keep only the first parsed person of a
    frame (..._kdh3d_ablation.py:198-201) -- in the 2D / 3D / visibility lists and in the raw-depth arm that follows the predicted persons;
    the perfect_2d arms follow the ground-truth persons and keep theirs.  A frame without a person stays an empty list."""
    cut = (lambda per_frame: [f[:1] for f in per_frame]) if first_person else (lambda per_frame: per_frame)
    out = {"human_pred_set_2d": cut(lists["human_pred_set_2d"]), "human_pred_set_3d": cut(lists["human_pred_set_3d"]),
           "visibility_pred_set": cut(lists["human_pred_set_visibility"])}
    if "human_pred_set_3d_read_raw_depth" in lists:
        out["human_pred_set_3d_read_raw_depth"] = cut(lists["human_pred_set_3d_read_raw_depth"])
        for k in ABLATION_KEYS[1:]:
            out[k] = lists[k]
    return out


def yolo_kdh3d_lists(recs, first_person=False, profile=None, input_size=224, w_org=None, h_org=None, intrinsics=None):
    """pn_yolo_frame records -> human_pred_set_{2d,3d} of the Yolo-Pose+ scripts of the composed and single-person KDH3D sets.
    first_person=False (evaluation_yolo_posenet_kdh3d_mpaug.py:185-225; engine with conf_threshold=0.5, nms_threshold=0.5): every person of
    a frame.  first_person=True (evaluation_yolo_posenet_kdh3d.py:189-233; engine with conf_threshold=0.1): the first one.  Either way a
    frame without a detection gets the scripts' placeholder person (yolo_placeholder_person), never an empty list.  w_org / h_org /
    intrinsics: the engine's overrides of the profile's, for the placeholder's rescale and back-projection."""
    prof = profiles.get(profile)
    out = {"human_pred_set_2d": [], "human_pred_set_3d": []}
    for fr in recs:
        # bit 0 truncates first-come in the reference's order, so the first person is exact all the same (see yolo_records_to_lists)
        if int(fr["status"]) & (~1 if first_person else ~0):
            raise _lib.PopnetError("yolo record overflow (status=%d)" % int(fr["status"]))
        n = min(int(fr["n_det"]), 1) if first_person else int(fr["n_det"])
        if n > 0:
            out["human_pred_set_2d"].append(np.asarray(fr["joints_2d"][:n]).tolist())
            out["human_pred_set_3d"].append(np.asarray(fr["joints_3d"][:n]).tolist())
        else:
            j2, j3 = yolo_placeholder_person(prof, input_size, w_org, h_org, intrinsics)
            out["human_pred_set_2d"].append([j2.tolist()])
            out["human_pred_set_3d"].append([j3.tolist()])
    return out


def yolo_placeholder_person(profile, input_size=224, w_org=None, h_org=None, intrinsics=None):
    """evaluation_yolo_posenet_itop.py:175-203 for a frame without a detection: np.ones * -1 joints and depths (float64) through the
    script's rescale, pos_3d_from_2d_and_depth (common.py: (x - cx) / fx * Z) and the Y flip -- the profile's negative fy.
    w_org / h_org / intrinsics override the profile's, as the engines' arguments of those names do."""
    prof = profiles.get(profile)
    human = np.ones([NUM_PARTS, 2]) * (-1)
    depth = np.ones(NUM_PARTS) * (-1)
    human[:, 0] = human[:, 0] / input_size * (prof.w_org if w_org is None else w_org)
    human[:, 1] = human[:, 1] / input_size * (prof.h_org if h_org is None else h_org)
    k = prof.intrinsics if intrinsics is None else intrinsics
    X = (human[:, 0] - k["cx"]) / k["fx"] * depth
    Y = (human[:, 1] - k["cy"]) / k["fy"] * depth
    return human, np.stack([X, Y, depth], axis=1)


def run_sweep(engine, frames, batch_size=32, rank=0, world=1, drop_last=False, group=None, ablation=False):
    """Runs `engine` (PoseEngine / YoloEngine) over this rank's shard of `frames` and returns the records of ALL frames
    in global order as a structured numpy array (one all-gather of fixed-size records when world > 1).
    ablation=True (PoseEngine only): also the depth-ablation arms (PoseEngine.predict_ablation against the labels' 2D joints), as fixed-size
    per-frame float64 arrays gathered next to the records -- returns (records, {"pred_raw" [n, PN_MAX_PERSONS, 15, 3], "perfect_map" /
    "perfect_raw" [n, Gmax, 15, 3], "gt_2d"}), Gmax = the split's largest ground-truth person count; eval_data_from_records takes the pair."""
    import torch
    from .pipeline import gather_records, shard_indices
    n = len(frames)
    if drop_last:
        n -= n % (batch_size * world)
    mine = shard_indices(n, rank, world)
    item = engine.frames.shape[1]
    local = torch.empty((len(mine), item), dtype=torch.uint8, device=engine.device)
    if ablation:
        if not hasattr(engine, "predict_ablation"):
            raise _lib.PopnetError("the depth-ablation arms exist for the Open-Pose+ path (PoseEngine) only")
        gt_2d = frames.ground_truth()[0]
        J, P = _lib.PN_NUM_JOINTS, _lib.PN_MAX_PERSONS
        gmax = max([len(g) for g in gt_2d[:n]] + [0])
        rows = P + 2 * gmax                          # per frame: the raw arm's rows, then perfect_map's, then perfect_raw's
        arms = torch.zeros((len(mine), rows, J, 3), dtype=torch.float64, device=engine.device)
    done = 0
    for chunk, host in frames.batches(mine, min(batch_size, engine.max_batch)):
        dev = torch.from_numpy(host).to(engine.device, non_blocking=True)
        if ablation:
            recs, raw, pm, pr = engine.predict_ablation(dev, [gt_2d[i] for i in chunk], gmax)
            local[done:done + len(chunk)].copy_(recs)
            arms[done:done + len(chunk)].copy_(torch.cat([raw, pm, pr], dim=1))
        else:
            local[done:done + len(chunk)].copy_(engine.predict(dev))
        done += len(chunk)
    if ablation:
        arms = arms.reshape(len(mine), rows * J * 3).view(torch.uint8)
        if world > 1:
            arms = gather_records(arms, n, rank, world, group)
        arms = arms.cpu().numpy().view(np.float64).reshape(-1, rows, J, 3)
        arms = {"pred_raw": arms[:, :P], "perfect_map": arms[:, P:P + gmax], "perfect_raw": arms[:, P + gmax:], "gt_2d": gt_2d[:n]}
    if world > 1:
        local = gather_records(local, n, rank, world, group)
    dtype = _lib.POSE_FRAME_DTYPE if item == _lib.POSE_FRAME_DTYPE.itemsize else _lib.YOLO_FRAME_DTYPE
    recs = local.cpu().numpy().view(dtype).reshape(-1)
    return (recs, arms) if ablation else recs


def run_sweep_streaming(se, frames, batch_size=32, rank=0, world=1, drop_last=False, group=None, gather=True, ablation=False):
    """Same result as run_sweep, through a pipeline.StreamingEngine: batch k+1 is read from disk, pinned and copied to
    the device (on its slot's stream) while batches k, k-1 are still being computed; a slot's records are collected right
    before the slot is reused.  gather=False returns this rank's shard only (device uint8 [n_local, item], frames
    rank, rank + world, ...) without touching torch.distributed."""
    import torch
    from .pipeline import gather_records, shard_indices
    if ablation:
        raise _lib.PopnetError("run_sweep_streaming: the depth-ablation arms are not part of the captured streaming step; use run_sweep(..., ablation=True)")
    n = len(frames)
    if drop_last:
        n -= n % (batch_size * world)
    mine = shard_indices(n, rank, world)
    if getattr(se, "wire", False):
        raise _lib.PopnetError("run_sweep_streaming collects the full records: build the StreamingEngine with wire=False")
    item = se.recs[0].shape[1]
    bs = min(batch_size, se.max_batch)
    local = torch.empty((len(mine), item), dtype=torch.uint8, device=se.device)
    pending = {}                                   # slot -> (ticket, offset, count)
    pinned = [None] * se.depth

    def collect(slot):
        t, off, cnt = pending.pop(slot)
        se.wait(t)
        with torch.cuda.stream(se.stream(slot)):
            local[off:off + cnt].copy_(se.records(t)[:cnt], non_blocking=True)

    done = 0
    for chunk, host in frames.batches(mine, bs):
        slot = se._tickets % se.depth
        if slot in pending:
            collect(slot)
        buf = se.input(slot)
        if tuple(host.shape[1:]) != tuple(buf.shape[1:]) or torch.from_numpy(host[:1]).dtype != buf.dtype:
            raise _lib.PopnetError("frames are %s %s, the StreamingEngine was built for %s %s" % (host.shape[1:], host.dtype, tuple(buf.shape[1:]), buf.dtype))
        if pinned[slot] is None:
            pinned[slot] = torch.empty((se.max_batch,) + tuple(host.shape[1:]), dtype=buf.dtype).pin_memory()
        se.stream(slot).synchronize()              # the previous H2D copy out of this pinned buffer has finished
        pinned[slot][:len(chunk)].copy_(torch.from_numpy(host))
        with torch.cuda.stream(se.stream(slot)):
            buf[:len(chunk)].copy_(pinned[slot][:len(chunk)], non_blocking=True)
            if len(chunk) < se.max_batch:
                buf[len(chunk):].zero_()          # a ragged tail batch runs full-size; its surplus records are dropped
        t = se.submit()
        pending[slot] = (t, done, len(chunk))
        done += len(chunk)
    for slot in list(pending):
        collect(slot)
    se.join()
    torch.cuda.synchronize(se.device)
    if not gather:
        return local
    if world > 1:
        local = gather_records(local, n, rank, world, group)
    dtype = _lib.POSE_FRAME_DTYPE if item == _lib.POSE_FRAME_DTYPE.itemsize else _lib.YOLO_FRAME_DTYPE
    return local.cpu().numpy().view(dtype).reshape(-1)


def eval_data_from_records(recs, frames, ablation=None, profile=None):
    """profile: the dataset profile the records were made with (None = MP3DHP); it selects the keys of the profile's evaluation script.
    The eval_data.json dictionary for a finished sweep (predictions from the records, ground truth from the labels).
    ablation: the arms run_sweep(..., ablation=True) returned next to the records -- all ten keys of the reference's ablation script."""
    if ablation is not None and recs.dtype != _lib.POSE_FRAME_DTYPE:
        raise _lib.PopnetError("the depth-ablation arms exist for the Open-Pose+ records only")
    data = (pose_records_to_lists(recs, ablation=ablation, profile=profile) if recs.dtype == _lib.POSE_FRAME_DTYPE
            else yolo_records_to_lists(recs, profile=profile))
    g2, g3 = frames.ground_truth()
    data["human_gt_set_2d"], data["human_gt_set_3d"] = g2[:len(recs)], g3[:len(recs)]
    return data
