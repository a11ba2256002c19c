"""Batched end-to-end engine: raw depth frames in, fixed-size pose records out, all on one GPU
stream with no host round trip in between.

    depth [B,H,W] f16/f32 (HBM) --pn_preprocess--> x [B,1,S,S] f32
        --pn_rtpose_forward--> paf / heat / z (f32 NCHW, 185 KB per frame)
        --pn_parse_paf--> pn_pose_frame[B]

This is the per-batch body of the reference's evaluation loop
(tpm/evaluate/evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py:161-316) minus Python.
Multi-GPU: frames are independent, so ranks take disjoint frame shards, there is no
collective on the data path, and ONE all-gather of the fixed-size records (RCCL over xGMI via
torch.distributed, backend "nccl") assembles the result in global frame order.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, profiles, synth
from .config import DEPTH_MAX, DEPTH_MEAN, DEPTH_STD, INTRINSICS, default_cfg
from .network._hipnet import _PREC
from .network.rtpose_light3d import rtpose_light3d
from .utils.paf_to_pose import make_parse_cfg


class PoseEngine:
    def __init__(self, precision="bf16", state_dict=None, device=None, max_batch=32, input_size=224,
                 w_org=None, h_org=None, intrinsics=None, weight_seed=0, private_ctx=False, calib_gain=1.0, parse_config=None, profile=None):
        """profile: the dataset profile (popnet_amd.profiles; None = MP3DHP) -- the depth clamp and normalisation of the pre-processing, the
        frame size, intrinsics and joint depth read-out of the parse; w_org / h_org / intrinsics override the profile's.
        private_ctx: give this engine its own pn_ctx (parse workspace), so that several engines can
        run concurrently on different HIP streams (bench.py pipelines consecutive batches that way).
        parse_config: a reference-style config namespace (TEST.THRESH_HEATMAP, TEST.THRESH_PAF, TEST.NUM_INTERMED_PTS_BETWEEN_KEYPOINTS,
        MODEL.DOWNSAMPLE, MODEL.NUM_KEYPOINTS) for the parse in place of default_cfg(); None = the defaults and the kernels built for them.
        Any other supported MODEL.DOWNSAMPLE (1, 2, 4, 8, 16) or number of sample points (2..32) runs the generic parse kernels.
        calib_gain: synthetic weights only -- logit gain of the heat head before calibrate_heads (1 = heat values crowd
        the detection threshold, the worst case for a reduced-precision forward; > 1 = peaks comfortably separated)."""
        if not torch.cuda.is_available():
            raise _lib.PopnetError("PoseEngine needs a GPU: the HIP path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_batch, self.S = int(max_batch), int(input_size)
        self.profile = profiles.get(profile)
        self.model = rtpose_light3d(15, 14, 2, input_dim=1).eval()
        if state_dict is None:
            synth.load_synth_weights(self.model, seed=weight_seed)
            calibrate_heads(self.model, self.device, gain=calib_gain)
        else:
            self.model.load_state_dict(state_dict)
        self.model.precision = precision
        self.ctx = _lib.Context(self.device.index) if private_ctx else _lib.Context.for_device(self.device.index)
        self.L = _lib.lib()
        self.cfg = make_parse_cfg(default_cfg() if parse_config is None else parse_config, input_size=self.S, w_org=w_org, h_org=h_org,
                                  intrinsics=intrinsics, profile=self.profile)
        # a PRIVATE context's parse scratch is sized once for max_batch and never moves again (a captured graph keeps the
        # pointer).  The shared per-device context keeps growing on demand: fixing it here would make an unrelated later
        # call with a larger batch (utils.paf_to_pose.parse_paf_batch) fail depending on construction order
        self.private_ctx = bool(private_ctx)
        if self.private_ctx:
            self.ctx.check(self.L.pn_parse_reserve(self.ctx.handle, self.max_batch), "pn_parse_reserve")
        self._locked = False
        self._locked_net = None
        h = self.S // 8
        d, f32 = self.device, torch.float32
        self.x = torch.empty((self.max_batch, 1, self.S, self.S), device=d, dtype=f32)
        self.paf = torch.empty((self.max_batch, 28, h, h), device=d, dtype=f32)
        self.heat = torch.empty((self.max_batch, 16, h, h), device=d, dtype=f32)
        self.z = torch.empty((self.max_batch, 15, h, h), device=d, dtype=f32)
        self.frames = torch.empty((self.max_batch, _lib.POSE_FRAME_DTYPE.itemsize), device=d, dtype=torch.uint8)
        self.flops_per_frame = self.L.pn_net_flops_per_frame(self.net)

    @property
    def net(self):
        """The model's CURRENT pn_net handle.  The module destroys its handle on invalidate() / load_state_dict() / a
        forward at another size or precision, so the engine never keeps a raw copy: it re-reads (or re-compiles) here."""
        # always through _compile: it compares the FULL key (device, precision, input size, weights version), so a net the
        # module compiled for another size / precision by a direct model(x) call is never run on this engine's buffers
        if self._locked:
            # a captured hipGraph refers to the pn_net this engine was locked on.  invalidate() / load_state_dict() / a train-mode
            # forward release the module's handle (the locked one is only retired, never freed: HipNetModule._release): refuse to
            # run -- and above all to silently compile a fresh net next to graphs that still replay the old one
            cur = self.model._net
            prec = _PREC.get(str(self.model.precision).lower())
            key = (self.device.index, prec, self.S, self.S, self.model._weights_version())
            if cur is None or cur[0] != self._locked_net or cur[1] != key or cur[2] < self.max_batch:
                raise _lib.PopnetError("PoseEngine: the module was invalidated, recompiled or modified while the engine is locked / captured "
                                       "(a captured hipGraph still refers to the pn_net of the lock): unlock -- lock(False) -- and capture again")
            return cur[0]
        return self.model._compile(self.device, self.max_batch, self.S, self.S)

    def lock(self, locked=True):
        """Freeze the net's launch descriptors (call after a warm-up forward, before capturing a hipGraph).  The locked handle
        is pinned in the module: nothing destroys it until lock(False)."""
        if locked:
            if self._locked:
                return
            net = self.net
            (self.model._ctx or self.ctx).check(self.L.pn_net_lock(net, 1), "pn_net_lock")
            self.model._pin(net)
            self._locked_net = net
            self._locked = True
        elif self._locked:
            net = self._locked_net
            self._locked = False
            self._locked_net = None
            (self.model._ctx or self.ctx).check(self.L.pn_net_lock(net, 0), "pn_net_lock")
            self.model._unpin(net)                                   # frees the handle if the module had retired it meanwhile

    # ---- stages (all asynchronous on the current stream) --------------------------------------
    def preprocess(self, depth):
        _lib.require_cuda_tensor(depth, "depth")
        if depth.dtype == torch.float16:
            dt = _lib.PN_DEPTH_F16
        elif depth.dtype == torch.float32:
            dt = _lib.PN_DEPTH_F32
        else:
            raise _lib.PopnetError("depth frames must be float16 or float32")
        B, H, W = depth.shape
        if B > self.max_batch:
            raise _lib.PopnetError("batch %d exceeds max_batch %d" % (B, self.max_batch))
        depth = depth.contiguous()
        self.ctx.check(self.L.pn_preprocess(self.ctx.handle, C.c_void_p(depth.data_ptr()), dt, B, H, W,
                                            C.c_void_p(self.x.data_ptr()), self.S, float(self.profile.depth_max), float(self.profile.depth_mean),
                                            float(self.profile.depth_std), _lib.current_stream_ptr(self.device)), "pn_preprocess")
        return B

    def forward(self, B):
        net = self.net                                               # (the net reports errors through the context it was created on)
        (self.model._ctx or self.ctx).check(self.L.pn_rtpose_forward(net, C.c_void_p(self.x.data_ptr()), B, C.c_void_p(self.paf.data_ptr()),
                                                                     C.c_void_p(self.heat.data_ptr()), C.c_void_p(self.z.data_ptr()),
                                                                     _lib.current_stream_ptr(self.device)), "pn_rtpose_forward")

    def _frames_args(self, depth):
        _lib.require_cuda_tensor(depth, "depth")
        if depth.dtype not in (torch.float16, torch.float32):
            raise _lib.PopnetError("depth frames must be float16 or float32")
        B, H, W = depth.shape
        if B > self.max_batch:
            raise _lib.PopnetError("batch %d exceeds max_batch %d" % (B, self.max_batch))
        depth = depth.contiguous()                                   # (a copy, if one is made, is stream-ordered like every torch allocation)
        dt = _lib.PN_DEPTH_F16 if depth.dtype == torch.float16 else _lib.PN_DEPTH_F32
        return B, (C.c_void_p(depth.data_ptr()), dt, B, H, W, float(self.profile.depth_max), float(self.profile.depth_mean), float(self.profile.depth_std))

    def _inputs_args(self, x):
        """_frames_args for the third input kind of the ablation entries (PN_DEPTH_NET): x [B,1,S,S] float32, the network input itself.
        -> (B, the entry's frame arguments, the contiguous tensor they point into)."""
        _lib.require_cuda_tensor(x, "x")
        if x.dtype != torch.float32 or x.dim() != 4 or tuple(x.shape[1:]) != (1, self.S, self.S):
            raise _lib.PopnetError("a network input must be a [B,1,%d,%d] float32 tensor, got %s %s" % (self.S, self.S, tuple(x.shape), x.dtype))
        B = x.shape[0]
        if B > self.max_batch:
            raise _lib.PopnetError("batch %d exceeds max_batch %d" % (B, self.max_batch))
        x = x.contiguous()      # handed back: the pointer in the arguments is into THIS tensor, which the caller keeps until the launch
        return B, (C.c_void_p(x.data_ptr()), _lib.PN_DEPTH_NET, B, self.S, self.S, float(self.profile.depth_max), float(self.profile.depth_mean),
                   float(self.profile.depth_std)), x

    def _depth_args(self, depth):
        """(B, the entry's frame arguments, the contiguous tensor they point into) of raw frames [B,H,W] or of a network input [B,1,S,S]."""
        if isinstance(depth, torch.Tensor) and depth.dim() == 4:
            return self._inputs_args(depth)
        depth = depth.contiguous() if isinstance(depth, torch.Tensor) else depth      # (_frames_args points into what it is given once contiguous)
        B, args = self._frames_args(depth)
        return B, args, depth

    def predict_inputs(self, x, frames=None, wire=None):
        """predict() on an already clamped and normalised network input x [B,1,S,S] float32 (device) -- what the scripts that compose or
        augment their frames feed the net (targets.augment_resize, KDH3DSingleSet.inputs).  In every precision x is copied into self.x
        and forward(B) runs: the fused frames-in stem resizes raw frames and has nothing to do here.  No sync."""
        B, _, x = self._inputs_args(x)
        self.x[:B].copy_(x)
        self.forward(B)
        self.parse(B, frames, wire)
        return (self.frames if frames is None else frames)[:B]

    def forward_frames(self, depth):
        """preprocess + forward as ONE call on the raw frames (pn_rtpose_forward_frames: the stem resizes / clamps / normalises its own
        input tile; bit-identical maps, the pre-processed tensor is never written).  The fp32 parity mode keeps the two calls."""
        if _PREC.get(str(self.model.precision).lower()) == _lib.PN_PREC_F32:
            B = self.preprocess(depth)
            self.forward(B)
            return B
        B, args = self._frames_args(depth)
        net = self.net
        (self.model._ctx or self.ctx).check(self.L.pn_rtpose_forward_frames(net, *args, C.c_void_p(self.paf.data_ptr()), C.c_void_p(self.heat.data_ptr()),
                                                                            C.c_void_p(self.z.data_ptr()), _lib.current_stream_ptr(self.device)),
                                            "pn_rtpose_forward_frames")
        return B

    def parse(self, B, frames=None, wire=None):
        """wire: optional device uint8 tensor [>= B, sizeof(pn_pose_wire)] that receives the compact records in the same launch."""
        frames = self.frames if frames is None else frames
        h = self.S // 8
        self.ctx.check(self.L.pn_parse_paf_wire(self.ctx.handle, C.c_void_p(self.heat.data_ptr()), C.c_void_p(self.paf.data_ptr()),
                                                C.c_void_p(self.z.data_ptr()), B, h, h, C.byref(self.cfg), C.c_void_p(frames.data_ptr()),
                                                C.c_void_p(wire.data_ptr() if wire is not None else None),
                                                _lib.current_stream_ptr(self.device)), "pn_parse_paf_wire")

    def predict(self, depth, frames=None, wire=None):
        """depth [B,H,W] CUDA f16/f32 -> device uint8 tensor [B, sizeof(pn_pose_frame)] (no sync)."""
        B = self.forward_frames(depth)
        self.parse(B, frames, wire)
        return (self.frames if frames is None else frames)[:B]

    def predict_host(self, depth):
        return records_to_numpy(self.predict(depth))

    def predict_lists(self, depth):
        """depth [B,H,W] -> the reference's per-frame result lists (dataset.pose_records_to_lists), with NO capacity limit:
        a frame whose fixed-size record overflows (more than 32 peaks in a joint map or 32 persons) is parsed again from the
        maps of this batch by the unbounded second pass (pn_parse_paf_unbounded), so it comes back as the reference would
        return it instead of raising."""
        return self.lists_from_records(records_to_numpy(self.predict(depth)))

    def lists_from_records(self, recs):
        """Result lists of the batch whose maps are in self.heat / self.paf / self.z and whose records are `recs` (numpy)."""
        from .dataset import pose_records_to_lists
        from .utils.paf_to_pose import parse_paf_unbounded
        over = {i: parse_paf_unbounded(self.heat[i], self.paf[i], self.z[i], self.cfg) for i in range(len(recs)) if int(recs[i]["status"])}
        return pose_records_to_lists(recs, over, profile=self.profile)

    # ---- depth-ablation arms (evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py:197-299) ----------
    def predict_ablation(self, depth, gt_2d, gmax=None):
        """predict() plus the three depth-ablation read-outs of the reference's evaluation script, on the same stream, no sync.
        depth [B,H,W] CUDA f16/f32; gt_2d: per frame the labels' [n_g][15][2] joints (original-frame pixels); gmax: rows per frame of the
        ground-truth arms (default: the batch's largest n_g).  Returns (records, pred_raw, perfect_map, perfect_raw): device tensors, records
        as predict(), pred_raw float64 [B, PN_MAX_PERSONS, 15, 3] = human_pred_set_3d_read_raw_depth per record row, perfect_map / perfect_raw
        float64 [B, gmax, 15, 3] = human_pred_set_3d_perfect_2d / _perfect_2d_read_raw_depth per ground-truth person (rows past a frame's count: zero)."""
        if len(gt_2d) != depth.shape[0]:
            raise _lib.PopnetError("predict_ablation: %d frames but ground truth for %d" % (depth.shape[0], len(gt_2d)))
        depth = depth.contiguous()                   # the three calls read the same frames
        recs = self.predict(depth)
        return (recs,) + self.ablation_arms(depth, recs, gt_2d, gmax)

    def ablation_arms(self, depth, recs, gt_2d, gmax=None):
        """The two launches behind predict_ablation: pn_ablation_pred_raw on the device records `recs` and pn_ablation_perfect_2d on the
        pose-depth maps in self.z, both reading the raw frames `depth` the records and maps came from.  -> (pred_raw, perfect_map, perfect_raw).
        depth may also be the network input itself, [B,1,S,S] float32 as predict_inputs took it (PN_DEPTH_NET): the raw depth is then
        that tensor un-normalised, as in the scripts that have no raw frame (evaluation_rtpose_light3d_kdh3d_mpaug_ablation.py:206-207)."""
        B, args, depth = self._depth_args(depth)
        if len(gt_2d) != B or recs.shape[0] != B:
            raise _lib.PopnetError("ablation_arms: %d frames, %d records, ground truth for %d" % (B, recs.shape[0], len(gt_2d)))
        J = _lib.PN_NUM_JOINTS
        counts = np.array([len(g) for g in gt_2d], dtype=np.int32)
        G = int(counts.max()) if gmax is None else int(gmax)
        if G < int(counts.max()):
            raise _lib.PopnetError("ablation_arms: gmax %d is below the %d ground-truth persons of a frame" % (G, int(counts.max())))
        gt = np.zeros((B, G, J, 2), np.float64)
        for b, g in enumerate(gt_2d):
            if len(g):
                a = np.asarray(g, dtype=np.float64)
                if a.shape != (len(g), J, 2):
                    raise _lib.PopnetError("ablation_arms: ground truth of frame %d has shape %s, expected [n][%d][2]" % (b, a.shape, J))
                gt[b, :len(g)] = a
        recs = recs.contiguous()
        d = self.device
        gt_dev = torch.from_numpy(gt).to(d, non_blocking=True)
        cnt_dev = torch.from_numpy(counts).to(d, non_blocking=True)
        pred_raw = torch.empty((B, _lib.PN_MAX_PERSONS, J, 3), device=d, dtype=torch.float64)
        pm = torch.empty((B, G, J, 3), device=d, dtype=torch.float64)
        pr = torch.empty((B, G, J, 3), device=d, dtype=torch.float64)
        st = _lib.current_stream_ptr(d)
        dargs = (C.c_void_p(depth.data_ptr()),) + args[1:6]          # frames, dtype, B, H, W, depth_max
        self.ctx.check(self.L.pn_ablation_pred_raw(self.ctx.handle, *dargs, C.byref(self.cfg), C.c_void_p(recs.data_ptr()),
                                                   C.c_void_p(pred_raw.data_ptr()), st), "pn_ablation_pred_raw")
        h = self.S // 8
        self.ctx.check(self.L.pn_ablation_perfect_2d(self.ctx.handle, *dargs, C.c_void_p(self.z.data_ptr()), h, h, C.byref(self.cfg),
                                                     C.c_void_p(gt_dev.data_ptr()), C.c_void_p(cnt_dev.data_ptr()), G,
                                                     C.c_void_p(pm.data_ptr()), C.c_void_p(pr.data_ptr()), st), "pn_ablation_perfect_2d")
        return pred_raw, pm, pr

    def depth_probe(self, depth, points):
        """The un-normalised network input ("raw depth" of the evaluation script) at `points` [n][3] = (frame, y, x) of the S x S frames the
        engine derives from depth [B,H,W], or of a network input [B,1,S,S] (see ablation_arms): float32 [n] (host).  A point outside the
        batch or the frame raises."""
        B, args, depth = self._depth_args(depth)
        pts = np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 3)
        pts_dev = torch.from_numpy(pts).to(self.device)
        out = torch.empty((len(pts),), device=self.device, dtype=torch.float32)
        self.ctx.check(self.L.pn_depth_probe(self.ctx.handle, C.c_void_p(depth.data_ptr()), *args[1:5], self.S, *args[5:8],
                                             C.c_void_p(pts_dev.data_ptr()), len(pts), C.c_void_p(out.data_ptr()),
                                             _lib.current_stream_ptr(self.device)), "pn_depth_probe")
        return out.cpu().numpy()

    def ablation_lists(self, depth, gt_2d, recs, pred_raw, perfect_map, perfect_raw):
        """The eval_data.json lists of one batch with the four ablation keys (dataset.pose_records_to_lists(..., ablation=...)): recs (numpy
        records) and the three arms (numpy or device) as predict_ablation returned them for depth / gt_2d, the batch's maps still in
        self.heat / self.paf / self.z.  A frame whose record overflowed is parsed again without capacities, as in lists_from_records; its raw
        arm then comes from pn_depth_probe at the re-parsed joints and the reference's float64 back-projection.  depth: raw frames or the
        network input, as in ablation_arms."""
        from .dataset import pose_records_to_lists
        from .utils.paf_to_pose import parse_paf_unbounded
        tonp = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        over, over_raw = {}, {}
        for i in range(len(recs)):
            if not int(recs[i]["status"]):
                continue
            r = over[i] = parse_paf_unbounded(self.heat[i], self.paf[i], self.z[i], self.cfg)
            pj = r["person_joint"]
            vis = pj >= 0
            raw = np.full(pj.shape, -1.0)
            if vis.any():
                xy = r["joint_list"][pj[vis]][:, :2]
                pts = np.stack([np.full(len(xy), i), xy[:, 1].astype(np.int64), xy[:, 0].astype(np.int64)], axis=1)
                raw[vis] = self.depth_probe(depth, pts).astype(np.float64)
            j2 = r["joints_2d"]
            over_raw[i] = np.stack([(j2[..., 0] - self.cfg.cx) * raw / self.cfg.fx, (j2[..., 1] - self.cfg.cy) * raw / self.cfg.fy, raw], axis=-1)
        abl = {"pred_raw": tonp(pred_raw), "perfect_map": tonp(perfect_map), "perfect_raw": tonp(perfect_raw), "gt_2d": gt_2d,
               "overflow_raw": over_raw}
        return pose_records_to_lists(recs, over, ablation=abl)

    def pack(self, frames, wire=None):
        """pn_pose_frame records (device, [B, sizeof]) -> compact pn_pose_wire records (device uint8 [B, sizeof], no sync):
        the form that is gathered across GPUs (6.2 KB instead of 33 KB per frame)."""
        B = frames.shape[0]
        if wire is None:
            wire = torch.empty((B, _lib.POSE_WIRE_DTYPE.itemsize), device=frames.device, dtype=torch.uint8)
        self.ctx.check(self.L.pn_pack_pose_frames(self.ctx.handle, C.c_void_p(frames.data_ptr()), B, C.c_void_p(wire.data_ptr()),
                                                  _lib.current_stream_ptr(self.device)), "pn_pack_pose_frames")
        return wire[:B]


class YoloEngine:
    """Batched Yolo-Pose+ twin of PoseEngine: depth frames -> pn_preprocess -> pn_yolo_forward ->
    pn_parse_yolo (decode + box NMS + skeletons + the evaluation script's rescale / back-projection)
    -> pn_yolo_frame records.  Per-batch body of
    tpm/evaluate/evaluation_yolo_posenet_kdh3d_mpreal.py:137-217 minus Python."""

    def __init__(self, precision="bf16", state_dict=None, device=None, max_batch=32, input_size=224,
                 w_org=None, h_org=None, intrinsics=None, weight_seed=1, anchors=None,
                 conf_threshold=0.5, nms_threshold=0.5, private_ctx=False, profile=None):
        from .config import YOLO_ANCHORS
        from .network.yolo_posenet import YoloPoseNet
        if not torch.cuda.is_available():
            raise _lib.PopnetError("YoloEngine needs a GPU: the HIP path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_batch, self.S = int(max_batch), int(input_size)
        self.profile = profiles.get(profile)
        self.anchors = list(YOLO_ANCHORS if anchors is None else anchors)
        self.model = YoloPoseNet(15, input_dim=1, anchors=self.anchors).eval()
        if state_dict is None:
            synth.load_synth_weights(self.model, seed=weight_seed)
            calibrate_yolo_conf(self.model, self.device)
        else:
            self.model.load_state_dict(state_dict)
        self.model.precision = precision
        self.ctx = _lib.Context(self.device.index) if private_ctx else _lib.Context.for_device(self.device.index)
        self.L = _lib.lib()
        self.cfg = make_parse_cfg(default_cfg(), input_size=self.S, w_org=w_org, h_org=h_org, intrinsics=intrinsics, profile=self.profile)
        self.conf_threshold, self.nms_threshold = float(conf_threshold), float(nms_threshold)
        flat = [float(v) for a in self.anchors for v in a]
        self._anchors_c = (C.c_float * len(flat))(*flat)
        d = self.device
        self.x = torch.empty((self.max_batch, 1, self.S, self.S), device=d, dtype=torch.float32)
        self.out = torch.empty((self.max_batch, len(self.anchors) * 50, self.S // 16, self.S // 16), device=d,
                               dtype=torch.float32)
        self.frames = torch.empty((self.max_batch, _lib.YOLO_FRAME_DTYPE.itemsize), device=d, dtype=torch.uint8)
        self._locked = False
        self._locked_net = None
        self.flops_per_frame = self.L.pn_net_flops_per_frame(self.net)

    preprocess = PoseEngine.preprocess
    net = PoseEngine.net
    lock = PoseEngine.lock

    def forward(self, B):
        net = self.net
        (self.model._ctx or self.ctx).check(self.L.pn_yolo_forward(net, C.c_void_p(self.x.data_ptr()), B, C.c_void_p(self.out.data_ptr()),
                                                                   _lib.current_stream_ptr(self.device)), "pn_yolo_forward")

    _frames_args = PoseEngine._frames_args
    _inputs_args = PoseEngine._inputs_args

    def predict_inputs(self, x, frames=None):
        """predict() on an already clamped and normalised network input x [B,1,S,S] float32 (device); see PoseEngine.predict_inputs."""
        B, _, x = self._inputs_args(x)
        self.x[:B].copy_(x)
        self.forward(B)
        self.parse(B, frames)
        return (self.frames if frames is None else frames)[:B]

    def forward_frames(self, depth):
        """preprocess + forward as one call on the raw frames (pn_yolo_forward_frames); fp32 keeps the two calls."""
        if _PREC.get(str(self.model.precision).lower()) == _lib.PN_PREC_F32:
            B = self.preprocess(depth)
            self.forward(B)
            return B
        B, args = self._frames_args(depth)
        net = self.net
        (self.model._ctx or self.ctx).check(self.L.pn_yolo_forward_frames(net, *args, C.c_void_p(self.out.data_ptr()), _lib.current_stream_ptr(self.device)),
                                            "pn_yolo_forward_frames")
        return B

    def parse(self, B, frames=None):
        frames = self.frames if frames is None else frames
        h = self.S // 16
        self.ctx.check(self.L.pn_parse_yolo(self.ctx.handle, C.c_void_p(self.out.data_ptr()), B, h, h, self._anchors_c,
                                            len(self.anchors), 15, self.S, self.S, float(self.profile.depth_mean), float(self.profile.depth_std),
                                            self.conf_threshold, self.nms_threshold, 0, C.byref(self.cfg),
                                            C.c_void_p(frames.data_ptr()), _lib.current_stream_ptr(self.device)),
                       "pn_parse_yolo")

    def predict(self, depth, frames=None):
        """depth [B,H,W] CUDA f16/f32 -> device uint8 tensor [B, sizeof(pn_yolo_frame)] (no sync)."""
        B = self.forward_frames(depth)
        self.parse(B, frames)
        return (self.frames if frames is None else frames)[:B]

    def predict_host(self, depth):
        return self.predict(depth).cpu().numpy().view(_lib.YOLO_FRAME_DTYPE).reshape(-1)


class A2JEngine:
    """The second stage of the Yolo-A2J baseline: depth frames + box rows -> per-box crops (pn_a2j_crop) -> A2J_model (pn_a2j_forward) ->
    anchor vote and map back to the frame (pn_a2j_vote) -> pn_a2j_record per box.  The per-box body of
    third_party_methods/A2J_experiments/a2j_test_pred_box_new.py:268-313,340-421 minus Python.  boxes: [n, 6] float32 rows
    (frame index, x0, y0, x1, y1, conf) in original-frame pixels, sorted by frame; a frame without a detection carries one row
    (f, -1, -1, -1, -1, 0) and comes out as one person at (-1, -1) with confidence 0, as in the reference."""

    def __init__(self, precision="bf16", state_dict=None, device=None, max_batch=32, crop=288, img_wh=(480, 512), intrinsics=None, weight_seed=3):
        from .network.a2j import A2J_model, A2JCfg, A2J_RECORD_DTYPE, generate_anchors, shift
        if not torch.cuda.is_available():
            raise _lib.PopnetError("A2JEngine needs a GPU: the HIP path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_batch = int(max_batch)
        self.crop_h, self.crop_w = (int(crop), int(crop)) if np.isscalar(crop) else (int(crop[0]), int(crop[1]))
        if state_dict is None:
            with torch.random.fork_rng(devices=[]):      # the module's own seeded initialisation (nothing is downloaded); the caller's RNG stays as it was
                torch.manual_seed(weight_seed)
                self.model = A2J_model(15).eval()
        else:
            self.model = A2J_model(15).eval()
            self.model.load_state_dict(state_dict)
        self.model.precision = precision
        self.L = _lib.lib()
        self.ctx = _lib.Context.for_device(self.device.index)
        self.cfg = A2JCfg()
        self.L.pn_a2j_cfg_default(C.byref(self.cfg))
        self.cfg.img_w, self.cfg.img_h = int(img_wh[0]), int(img_wh[1])
        self.cfg.crop_w, self.cfg.crop_h = self.crop_w, self.crop_h
        if intrinsics is not None:
            self.cfg.fx, self.cfg.fy, self.cfg.cx, self.cfg.cy = (float(intrinsics[k]) for k in ("fx", "fy", "cx", "cy"))
        if self.L.pn_sizeof_a2j_record() != A2J_RECORD_DTYPE.itemsize:
            raise _lib.PopnetError("pn_a2j_record layout mismatch")
        self.record_dtype = A2J_RECORD_DTYPE
        d = self.device
        self.anchors = torch.from_numpy(shift([self.crop_h // 16, self.crop_w // 16], 16, generate_anchors())).float().to(d)
        self.x = torch.empty((self.max_batch, 1, self.crop_h, self.crop_w), device=d, dtype=torch.float32)
        self.last_flags = None
        self._votes = torch.empty((self.max_batch, 15, 3), device=d, dtype=torch.float32)

    @property
    def net(self):
        """The compiled pn_net (built on first use: the crops need none)."""
        return self.model._compile(self.device, self.max_batch, self.crop_h, self.crop_w)

    def _frames(self, frames):
        _lib.require_cuda_tensor(frames, "frames")
        if frames.dim() != 3 or frames.dtype not in (torch.float16, torch.float32):
            raise _lib.PopnetError("frames must be a [F, H, W] float16 / float32 tensor")
        return frames.contiguous(), (_lib.PN_DEPTH_F16 if frames.dtype == torch.float16 else _lib.PN_DEPTH_F32)

    def _rows(self, boxes):
        rows = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 6).to(self.device).contiguous()
        return rows

    def crops(self, frames, boxes):
        """-> ([n, 1, crop_h, crop_w] float32 crops, [n] int32 flags: 1 where the reference would raise, the crop is zeros)."""
        frames, dt = self._frames(frames)
        rows = self._rows(boxes)
        n = rows.shape[0]
        out = torch.empty((n, 1, self.crop_h, self.crop_w), device=self.device, dtype=torch.float32)
        flags = torch.zeros((n,), device=self.device, dtype=torch.int32)
        self.ctx.check(self.L.pn_a2j_crop(self.ctx.handle, C.c_void_p(frames.data_ptr()), dt, frames.shape[0], frames.shape[1], frames.shape[2],
                                          C.c_void_p(rows.data_ptr()), n, C.byref(self.cfg), C.c_void_p(out.data_ptr()), C.c_void_p(flags.data_ptr()),
                                          _lib.current_stream_ptr(self.device)), "pn_a2j_crop")
        return out, flags

    def train_crops(self, frames, items):
        """The trainers' crop-level augmentation (pn_a2j_train_crop): frames [F, H, W] float16 / float32 and the pn_a2j_crop_item records of
        popnet_amd.a2j_crops.itop_items / box_items -> ([n, 1, crop_h, crop_w] float32, [n] int32 flags: 1 where the reference would
        raise, the crop is zeros).  One launch, no sync; mean / std are self.cfg's.  The records are copied to the device in stream order
        and must stay untouched until the stream has passed the call: the engine holds on to `items` until its next train_crops, so
        a caller may drop or rebind them at once, but must not write into them before a synchronise."""
        frames, dt = self._frames(frames)
        n = len(items)
        self._items_host = items
        out = torch.empty((n, 1, self.crop_h, self.crop_w), device=self.device, dtype=torch.float32)
        flags = torch.zeros((n,), device=self.device, dtype=torch.int32)
        items_dev = torch.empty((max(n, 1) * C.sizeof(_lib.A2JCropItem),), device=self.device, dtype=torch.uint8)      # the call uploads the records it has checked
        self.ctx.check(self.L.pn_a2j_train_crop(self.ctx.handle, C.c_void_p(frames.data_ptr()), dt, frames.shape[0], frames.shape[1], frames.shape[2],
                                                C.cast(items, C.c_void_p), C.c_void_p(items_dev.data_ptr()), n, C.byref(self.cfg), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(flags.data_ptr()), _lib.current_stream_ptr(self.device)), "pn_a2j_train_crop")
        return out, flags

    def votes(self, crops):
        """crops [n, 1, crop_h, crop_w] float32 (device) -> [n, 15, 3] float32 (y, x, z) in crop pixels: pn_a2j_forward and pn_a2j_vote in
        chunks of max_batch, no map back to a frame (post_process of the eval-mode module; no sync)."""
        _lib.require_cuda_tensor(crops, "crops")
        if crops.dim() != 4 or tuple(crops.shape[1:]) != (1, self.crop_h, self.crop_w) or crops.dtype != torch.float32:
            raise _lib.PopnetError("crops must be a [n, 1, %d, %d] float32 tensor, got %s %s" % (self.crop_h, self.crop_w, tuple(crops.shape), crops.dtype))
        crops = crops.contiguous()
        n = crops.shape[0]
        out = torch.empty((n, 15, 3), device=self.device, dtype=torch.float32)
        net = self.net
        prec = self.model._net[1][1]
        stream = _lib.current_stream_ptr(self.device)
        for i in range(0, n, self.max_batch):
            m = min(self.max_batch, n - i)
            ptrs = [C.c_void_p() for _ in range(3)]
            self.ctx.check(self.L.pn_a2j_forward(net, C.c_void_p(crops[i:].data_ptr()), m, *(C.byref(p) for p in ptrs), stream), "pn_a2j_forward")
            self.ctx.check(self.L.pn_a2j_vote(self.ctx.handle, ptrs[0], ptrs[1], ptrs[2], prec, m, self.crop_h // 16, self.crop_w // 16, 16, 15,
                                              C.c_void_p(self.anchors.data_ptr()), C.c_void_p(out[i:].data_ptr()), None, None, None, stream), "pn_a2j_vote")
        return out

    def predict(self, frames, boxes):
        """-> device uint8 tensor [n, sizeof(pn_a2j_record)], the rows in chunks of max_batch (no sync).  self.last_flags: device int32 [n],
        1 where the reference would raise on the row's box (zero crop, see crops())."""
        frames, dt = self._frames(frames)
        rows = self._rows(boxes)
        n = rows.shape[0]
        recs = torch.zeros((n, self.record_dtype.itemsize), device=self.device, dtype=torch.uint8)
        flags = torch.zeros((n,), device=self.device, dtype=torch.int32)
        self.last_flags = flags
        net = self.net
        for i in range(0, n, self.max_batch):
            m = min(self.max_batch, n - i)
            self.ctx.check(self.L.pn_a2j_predict(
                net, C.c_void_p(frames.data_ptr()), dt, frames.shape[0], frames.shape[1], frames.shape[2], C.c_void_p(rows[i:].data_ptr()), m,
                C.byref(self.cfg), C.c_void_p(self.anchors.data_ptr()), C.c_void_p(self.x.data_ptr()), C.c_void_p(flags[i:].data_ptr()),
                C.c_void_p(self._votes.data_ptr()), C.c_void_p(recs[i:].data_ptr()), _lib.current_stream_ptr(self.device)), "pn_a2j_predict")
        return recs

    def predict_host(self, frames, boxes):
        return self.predict(frames, boxes).cpu().numpy().view(self.record_dtype).reshape(-1)

    def predict_lists(self, frames, boxes, n_frames=None):
        """-> (pred_2d, pred_3d, part_conf): per frame a list of persons, each 15 x [x, y] / [X, Y, Z] / confidences -- the reference's
        human_pred_set_2d / _3d / part_conf lists (a2j_test_pred_box_new.py:397-421)."""
        recs = self.predict_host(frames, boxes)
        return lists_from_a2j_records(recs, frames.shape[0] if n_frames is None else n_frames)


def a2j_set_votes(engine, batch_fn, n, batch_size):
    """The test loop of the A2J trainers (itop_train_64.py:417-424): items 0 .. n - 1 in order, batch_fn(indices) -> (frames, records, labels)
    (ItopA2JSet.batch / KDH3DSingleSet.crop_batch) -> engine.train_crops -> engine.votes.  -> [n, 15, 3] float32 host array (y, x, z)."""
    out = []
    for s in range(0, n, batch_size):
        frames, items, _ = batch_fn(list(range(s, min(s + batch_size, n))))
        crops, _ = engine.train_crops(frames, items)
        out.append(engine.votes(crops))
    return torch.cat(out).cpu().numpy() if out else np.zeros((0, 15, 3), np.float32)


def lists_from_a2j_records(recs, n_frames):
    p2, p3, pc = [[] for _ in range(n_frames)], [[] for _ in range(n_frames)], [[] for _ in range(n_frames)]
    for r in recs:
        f = int(r["frame"])
        p2[f].append(r["joint"][:, 0:2].astype(np.float64).tolist())
        p3[f].append(r["joint"][:, 2:5].astype(np.float64).tolist())
        pc[f].append([float(r["conf"])] * 15)
    return p2, p3, pc


def yolo_box_rows(yolo_frames):
    """pn_yolo_frame records (host) -> A2J box rows [n, 6]: per detection (frame, bbox_org x0, y0, x1, y1, conf); a frame without a
    detection gives (frame, -1, -1, -1, -1, 0) (evaluation_yolo_posenet_kdh3d_mpreal_a2j_preprocess.py:197-228)."""
    rows = []
    for f, fr in enumerate(yolo_frames):
        n = int(fr["n_det"])
        if n == 0:
            rows.append([f, -1, -1, -1, -1, 0])
        for k in range(n):
            rows.append([f] + [float(v) for v in fr["bbox_org"][k]] + [float(fr["bbox"][k][4])])
    return np.asarray(rows, dtype=np.float32).reshape(-1, 6)


class YoloA2JEngine:
    """YoloEngine -> A2JEngine: the boxes of pn_yolo_frame.bbox_org with their confidences become the A2J rows; the crops are chunked by
    the A2J engine's max_batch."""

    def __init__(self, precision="bf16", yolo_state_dict=None, a2j_state_dict=None, device=None, max_batch=32, crop=288, img_wh=(480, 512), **yolo_kw):
        self.yolo = YoloEngine(precision=precision, state_dict=yolo_state_dict, device=device, max_batch=max_batch, **yolo_kw)
        self.a2j = A2JEngine(precision=precision, state_dict=a2j_state_dict, device=device, max_batch=max_batch, crop=crop, img_wh=img_wh)

    def predict_lists(self, depth):
        rows = yolo_box_rows(self.yolo.predict_host(depth))
        return self.a2j.predict_lists(depth, rows, n_frames=depth.shape[0])


def calibrate_yolo_conf(model, device=None, frac=0.012, calib_frames=8, seed=99):
    """Synthetic-checkpoint calibration for YoloPoseNet (bench / smoke only; never applied to user
    weights).  Seeded random weights put every cell's confidence near sigmoid(0) = 0.5, i.e. ~200
    candidate boxes per frame.  The last conv has no bias, so the two confidence filters (channels 4
    and 54) are shifted by a constant -delta on every tap: delta is grid-searched on a seeded
    calibration batch (fp32 forward of the HIP path itself) so ~frac of the cells pass conf > 0.5."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    depth = torch.from_numpy(synth.synth_depth(calib_frames, seed=seed)).to(device)
    ctx = _lib.Context.for_device(device.index)
    x = torch.empty((calib_frames, 1, 224, 224), device=device, dtype=torch.float32)
    ctx.check(_lib.lib().pn_preprocess(ctx.handle, C.c_void_p(depth.data_ptr()), _lib.PN_DEPTH_F16, calib_frames,
                                       depth.shape[1], depth.shape[2], C.c_void_p(x.data_ptr()), 224, float(DEPTH_MAX),
                                       float(DEPTH_MEAN), float(DEPTH_STD), _lib.current_stream_ptr(device)), "pn_preprocess")
    prec = model.precision
    model.precision = "fp32"
    w0 = model.model2_4[0].weight.detach().clone()

    def frac_at(delta):
        with torch.no_grad():
            model.model2_4[0].weight.copy_(w0)
            model.model2_4[0].weight[[4, 54]] -= delta
        model.invalidate()
        out = model(x)
        return float((out[:, [4, 54]] > 0.5).float().mean())

    lo, hi = 0.0, 0.2
    for _ in range(12):                      # fraction above 0.5 falls as delta grows (inputs are mostly positive)
        mid = 0.5 * (lo + hi)
        if frac_at(mid) > frac:
            lo = mid
        else:
            hi = mid
    frac_at(hi)
    model.precision = prec
    model.invalidate()
    return model


class StreamingEngine:
    """Throughput front end: `depth` batches in flight on one GPU.

    Slot i owns a PoseEngine / YoloEngine (activations, a PRIVATE pn_ctx = its own parse scratch), `pool` static input
    buffers, a device and a pinned host record buffer, a HIP stream and -- once `capture()` has run -- one hipGraph of
    the whole step (pre-processing, forward, parsing, record D2H copy) PER INPUT BUFFER.  `submit(j)` replays slot
    (ticket mod depth) on input buffer j of that slot and returns at once; the latency-bound tail of a batch (head
    convolutions, pose assembly, the record copy) then overlaps with the convolutions of the next batches.  Fill
    `input(slot, j)` (e.g. with a non_blocking copy from pinned host memory issued on `stream(slot)`) before
    submitting; read `records(ticket)` / `host_records(ticket)` after `wait(ticket)`.  A slot must be waited for
    before it is submitted again.

    wire=True: what leaves the GPU per step is the compact pn_pose_wire form (6.2 KB instead of 33 KB per frame; PAF
    path only): `host_records()` then holds pn_pose_wire records, `records()` still the full pn_pose_frame ones.

    Engine arguments (PoseEngine's parse_config and the dataset `profile` among them) pass through **engine_kw to every slot's engine;
    frame_hw=None takes the profile's frame size (640 x 480 for the default MP3DHP).

    Every engine gets its own context and its net is locked after the warm-up (pn_net_lock): nothing a captured graph
    points at (parse scratch, launch descriptors) can be reallocated or rewritten by a later eager call."""

    def __init__(self, engine_cls=None, depth=3, frame_hw=None, frame_dtype=torch.float16, graph=True, pool=1,
                 wire=False, **engine_kw):
        engine_cls = PoseEngine if engine_cls is None else engine_cls
        if frame_hw is None:
            prof = profiles.get(engine_kw.get("profile"))
            frame_hw = (prof.h_org, prof.w_org)
        self.depth = max(1, int(depth))
        self.pool = max(1, int(pool))
        engine_kw["private_ctx"] = True
        self.engines = [engine_cls(**engine_kw) for _ in range(self.depth)]
        e0 = self.engines[0]
        self.device, self.max_batch = e0.device, e0.max_batch
        item = e0.frames.shape[1]
        self.wire = bool(wire) and isinstance(e0, PoseEngine)
        hitem = _lib.POSE_WIRE_DTYPE.itemsize if self.wire else item
        self.inputs = [[torch.zeros((self.max_batch,) + tuple(frame_hw), device=self.device, dtype=frame_dtype)
                        for _ in range(self.pool)] for _ in range(self.depth)]
        self.recs = [torch.empty((self.max_batch, item), device=self.device, dtype=torch.uint8) for _ in range(self.depth)]
        self.wires = [torch.empty((self.max_batch, hitem), device=self.device, dtype=torch.uint8) if self.wire else None
                      for _ in range(self.depth)]
        self.host = [torch.empty((self.max_batch, hitem), dtype=torch.uint8, pin_memory=True) for _ in range(self.depth)]
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(self.depth)]
        self.events = [torch.cuda.Event() for _ in range(self.depth)]
        # host hand-over (submit_host): a copy stream per slot, "copied" / "no longer read" events per input buffer
        cs = torch.cuda.Stream(device=self.device)             # ONE copy stream: transfers leave in batch order, one at a time at link rate
        self.copy_streams = [cs for _ in range(self.depth)]
        self._copied = [[torch.cuda.Event() for _ in range(self.pool)] for _ in range(self.depth)]
        self._released = [[None] * self.pool for _ in range(self.depth)]
        self._next_buf = [0] * self.depth
        self._posted = []                                      # (slot, buffer) of the batches posted ahead by post_host, oldest first
        self.graphs = [[None] * self.pool for _ in range(self.depth)]
        self._want_graph = bool(graph)
        self._tickets = 0
        cur = torch.cuda.current_stream(self.device)
        for st in self.streams:
            st.wait_stream(cur)

    def input(self, slot, j=0):
        return self.inputs[slot % self.depth][j % self.pool]

    def stream(self, slot):
        return self.streams[slot % self.depth]

    def _body(self, s, j=0):
        e = self.engines[s]
        if self.wire:
            e.predict(self.inputs[s][j], self.recs[s], self.wires[s])      # full and compact records from the same read-out launch
            self.host[s].copy_(self.wires[s], non_blocking=True)
        else:
            e.predict(self.inputs[s][j], self.recs[s])
            self.host[s].copy_(self.recs[s], non_blocking=True)

    def capture(self):
        """Warm every slot eagerly, lock its net, then record its step as one hipGraph per input buffer (same kernels,
        same arguments)."""
        for s in range(self.depth):
            with torch.cuda.stream(self.streams[s]):
                self._body(s)
                self._body(s)
            torch.cuda.synchronize(self.device)
            self.engines[s].lock()
            if self._want_graph:
                for j in range(self.pool):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=self.streams[s]):
                        self._body(s, j)
                    self.graphs[s][j] = g
        torch.cuda.synchronize(self.device)

    def submit(self, j=0, eager=False):
        """Runs the next slot on input buffer j of that slot, on the slot's stream (asynchronous).  Returns the ticket."""
        t = self._tickets
        s = t % self.depth
        j %= self.pool
        with torch.cuda.stream(self.streams[s]):
            if self.graphs[s][j] is not None and not eager:
                self.graphs[s][j].replay()
            else:
                self._body(s, j)
            self.events[s].record(self.streams[s])
        self._tickets += 1
        return t

    def post_host(self, host_batch):
        """First half of the host hand-over: enqueues the PCIe transfer of a pinned host batch into the NEXT input buffer of the
        slot that will run it -- the slot of ticket `tickets + posted` -- on the copy stream, ordered only after the step that last
        read that buffer.  A streaming caller posts batch k + depth when it submits batch k, so a transfer is always in flight under
        the kernels of earlier batches (also across the start of a timed region: the frames of a live stream do not wait for the
        previous ones to finish).  At most depth * (pool - 1) batches may be posted ahead.  Returns the number now posted."""
        if len(self._posted) >= self.depth * max(1, self.pool - 1):
            raise _lib.PopnetError("StreamingEngine.post_host: %d batches already posted (depth %d, pool %d)" % (len(self._posted), self.depth, self.pool))
        s = (self._tickets + len(self._posted)) % self.depth
        j = self._next_buf[s]
        self._next_buf[s] = (j + 1) % self.pool
        cs = self.copy_streams[s]
        if self._released[s][j] is not None:
            cs.wait_event(self._released[s][j])
        with torch.cuda.stream(cs):
            self.inputs[s][j][:len(host_batch)].copy_(host_batch, non_blocking=True)
            self._copied[s][j].record(cs)
        self._posted.append((s, j))
        return len(self._posted)

    def submit_posted(self, eager=False):
        """Second half: runs the oldest posted batch on its slot once its transfer has landed.  Returns the ticket."""
        if not self._posted:
            raise _lib.PopnetError("StreamingEngine.submit_posted: nothing posted")
        s, j = self._posted.pop(0)
        assert s == self._tickets % self.depth
        self.streams[s].wait_event(self._copied[s][j])
        t = self.submit(j, eager)
        if self._released[s][j] is None:
            self._released[s][j] = torch.cuda.Event()
        self._released[s][j].record(self.streams[s])
        return t

    def drop_posted(self):
        """Forgets the batches posted but not submitted (their transfers still complete; the buffers are simply overwritten later)."""
        self._posted = []

    def submit_host(self, host_batch, eager=False):
        """Host hand-over: copies a pinned host batch into the slot's NEXT input buffer on the slot's copy stream -- ordered only
        after the step that last read that buffer, so with pool >= 2 the PCIe transfer of this slot's next batch runs under
        the kernels of its current one -- and runs the step once the copy has landed.  Returns the ticket."""
        if self._posted:
            raise _lib.PopnetError("StreamingEngine.submit_host: batches are posted ahead (post_host); use submit_posted")
        self.post_host(host_batch)
        return self.submit_posted(eager)

    def wait(self, ticket):
        self.events[ticket % self.depth].synchronize()

    def records(self, ticket):
        return self.recs[ticket % self.depth]

    def host_records(self, ticket):
        return self.host[ticket % self.depth]

    def join(self, stream=None):
        """Makes `stream` (default: the current one) wait for everything submitted so far; no host synchronisation."""
        stream = torch.cuda.current_stream(self.device) if stream is None else stream
        for st in self.streams:
            stream.wait_stream(st)


def wire_to_lists(wire):
    """pn_pose_wire records (numpy) -> the per-frame result-schema entries (float32 values widened to Python floats)."""
    out = {"human_pred_set_2d": [], "human_pred_set_3d": [], "human_pred_set_visibility": [], "human_pred_set_part_conf": []}
    for fr in wire:
        if int(fr["status"]):        # peak / person overflow, or more persons than the wire form carries: never truncate silently
            raise _lib.PopnetError("pose wire record overflow (status=%d, %d persons; the wire form carries %d): use the full pn_pose_frame records"
                                   % (int(fr["status"]), int(fr["n_persons"]), _lib.PN_WIRE_MAX_PERSONS))
        n = int(fr["n_persons"])
        v = fr["vals"][:n].astype(np.float64)
        out["human_pred_set_2d"].append(v[:, :, 0:2].tolist())
        out["human_pred_set_3d"].append(v[:, :, 2:5].tolist())
        out["human_pred_set_part_conf"].append(v[:, :, 5].tolist())
        out["human_pred_set_visibility"].append((fr["person_joint"][:n] >= 0).astype(int).tolist())
    return out


def records_to_numpy(frames_dev):
    return frames_dev.cpu().numpy().view(_lib.POSE_FRAME_DTYPE).reshape(-1)


def calibrate_heads(model, device=None, frac=0.004, calib_frames=8, seed=99, gain=1.0):
    """Synthetic-checkpoint calibration (bench / smoke only; never applied to user weights).

    With seeded random weights every heat map hovers around sigmoid(0) = 0.5 > THRESH_HEATMAP, i.e.
    hundreds of plateau peaks per joint -- an invalid parse workload (52 s/frame
    in the reference).  This shifts each stage-2 heat channel's bias so that only `frac` of its
    cells exceed the threshold on a seeded calibration batch (about three peaks per joint map, the
    density a trained network emits for a 2-3 person frame), so the end-to-end bench runs NMS,
    refinement, limb scoring and assembly on a realistic number of candidates with nothing skipped.
    The statistics come from one fp32 forward of the HIP path itself."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    depth = torch.from_numpy(synth.synth_depth(calib_frames, seed=seed)).to(device)
    ctx = _lib.Context.for_device(device.index)
    x = torch.empty((calib_frames, 1, 224, 224), device=device, dtype=torch.float32)
    ctx.check(_lib.lib().pn_preprocess(ctx.handle, C.c_void_p(depth.data_ptr()), _lib.PN_DEPTH_F16, calib_frames,
                                       depth.shape[1], depth.shape[2], C.c_void_p(x.data_ptr()), 224, float(DEPTH_MAX),
                                       float(DEPTH_MEAN), float(DEPTH_STD), _lib.current_stream_ptr(device)), "pn_preprocess")
    prec = model.precision
    model.precision = "fp32"
    if gain != 1.0:                          # spread the heat logits: fewer cells within a rounding error of the threshold
        with torch.no_grad():
            model.model2_2[12].weight[:15] *= float(gain)
            model.model2_2[12].bias[:15] *= float(gain)
        model.invalidate()
    (_, heat, _), _ = model(x)
    s = heat[:, :15].double().clamp(1e-12, 1 - 1e-12)
    logit = torch.log(s / (1 - s)).permute(1, 0, 2, 3).reshape(15, -1)
    q = torch.quantile(logit, 1.0 - frac, dim=1)
    thr = float(np.log(0.1 / 0.9))
    with torch.no_grad():
        model.model2_2[12].bias[:15] += (thr - q).float().cpu()
    model.precision = prec
    model.invalidate()
    return model


def shard_indices(n_frames, rank, world):
    """Frame i goes to rank i % world."""
    return list(range(rank, n_frames, world))


def gather_records(local_frames, n_frames, rank, world, group=None):
    """ONE all-gather of fixed-size records; returns [n_frames, itemsize] uint8 in global frame
    order on every rank.  local_frames: [ceil(n_frames/world) or fewer, itemsize] uint8 tensor on the
    rank's device (or CPU tensor with the gloo backend)."""
    import torch.distributed as dist
    per = (n_frames + world - 1) // world
    item = local_frames.shape[1]
    pad = torch.zeros((per, item), dtype=torch.uint8, device=local_frames.device)
    pad[:local_frames.shape[0]] = local_frames
    out = torch.empty((world * per, item), dtype=torch.uint8, device=local_frames.device)
    dist.all_gather_into_tensor(out, pad, group=group)
    return deinterleave(out.view(world, per, item), n_frames)


def deinterleave(per_rank, n_frames):
    """[world, per, item] records as the all-gather delivers them (rank-major) -> [n_frames, item] in global frame order:
    frame i was processed by rank i % world as its (i // world)-th frame (shard_indices)."""
    world = per_rank.shape[0]
    idx = torch.arange(n_frames, device=per_rank.device)
    return per_rank[idx % world, idx // world]
