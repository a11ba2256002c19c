"""Training targets on the GPU: the multi-person depth compositor and the ground-truth rasterisers.

Host-side mirror of the reference's training dataset item, batched and on the device:
  KDH3D_Keypoints.__getitem__   third_party_methods/lib/datasets/datasets_kdh3d_rtpose_mpaug.py:223-286 (CR line endings)
  get_ground_truth              ...:318-401 (putGaussianMaps heatmap.py:20-36, putVecMaps paf.py:18-69, putJointZ posemap.py:83-106)
  Compose([Cvt2ndarray, Resize]) third_party_methods/lib/datasets/data_augmentation_2d3d.py:70-89,497-522
  Compose([Cvt2ndarray, Rotate, RenderDepth, Crop, Resize])   ...:411-448,283-350,94-128 -- the random training transform
  Compose([Cvt2ndarray, Rotate(), RenderDepth(), Hflip(swap), Crop(), Resize])   ...:452-493 -- the ITOP trainers' transform; the single-person
                                 batches without composition (itop_batch, itop_batch_yolo, ItopSet) mirror datasets_itop_rtpose.py / datasets_itop.py
Dataset constants (depth clamp and normalisation, augmentation defaults) come from a `profile=` argument (popnet_amd/profiles.py, default MP3DHP).
The arithmetic lives in csrc/targets.hip (pn_compose_depth, pn_rasterize_targets), csrc/augment.hip (pn_augment_resize) and
csrc/api.hip (pn_preprocess); this module only owns tensors and the call order.  There is no CPU fallback: images must be device
tensors.  The random transform's LABEL half (15 joints per person) and its integer geometry are host work, in numpy, mirroring the
reference operation for operation so that every dtype rounds the same way.
"""
import ctypes as C
import random

import numpy as np
import torch

from . import _lib, a2j_crops, profiles, warp_affine
from .config import DEPTH_MAX, DEPTH_MEAN, DEPTH_STD

NUM_JOINTS, NUM_LIMBS = 15, 14


def _ctx(device):
    return _lib.Context.for_device(torch.device(device).index or 0)


def _input_xy(input_size):
    """input_size: one int (square) or (input_x, input_y)"""
    if isinstance(input_size, (tuple, list)):
        input_x, input_y = input_size
        return int(input_x), int(input_y)
    return int(input_size), int(input_size)


def target_cfg(input_size=224, stride=8, z_radius=2, sigma=7.0, profile=None):
    """profile (popnet_amd.profiles, None = MP3DHP): the depth clamp and normalisation of the z maps."""
    prof = profiles.get(profile)
    cfg = _lib.TargetCfg()
    _lib.lib().pn_target_cfg_default(C.byref(cfg))
    cfg.input_x, cfg.input_y = _input_xy(input_size)
    cfg.stride, cfg.z_radius, cfg.sigma = int(stride), int(z_radius), float(sigma)
    cfg.depth_max, cfg.depth_mean, cfg.depth_std = float(prof.depth_max), float(prof.depth_mean), float(prof.depth_std)
    return cfg


def compose_depth(fg_depth, fg_mask, n_src, bg, depth_max=DEPTH_MAX):
    """z-buffer composition of up to S source frames per output frame (:231-266).
    fg_depth [B,S,H,W] float16/float32 metres, fg_mask [B,S,H,W] uint8 (0/1), n_src [B] int32 (sources used), bg [B,H,W]
    (same dtype as fg_depth) -> [B,H,W] float32."""
    for t, n in ((fg_depth, "fg_depth"), (fg_mask, "fg_mask"), (n_src, "n_src"), (bg, "bg")):
        _lib.require_cuda_tensor(t, n)
    if fg_depth.dtype not in (torch.float16, torch.float32) or bg.dtype != fg_depth.dtype:
        raise _lib.PopnetError("compose_depth: fg_depth / bg must both be float16 or float32")
    if fg_mask.dtype != torch.uint8 or n_src.dtype != torch.int32:
        raise _lib.PopnetError("compose_depth: fg_mask must be uint8 and n_src int32")
    B, S, H, W = fg_depth.shape
    if fg_mask.shape != fg_depth.shape or bg.shape != (B, H, W) or n_src.shape != (B,):
        raise _lib.PopnetError("compose_depth: shape mismatch")
    fg_depth, fg_mask, bg, n_src = fg_depth.contiguous(), fg_mask.contiguous(), bg.contiguous(), n_src.contiguous()
    out = torch.empty((B, H, W), dtype=torch.float32, device=fg_depth.device)
    ctx = _ctx(fg_depth.device)
    dt = _lib.PN_DEPTH_F16 if fg_depth.dtype == torch.float16 else _lib.PN_DEPTH_F32
    ctx.check(_lib.lib().pn_compose_depth(ctx.handle, C.c_void_p(fg_depth.data_ptr()), C.c_void_p(fg_mask.data_ptr()),
                                          C.c_void_p(n_src.data_ptr()), C.c_void_p(bg.data_ptr()), dt, B, S, H, W, float(depth_max),
                                          C.c_void_p(out.data_ptr()), _lib.current_stream_ptr(fg_depth.device)), "pn_compose_depth")
    return out


def compose_bg(fg_depth, fg_mask, bg):
    """The single-person loader's background swap (datasets_kdh3d_rtpose.py:227-234): fg_mask > 0 ? fg_depth : bg per pixel, with no
    z-buffer and no 2 * depth_max cap (compose_depth with one source cuts a foreground pixel beyond the cap; this keeps it).
    fg_depth, bg [B,H,W] float16 / float32 metres (same dtype), fg_mask [B,H,W] uint8 -> [B,H,W] float32."""
    for t, n in ((fg_depth, "fg_depth"), (fg_mask, "fg_mask"), (bg, "bg")):
        _lib.require_cuda_tensor(t, n)
    if fg_depth.dtype not in (torch.float16, torch.float32) or bg.dtype != fg_depth.dtype:
        raise _lib.PopnetError("compose_bg: fg_depth / bg must both be float16 or float32")
    if fg_mask.dtype != torch.uint8:
        raise _lib.PopnetError("compose_bg: fg_mask must be uint8")
    if fg_depth.dim() != 3 or fg_mask.shape != fg_depth.shape or bg.shape != fg_depth.shape:
        raise _lib.PopnetError("compose_bg: shape mismatch")
    B, H, W = fg_depth.shape
    fg_depth, fg_mask, bg = fg_depth.contiguous(), fg_mask.contiguous(), bg.contiguous()
    out = torch.empty((B, H, W), dtype=torch.float32, device=fg_depth.device)
    ctx = _ctx(fg_depth.device)
    dt = _lib.PN_DEPTH_F16 if fg_depth.dtype == torch.float16 else _lib.PN_DEPTH_F32
    ctx.check(_lib.lib().pn_compose_bg(ctx.handle, C.c_void_p(fg_depth.data_ptr()), C.c_void_p(fg_mask.data_ptr()), C.c_void_p(bg.data_ptr()), dt,
                                       B, H, W, C.c_void_p(out.data_ptr()), _lib.current_stream_ptr(fg_depth.device)), "pn_compose_bg")
    return out


def rasterize_targets(kp2d, kp_z, n_persons, depth_resize, input_size=224, stride=8, z_radius=2, sigma=7.0, profile=None):
    """get_ground_truth for a batch.  kp2d [B,P,15,2] float32 (network-input pixels), kp_z [B,P,15] float64 (metres), n_persons [B]
    int32, depth_resize [B,h,w] float32 -> (heat [B,16,h,w], paf [B,28,h,w], z [B,15,h,w], fg [B,15,h,w]) float32.
    input_size: an int, or (input_x, input_y) for a network input that is not square; h = input_y // stride, w = input_x // stride."""
    for t, n in ((kp2d, "kp2d"), (kp_z, "kp_z"), (n_persons, "n_persons"), (depth_resize, "depth_resize")):
        _lib.require_cuda_tensor(t, n)
    if kp2d.dtype != torch.float32 or kp_z.dtype != torch.float64 or n_persons.dtype != torch.int32 or depth_resize.dtype != torch.float32:
        raise _lib.PopnetError("rasterize_targets: kp2d float32, kp_z float64, n_persons int32, depth_resize float32")
    B, P = kp2d.shape[0], kp2d.shape[1]
    input_x, input_y = _input_xy(input_size)
    gh, gw = int(input_y / stride), int(input_x / stride)
    if kp2d.shape != (B, P, NUM_JOINTS, 2) or kp_z.shape != (B, P, NUM_JOINTS) or n_persons.shape != (B,) or depth_resize.shape != (B, gh, gw):
        raise _lib.PopnetError("rasterize_targets: shape mismatch")
    dev = kp2d.device
    if P == 0:      # nobody annotated anywhere in the batch: one dummy slot that n_persons = 0 never reads
        kp2d, kp_z, P = torch.zeros((B, 1, NUM_JOINTS, 2), dtype=torch.float32, device=dev), torch.zeros((B, 1, NUM_JOINTS), dtype=torch.float64, device=dev), 1
    kp2d, kp_z, n_persons, depth_resize = kp2d.contiguous(), kp_z.contiguous(), n_persons.contiguous(), depth_resize.contiguous()
    heat = torch.empty((B, NUM_JOINTS + 1, gh, gw), dtype=torch.float32, device=dev)
    paf = torch.empty((B, 2 * NUM_LIMBS, gh, gw), dtype=torch.float32, device=dev)
    z = torch.empty((B, NUM_JOINTS, gh, gw), dtype=torch.float32, device=dev)
    fg = torch.empty((B, NUM_JOINTS, gh, gw), dtype=torch.float32, device=dev)
    cfg = target_cfg(input_size, stride, z_radius, sigma, profile)
    ctx = _ctx(dev)
    ctx.check(_lib.lib().pn_rasterize_targets(ctx.handle, C.c_void_p(kp2d.data_ptr()), C.c_void_p(kp_z.data_ptr()), C.c_void_p(n_persons.data_ptr()),
                                              B, P, C.c_void_p(depth_resize.data_ptr()), C.byref(cfg), C.c_void_p(heat.data_ptr()),
                                              C.c_void_p(paf.data_ptr()), C.c_void_p(z.data_ptr()), C.c_void_p(fg.data_ptr()),
                                              _lib.current_stream_ptr(dev)), "pn_rasterize_targets")
    return heat, paf, z, fg


def yolo_target_cfg(input_size=224, stride_prior=16, anchors=((6., 3.), (12., 6.)), num_joints=NUM_JOINTS, noobject_scale=0.1, object_scale=1.0,
                    profile=None):
    prof = profiles.get(profile)
    cfg = _lib.YoloTargetCfg()
    _lib.lib().pn_yolo_target_cfg_default(C.byref(cfg))
    if not 1 <= len(anchors) <= _lib.PN_YOLO_MAX_ANCHORS:
        raise _lib.PopnetError("prior_targets: 1 to %d anchors" % _lib.PN_YOLO_MAX_ANCHORS)
    cfg.input_x = cfg.input_y = int(input_size)
    cfg.stride_prior, cfg.num_joints, cfg.num_anchors = int(stride_prior), int(num_joints), len(anchors)
    for a, (aw, ah) in enumerate(anchors):
        cfg.anchors[a][0], cfg.anchors[a][1] = float(aw), float(ah)
    cfg.noobject_scale, cfg.object_scale = float(noobject_scale), float(object_scale)
    cfg.depth_mean, cfg.depth_std = float(prof.depth_mean), float(prof.depth_std)
    return cfg


def prior_targets(boxes, kp2d, kp_z, pose_weight, n_persons, input_size=224, stride_prior=16, anchors=((6., 3.), (12., 6.)), noobject_scale=0.1,
                  object_scale=1.0, profile=None):
    """The YOLO training targets of a batch: build_prior_targets + bbox_ious (tpm/lib/datasets/datasets_kdh3d_mpaug.py:353-417,505-533, CR),
    fed like get_ground_truth feeds it (:556-585).  boxes [B,P,4] float64 (x0, y0, x1, y1 in network-input pixels, as Resize leaves
    ann['bbox']), kp2d [B,P,J,2] float32 (network-input pixels), kp_z [B,P,J] float64 (metres), pose_weight [B,P] float64, n_persons [B]
    int32 -> (prior_map [B,A(5+3J),g,g], prior_mask_conf, prior_mask_coord, prior_weight_map [B,A,g,g]) float32, g = int(input / stride_prior)."""
    for t, n in ((boxes, "boxes"), (kp2d, "kp2d"), (kp_z, "kp_z"), (pose_weight, "pose_weight"), (n_persons, "n_persons")):
        _lib.require_cuda_tensor(t, n)
    if (boxes.dtype != torch.float64 or kp2d.dtype != torch.float32 or kp_z.dtype != torch.float64 or pose_weight.dtype != torch.float64
            or n_persons.dtype != torch.int32):
        raise _lib.PopnetError("prior_targets: boxes float64, kp2d float32, kp_z float64, pose_weight float64, n_persons int32")
    B, P = kp2d.shape[0], kp2d.shape[1]
    J = kp2d.shape[2] if kp2d.dim() == 4 else -1
    if (kp2d.dim() != 4 or kp2d.shape[3] != 2 or boxes.shape != (B, P, 4) or kp_z.shape != (B, P, J) or pose_weight.shape != (B, P)
            or n_persons.shape != (B,) or B < 1):
        raise _lib.PopnetError("prior_targets: shape mismatch")
    dev = kp2d.device
    cfg = yolo_target_cfg(input_size, stride_prior, anchors, J, noobject_scale, object_scale, profile)
    A = len(anchors)
    g = int(input_size / stride_prior)
    boxes, kp2d, kp_z, pose_weight, n_persons = (t.contiguous() for t in (boxes, kp2d, kp_z, pose_weight, n_persons))
    prior = torch.empty((B, A * (5 + 3 * J), g, g), dtype=torch.float32, device=dev)
    conf, coord, weight = (torch.empty((B, A, g, g), dtype=torch.float32, device=dev) for _ in range(3))
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None      # noqa: E731
    ctx = _ctx(dev)
    ctx.check(_lib.lib().pn_build_prior_targets(ctx.handle, ptr(boxes), ptr(kp2d), ptr(kp_z), ptr(pose_weight), ptr(n_persons), B, P, C.byref(cfg),
                                                ptr(prior), ptr(conf), ptr(coord), ptr(weight), _lib.current_stream_ptr(dev)), "pn_build_prior_targets")
    return prior, conf, coord, weight


def _resize(frames, S, depth_max):
    """cv2.resize(INTER_LINEAR) to S x S + the [0, depth_max] clamp, un-normalised (pn_preprocess with mean 0, std 1)."""
    B, H, W = frames.shape
    out = torch.empty((B, 1, S, S), dtype=torch.float32, device=frames.device)
    ctx = _ctx(frames.device)
    ctx.check(_lib.lib().pn_preprocess(ctx.handle, C.c_void_p(frames.data_ptr()), _lib.PN_DEPTH_F32, B, H, W, C.c_void_p(out.data_ptr()), S,
                                       float(depth_max), 0.0, 1.0, _lib.current_stream_ptr(frames.device)), "pn_preprocess")
    return out[:, 0]


def augmentation(rot, a, crops, H, W, cx, cy, input_size=224, hflip=False, swap_indices=None):
    """One item's random transform from explicit values: rot (degrees, Rotate), a (the ratio RenderDepth draws), crops = (left, right,
    top, bottom) fractions (Crop), for H x W frames with the intrinsics' principal point (cx, cy).  -> dict with the values, the
    forward rotation matrix (labels), the inverted one (image, for the kernel) and every integer the chain derives:
      render_corner   (new_xmin, new_ymin, new_xmax, new_ymax) of RenderDepth, int() truncated;   render_a  a recomputed from them
      render_x/_y/_w/_h   the render image in the rotated frame (slice with numpy's clamping for a <= 1, zero image with the frame
                      pasted at (dy, dx) otherwise);   crop_bounds   (xmin, ymin, xmax, ymax) of Crop;   crop_x0.. the clamped slice
      src_w, src_h    the size Resize sees.
    hflip: Hflip's coin came up (data_augmentation_2d3d.py:452-493, between RenderDepth and Crop): the render image is mirrored left to
    right; swap_indices (the profile's get_swap_part_indices()) is then required -- the labels' left / right joints trade places.
    crops=None: the chain has no Crop (the composed test set's Compose([Cvt2ndarray, Rotate, RenderDepth, Resize]),
    evaluation_rtpose_light3d_kdh3d_mpaug_ablation.py:118-123): Resize reads the whole render image, crop_bounds = (0, 0, render_w, render_h).
    Nothing here touches the GPU.  A geometry the reference itself cannot run (the paste does not fit, an empty image) raises."""
    rot, a_drawn, crops = float(rot), float(a), None if crops is None else tuple(float(c) for c in crops)
    hflip = bool(hflip)
    if hflip and (swap_indices is None or sorted(int(i) for i in swap_indices) != list(range(NUM_JOINTS))):
        raise _lib.PopnetError("augmentation: hflip needs swap_indices, a permutation of the %d joints" % NUM_JOINTS)
    cx, cy, H, W = float(cx), float(cy), int(H), int(W)
    # getRotationMatrix2D: the centre is a Point2f; alpha, beta in double.  This and the inversion below (warp_affine.py, shared with A2J's
    # crop-level warp) are the product's own copy of what tests/cv2_warp_reference.py restates; tests/test_augment_reference.py compares
    # inv_mat with that restatement, and the exact-rational derivation of tests/test_cv2_warp_kat.py pins the restatement -- through that
    # equality it guards this copy too.
    fwd = warp_affine.rotation_matrix((cx, cy), rot, 1.0)
    m = warp_affine.invert_affine(fwd)      # warpAffine's inversion, in its operation order (imgwarp.cpp)
    # RenderDepth (data_augmentation_2d3d.py:303-335)
    xmin, ymin, xmax, ymax = float(0), float(0), float(W), float(H)
    new_xmin, new_ymin = int(a_drawn * (xmin - cx) + cx), int(a_drawn * (ymin - cy) + cy)
    new_xmax, new_ymax = int(a_drawn * (xmax - cx) + cx), int(a_drawn * (ymax - cy) + cy)
    ax, ay = (new_xmin - cx) / (xmin - cx), (new_ymin - cy) / (ymin - cy)
    a = (ax + ay) / 2
    if a <= 1:
        y0, y1, _ = slice(new_ymin, new_ymax).indices(H)
        x0, x1, _ = slice(new_xmin, new_xmax).indices(W)
        render_x, render_y, render_w, render_h = x0, y0, max(x1 - x0, 0), max(y1 - y0, 0)
    else:
        dx, dy = int(xmin - new_xmin), int(ymin - new_ymin)
        render_w, render_h = new_xmax - new_xmin + 1, new_ymax - new_ymin + 1
        fits = render_w > 0 and render_h > 0
        if fits:
            y0, y1, _ = slice(dy, dy + H).indices(render_h)
            x0, x1, _ = slice(dx, dx + W).indices(render_w)
            fits = (y0, y1 - y0, x0, x1 - x0) == (dy, H, dx, W)
        if not fits:
            raise _lib.PopnetError("augmentation: RenderDepth with a = %r cannot paste the %dx%d frame at (%d, %d) into its %dx%d image "
                                   "(the reference raises here too)" % (a_drawn, W, H, dx, dy, render_w, render_h))
        render_x, render_y = -dx, -dy
    if render_w < 1 or render_h < 1:
        raise _lib.PopnetError("augmentation: RenderDepth with a = %r leaves an empty image" % a_drawn)
    if crops is None:
        # no Crop in the chain (the evaluation scripts' Compose): Resize sees the whole render image.  Zero fractions are NOT this: Crop's
        # xmax = w - 1 still drops the last row and column
        c_xmin, c_ymin, c_xmax, c_ymax = 0, 0, render_w, render_h
        cx0, cy0, cx1, cy1 = 0, 0, render_w, render_h
    else:
        # Crop (:102-118) on the render image
        c_xmin, c_ymin = int(min(crops[0] * render_w, render_w)), int(min(crops[2] * render_h, render_h))
        c_xmax, c_ymax = int(max(render_w - 1 - crops[1] * render_w, 0)), int(max(render_h - 1 - crops[3] * render_h, 0))
        cy0, cy1, _ = slice(c_ymin, c_ymax).indices(render_h)
        cx0, cx1, _ = slice(c_xmin, c_xmax).indices(render_w)
    if crops is not None and (cx1 - cx0 < 1 or cy1 - cy0 < 1):      # (without Crop the source is the render image, checked above)
        raise _lib.PopnetError("augmentation: Crop %r leaves an empty image" % (crops,))
    return dict(rot=rot, a=a_drawn, crops=crops, cx=cx, cy=cy, H=H, W=W, input_size=int(input_size), rot_mat=fwd, inv_mat=tuple(m),
                render_corner=(new_xmin, new_ymin, new_xmax, new_ymax), render_a=a, render_x=render_x, render_y=render_y,
                render_w=render_w, render_h=render_h, crop_bounds=(c_xmin, c_ymin, c_xmax, c_ymax), crop_x0=cx0, crop_y0=cy0,
                crop_x1=cx1, crop_y1=cy1, src_w=cx1 - cx0, src_h=cy1 - cy0, hflip=hflip,
                swap_indices=[int(i) for i in swap_indices] if hflip else None)


def draw_augmentation(H, W, cx, cy, min_ratio=0.7, max_ratio=1.7, max_crop=0.1, input_size=224, hflip=False, swap_indices=None, crop=True):
    """Draws one item's transform from Python's `random` in the reference's order -- Rotate: uniform(-10, 10); RenderDepth:
    uniform(min_ratio, max_ratio); with hflip (the ITOP trainers' Hflip) the coin uniform(0, 1) >= 0.5; Crop: four uniform(0, max_crop)
    for left, right, top, bottom -- and derives its geometry.  Without hflip no coin is drawn: the six draws of the MP-3DHP chain.
    crop=False: the chain without Crop (augmentation(crops=None)); its four draws are not made, the others are, in the same order."""
    rot = random.uniform(-10, 10)
    a = random.uniform(min_ratio, max_ratio)
    flip = (random.uniform(0, 1) >= 0.5) if hflip else False
    crops = tuple(random.uniform(0, max_crop) for _ in range(4)) if crop else None
    return augmentation(rot, a, crops, H, W, cx, cy, input_size, hflip=flip, swap_indices=swap_indices if flip else None)


class AugmentationBatch:
    """The transforms of a batch's items (dicts of augmentation()): the pn_augment_item records for the image kernel and the host
    transform of the labels."""

    def __init__(self, items):
        self.items = list(items)
        if not self.items:
            raise _lib.PopnetError("AugmentationBatch: no items")
        self.H, self.W, self.input_size = self.items[0]["H"], self.items[0]["W"], self.items[0]["input_size"]
        if any((it["H"], it["W"], it["input_size"]) != (self.H, self.W, self.input_size) for it in self.items):
            raise _lib.PopnetError("AugmentationBatch: the items of a batch share the frame size and the input size")
        self.records = (_lib.AugmentItem * len(self.items))()
        for r, it in zip(self.records, self.items):
            r.m[:] = it["inv_mat"]
            r.scale = float(np.float32(it["render_a"]))
            for k in ("render_x", "render_y", "render_w", "render_h", "crop_x0", "crop_y0", "crop_x1", "crop_y1", "src_w", "src_h"):
                setattr(r, k, it[k])
            r.hflip = 1 if it.get("hflip") else 0

    def __len__(self):
        return len(self.items)

    def transform_labels(self, kp2d_org, kp3d, boxes=None, visible=None):
        """kp2d_org [B,P,15,2] float32 (original pixels), kp3d [B,P,15,3] float64, boxes [B,P,4] float64 (original pixels) or None, as
        host arrays -> (kp2d [B,P,15,2] float32 in network-input pixels, kp_z [B,P,15] float64, boxes [B,P,4] float64 or None).
        visible [B,P,15] ('visible_joints') or None: when given, a fourth result, the array with Hflip's left / right swap applied.
        Hflip (items whose coin came up), after RenderDepth and before Crop, the reference's rule as written: x' = -x + width with width
        the render image's width (NOT width - 1: one pixel off the mirrored pixel centre), then the left / right swap of the joints and
        of visible_joints, bbox = [-x1 + width, y0, -x0 + width, y1]; 3D X is not negated and the 3D joints are not swapped
        (is_3d=False), so kp_z stays in the order of the labels.
        Rotate: homographic_transform of the float32 joints by the float64 3x3 (lib/utils/common.py:96-104), assigned back to float32;
        boxes are NOT rotated, as in the reference.  RenderDepth: minus its corner, z times the recomputed a (float64).  Crop: minus its
        corner.  Resize: times S / w, S / h of the item (float32 joints times a Python float; boxes in float64).  Padding slots are
        transformed like persons; nobody reads them."""
        kp = np.array(kp2d_org, dtype=np.float32)
        kz = np.array(np.asarray(kp3d)[..., 2], dtype=np.float64)
        bx = None if boxes is None else np.array(boxes, dtype=np.float64)
        vs = None if visible is None else np.array(visible)
        if kp.shape[0] != len(self.items):
            raise _lib.PopnetError("AugmentationBatch: %d items for a batch of %d" % (len(self.items), kp.shape[0]))
        for b, it in enumerate(self.items):
            M = np.vstack([it["rot_mat"], [0, 0, 1]])
            ox, oy = it["render_corner"][0], it["render_corner"][1]
            qx, qy = it["crop_bounds"][0], it["crop_bounds"][1]
            wr, hr = float(it["input_size"]) / it["src_w"], float(it["input_size"]) / it["src_h"]
            for p in range(kp.shape[1]):
                j = kp[b, p]
                x, y = j[:, 0], j[:, 1]
                trans = np.matmul(M, np.vstack([x, y, np.ones_like(y)]))
                j[:, 0], j[:, 1] = trans[0, :] / trans[2, :], trans[1, :] / trans[2, :]
                j[:, 0] -= ox
                j[:, 1] -= oy
                if it.get("hflip"):
                    j[:, 0] = - j[:, 0] + it["render_w"]
                    j[:] = j[it["swap_indices"], :]
                    if vs is not None:
                        vs[b, p] = vs[b, p][it["swap_indices"]]
                j[:, 0] -= qx
                j[:, 1] -= qy
                j[:, 0] *= wr
                j[:, 1] *= hr
            kz[b] *= it["render_a"]
            if bx is not None:
                bx[b, :, 0:4:2] -= ox
                bx[b, :, 1:4:2] -= oy
                if it.get("hflip"):
                    xmin, xmax = -bx[b, :, 2] + it["render_w"], -bx[b, :, 0] + it["render_w"]
                    bx[b, :, 0], bx[b, :, 2] = xmin, xmax
                bx[b, :, 0:4:2] -= qx
                bx[b, :, 1:4:2] -= qy
                bx[b, :, 0:4:2] = bx[b, :, 0:4:2] * wr
                bx[b, :, 1:4:2] = bx[b, :, 1:4:2] * hr
        return (kp, kz, bx) if visible is None else (kp, kz, bx, vs)


def composed_ground_truth(kp2d, kp3d, kp_z, n_persons, w_org, h_org, input_size=224):
    """The ground truth the composed-test-set scripts collect per frame (evaluation_rtpose_light3d_kdh3d_mpaug_ablation.py:176-189) from
    transform_labels' results: kp2d [B,P,15,2] float32 (network-input pixels) scaled back with `*= w_org / input_size`, `*= h_org /
    input_size` on the float32 array, and the labels' 3D joints kp3d [B,P,15,3] with the depth RenderDepth scaled (kp_z [B,P,15]; X and
    Y stay as labelled).  -> (human_gt_set_2d, human_gt_set_3d): per frame a list of its n_persons[b] persons' [15][2] / [15][3] lists."""
    kp = np.array(kp2d, dtype=np.float32)
    kp[..., 0] *= (w_org / input_size)
    kp[..., 1] *= (h_org / input_size)
    k3 = np.array(kp3d, dtype=np.float64)
    k3[..., 2] = np.asarray(kp_z, dtype=np.float64)
    n = [int(v) for v in _host(n_persons)]
    return [kp[b, :n[b]].tolist() for b in range(len(n))], [k3[b, :n[b]].tolist() for b in range(len(n))]


def augment_resize(frames, aug, input_size=224, depth_max=None, mean=0.0, std=1.0, profile=None):
    """depth_max=None: the clamp of the dataset profile (popnet_amd.profiles; None = MP3DHP, 6 m).  Items with Hflip set mirror their
    render image inside the same launch.
    Rotate -> RenderDepth -> [Hflip ->] Crop -> Resize -> clamp to [0, depth_max] -> (x - mean) / std of composed frames [B,H,W] float32 (device)
    with the per-item transforms of `aug` (AugmentationBatch): ONE launch for the batch (pn_augment_resize).  -> [B,1,S,S] float32.
    An item that Resize would decimate by exactly 2 in both axes is refused with a PopnetError naming it: cv2.resize(INTER_LINEAR)
    switches to INTER_AREA there, which is not built (as in pn_preprocess).  With the MP-3DHP geometry (480 x 512 frames, S = 224,
    a in [0.7, 1.7], crops up to 0.1) this cannot occur: a crop that is 448 wide needs a >= 0.93, which leaves at least 477 rows."""
    _lib.require_cuda_tensor(frames, "frames")
    if depth_max is None:
        depth_max = profiles.get(profile).depth_max
    if frames.dtype != torch.float32 or frames.dim() != 3:
        raise _lib.PopnetError("augment_resize: frames must be [B,H,W] float32")
    B, H, W = frames.shape
    if len(aug) != B or (aug.H, aug.W) != (H, W) or aug.input_size != int(input_size):
        raise _lib.PopnetError("augment_resize: the augmentation was drawn for %d items of %dx%d -> %d, the call has %d of %dx%d -> %d"
                               % (len(aug), aug.W, aug.H, aug.input_size, B, W, H, int(input_size)))
    frames = frames.contiguous()
    items = torch.empty(C.sizeof(aug.records), dtype=torch.uint8, device=frames.device)      # the call uploads the records it has checked
    out = torch.empty((B, 1, int(input_size), int(input_size)), dtype=torch.float32, device=frames.device)
    ctx = _ctx(frames.device)
    ctx.check(_lib.lib().pn_augment_resize(ctx.handle, C.c_void_p(frames.data_ptr()), C.cast(aug.records, C.c_void_p), C.c_void_p(items.data_ptr()),
                                           B, H, W, C.c_void_p(out.data_ptr()), int(input_size), float(depth_max), float(mean), float(std),
                                           _lib.current_stream_ptr(frames.device)), "pn_augment_resize")
    return out


def _host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def mpaug_batch(fg_depth, fg_mask, n_src, bg, kp2d_org, kp3d, n_persons, input_size=224, stride=8, z_radius=2, aug=None):
    """A batch of training items as KDH3D_Keypoints.__getitem__ builds them for given source choices.  kp2d_org [B,P,15,2] float32 in
    ORIGINAL pixel coordinates, kp3d [B,P,15,3] float64 metres.  Returns image [B,1,S,S] (normalised), heat, paf, z, fg.
    aug=None: the evaluation transform Compose([Cvt2ndarray, Resize]); the labels are device tensors.
    aug (AugmentationBatch): the random training transform Compose([Cvt2ndarray, Rotate, RenderDepth, Crop, Resize]) -- the image
    through one pn_augment_resize launch, the labels through the host transform, the rest as without it.  Hand kp2d_org / kp3d over
    as HOST arrays then (MPAugTrainSet.batch(augment=True) returns them so).  Device tensors are accepted, but reading them back is
    a device synchronisation in the middle of the batch."""
    if aug is not None:
        image = compose_depth(fg_depth, fg_mask, n_src, bg)
        img224 = augment_resize(image, aug, input_size, DEPTH_MAX)[:, 0]
        depth_resize = _resize(img224, int(input_size / stride), 3.0e38)
        kp, kz, _ = aug.transform_labels(_host(kp2d_org), _host(kp3d))
        dev = image.device
        heat, paf, z, fg = rasterize_targets(torch.from_numpy(kp).to(dev), torch.from_numpy(kz).to(dev), n_persons.to(dev), depth_resize,
                                             input_size, stride, z_radius)
        x = ((img224 - float(DEPTH_MEAN)) / float(DEPTH_STD)).unsqueeze(1)
        return x, heat, paf, z, fg
    _lib.require_cuda_tensor(kp2d_org, "kp2d_org")
    _lib.require_cuda_tensor(kp3d, "kp3d")
    image = compose_depth(fg_depth, fg_mask, n_src, bg)
    H, W = image.shape[1:]
    img224 = _resize(image, input_size, DEPTH_MAX)                       # Resize + the clamp of __getitem__ :277-278
    depth_resize = _resize(img224, int(input_size / stride), 3.0e38)     # cv2.resize of the clamped input (:347); no second clamp there
    kp = kp2d_org.to(torch.float32).clone()
    kp[..., 0] *= float(input_size) / W                                  # Resize.__call__: float32 array times a Python float
    kp[..., 1] *= float(input_size) / H
    heat, paf, z, fg = rasterize_targets(kp, kp3d[..., 2].to(torch.float64).contiguous(), n_persons, depth_resize, input_size, stride, z_radius)
    x = ((img224 - float(DEPTH_MEAN)) / float(DEPTH_STD)).unsqueeze(1)
    return x, heat, paf, z, fg


def mpaug_batch_yolo(fg_depth, fg_mask, n_src, bg, kp2d_org, kp3d, n_persons, boxes, pose_weight, input_size=224, aug=None):
    """mpaug_batch for the YoloPoseNet trainer (datasets_kdh3d_mpaug.py:245-340 (CR), evaluation transform): the same composed, resized and
    normalised image, and the prior targets of its persons.  boxes [B,P,4] float64 already scaled to input_size (MPAugTrainSet.batch(...,
    with_boxes=True)).  Returns image [B,1,S,S], prior_map, prior_mask_conf, prior_mask_coord, prior_weight_map.
    aug (AugmentationBatch): the random training transform, as in mpaug_batch (host arrays for the labels; device tensors force a
    synchronisation); boxes are then in ORIGINAL pixels (float64, as MPAugTrainSet.batch(with_boxes=True, augment=True) returns
    them) and take the offsets and scales of the joints, but not the rotation."""
    if aug is not None:
        image = compose_depth(fg_depth, fg_mask, n_src, bg)
        img = augment_resize(image, aug, input_size, DEPTH_MAX)[:, 0]
        kp, kz, bx = aug.transform_labels(_host(kp2d_org), _host(kp3d), _host(boxes))
        dev = image.device
        prior = prior_targets(torch.from_numpy(bx).to(dev), torch.from_numpy(kp).to(dev), torch.from_numpy(kz).to(dev), pose_weight.to(dev),
                              n_persons.to(dev), input_size)
        x = ((img - float(DEPTH_MEAN)) / float(DEPTH_STD)).unsqueeze(1)
        return (x,) + prior
    _lib.require_cuda_tensor(kp2d_org, "kp2d_org")
    _lib.require_cuda_tensor(kp3d, "kp3d")
    image = compose_depth(fg_depth, fg_mask, n_src, bg)
    H, W = image.shape[1:]
    img = _resize(image, input_size, DEPTH_MAX)
    kp = kp2d_org.to(torch.float32).clone()
    kp[..., 0] *= float(input_size) / W
    kp[..., 1] *= float(input_size) / H
    prior = prior_targets(boxes, kp, kp3d[..., 2].to(torch.float64).contiguous(), pose_weight, n_persons, input_size)
    x = ((img - float(DEPTH_MEAN)) / float(DEPTH_STD)).unsqueeze(1)
    return (x,) + prior


AUG_MODS = [[0, 3], [1, 2], [0, 1], [2, 3], [4]]    # datasets_kdh3d_rtpose_mpaug.py:51 -- which annotation sets may share a frame


class MPAugSampler:
    """The random control flow of KDH3D_Keypoints.__getitem__ (:231-262) on the host: which source frames join item `index`.
    The dataset holds several annotation sets (one list of ids each); a random entry of aug_mods names the sets that may
    contribute, each joins with probability 0.8 (`uniform(0, 1) > 0.8: continue`), set ii contributes its frame
    index % len(ids[ii]); when nobody joined one random set is taken; the background is index % n_backgrounds.  Draws from
    Python's `random` in the reference's order (randint, then one uniform per candidate, then randint), so that a seeded run
    picks the same sources as the reference does.  With augment=True each item's six augmentation draws (draw_augmentation) follow
    that item's source draws, because the reference interleaves them inside __getitem__."""

    def __init__(self, set_sizes, n_backgrounds, aug_mods=AUG_MODS, p_join=0.8):
        self.set_sizes, self.n_backgrounds, self.aug_mods, self.p_join = list(set_sizes), int(n_backgrounds), [list(m) for m in aug_mods], p_join
        self.max_sources = max(len(m) for m in self.aug_mods)

    def sources(self, index):
        """-> ([(set, frame-in-set), ...], background id)"""
        mod = self.aug_mods[random.randint(0, len(self.aug_mods) - 1)]
        src = []
        for ii in mod:
            if random.uniform(0, 1) > self.p_join:
                continue
            src.append((ii, index % self.set_sizes[ii]))
        if not src:
            ii = random.randint(0, len(self.set_sizes) - 1)
            src.append((ii, index % self.set_sizes[ii]))
        return src, index % self.n_backgrounds

    def batch(self, indices, augment=False, **aug_args):
        """-> (src [B,S,2] int64 (set, frame) padded with -1, n_src [B] int32, bg [B] int64) for the caller's gather.
        augment=True: aug_args are draw_augmentation's (H, W, cx, cy, ...), and the AugmentationBatch of the items comes fourth."""
        picks, items = [], []
        for i in indices:
            picks.append(self.sources(i))
            if augment:
                items.append(draw_augmentation(**aug_args))
        if augment:
            return self._arrays(picks) + (AugmentationBatch(items),)
        return self._arrays(picks)

    def test_batch(self, batch_size, dataset_len, **aug_args):
        """The draws of generate_test_batch (datasets_kdh3d_rtpose_mpaug.py:431-476): per item the index FIRST
        (random.randint(0, dataset_len - 1)), then its source draws, then its augmentation draws (draw_augmentation(**aug_args); the
        evaluation scripts' chain has no Crop: pass crop=False).  -> (indices [B] int64, src, n_src, bg, AugmentationBatch)."""
        indices, picks, items = [], [], []
        for _ in range(int(batch_size)):
            index = random.randint(0, int(dataset_len) - 1)
            indices.append(index)
            picks.append(self.sources(index))
            items.append(draw_augmentation(**aug_args))
        return (np.array(indices, dtype=np.int64),) + self._arrays(picks) + (AugmentationBatch(items),)

    def _arrays(self, picks):
        src = np.full((len(picks), self.max_sources, 2), -1, dtype=np.int64)
        for r, (s, _) in enumerate(picks):
            src[r, :len(s)] = s
        return src, np.array([len(s) for s, _ in picks], dtype=np.int32), np.array([b for _, b in picks], dtype=np.int64)


class MPAugTrainSet:
    """The files behind KDH3D_Keypoints of the mpaug trainer (datasets_kdh3d_rtpose_mpaug.py:166-221 (CR)): several annotation
    sets (`labels_*.json`: image id -> list of persons with `2d_joints` / `3d_joints`, plus `intrinsics`), depth frames and
    foreground masks as `<id>` .npy files under img_dir / seg_dir, background frames listed in bg_file.  `batch(indices)` draws
    the sources like the reference (MPAugSampler), loads them on the host and returns DEVICE tensors ready for mpaug_batch:
    (fg_depth [B,S,H,W], fg_mask [B,S,H,W] uint8, n_src [B], bg [B,H,W], kp2d_org [B,P,15,2], kp3d [B,P,15,3], n_persons [B]).
    The id lists are shuffled once at construction like the reference's (random.shuffle)."""

    def __init__(self, img_dir, ann_file_list, bg_file, bg_dir, seg_dir, device="cuda:0", shuffle=True):
        import json
        self.img_dir, self.bg_dir, self.seg_dir, self.device = img_dir, bg_dir, seg_dir, torch.device(device)
        self.annos, self.ids = [], []
        for f in ann_file_list:
            a = json.load(open(f, "r"))
            ids = [k for k in a if k != "intrinsics"]
            if shuffle:
                random.shuffle(ids)
            self.annos.append(a)
            self.ids.append(ids)
        self.bg = list(json.load(open(bg_file, "r")).values())
        if shuffle:
            random.shuffle(self.bg)
        self.sampler = MPAugSampler([len(i) for i in self.ids], len(self.bg), aug_mods=[m for m in AUG_MODS if max(m) < len(self.ids)] or [[0]])
        self.max_sources = self.sampler.max_sources
        self._hw = None

    def __len__(self):
        return max(len(i) for i in self.ids)              # dataset_len (:181)

    def _principal_point(self):
        """cx, cy of the annotation files' `intrinsics` (Rotate and RenderDepth turn and scale about it); every file must name the same."""
        pts = set()
        for a in self.annos:
            intr = a.get("intrinsics")
            if not intr or "cx" not in intr or "cy" not in intr:
                raise KeyError("MPAugTrainSet.batch(augment=True): every annotation file needs 'intrinsics' with 'cx' and 'cy' (Rotate and RenderDepth turn and scale about the principal point)")
            pts.add((float(intr["cx"]), float(intr["cy"])))
        if len(pts) != 1:
            raise _lib.PopnetError("MPAugTrainSet.batch(augment=True): the annotation files disagree on the principal point: %s" % sorted(pts))
        return pts.pop()

    def _frame_size(self):
        """(H, W) of the dataset's frames, needed before an item's transform can be drawn: read once from the first background's header
        and kept; batch() checks every batch against it."""
        if self._hw is None:
            import os
            self._hw = tuple(np.load(os.path.join(self.bg_dir, self.bg[0]["file_name"]), mmap_mode="r").shape)
        return self._hw

    def batch(self, indices, with_boxes=False, input_size=224, augment=False, max_aug_ratio=1.7, crop=True):
        """with_boxes: also return boxes [B,P,4] float64 (ann['bbox'] scaled by Resize to input_size, in float64 like
        data_augmentation_2d3d.py:497-522) and pose_weight [B,P] float64 (ann['pose_weight']) -- the YoloPoseNet trainer's extra inputs.
        augment: draw the random training transform of every item (Rotate / RenderDepth(max_ratio=max_aug_ratio) / Crop about the
        `intrinsics` cx, cy of the first annotation file, interleaved with the source draws like the reference's __getitem__) and
        append the batch's AugmentationBatch as the LAST element, for mpaug_batch(..., aug=) / mpaug_batch_yolo(..., aug=).  The
        labels then stay on the host (kp2d_org, kp3d and boxes as numpy arrays: their transform is host work) and boxes stay in
        ORIGINAL pixels, because the transform's offsets come before its scale.  crop=False: the chain without Crop (draw_augmentation)."""
        if augment:
            cx, cy = self._principal_point()
            H0, W0 = self._frame_size()
            src, n_src, bg_id, aug = self.sampler.batch(indices, augment=True, H=H0, W=W0, cx=cx, cy=cy, max_ratio=float(max_aug_ratio),
                                                        input_size=input_size, crop=crop)
        else:
            src, n_src, bg_id, aug = self.sampler.batch(indices) + (None,)
        return self._load(src, n_src, bg_id, aug, with_boxes, input_size)

    def test_batch(self, batch_size, input_size=224, max_aug_ratio=1.7, with_boxes=False):
        """A batch of the composed TEST set as generate_test_batch draws it (datasets_kdh3d_rtpose_mpaug.py:415-488): random indices, each
        followed by its source draws and the two draws of the evaluation scripts' chain Rotate / RenderDepth(max_ratio=max_aug_ratio) /
        Resize -- no Crop.  Returns what batch(augment=True) returns (labels on the host, the AugmentationBatch last)."""
        cx, cy = self._principal_point()
        H0, W0 = self._frame_size()
        _, src, n_src, bg_id, aug = self.sampler.test_batch(batch_size, len(self), H=H0, W=W0, cx=cx, cy=cy, max_ratio=float(max_aug_ratio),
                                                            input_size=input_size, crop=False)
        return self._load(src, n_src, bg_id, aug, with_boxes, input_size)

    def _load(self, src, n_src, bg_id, aug, with_boxes, input_size):
        import os
        augment = aug is not None
        B, S = len(n_src), self.max_sources
        frames, masks, bgs, persons = [], [], [], []
        for b in range(B):
            fr, mk, pp = [], [], []
            for s in range(int(n_src[b])):
                ii, f = int(src[b, s, 0]), int(src[b, s, 1])
                image_id = self.ids[ii][f]
                fr.append(np.load(os.path.join(self.img_dir, image_id)))
                mk.append(np.load(os.path.join(self.seg_dir, image_id)))
                pp += self.annos[ii][image_id]
            bgs.append(np.load(os.path.join(self.bg_dir, self.bg[int(bg_id[b])]["file_name"])))
            frames.append(fr)
            masks.append(mk)
            persons.append(pp)
        H, W = bgs[0].shape
        dt = np.float16 if bgs[0].dtype == np.float16 and all(f.dtype == np.float16 for fr in frames for f in fr) else np.float32
        fd = np.zeros((B, S, H, W), dtype=dt)
        fm = np.zeros((B, S, H, W), dtype=np.uint8)
        P = max(1, max(len(p) for p in persons))
        k2 = np.zeros((B, P, NUM_JOINTS, 2), dtype=np.float32)
        k3 = np.zeros((B, P, NUM_JOINTS, 3), dtype=np.float64)
        npers = np.zeros(B, dtype=np.int32)
        for b in range(B):
            for s, (f, m) in enumerate(zip(frames[b], masks[b])):
                fd[b, s], fm[b, s] = f, (np.asarray(m) > 0)
            npers[b] = len(persons[b])
            for p, ann in enumerate(persons[b]):
                k2[b, p] = np.asarray(ann["2d_joints"], dtype=np.float32)
                k3[b, p] = np.asarray(ann["3d_joints"], dtype=np.float64)
        dev = self.device
        t = lambda a: torch.from_numpy(a).to(dev, non_blocking=True)      # noqa: E731
        if augment and (H, W) != (aug.H, aug.W):
            raise _lib.PopnetError("MPAugTrainSet.batch: frames of %dx%d after a background of %dx%d" % (W, H, aug.W, aug.H))
        out = (t(fd), t(fm), t(n_src), t(np.stack(bgs).astype(dt)), k2 if augment else t(k2), k3 if augment else t(k3), t(npers))
        if not with_boxes:
            return out + ((aug,) if augment else ())
        boxes = np.zeros((B, P, 4), dtype=np.float64)
        pw = np.zeros((B, P), dtype=np.float64)
        for b in range(B):
            for p, ann in enumerate(persons[b]):
                missing = [k for k in ("bbox", "pose_weight") if k not in ann]
                if missing:
                    raise KeyError("MPAugTrainSet.batch(with_boxes=True): an annotation lacks %s -- the YoloPoseNet trainer needs "
                                   "'bbox' ([x0, y0, x1, y1], original pixels) and 'pose_weight' on every person" % " and ".join(repr(k) for k in missing))
                bb = np.asarray(ann["bbox"], dtype=np.float64)
                if augment:
                    boxes[b, p] = bb
                else:
                    boxes[b, p, 0:4:2] = bb[0:4:2] * (float(input_size) / W)   # Resize: x by the width ratio, y by the height ratio (float64)
                    boxes[b, p, 1:4:2] = bb[1:4:2] * (float(input_size) / H)
                pw[b, p] = float(ann["pose_weight"])
        return out + ((boxes, t(pw), aug) if augment else (t(boxes), t(pw)))


# ---- single-person datasets without composition (ITOP) ---------------------------------------------------------------------------
JOINT2BOX_MARGIN = 25      # datasets_itop.py: the prior box is the joints' bounding box grown by this many network-input pixels


def _single_image(frames, aug, input_size, prof):
    """The image half of ItopKeypoints.__getitem__ (datasets_itop_rtpose.py:213-223, datasets_itop.py:239-251): frames [B,H,W] float16 /
    float32 (device) as stored, widened to float32 (Cvt2ndarray), through Resize or the random chain, clamped to [0, depth_max].
    -> [B,S,S] float32, un-normalised."""
    _lib.require_cuda_tensor(frames, "frames")
    if frames.dim() != 3 or frames.dtype not in (torch.float16, torch.float32):
        raise _lib.PopnetError("frames must be a [B,H,W] float16 / float32 tensor")
    frames = frames.to(torch.float32).contiguous()
    if aug is not None:
        return augment_resize(frames, aug, input_size, prof.depth_max)[:, 0]
    return _resize(frames, input_size, prof.depth_max)


def _single_labels(frames, kp2d_org, kp3d, aug, input_size, boxes=None):
    """The label half: Resize alone (float32 joints times a Python float) or the random chain's host transform.  -> host arrays
    (kp2d [B,1,15,2] float32, kp_z [B,1,15] float64)."""
    B, H, W = frames.shape
    k2 = np.array(_host(kp2d_org), dtype=np.float32).reshape(B, 1, NUM_JOINTS, 2)
    k3 = np.array(_host(kp3d), dtype=np.float64).reshape(B, 1, NUM_JOINTS, 3)
    if aug is not None:
        kp, kz, _ = aug.transform_labels(k2, k3)
        return kp, kz
    k2[..., 0] *= float(input_size) / W
    k2[..., 1] *= float(input_size) / H
    return k2, np.ascontiguousarray(k3[..., 2])


def itop_batch(frames, kp2d_org, kp3d, input_size=224, stride=8, z_radius=2, aug=None, profile=None):
    """A batch of Open-Pose+ training items of a single-person dataset as datasets_itop_rtpose.ItopKeypoints.__getitem__ builds them
    (mpaug_batch minus the composition: the frames are used as they are).  frames [B,H,W] float16 / float32 (device), kp2d_org [B,15,2]
    original pixels, kp3d [B,15,3] metres (host arrays or tensors; their transform is host work).  aug=None: Compose([Cvt2ndarray, Resize]);
    aug (AugmentationBatch): Compose([Cvt2ndarray, Rotate(), RenderDepth(), Hflip(swap), Crop(), Resize]) -- the image through one
    pn_augment_resize launch.  The maps follow the ITOP loader: joints are kept by the in-bounds test alone (remove_illegal_joint);
    visible_joints does not gate them; the z maps clamp at the profile's depth_max (5 m).  get_ground_truth of that file mixes
    self.joint_names / self.JOINT_NAMES and uses self.strideA / self.align_radius, which do not exist: with the names fixed and the unused
    PoseAlign maps left out it is the kdh3d loader's get_ground_truth with depth_max = 5, which pn_rasterize_targets computes.
    profile=None: ITOP.  Returns image [B,1,S,S] (normalised), heat, paf, z, fg."""
    prof = profiles.ITOP if profile is None else profiles.get(profile)
    img = _single_image(frames, aug, input_size, prof)
    depth_resize = _resize(img, int(input_size / stride), 3.0e38)
    kp, kz = _single_labels(frames, kp2d_org, kp3d, aug, input_size)
    dev = img.device
    n = torch.ones((img.shape[0],), dtype=torch.int32, device=dev)
    heat, paf, z, fg = rasterize_targets(torch.from_numpy(kp).to(dev), torch.from_numpy(kz).to(dev), n, depth_resize, input_size, stride, z_radius,
                                         profile=prof)
    x = ((img - float(prof.depth_mean)) / float(prof.depth_std)).unsqueeze(1)
    return x, heat, paf, z, fg


def joints_box(kp2d, margin=JOINT2BOX_MARGIN):
    """The prior box of the ITOP loader (datasets_itop.py:429-430): [min x - margin, min y - margin, max x + margin, max y + margin] over
    ALL joints of the transformed labels.  The margin is added in float32 (a float32 extreme and a Python int: float32 under NumPy 2's
    promotion rules, which is how the reference's line runs today); the box then enters the float64 object row."""
    k = np.asarray(kp2d, dtype=np.float32)
    lo, hi = k.min(axis=-2) - np.float32(margin), k.max(axis=-2) + np.float32(margin)
    return np.concatenate([lo, hi], axis=-1).astype(np.float64)


def itop_batch_yolo(frames, kp2d_org, kp3d, pose_weight=None, input_size=224, aug=None, profile=None):
    """itop_batch for the YoloPoseNet trainer (datasets_itop.ItopKeypoints): the same image and the prior targets of its one person.  The box
    is joints_box of the transformed joints (the loader never reads ann['bbox']); pose_weight [B] or None = 1.0 for everybody
    (datasets_itop.py:425-428).  Returns image [B,1,S,S], prior_map, prior_mask_conf, prior_mask_coord, prior_weight_map."""
    prof = profiles.ITOP if profile is None else profiles.get(profile)
    img = _single_image(frames, aug, input_size, prof)
    kp, kz = _single_labels(frames, kp2d_org, kp3d, aug, input_size)
    B, dev = img.shape[0], img.device
    pw = np.ones((B, 1), dtype=np.float64) if pose_weight is None else np.array(_host(pose_weight), dtype=np.float64).reshape(B, 1)
    n = torch.ones((B,), dtype=torch.int32, device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    prior = prior_targets(t(joints_box(kp)), t(kp), t(kz), t(pw), n, input_size, profile=prof)
    x = ((img - float(prof.depth_mean)) / float(prof.depth_std)).unsqueeze(1)
    return (x,) + prior


class ItopSet:
    """The files of the ITOP side-view splits (datasets_itop_rtpose.py:171-178, datasets_itop.py:177-181): `annotations/ITOP_side_{train,test}
    _labels.json` maps an image id to a list of persons ('2d_joints' [15][2], '3d_joints' [15][3], 'visible_joints' [15], optionally 'bbox'
    and 'pose_weight'); the frame of id X is `<img_dir>/X.npy`, 240 x 320 float16 metres.  An 'intrinsics' entry is skipped.  `batch(indices)`
    loads the frames and the FIRST person's labels (the dataset is single-person) for itop_batch / itop_batch_yolo."""

    def __init__(self, img_dir, ann_file, device="cuda:0", profile=None):
        import json
        self.img_dir, self.device = img_dir, torch.device(device)
        self.profile = profiles.ITOP if profile is None else profiles.get(profile)
        self.anno_dic = json.load(open(ann_file, "r"))
        self.ids = [k for k in self.anno_dic if k != "intrinsics"]

    def __len__(self):
        return len(self.ids)

    def load(self, index):
        import os
        a = np.load(os.path.join(self.img_dir, self.ids[index] + ".npy"))
        if a.ndim != 2:
            raise _lib.PopnetError("%s: expected one [H, W] depth frame, got shape %s" % (self.ids[index], a.shape))
        return a if a.dtype in (np.float16, np.float32) else a.astype(np.float32)

    def ground_truth(self):
        """(human_gt_set_2d, human_gt_set_3d) in frame order, as the evaluation scripts collect them."""
        return ([[p["2d_joints"] for p in self.anno_dic[k]] for k in self.ids], [[p["3d_joints"] for p in self.anno_dic[k]] for k in self.ids])

    def batches(self, indices, batch_size, drop_last=False):
        """Yields (index list, host array [b, H, W]) like dataset.MP3DHPFrames.batches."""
        indices = list(indices)
        for s in range(0, len(indices), batch_size):
            chunk = indices[s:s + batch_size]
            if drop_last and len(chunk) < batch_size:
                return
            yield chunk, np.stack([self.load(i) for i in chunk])

    def batch(self, indices, input_size=224, augment=False):
        """-> (frames [B,H,W] device, kp2d_org [B,15,2] float32, kp3d [B,15,3] float64, visible [B,15], pose_weight [B] float64) -- host arrays
        but the frames -- and, with augment=True, the batch's AugmentationBatch drawn with the profile's trainer defaults as the last element."""
        frames = np.stack([self.load(i) for i in indices])
        first = [self.anno_dic[self.ids[i]][0] for i in indices]
        k2 = np.array([np.asarray(p["2d_joints"], dtype=np.float32).reshape(NUM_JOINTS, 2) for p in first])
        k3 = np.array([np.asarray(p["3d_joints"], dtype=np.float64).reshape(NUM_JOINTS, 3) for p in first])
        vis = np.array([np.asarray(p.get("visible_joints", [1] * NUM_JOINTS)).reshape(NUM_JOINTS) for p in first])
        pw = np.array([float(p.get("pose_weight", 1.0)) for p in first], dtype=np.float64)
        out = (torch.from_numpy(frames).to(self.device, non_blocking=True), k2, k3, vis, pw)
        if not augment:
            return out
        H, W = frames.shape[1:]
        a = self.profile.aug
        cx, cy = self.profile.aug_centre(H, W)
        items = [draw_augmentation(H, W, cx, cy, min_ratio=a["min_ratio"], max_ratio=a["max_ratio"], max_crop=a["max_crop"], input_size=input_size,
                                   hflip=a["hflip"], swap_indices=self.profile.swap_indices) for _ in indices]
        return out + (AugmentationBatch(items),)


class ItopA2JSet(ItopSet):
    """The ITOP side-view split as the A2J trainer reads it (A2J_experiments/itop_train_64.py:88-185): the frames and labels of ItopSet plus
    `center_{train,test}.txt`, one line `u v depth` per frame.  keypoints [N,15,3] float32 are the FIRST person's '3d_joints' (the script's
    keypointsUVD: u, v, depth), lefttop / rightbottom the boxes of a2j_crops.itop_boxes.
    A line containing `invalid` drops THAT FRAME from the set.  (The reference compacts the centre list only, which silently pairs every
    later frame and label with the wrong centre.)
    `batch(indices, draws)` -> (frames [B,H,W] device, pn_a2j_crop_item records, labels [B,15,3] float32 host) for A2JEngine.train_crops."""

    def __init__(self, img_dir, ann_file, centre_file, device="cuda:0"):
        super().__init__(img_dir, ann_file, device=device)
        self.centres, kept, n = a2j_crops.read_centres(centre_file)
        if n != len(self.ids):
            raise _lib.PopnetError("%s has %d lines (invalid ones included), %s has %d frames" % (centre_file, n, ann_file, len(self.ids)))
        self.ids = [self.ids[i] for i in kept]
        self.keypoints = np.asarray([self.anno_dic[k][0]["3d_joints"] for k in self.ids], dtype=np.float32).reshape(-1, NUM_JOINTS, 3)
        self.lefttop, self.rightbottom = a2j_crops.itop_boxes(self.centres)

    def batch(self, indices, draws=None, crop=288):
        """draws: one A2JCropSampler.draw() per item (augment=True) or None (augment=False)."""
        frames = np.stack([self.load(i) for i in indices])
        items, labels = a2j_crops.itop_items(list(indices), self.centres, self.lefttop, self.rightbottom, self.keypoints, frames.shape[1:], draws=draws,
                                             crop_w=crop, crop_h=crop)
        return torch.from_numpy(frames).to(self.device, non_blocking=True), items, labels


class KDH3DSingleSet:
    """The files of the single-person KDH3D sets (`val`, and `test_bgaug` with bg_aug=True) as datasets_kdh3d_rtpose.KDH3D_Keypoints reads them
    (:161-180, :222-234): one annotation file (image id -> list of persons; an 'intrinsics' entry is skipped), the frame of id X is
    `<img_dir>/X`.  bg_aug: the frame's foreground (`<seg_dir>/X`, > 0) is pasted over background index % n_bg of bg_file's list, which is
    shuffled once at construction (random.shuffle, as the reference does) -- compose_bg, not the z-buffer composition.
    `inputs(indices)` returns the network input [B,1,S,S] (device): Resize, the clamp and the normalisation of __getitem__ in one
    pn_preprocess launch.
    boxes=True: the arrays the A2J trainers build at import (A2J_experiments/train_a2j_base.py:70-103) from the FIRST person of every frame --
    bndbox [N,4], keypoints_2d [N,15,2], keypoints_3d [N,15,3] float32 -- for `crop_batch`."""

    def __init__(self, img_dir, ann_file, bg_aug=False, bg_file=None, bg_dir=None, seg_dir=None, device="cuda:0", profile=None, shuffle=True, boxes=False):
        import json
        self.img_dir, self.bg_dir, self.seg_dir, self.device = img_dir, bg_dir, seg_dir, torch.device(device)
        self.profile = profiles.get(profile)
        self.anno_dic = json.load(open(ann_file, "r"))
        self.ids = [k for k in self.anno_dic if k != "intrinsics"]
        if boxes:
            first = [self.anno_dic[k][0] for k in self.ids]
            self.bndbox = np.asarray([p["bbox"] for p in first], dtype=np.float32).reshape(-1, 4)
            self.keypoints_2d = np.asarray([p["2d_joints"] for p in first], dtype=np.float32).reshape(-1, NUM_JOINTS, 2)
            self.keypoints_3d = np.asarray([p["3d_joints"] for p in first], dtype=np.float32).reshape(-1, NUM_JOINTS, 3)
        self.bg_aug = bool(bg_aug)
        self.bg = []
        if self.bg_aug:
            if not (bg_file and bg_dir and seg_dir):
                raise _lib.PopnetError("KDH3DSingleSet(bg_aug=True) needs bg_file, bg_dir and seg_dir")
            self.bg = list(json.load(open(bg_file, "r")).values())
            if shuffle:
                random.shuffle(self.bg)

    def __len__(self):
        return len(self.ids)

    def ground_truth(self, indices=None):
        """(human_gt_set_2d, human_gt_set_3d) of the frames `indices` (None = all), as the evaluation scripts collect them (:164-171)."""
        ids = self.ids if indices is None else [self.ids[i] for i in indices]
        return ([[p["2d_joints"] for p in self.anno_dic[k]] for k in ids], [[p["3d_joints"] for p in self.anno_dic[k]] for k in ids])

    def frames(self, indices):
        """-> [B,H,W] float32 (device): the stored frames, with the background swapped in when bg_aug."""
        import os
        dev = self.device
        fg = np.stack([np.load(os.path.join(self.img_dir, self.ids[i])) for i in indices])
        dt = np.float16 if fg.dtype == np.float16 else np.float32
        if not self.bg_aug:
            return torch.from_numpy(fg.astype(dt)).to(dev).to(torch.float32)
        mask = np.stack([np.asarray(np.load(os.path.join(self.seg_dir, self.ids[i]))) > 0 for i in indices]).astype(np.uint8)
        bg = np.stack([np.load(os.path.join(self.bg_dir, self.bg[i % len(self.bg)]["file_name"])) for i in indices])
        if bg.dtype != np.float16:
            dt = np.float32
        return compose_bg(torch.from_numpy(fg.astype(dt)).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(bg.astype(dt)).to(dev))

    def crop_batch(self, indices, draws=None, crop=288, img_wh=None):
        """boxes=True sets only: the A2J trainers' item (train_a2j_base.py / train_a2j_bgaug_new.py dataPreprocess) -> (frames [B,H,W] float32
        device -- with the background swapped in when bg_aug --, pn_a2j_crop_item records, labels [B,15,3] float32 host) for
        A2JEngine.train_crops.  draws: one A2JCropSampler('box').draw() per item (augment=True) or None."""
        if not hasattr(self, "bndbox"):
            raise _lib.PopnetError("KDH3DSingleSet.crop_batch needs boxes=True at construction")
        frames = self.frames(indices)
        items, labels = a2j_crops.box_items(list(indices), self.bndbox, self.keypoints_2d, self.keypoints_3d, frames.shape[1:], draws=draws,
                                            crop_w=crop, crop_h=crop, img_wh=img_wh)
        return frames, items, labels

    def inputs(self, indices, input_size=224, frames=None):
        """frames: what frames(indices) returned, when the caller has it already."""
        frames = self.frames(indices) if frames is None else frames
        B, H, W = frames.shape
        out = torch.empty((B, 1, int(input_size), int(input_size)), dtype=torch.float32, device=frames.device)
        p = self.profile
        ctx = _ctx(frames.device)
        ctx.check(_lib.lib().pn_preprocess(ctx.handle, C.c_void_p(frames.data_ptr()), _lib.PN_DEPTH_F32, B, H, W, C.c_void_p(out.data_ptr()),
                                           int(input_size), float(p.depth_max), float(p.depth_mean), float(p.depth_std),
                                           _lib.current_stream_ptr(frames.device)), "pn_preprocess")
        return out
