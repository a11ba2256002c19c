"""ctypes binding of libpopnet_hip.so (the C ABI declared in include/popnet_hip.h).

There is NO fallback: if the HIP library is missing or fails to load, importing any compute entry
point of this package raises.  The library is built in-tree by ``popnet_amd/build.py`` (or
``__graft_entry__.build()``).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("POPNET_LIB_PATH") or os.path.join(_HERE, "libpopnet_hip.so")      # the override is for kernel experiments (variant builds)

PN_OK = 0
PN_PREC_F32, PN_PREC_BF16, PN_PREC_BF16X3 = 0, 1, 2
PN_NET_RTPOSE_LIGHT3D, PN_NET_YOLO_POSENET, PN_NET_A2J = 0, 1, 2
PN_DEPTH_F16, PN_DEPTH_F32, PN_DEPTH_NET = 0, 1, 2

PN_NUM_JOINTS = 15
PN_NUM_LIMBS = 14
PN_MAX_PEAKS_PER_JOINT = 32
PN_MAX_PEAKS = PN_NUM_JOINTS * PN_MAX_PEAKS_PER_JOINT
PN_MAX_PERSONS = 32
PN_YOLO_MAX_DET = 64
PN_PLAN_FORWARD, PN_PLAN_DGRAD, PN_PLAN_DGRAD_STRIDED, PN_PLAN_WGRAD = 0, 1, 2, 3
PN_FRAME_OVERFLOW_PEAKS, PN_FRAME_OVERFLOW_PERSONS = 1, 2


class PopnetError(RuntimeError):
    pass


class TargetCfg(C.Structure):
    """pn_target_cfg"""
    _fields_ = [("input_x", C.c_int), ("input_y", C.c_int), ("stride", C.c_int), ("z_radius", C.c_int),
                ("sigma", C.c_double), ("depth_max", C.c_double), ("depth_mean", C.c_double), ("depth_std", C.c_double)]


PN_YOLO_MAX_ANCHORS = 8


class YoloTargetCfg(C.Structure):
    """pn_yolo_target_cfg"""
    _fields_ = [("input_x", C.c_int), ("input_y", C.c_int), ("stride_prior", C.c_int), ("num_joints", C.c_int), ("num_anchors", C.c_int),
                ("anchors", (C.c_double * 2) * PN_YOLO_MAX_ANCHORS), ("noobject_scale", C.c_double), ("object_scale", C.c_double),
                ("depth_mean", C.c_double), ("depth_std", C.c_double)]


class AugmentItem(C.Structure):
    """pn_augment_item"""
    _fields_ = [("m", C.c_double * 6), ("scale", C.c_float), ("render_x", C.c_int), ("render_y", C.c_int), ("render_w", C.c_int),
                ("render_h", C.c_int), ("crop_x0", C.c_int), ("crop_y0", C.c_int), ("crop_x1", C.c_int), ("crop_y1", C.c_int),
                ("src_w", C.c_int), ("src_h", C.c_int), ("hflip", C.c_int)]


class A2JCropItem(C.Structure):
    """pn_a2j_crop_item"""
    _fields_ = [("m", C.c_double * 6), ("frame", C.c_int), ("cy0", C.c_int), ("cx0", C.c_int), ("ih", C.c_int), ("iw", C.c_int),
                ("sh", C.c_int), ("sw", C.c_int), ("padded", C.c_int), ("start1", C.c_float), ("start2", C.c_float), ("end1", C.c_float),
                ("end2", C.c_float), ("window", C.c_int), ("hi", C.c_float), ("lo", C.c_float), ("fill", C.c_float), ("sub", C.c_float),
                ("scale", C.c_float), ("warp", C.c_int)]


class NmsOpt(C.Structure):
    """pn_nms_opt"""
    _fields_ = [("upsample", C.c_int), ("refine_center", C.c_int), ("gaussian_filt", C.c_int)]


class ParseCfg(C.Structure):
    """pn_parse_cfg"""
    _fields_ = [("thresh_heatmap", C.c_float), ("thresh_paf", C.c_float),
                ("num_intermed_pts", C.c_int), ("downsample", C.c_int), ("input_size", C.c_int),
                ("w_org", C.c_int), ("h_org", C.c_int),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("depth_mean", C.c_float), ("depth_std", C.c_float),
                ("z_readout", C.c_int), ("z_chn", C.c_int * 15)]


PN_Z_READOUT_HEAT_WEIGHTED, PN_Z_READOUT_CELL = 0, 1

# numpy mirror of pn_pose_frame / pn_yolo_frame (align=True reproduces the C struct layout; the
# sizes are cross-checked against pn_sizeof_* at load time)
POSE_FRAME_DTYPE = np.dtype([
    ("n_persons", np.int32), ("n_peaks", np.int32), ("status", np.uint32), ("reserved", np.int32),
    ("peak_x", np.float32, (PN_MAX_PEAKS,)), ("peak_y", np.float32, (PN_MAX_PEAKS,)),
    ("peak_score", np.float32, (PN_MAX_PEAKS,)), ("peak_type", np.int32, (PN_MAX_PEAKS,)),
    ("person_joint", np.int32, (PN_MAX_PERSONS, PN_NUM_JOINTS)),
    ("person_score", np.float64, (PN_MAX_PERSONS,)),
    ("person_count", np.int32, (PN_MAX_PERSONS,)),
    ("joints_2d", np.float64, (PN_MAX_PERSONS, PN_NUM_JOINTS, 2)),
    ("joints_3d", np.float64, (PN_MAX_PERSONS, PN_NUM_JOINTS, 3)),
    ("part_conf", np.float64, (PN_MAX_PERSONS, PN_NUM_JOINTS)),
], align=True)

YOLO_FRAME_DTYPE = np.dtype([
    ("n_det", np.int32), ("n_candidates", np.int32), ("status", np.uint32), ("reserved", np.int32),
    ("bbox", np.float32, (PN_YOLO_MAX_DET, 5)),
    ("human", np.float32, (PN_YOLO_MAX_DET, PN_NUM_JOINTS, 3)),
    ("visibility", np.int32, (PN_YOLO_MAX_DET, PN_NUM_JOINTS)),
    ("joints_2d", np.float32, (PN_YOLO_MAX_DET, PN_NUM_JOINTS, 2)),
    ("joints_3d", np.float32, (PN_YOLO_MAX_DET, PN_NUM_JOINTS, 3)),
    ("bbox_org", np.float32, (PN_YOLO_MAX_DET, 4)),
], align=True)

PN_WIRE_MAX_PERSONS = 16
POSE_WIRE_DTYPE = np.dtype([
    ("n_persons", np.int32), ("status", np.uint32),
    ("person_joint", np.int16, (PN_WIRE_MAX_PERSONS, PN_NUM_JOINTS)),
    ("vals", np.float32, (PN_WIRE_MAX_PERSONS, PN_NUM_JOINTS, 6)),      # x, y (original frame), X, Y, Z (m), part confidence
], align=True)

_lib = None

_vp, _i, _f, _d, _sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t
_SIGNATURES = {
    "pn_abi_version": (_i, []),
    "pn_build_experiments": (_i, []),
    "pn_mfma_sustained": (_i, [_vp, _d, _i, C.POINTER(_d), C.POINTER(_d), _vp]),
    "pn_create": (_vp, [_i]),
    "pn_destroy": (None, [_vp]),
    "pn_last_error": (_i, [_vp, C.c_char_p, _sz]),
    "pn_preprocess": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _f, _f, _f, _vp]),
    "pn_net_create": (_vp, [_vp, _i, _i, _i, _i]),
    "pn_net_destroy": (None, [_vp]),
    "pn_net_set_tensor": (_i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    "pn_net_finalize": (_i, [_vp, _i, _i, _i, _i]),
    "pn_rtpose_forward": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "pn_yolo_forward": (_i, [_vp, _vp, _i, _vp, _vp]),
    "pn_rtpose_forward_frames": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _vp, _vp]),
    "pn_yolo_forward_frames": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f, _f, _vp, _vp]),
    "pn_net_read_activation": (_i, [_vp, C.c_char_p, _i, _vp, _sz, _vp]),
    "pn_net_copy_activation": (_i, [_vp, C.c_char_p, _i, _vp, _vp]),
    "pn_net_read_zero_page": (_i, [_vp, _i, _vp, _sz]),
    "pn_net_forward_partial": (_i, [_vp, _vp, _i, _i, _vp]),
    "pn_net_forward_frames_partial": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f, _f, _i, _vp]),
    "pn_net_num_steps": (_i, [_vp]),
    "pn_net_step_info": (_i, [_vp, _i, C.c_char_p, _sz]),
    "pn_conv_level_plan_info": (_i, [_vp] + [_i] * 8 + [_vp] * 4 + [C.c_char_p, _sz]),
    "pn_conv_has_instance": (_i, [_i] * 5),
    "pn_net_flops_per_frame": (_d, [_vp]),
    "pn_net_lock": (_i, [_vp, _i]),
    "pn_parse_reserve": (_i, [_vp, _i]),
    "pn_net_profile_begin": (_i, [_vp]),
    "pn_net_profile_end": (_i, [_vp, C.POINTER(_d), C.POINTER(C.c_int64), C.POINTER(_d), C.POINTER(_d), C.POINTER(C.c_int64)]),
    "pn_net_profile_kernel": (_i, [_vp, _i, C.c_char_p, _sz, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "pn_parse_cfg_default": (None, [C.POINTER(ParseCfg)]),
    "pn_parse_paf": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, C.POINTER(ParseCfg), _vp, _vp]),
    "pn_parse_paf_wire": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, C.POINTER(ParseCfg), _vp, _vp, _vp]),
    "pn_target_cfg_default": (None, [C.POINTER(TargetCfg)]),
    "pn_compose_depth": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "pn_compose_bg": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "pn_rasterize_targets": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, C.POINTER(TargetCfg), _vp, _vp, _vp, _vp, _vp]),
    "pn_sizeof_augment_item": (_sz, []),
    "pn_sizeof_parse_cfg": (_sz, []),
    "pn_augment_resize": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _f, _f, _f, _vp]),
    "pn_train_set_precision": (_i, [_vp, _i]),
    "pn_train_ws_keep": (_i, [_vp, _i]),
    "pn_train_pack_cache": (_i, [_vp, _i]),
    "pn_train_pack_refresh": (_i, [_vp, _vp]),
    "pn_conv2d_forward": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 9 + [_vp]),
    "pn_conv2d_dgrad": (_i, [_vp, _vp, _vp, _vp] + [_i] * 8 + [_vp]),
    "pn_conv2d_wgrad": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 8 + [_vp]),
    "pn_bn_train_forward": (_i, [_vp] * 10 + [_f, _f] + [_i] * 4 + [_vp]),
    "pn_bn_train_backward": (_i, [_vp] * 8 + [_i] * 4 + [_vp] * 4 + [_i, _vp]),
    "pn_avgpool3s2_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "pn_avgpool3s2_backward": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "pn_head_forward": (_i, [_vp, _vp, _vp, _vp] + [_i] * 4 + [_vp, _vp, _i, _vp, _vp]),
    "pn_head_backward": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 5 + [_vp, _vp]),
    "pn_slice_copy": (_i, [_vp, _vp, _i, _vp] + [_i] * 5 + [_vp]),
    "pn_sgd_nesterov": (_i, [_vp, _vp, _vp, _vp, C.c_size_t, _f, _f, _f, _i, _f, _vp]),
    "pn_train_conv_plan_info": (_i, [_vp] + [_i] * 9 + [C.c_char_p, _sz]),
    "pn_train_reduce_slices": (_i, [_vp, _i, _i, _i]),
    "pn_conv2d_dgrad_strided": (_i, [_vp, _vp, _vp, _vp] + [_i] * 9 + [_vp]),
    "pn_maxpool_forward": (_i, [_vp, _vp, _vp, _vp] + [_i] * 6 + [_vp]),
    "pn_maxpool_backward": (_i, [_vp, _vp, _vp, _vp] + [_i] * 6 + [_vp]),
    "pn_yolo_loss": (_i, [_vp] * 6 + [_i] * 5 + [_vp] * 4),
    "pn_conv2d_forward_dil": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 10 + [_vp]),
    "pn_conv2d_dgrad_dil": (_i, [_vp, _vp, _vp, _vp] + [_i] * 9 + [_vp]),
    "pn_conv2d_wgrad_dil": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 9 + [_vp]),
    "pn_a2j_loss": (_i, [_vp, _vp, _vp, _vp] + [_i] * 5 + [_vp, _vp, _f] + [_vp] * 6),
    "pn_adam": (_i, [_vp, _vp, _vp, _vp, _vp, C.c_size_t, _d, _d, _d, _d, _d, _i, _d, _vp]),
    "pn_conv1x1_x3_forward": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 5 + [_vp]),
    "pn_conv1x1_x3_dgrad": (_i, [_vp, _vp, _vp, _vp] + [_i] * 5 + [_vp]),
    "pn_conv1x1_x3_wgrad": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 4 + [_vp]),
    "pn_conv1x1_x3_plan_info": (_i, [_vp] + [_i] * 5 + [C.c_char_p, _sz]),
    "pn_yolo_target_cfg_default": (None, [C.POINTER(YoloTargetCfg)]),
    "pn_build_prior_targets": (_i, [_vp] * 6 + [_i, _i, C.POINTER(YoloTargetCfg)] + [_vp] * 5),
    "pn_trainer_create": (_vp, [_vp]),
    "pn_trainer_destroy": (None, [_vp]),
    "pn_trainer_set_precision": (_i, [_vp, _i]),
    "pn_trainer_set_param": (_i, [_vp, C.c_char_p, _sz, _sz]),
    "pn_trainer_set_stat": (_i, [_vp, C.c_char_p, _vp]),
    "pn_trainer_finalize": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _f]),
    "pn_trainer_forward_backward": (_i, [_vp] * 8),
    "pn_trainer_conv_flops": (_d, [_vp]),
    "pn_trainer_num_ops": (_i, [_vp]),
    "pn_trainer_op_info": (_i, [_vp, _i, C.c_char_p, _sz]),
    "pn_trainer_run_ops": (_i, [_vp] * 7 + [_i, _i, _vp]),
    "pn_trainer_read_tensor": (_i, [_vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "pn_trainer_write_tensor": (_i, [_vp, _i, _i, _i, _vp, _sz, _vp]),
    "pn_trainer_read_vector": (_i, [_vp, C.c_char_p, _vp, _sz, _vp]),
    "pn_retrieve_depth": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp]),
    "pn_nms_peaks": (_i, [_vp, _vp, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    "pn_nms_opt_default": (None, [C.POINTER(NmsOpt)]),
    "pn_nms_peaks_opt": (_i, [_vp, _vp, _i, _i, _i, _f, C.POINTER(NmsOpt), _vp, _vp, _vp, _vp, _vp]),
    "pn_parse_yolo": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(C.c_float), _i, _i, _i, _i, _f, _f, _f, _f, _i, C.POINTER(ParseCfg), _vp, _vp]),
    "pn_parse_paf_unbounded": (_i, [_vp, _vp, _vp, _vp, _i, _i, C.POINTER(ParseCfg), C.POINTER(C.c_int), C.POINTER(C.c_int), _vp]),
    "pn_parse_paf_unbounded_fetch": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn_parse_debug_connections": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "pn_parse_paf_unbounded_connections": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "pn_parse_yolo_predvis": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(C.c_float), _i, _i, _i, _i, _f, _f, _f, _f, _i, C.POINTER(ParseCfg), _vp, _vp, _vp]),
    "pn_ablation_pred_raw": (_i, [_vp, _vp, _i, _i, _i, _i, _f, C.POINTER(ParseCfg), _vp, _vp, _vp]),
    "pn_ablation_perfect_2d": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp, _i, _i, C.POINTER(ParseCfg), _vp, _vp, _i, _vp, _vp, _vp]),
    "pn_depth_probe": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _vp, _i, _vp, _vp]),
    "pn_sizeof_pose_frame": (_sz, []),
    "pn_pack_pose_frames": (_i, [_vp, _vp, _i, _vp, _vp]),
    "pn_sizeof_pose_wire": (_sz, []),
    "pn_sizeof_yolo_frame": (_sz, []),
    "pn_a2j_cfg_default": (None, [_vp]),
    "pn_sizeof_a2j_record": (_sz, []),
    "pn_a2j_crop": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "pn_a2j_forward": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "pn_a2j_head_shape": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "pn_a2j_vote": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn_a2j_predict": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn_sizeof_a2j_crop_item": (_sz, []),
    "pn_a2j_train_crop": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "pn_debug_cubic_coeffs": (None, [_f, C.POINTER(C.c_float)]),
    "process_paf": (_i, [_i, _i, _i, _vp, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    "get_num_humans": (_i, []),
    "get_part_cid": (_i, [_i, _i]),
    "get_score": (_f, [_i]),
    "get_part_x": (_i, [_i]),
    "get_part_y": (_i, [_i]),
    "get_part_score": (_f, [_i]),
}


def lib():
    """Loads (once) and returns the ctypes handle.  Raises PopnetError when the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PopnetError(
            "popnet_amd: %s not found -- the HIP extension is required (no CPU fallback). "
            "Build it with `python popnet_amd/build.py`." % LIB_PATH)
    try:
        handle = C.CDLL(LIB_PATH)
    except OSError as e:
        raise PopnetError("popnet_amd: cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(handle, name)      # AttributeError => ABI mismatch, let it surface
        fn.restype = res
        fn.argtypes = args
    if handle.pn_abi_version() != 1:
        raise PopnetError("popnet_amd: ABI version mismatch")
    if handle.pn_sizeof_pose_frame() != POSE_FRAME_DTYPE.itemsize:
        raise PopnetError("pn_pose_frame layout mismatch: C %d vs numpy %d"
                          % (handle.pn_sizeof_pose_frame(), POSE_FRAME_DTYPE.itemsize))
    if handle.pn_sizeof_pose_wire() != POSE_WIRE_DTYPE.itemsize:
        raise PopnetError("pn_pose_wire layout mismatch: C %d vs numpy %d" % (handle.pn_sizeof_pose_wire(), POSE_WIRE_DTYPE.itemsize))
    if handle.pn_sizeof_yolo_frame() != YOLO_FRAME_DTYPE.itemsize:
        raise PopnetError("pn_yolo_frame layout mismatch")
    if handle.pn_sizeof_augment_item() != C.sizeof(AugmentItem):
        raise PopnetError("pn_augment_item layout mismatch: C %d vs ctypes %d" % (handle.pn_sizeof_augment_item(), C.sizeof(AugmentItem)))
    if handle.pn_sizeof_a2j_crop_item() != C.sizeof(A2JCropItem):
        raise PopnetError("pn_a2j_crop_item layout mismatch: C %d vs ctypes %d" % (handle.pn_sizeof_a2j_crop_item(), C.sizeof(A2JCropItem)))
    if handle.pn_sizeof_parse_cfg() != C.sizeof(ParseCfg):
        raise PopnetError("pn_parse_cfg layout mismatch: C %d vs ctypes %d" % (handle.pn_sizeof_parse_cfg(), C.sizeof(ParseCfg)))
    _lib = handle
    return _lib


def declared_symbols():
    return sorted(_SIGNATURES)


class Context:
    """pn_ctx wrapper (one per device)."""
    _cache = {}

    def __init__(self, device_index):
        self.device_index = device_index
        self.handle = lib().pn_create(device_index)
        if not self.handle:
            raise PopnetError("pn_create failed")
        msg = self.last_error()
        if msg:
            raise PopnetError(msg)

    @classmethod
    def for_device(cls, device_index):
        ctx = cls._cache.get(device_index)
        if ctx is None:
            ctx = cls._cache[device_index] = cls(device_index)
        return ctx

    def __del__(self):                     # private contexts (engines that own their scratch) release it; the per-device ones live on
        try:
            if self.handle and Context._cache.get(self.device_index) is not self:
                lib().pn_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def last_error(self):
        buf = C.create_string_buffer(1024)
        lib().pn_last_error(self.handle, buf, 1024)
        return buf.value.decode()

    def check(self, rc, what):
        if rc != PN_OK:
            raise PopnetError("%s failed (%d): %s" % (what, rc, self.last_error()))


def require_cuda_tensor(t, name):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise PopnetError("popnet_amd: %s must be a CUDA/ROCm tensor -- the HIP path has no CPU fallback" % name)


def current_stream_ptr(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
