"""Dataset profiles: everything the engines, the target rasterisers, the augmentation and the scripts need to know about ONE dataset,
carried through every layer as a `profile=` argument (default MP3DHP: the constants of popnet_amd/config.py, unchanged).

  MP3DHP   util/util_functions.py:4,11-13, evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py (480 x 640 frames, the calibrated pinhole,
           depth clamp 6 m, joint depth = retrieve_depth_heat_weighted around the peak's cell, channel j for joint j)
  ITOP     lib/datasets/datasets_itop_rtpose.py:32-42, lib/datasets/datasets_itop.py, evaluation_rtpose_light3d_itop.py:176-209 (320 x 240
           frames, f = 1 / 0.0035, centre (160, 120), depth clamp 5 m, ONE person per frame, joint depth = the one cell under the peak of
           channel joint2chn[j], 3D Y flipped)

ITOP flips 3D Y: Y = -(y - cy) z / f.  The profile carries that as fy = -f: IEEE division is sign-symmetric, (y - cy) z / (-f) has the bits
of -((y - cy) z / f), which has the bits of the reference's (-(y - cy)) z / f -- no kernel branch.
"""
from . import _lib
from . import config as _config

Z_READOUT_HEAT_WEIGHTED, Z_READOUT_CELL = 0, 1      # PN_Z_READOUT_* of include/popnet_hip.h


def kp_connections(keypoints):
    """datasets_itop_rtpose.py:45-62 (== util/util_functions.py:17-34): the 14 limbs as [source, destination] joint indices."""
    pairs = [('torso', 'right_hip'), ('right_hip', 'right_knee'), ('right_knee', 'right_ankle'), ('torso', 'left_hip'), ('left_hip', 'left_knee'),
             ('left_knee', 'left_ankle'), ('torso', 'neck'), ('neck', 'right_shoulder'), ('right_shoulder', 'right_elbow'),
             ('right_elbow', 'right_wrist'), ('neck', 'left_shoulder'), ('left_shoulder', 'left_elbow'), ('left_elbow', 'left_wrist'), ('neck', 'head')]
    return [[keypoints.index(a), keypoints.index(b)] for a, b in pairs]


def joint2chn(keypoints, limbs, root_joint='torso'):
    """get_joint2chn (datasets_itop_rtpose.py:65-76): the root joint reads channel 0, the destination joint of limb k channel k + 1."""
    out = [0] * len(keypoints)
    out[keypoints.index(root_joint)] = 0
    for k, limb in enumerate(limbs):
        out[limb[1]] = k + 1
    return out


def swap_part_indices(keypoints):
    """get_swap_part_indices (datasets_itop_rtpose.py:100-154): every 'left_x' trades places with 'right_x', the rest stay."""
    def other(name):
        if name.startswith('left_'):
            return 'right_' + name[5:]
        if name.startswith('right_'):
            return 'left_' + name[6:]
        return name
    return [keypoints.index(other(k)) for k in keypoints]


class Profile:
    """One dataset.  intrinsics: fx, fy, cx, cy (fy negative where the dataset flips 3D Y).  z_chn: the pose-depth channel the CELL
    read-out takes for joint j (the evaluation script's joint2chn); the HEAT_WEIGHTED read-out reads channel j, as its script does.
    aug: the defaults of the dataset's trainers for draw_augmentation (centre None = width / 2, height / 2, as Rotate() and RenderDepth()
    do without arguments)."""

    def __init__(self, name, w_org, h_org, intrinsics, depth_mean, depth_std, depth_max, keypoints, root_joint, single_person, z_readout,
                 identity_z_chn, aug):
        self.name, self.w_org, self.h_org = name, int(w_org), int(h_org)
        self.intrinsics = dict(intrinsics)
        self.depth_mean, self.depth_std, self.depth_max = depth_mean, depth_std, depth_max
        self.keypoints = list(keypoints)
        self.limbs = kp_connections(self.keypoints)
        self.root_joint = root_joint
        self.joint2chn = joint2chn(self.keypoints, self.limbs, root_joint)
        self.swap_indices = swap_part_indices(self.keypoints)
        self.single_person = bool(single_person)
        self.z_readout = int(z_readout)
        self.z_chn = list(range(len(self.keypoints))) if identity_z_chn else list(self.joint2chn)
        self.aug = dict(aug)

    def __repr__(self):
        return "Profile(%s)" % self.name

    def get_swap_part_indices(self):
        return list(self.swap_indices)

    def dist_th_2d(self):
        """The 2D PCK threshold of the ITOP scripts: 2 % of the frame diagonal (evaluation_rtpose_light3d_itop.py:303)."""
        import numpy as np
        return 0.02 * np.sqrt(self.w_org ** 2 + self.h_org ** 2)

    def aug_centre(self, H, W):
        """(cx, cy) Rotate and RenderDepth turn and scale about for H x W frames."""
        cx, cy = self.aug.get("cx"), self.aug.get("cy")
        return (W / 2 if cx is None else cx), (H / 2 if cy is None else cy)


MP3DHP = Profile("MP3DHP", w_org=480, h_org=640, intrinsics=_config.INTRINSICS, depth_mean=_config.DEPTH_MEAN, depth_std=_config.DEPTH_STD,
                 depth_max=_config.DEPTH_MAX, keypoints=_config.KEYPOINTS, root_joint='torso', single_person=False,
                 z_readout=Z_READOUT_HEAT_WEIGHTED, identity_z_chn=True,
                 # train_rtpose_light3d_kdh3d_mpaug.py: Rotate / RenderDepth about the intrinsics' principal point, max_ratio 1.7, no Hflip
                 aug=dict(cx=_config.INTRINSICS['cx'], cy=_config.INTRINSICS['cy'], min_ratio=0.7, max_ratio=1.7, max_crop=0.1, hflip=False))

_ITOP_F = 1 / 0.0035
ITOP = Profile("ITOP", w_org=320, h_org=240, intrinsics={'fx': _ITOP_F, 'fy': -_ITOP_F, 'cx': 160, 'cy': 120}, depth_mean=3, depth_std=2, depth_max=5,
               keypoints=_config.KEYPOINTS, root_joint='torso', single_person=True, z_readout=Z_READOUT_CELL, identity_z_chn=False,
               # train_rtpose_light3d_itop.py / train_yolo_posenet_itop.py: Rotate(), RenderDepth() with their defaults, Hflip(swap), Crop()
               aug=dict(cx=None, cy=None, min_ratio=0.7, max_ratio=1.2, max_crop=0.1, hflip=True))

PROFILES = {"MP3DHP": MP3DHP, "ITOP": ITOP}


def get(profile):
    """A Profile, its name, or None (= MP3DHP)."""
    if profile is None:
        return MP3DHP
    if isinstance(profile, Profile):
        return profile
    try:
        return PROFILES[str(profile).upper().replace("-", "")]
    except KeyError:
        raise _lib.PopnetError("unknown dataset profile %r (known: %s)" % (profile, ", ".join(sorted(PROFILES))))
