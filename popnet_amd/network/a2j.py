"""``A2J_model`` (the second stage of the "Yolo-A2J" baseline) with the reference's Python surface, computed by HIP kernels.

Drop-in for third_party_methods/A2J_experiments/model.py:145-186 (+ resnet.py:61-164, ResNet-50 with a dilated layer4) and
anchor.py:7-82: the same 410 ``state_dict`` keys, so a reference ``.pth`` loads -- including ``Backbone.model.fc.*``, which the
reference builds and never executes and which is held here and skipped at compile time -- the same
``forward(x) -> (classification [B, K, P], regression [B, K, P, 2], depth [B, K, P])`` with K = (W/16) (H/16) 16 anchors in the
reference's W-major order, and ``post_process(...).forward(heads) -> [B, P, 3]`` (y, x, z).  Nothing is downloaded: the reference's
constructor fetches ImageNet weights, this one starts from its own initialisation.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ._hipnet import HipNetModule, bn_


class A2JCfg(C.Structure):
    """pn_a2j_cfg"""
    _fields_ = [("img_w", C.c_int), ("img_h", C.c_int), ("crop_w", C.c_int), ("crop_h", C.c_int), ("mean", C.c_float), ("std", C.c_float),
                ("conf_min", C.c_float), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


A2J_RECORD_DTYPE = np.dtype([("joint", np.float32, (15, 5)), ("conf", np.float32), ("frame", np.int32)], align=True)


# ---- anchors: the arrays of anchor.py:7-42, built by broadcasting (tests/test_a2j_cpu.py pins them to the reference's) ---------------
def generate_anchors(P_h=None, P_w=None):
    """[A, 2] float64 in-cell anchor offsets (y, x): every y of P_h (slow index) paired with every x of P_w (fast index); A is the square
    of the number of y offsets, as in the reference, which only ever uses equally long lists."""
    ys = np.asarray([2, 6, 10, 14] if P_h is None else P_h, dtype=np.float64)
    xs = np.asarray([2, 6, 10, 14] if P_w is None else P_w, dtype=np.float64)
    if len(xs) != len(ys):
        raise ValueError("generate_anchors: P_h and P_w must have the same length, got %d and %d" % (len(ys), len(xs)))
    return np.stack([np.repeat(ys, len(xs)), np.tile(xs, len(ys))], axis=1)


def shift(shape, stride, anchors):
    """[h * w * A, 2] float64: the anchors placed on every cell of an h x w map, cells in W-major order (column by column, rows within a
    column), the A anchors of a cell together -- the order of the head tensors."""
    h, w = int(shape[0]), int(shape[1])
    col, row = np.divmod(np.arange(h * w), h)                    # cell index -> (column, row)
    cells = np.stack([row, col], axis=1) * stride                # (y, x) of each cell's corner; integer, exact
    anchors = np.asarray(anchors)
    return (cells[:, None, :] + anchors[None, :, :]).reshape(h * w * anchors.shape[0], 2)


# ---- parameter holders -------------------------------------------------------------------------------
class _Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride=1, downsample=None, dilation=1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = bn_(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = bn_(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = bn_(planes * 4)
        self.downsample = downsample


class _ResNet50(nn.Module):
    def __init__(self):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = bn_(64)
        self.layer1 = self._make_layer(64, 3)
        self.layer2 = self._make_layer(128, 4, stride=2)
        self.layer3 = self._make_layer(256, 6, stride=2)
        self.layer4 = self._make_layer(512, 3, stride=1, dilation=2)      # block 0 is NOT dilated (resnet.py:142)
        self.fc = nn.Linear(2048, 1000)                                   # never executed (model.py:158-167)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def _make_layer(self, planes, blocks, stride=1, dilation=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * 4:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride=stride, bias=False), bn_(planes * 4))
        layers = [_Bottleneck(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * 4
        for _ in range(1, blocks):
            layers.append(_Bottleneck(self.inplanes, planes, dilation=dilation))
        return nn.Sequential(*layers)


class _BackBone(nn.Module):
    def __init__(self):
        super().__init__()
        self.model = _ResNet50()


class _Head(nn.Module):
    def __init__(self, cin, cout, feature_size=256):
        super().__init__()
        for i, c in enumerate((cin, feature_size, feature_size, feature_size), 1):
            setattr(self, "conv%d" % i, nn.Conv2d(c, feature_size, 3, padding=1))
            setattr(self, "bn%d" % i, bn_(feature_size))
        self.output = nn.Conv2d(feature_size, cout, 3, padding=1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_normal_(m.weight.data)


class A2J_model(HipNetModule):
    _kind = _lib.PN_NET_A2J
    num_anchors = 16

    def __init__(self, num_classes, is_3D=True):
        super().__init__()
        if not is_3D:
            raise _lib.PopnetError("A2J_model: the HIP net is built with the depth head (is_3D=True), as the reference's evaluation uses it")
        self.is_3D, self.num_classes, self.input_dim = is_3D, int(num_classes), 1
        self.Backbone = _BackBone()
        self.regressionModel = _Head(2048, self.num_anchors * num_classes * 2)
        self.classificationModel = _Head(1024, self.num_anchors * num_classes)
        self.DepthRegressionModel = _Head(2048, self.num_anchors * num_classes)

    def _net_args(self):
        return self._kind, self.num_classes, self.num_anchors, 1

    def run(self, x):
        """x [B, 1, H, W] CUDA f32 -> device pointers of the NHWC head maps (cls, reg, dep), (h, w), the net's precision id."""
        x = self._check_input(x)
        B, _, H, W = x.shape
        if self.training:
            raise _lib.PopnetError("A2J_model: inference only -- call .eval()")
        net = self._compile(x.device, B, H, W)
        ptrs = [C.c_void_p() for _ in range(3)]
        self._ctx.check(_lib.lib().pn_a2j_forward(net, C.c_void_p(x.data_ptr()), B, *(C.byref(p) for p in ptrs), _lib.current_stream_ptr(x.device)),
                        "pn_a2j_forward")
        return ptrs, (H // 16, W // 16), self._net[1][1]

    def forward(self, x):
        self.run(x)
        B, dev = x.shape[0], x.device
        h, w = x.shape[2] // 16, x.shape[3] // 16
        A, P = self.num_anchors, self.num_classes
        # the reference's own re-layout of the NCHW maps (model.py:47-50, 93-96, 139-142): W-major, then H, anchors, joints
        cls = self._activation("cls", B, (A * P, h, w), dev).permute(0, 3, 2, 1).reshape(B, w, h, A, P).reshape(B, -1, P)
        reg = self._activation("reg", B, (A * P * 2, h, w), dev).permute(0, 3, 2, 1).reshape(B, w, h, A, P, 2).reshape(B, -1, P, 2)
        dep = self._activation("dep", B, (A * P, h, w), dev).permute(0, 3, 2, 1).reshape(B, w, h, A, P).reshape(B, -1, P)
        return cls, reg, dep


class post_process(nn.Module):
    """anchor.py:44-82.  forward(heads): heads = (classification [B, K, P], regression [B, K, P, 2], depth [B, K, P]) CUDA tensors in the
    reference's layout -> [B, P, 3] (y, x, z), by pn_a2j_vote's strided entry."""

    def __init__(self, P_h=[2, 6], P_w=[2, 6], shape=[48, 26], stride=8, thres=8, is_3D=True):
        super().__init__()
        if not is_3D:
            raise _lib.PopnetError("post_process: built with the depth head (is_3D=True)")
        self.all_anchors_np = shift(shape, stride, generate_anchors(P_h=P_h, P_w=P_w))
        self.all_anchors = torch.from_numpy(self.all_anchors_np).float()
        self.is_3D = is_3D

    def forward(self, heads, voting=False):
        cls, reg, dep = heads
        _lib.require_cuda_tensor(cls, "classification")
        dev = cls.device
        cls, reg, dep = (t.contiguous().float() for t in (cls, reg, dep))
        B, K, P = cls.shape
        if self.all_anchors.device != dev:
            self.all_anchors = self.all_anchors.to(dev)
        if K != self.all_anchors.shape[0] or tuple(reg.shape) != (B, K, P, 2) or tuple(dep.shape) != (B, K, P):
            raise _lib.PopnetError("post_process: heads of %s / %s / %s against %d anchors" % (tuple(cls.shape), tuple(reg.shape), tuple(dep.shape), self.all_anchors.shape[0]))
        out = torch.empty((B, P, 3), device=dev, dtype=torch.float32)
        ctx = _lib.Context.for_device(dev.index)
        ctx.check(_lib.lib().pn_a2j_vote(ctx.handle, C.c_void_p(cls.data_ptr()), C.c_void_p(reg.data_ptr()), C.c_void_p(dep.data_ptr()), _lib.PN_PREC_F32,
                                         B, 0, K, 1, P, C.c_void_p(self.all_anchors.data_ptr()), C.c_void_p(out.data_ptr()), None, None, None,
                                         _lib.current_stream_ptr(dev)), "pn_a2j_vote")
        return out
