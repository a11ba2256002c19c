"""``YoloPoseNet`` ("Yolo-Pose+") with the reference's Python surface, computed by HIP kernels.

Drop-in for tpm/lib/network/yolo_posenet.py:87-158 (+ ResNetBackBone :26-56, resnet34 layers
tpm/lib/network/resnet.py:27-56,134-148): same constructor, same 223 ``state_dict`` keys --
including ``model0.layer3.*``, which the reference builds and checkpoints but never executes
(yolo_posenet.py:42,54) and which is therefore held here and skipped at compile time -- and the
same ``forward(x) -> Tensor[B, A*(5+3J), H/16, W/16]`` with the per-slice sigmoid casts applied.
"""
import ctypes as C

import torch
import torch.nn as nn
from torch.nn import init

from .. import _lib
from ._hipnet import HipNetModule, bn_, conv_
from .rtpose_light3d import _ResUnit


def _res_layer(cin, cout, blocks, stride):
    return nn.Sequential(*([_ResUnit(cin, cout, stride)] + [_ResUnit(cout, cout) for _ in range(blocks - 1)]))


class _BackBone(nn.Module):
    def __init__(self, input_dim):
        super().__init__()
        self.conv1 = nn.Conv2d(input_dim, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = bn_(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.avgpool = nn.AvgPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = _res_layer(64, 64, 3, 1)
        self.layer2 = _res_layer(64, 128, 4, 2)
        self.layer3 = _res_layer(128, 256, 6, 2)     # dead weight, kept for checkpoint compatibility


def _cbl(cin, cout, pool=False):
    mods = [conv_(cin, cout, 3, bias=False), bn_(cout), nn.LeakyReLU(0.1, inplace=True)]
    if pool:
        mods.append(nn.MaxPool2d(2, 2))
    return nn.Sequential(*mods)


class YoloPoseNet(HipNetModule):
    _kind = _lib.PN_NET_YOLO_POSENET

    def __init__(self, num_parts=15, input_dim=3, anchors=[(6., 3.), (12., 6.)]):
        super().__init__()
        self.num_parts, self.anchors, self.input_dim = num_parts, anchors, input_dim
        self.model0 = _BackBone(input_dim)
        neck = []
        for i, (cin, cout) in enumerate([(128, 256), (256, 256), (256, 256), (256, 256)]):
            neck += [conv_(cin, cout, 3, bias=True), bn_(cout), nn.LeakyReLU(0.1, inplace=True)]
        neck.append(conv_(256, 256, 3, bias=True))
        self.model1 = nn.Sequential(*neck)
        self.model2_1 = _cbl(256, 256, pool=True)
        self.model2_2 = _cbl(256, 256)
        self.model2_3 = _cbl(256, 128)
        self.model2_4 = nn.Sequential(conv_(128, len(anchors) * (5 + 3 * num_parts), 3, bias=False))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                init.normal_(m.weight, mean=0, std=0.01)

    def _net_args(self):
        return self._kind, self.num_parts, len(self.anchors), self.input_dim

    # ---- train mode: the reference's forward (yolo_posenet.py:42-54,137-158, resnet.py BasicBlock) on the autograd-wrapped HIP primitives ----
    def _forward_train(self, x):
        from . import _autograd as ag
        x = self._check_input(x)
        if x.shape[2] % 16 or x.shape[3] % 16:
            raise _lib.PopnetError("input size must be a multiple of 16")
        for p in self.parameters():
            if p.device != x.device:
                raise _lib.PopnetError("popnet_amd: module parameters are on %s, the input on %s -- call model.cuda() (the HIP path has no CPU fallback)" % (p.device, x.device))

        def block(u, a):                       # BasicBlock: conv1 carries the stride, downsample = 1x1 conv (same stride) + BN
            y = ag.bn_act(ag.conv(a, u.conv1), u.bn1, ag.ACT_RELU)
            y = ag.conv(y, u.conv2)
            idn = a if u.downsample is None else ag.bn_act(ag.conv(a, u.downsample[0]), u.downsample[1], ag.ACT_NONE)
            return ag.bn_act(y, u.bn2, ag.ACT_RELU, res=idn)

        m0 = self.model0
        a = ag.maxpool(ag.bn_act(ag.conv(x, m0.conv1), m0.bn1, ag.ACT_RELU), m0.maxpool)
        for u in m0.layer1:
            a = block(u, a)
        for u in m0.layer2:                    # layer3 is built but never run by the reference (yolo_posenet.py:54)
            a = block(u, a)
        for i in (0, 3, 6, 9):                 # model1: make_stages, conv BN LeakyReLU(0.1) x 4 + a bare conv
            a = ag.bn_act(ag.conv(a, self.model1[i]), self.model1[i + 1], ag.ACT_LEAKY)
        a = ag.conv(a, self.model1[12])
        a = ag.maxpool(ag.bn_act(ag.conv(a, self.model2_1[0]), self.model2_1[1], ag.ACT_LEAKY), self.model2_1[3])
        for seq in (self.model2_2, self.model2_3):
            a = ag.bn_act(ag.conv(a, seq[0]), seq[1], ag.ACT_LEAKY)
        v = ag.conv(a, self.model2_4[0])
        # the per-slice range casts of :146-156 are element-wise glue: left to torch (autograd orders them)
        B, _, h, w = v.shape
        s = v.view(B, len(self.anchors), 5 + 3 * self.num_parts, h, w).sigmoid()
        out = torch.cat([(s[:, :, 0:2] - 0.5) * 2, s[:, :, 2:4] * 2, s[:, :, 4:5], (s[:, :, 5:] - 0.5) * 4], 2).view(v.shape)
        self.invalidate()                      # the weights are about to change: the eval-mode net is re-folded on its next use
        return out

    def forward(self, x):
        if self.training:
            return self._forward_train(x)
        x = self._check_input(x)
        B, _, H, W = x.shape
        dev = x.device
        net = self._compile(dev, B, H, W)
        out = torch.empty((B, len(self.anchors) * (5 + 3 * self.num_parts), H // 16, W // 16),
                          device=dev, dtype=torch.float32)
        self._ctx.check(_lib.lib().pn_yolo_forward(net, C.c_void_p(x.data_ptr()), B, C.c_void_p(out.data_ptr()),
                                                   _lib.current_stream_ptr(dev)), "pn_yolo_forward")
        return out

    def backbone_features(self, B):
        key = self._net[1]
        return self._activation("feat", B, (128, key[2] // 8, key[3] // 8), torch.device("cuda", key[0]))
