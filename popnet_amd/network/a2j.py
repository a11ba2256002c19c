"""``A2J_model`` (the second stage of the "Yolo-A2J" baseline) with the reference's Python surface, computed by HIP kernels.

Drop-in for third_party_methods/A2J_experiments/model.py:145-186 (+ resnet.py:61-164, ResNet-50 with a dilated layer4) and
anchor.py:7-82: the same 410 ``state_dict`` keys, so a reference ``.pth`` loads -- including ``Backbone.model.fc.*``, which the
reference builds and never executes and which is held here and skipped at compile time -- the same
``forward(x) -> (classification [B, K, P], regression [B, K, P, 2], depth [B, K, P])`` with K = (W/16) (H/16) 16 anchors in the
reference's W-major order, and ``post_process(...).forward(heads) -> [B, P, 3]`` (y, x, z).  In train mode ``forward`` runs the autograd-wrapped training primitives
(network/_autograd.py) and returns the same three heads with ``grad_fn``; ``A2J_loss`` is anchor.py:84-154 on one HIP kernel, so the loop of
train_a2j_mpaug_new.py:226-238 runs with the imports swapped (at most 31 crops per call, see ``A2J_model.max_train_batch``).  Nothing is downloaded: the reference's
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
            raise _lib.PopnetError("A2J_model.run: the NHWC head maps are the compiled eval-mode net's -- call .eval(); in train mode use forward()")
        net = self._compile(x.device, B, H, W)
        ptrs = [C.c_void_p() for _ in range(3)]
        self._ctx.check(_lib.lib().pn_a2j_forward(net, C.c_void_p(x.data_ptr()), B, *(C.byref(p) for p in ptrs), _lib.current_stream_ptr(x.device)),
                        "pn_a2j_forward")
        return ptrs, (H // 16, W // 16), self._net[1][1]

    # ---- train mode: the reference's forward (model.py:152-186, resnet.py Bottleneck) on the autograd-wrapped HIP primitives ----
    max_train_batch = 31          # pn_bn_train_* takes N * C <= 65535 and layer4 has C = 2048

    def _forward_train(self, x):
        from . import _autograd as ag
        x = self._check_input(x)
        B, _, H, W = x.shape
        if H % 16 or W % 16:
            raise _lib.PopnetError("A2J_model: the input size must be a multiple of 16, got %d x %d" % (H, W))
        if B > self.max_train_batch:
            raise _lib.PopnetError("A2J_model: train mode takes at most %d crops per call (the BatchNorm primitives take N * C <= 65535 and layer4 "
                                   "has 2048 channels); split the batch over data-parallel replicas, got %d" % (self.max_train_batch, B))
        if B * (H // 16) * (W // 16) == 1:
            raise _lib.PopnetError("A2J_model: train mode needs more than one value per channel (one %d x %d crop leaves a 1 x 1 map)" % (H, W))
        for p in self.parameters():
            if p.device != x.device:
                raise _lib.PopnetError("popnet_amd: module parameters are on %s, the input on %s -- call model.cuda() (the HIP path has no CPU fallback)" % (p.device, x.device))

        def block(u, a):                       # Bottleneck (resnet.py:61-104): conv2 carries the stride and the dilation
            y = ag.bn_act(ag.conv(a, u.conv1), u.bn1, ag.ACT_RELU)
            y = ag.bn_act(ag.conv(y, u.conv2), u.bn2, ag.ACT_RELU)
            y = ag.conv(y, u.conv3)
            idn = a if u.downsample is None else ag.bn_act(ag.conv(a, u.downsample[0]), u.downsample[1], ag.ACT_NONE)
            return ag.bn_act(y, u.bn3, ag.ACT_RELU, res=idn)

        def head(m, a):
            for i in (1, 2, 3, 4):
                a = ag.bn_act(ag.conv(a, getattr(m, "conv%d" % i)), getattr(m, "bn%d" % i), ag.ACT_RELU)
            return ag.conv(a, m.output)

        r = self.Backbone.model
        a = ag.bn_act(ag.conv(x.expand(B, 3, H, W), r.conv1), r.bn1, ag.ACT_RELU)        # model.py:155-156: the depth channel three times
        a = ag.MaxPoolFn.apply(a, 3, 2, 1)[0]
        for layer in (r.layer1, r.layer2, r.layer3):
            for u in layer:
                a = block(u, a)
        x3 = a
        for u in r.layer4:
            a = block(u, a)
        x4 = a
        A, P = self.num_anchors, self.num_classes
        h, w = H // 16, W // 16
        # the reference's re-layout of the NCHW maps (model.py:47-50, 93-96, 139-142) is element-wise glue: left to torch (autograd orders it)
        cls = head(self.classificationModel, x3).permute(0, 3, 2, 1).reshape(B, w, h, A, P).reshape(B, -1, P)
        reg = head(self.regressionModel, x4).permute(0, 3, 2, 1).reshape(B, w, h, A, P, 2).reshape(B, -1, P, 2)
        dep = head(self.DepthRegressionModel, x4).permute(0, 3, 2, 1).reshape(B, w, h, A, P).reshape(B, -1, P)
        self.invalidate()                      # the weights are about to change: the eval-mode net is re-folded on its next use
        return cls, reg, dep

    def forward(self, x):
        if self.training:
            return self._forward_train(x)
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


class _A2JLossFn(torch.autograd.Function):
    """terms [2] = (Cls_loss, Reg_loss) of pn_a2j_loss on heads in the reference's layout; backward is the kernel's gradient mode with the
    incoming gradient of the two terms as (s_cls, s_reg), read on the device."""

    @staticmethod
    def _call(cls, reg, dep, anchors, labels, sf, scale, grads):
        B, K, P = cls.shape
        dev = cls.device
        terms = torch.empty((2,), device=dev, dtype=torch.float32)
        ctx = _lib.Context.for_device(dev.index)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        ctx.check(_lib.lib().pn_a2j_loss(ctx.handle, ptr(cls), ptr(reg), ptr(dep), B, 0, K, 1, P, ptr(anchors), ptr(labels), float(sf), ptr(scale), ptr(terms),
                                         ptr(grads[0]), ptr(grads[1]), ptr(grads[2]), _lib.current_stream_ptr(dev)), "pn_a2j_loss")
        return terms

    @staticmethod
    def forward(ctx, cls, reg, dep, anchors, labels, sf):
        cls, reg, dep, labels = (t.contiguous() for t in (cls, reg, dep, labels))
        ctx.save_for_backward(cls, reg, dep, anchors, labels)
        ctx.sf = sf
        return _A2JLossFn._call(cls, reg, dep, anchors, labels, sf, None, (None, None, None))

    @staticmethod
    def backward(ctx, gterms):
        cls, reg, dep, anchors, labels = ctx.saved_tensors
        grads = (torch.empty_like(cls), torch.empty_like(reg), torch.empty_like(dep))
        _A2JLossFn._call(cls, reg, dep, anchors, labels, ctx.sf, gterms.contiguous().float(), grads)
        return grads + (None, None, None)


class A2J_loss(nn.Module):
    """anchor.py:84-154 with the reference's constructor.  forward(heads, annotations): heads = (classification [B, K, P], regression
    [B, K, P, 2], depth [B, K, P]) CUDA tensors in the reference's layout, annotations [B, P, 3] (two columns in the anchors' (y, x) order,
    then z) -> (Cls_loss [1], Reg_loss [1]), differentiable with respect to the heads.  One HIP kernel (pn_a2j_loss) per direction.
    `thres` and `img_shape` are kept and, as in the reference's forward, never used."""

    def __init__(self, P_h=[2, 6], P_w=[2, 6], shape=[8, 4], stride=8, thres=[10.0, 20.0], spatialFactor=0.1, img_shape=[0, 0], is_3D=True):
        super().__init__()
        if not is_3D:
            raise _lib.PopnetError("A2J_loss: built with the depth head (is_3D=True)")
        self.all_anchors_np = shift(shape, stride, generate_anchors(P_h=P_h, P_w=P_w))
        self.all_anchors = torch.from_numpy(self.all_anchors_np).float()
        self.thres, self.spatialFactor, self.img_shape, self.is_3D = thres, float(spatialFactor), img_shape, is_3D

    def forward(self, heads, annotations):
        cls, reg, dep = heads
        _lib.require_cuda_tensor(cls, "classification")
        dev = cls.device
        if self.all_anchors.device != dev:
            self.all_anchors = self.all_anchors.to(dev)
        B, K, P = cls.shape
        if (K != self.all_anchors.shape[0] or tuple(reg.shape) != (B, K, P, 2) or tuple(dep.shape) != (B, K, P) or tuple(annotations.shape) != (B, P, 3)
                or any(t.dtype != torch.float32 for t in (cls, reg, dep))):
            raise _lib.PopnetError("A2J_loss: float32 heads of %s / %s / %s and labels %s against %d anchors" % (
                tuple(cls.shape), tuple(reg.shape), tuple(dep.shape), tuple(annotations.shape), self.all_anchors.shape[0]))
        labels = annotations.to(device=dev, dtype=torch.float32)
        terms = _A2JLossFn.apply(cls, reg, dep, self.all_anchors, labels, self.spatialFactor)
        return terms[0:1], terms[1:2]
