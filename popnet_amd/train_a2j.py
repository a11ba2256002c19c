"""One training step of A2J_model (the second stage of the "Yolo-A2J" baseline) on the GPU.

Host-side mirror of the per-batch body of the reference trainer
  third_party_methods/A2J_experiments/train_a2j_mpaug_new.py:459-502   heads = net(img) -> A2J_loss -> (Cls + 3 Reg).backward() -> Adam
  third_party_methods/A2J_experiments/model.py:145-186, resnet.py      the module in train mode (ResNet-50, layer4.1 / layer4.2 conv2 dilated)
  third_party_methods/A2J_experiments/anchor.py:84-154                 the loss
  torch.optim.Adam(lr 0.00035, weight_decay 1e-4)                      the trainer's optimiser
on the NCHW primitives of csrc/train.hip (fp32; in precision="bf16x3" the split-bf16 3x3 kernels and csrc/conv1x1_x3.hip) (convolutions -- the dilated ones included --, BatchNorm), csrc/train_yolo.hip (strided data
gradient, max pooling) and csrc/train_a2j.hip (pn_a2j_loss on the raw NCHW head maps, pn_adam).  popnet_amd.train.TrainEngine supplies the flat
parameter / gradient buffers, the per-layer plumbing, the data-parallel exchange and the checkpoint format; this class adds A2J's call order.

Backbone.model.fc.* is carried unchanged: the reference builds it and never runs it, it has no gradient, so Adam skips it (weight decay
included).  At most 31 crops per replica: pn_bn_train_* takes N * C <= 65535 and layer4 has 2048 channels; the reference's batch of 64 is
reached with data-parallel replicas, whose BatchNorm statistics are per replica, as under DataParallel.

crop_labels() is the label half of the trainer's dataPreprocess (train_a2j_mpaug_new.py:290-345).
"""
import numpy as np
import torch

from . import _lib
from .network.a2j import generate_anchors, shift
from .train import ACT_NONE, ACT_RELU, TrainEngine

LOSS_NAMES = ["Cls_loss", "Reg_loss"]
MAX_BATCH = 31
LAYERS = (("layer1", 1, 1), ("layer2", 2, 1), ("layer3", 2, 1), ("layer4", 1, 2))       # name, stride of block 0, dilation of the blocks after it
HEADS = ("classificationModel", "regressionModel", "DepthRegressionModel")


def crop_labels(bbox, joints_2d, joints_3d, frame_shape=(512, 480), crop_w=288, crop_h=288):
    """The label of one person as dataPreprocess computes it (train_a2j_mpaug_new.py:290-345): bbox (x0, y0, x1, y1) in the frame of
    frame_shape = (rows, columns), joints_2d [P, 2] (x, y) frame pixels, joints_3d [P, 3] -> [P, 3] float32 (y, x, z) in crop pixels.
    The box is clamped to the frame, a box that starts before the frame shifts the joints by start2 / start1 (the zero padding of the crop),
    and the scale is the crop size over the PADDED size int(x1 - x0) x int(y1 - y0), in float64 as numpy computes it there."""
    x0, y0, x1, y1 = (float(v) for v in bbox)
    new_xmin, new_ymin = max(x0, 0), max(y0, 0)
    padded_h, padded_w = int(y1 - y0), int(x1 - x0)
    start1 = 0 - y0 if y0 < 0 else 0
    start2 = 0 - x0 if x0 < 0 else 0
    k2 = np.asarray(joints_2d, dtype=np.float64)
    out = np.ones((k2.shape[0], 3), dtype=np.float32)
    out[:, 1] = (k2[:, 0] - new_xmin + start2) * crop_w / padded_w
    out[:, 0] = (k2[:, 1] - new_ymin + start1) * crop_h / padded_h
    out[:, 2] = np.asarray(joints_3d, dtype=np.float64)[:, 2]
    return out


class A2JTrainEngine(TrainEngine):
    """state_dict: reference-format (optionally `module.`-prefixed) A2J_model(num_classes) checkpoint.

    precision (reported by engine.precision): "fp32", the default -- every product an exact fp32 FMA chain -- or "bf16x3": the split-bf16
    matrix-core kernels (both operands hi + lo bf16, three MFMAs per product block, fp32 accumulators) wherever they exist:
      * every 3x3 stride-1 undilated convolution with Cin >= 32 (most bottleneck conv2, the 15 head convolutions), through the base
        engine's "bf16x3-nchw" mode (tconv3_tile_x3* / tconv3_wgrad_x3*);
      * the 34 stride-1 1x1 convolutions (conv1 / conv3 of the 16 bottlenecks, the downsample of layer1.0 and layer4.0), forward, data
        and weight gradient, through pn_conv1x1_x3_forward / _dgrad / _wgrad.
    Still fp32 in "bf16x3": the two stride-2 downsample convolutions, the two stride-2 3x3, the two dilated 3x3 (layer4.1 / layer4.2
    conv2), the 7x7 stem, BatchNorm, pooling, the loss and Adam.  Parameters, gradients, optimiser state and checkpoints are fp32 in
    both modes."""

    _carry_prefix = "Backbone.model.fc."
    num_anchors = 16

    def __init__(self, state_dict, device="cuda:0", lr=0.00035, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, spatial_factor=0.5, reg_loss_factor=3,
                 num_classes=15, process_group=None, world_size=1, precision="fp32"):
        if precision not in ("fp32", "bf16x3"):
            raise ValueError("A2JTrainEngine: precision must be 'fp32' or 'bf16x3', got %r" % (precision,))
        super().__init__(state_dict, device=device, lr=lr, momentum=0.0, weight_decay=weight_decay, process_group=process_group, world_size=world_size,
                         precision=precision + "-nchw")
        self.precision = precision
        self._x3 = precision == "bf16x3"
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.spatial_factor, self.reg_loss_factor, self.num_classes = float(spatial_factor), float(reg_loss_factor), int(num_classes)
        A, P = self.num_anchors, self.num_classes
        for head, n in zip(HEADS, (A * P, A * P * 2, A * P)):
            if tuple(self.p[head + ".output.weight"].shape[:2]) != (n, 256):
                raise _lib.PopnetError("popnet_amd.train_a2j: %s.output.weight is %s, expected [%d, 256, 3, 3] for %d joints"
                                       % (head, tuple(self.p[head + ".output.weight"].shape), n, P))
        self.flat_v = torch.zeros_like(self.flat_m)          # Adam: flat_m = exp_avg, flat_v = exp_avg_sq
        self.loss_terms = torch.zeros(2, dtype=torch.float32, device=self.device)
        self._scale = torch.tensor([1.0, self.reg_loss_factor], dtype=torch.float32, device=self.device)
        self._anchors = {}
        self.head_grads = None     # (d cls, d reg, d dep) of the last step: NCHW, the gradient of Cls + reg_loss_factor Reg

    @classmethod
    def from_module(cls, module, **kw):
        """From a popnet_amd.network.a2j.A2J_model (or the reference's own module); module.load_state_dict(engine.state_dict()) hands the
        trained weights back to the inference path."""
        kw.setdefault("num_classes", getattr(module, "num_classes", 15))
        return cls(module.state_dict(), **kw)

    def _trainer(self, N, H, W):
        raise _lib.PopnetError("popnet_amd.train_a2j: A2J has no planes engine")

    def capture(self, *a, **k):
        raise _lib.PopnetError("popnet_amd.train_a2j: the A2J step is not captured as a hipGraph; call step()")

    # ---- convolutions with a dilation ----
    def _conv(self, name, x, ks, stride=1, pad=0, dil=1):
        if self._x3 and ks == 1 and stride == 1 and pad == 0:
            w = self.p[name + ".weight"]
            N, Cin, H, W = x.shape
            Cout = w.shape[0]
            y = self._buf("c:" + name, (N, Cout, H, W))
            self._check(self.L.pn_conv1x1_x3_forward(self.ctx.handle, self._ptr(x), self._ptr(w), self._ptr(self.p.get(name + ".bias")), self._ptr(y), N, Cin, H * W,
                                                     Cout, 0, self._s()), "pn_conv1x1_x3_forward")
            self.A["x:" + name] = x
            return y
        if dil == 1:
            return super()._conv(name, x, ks, stride, pad)
        w = self.p[name + ".weight"]
        N, Cin, H, W = x.shape
        Cout = w.shape[0]
        y = self._buf("c:" + name, (N, Cout, H + 2 * pad - 2 * dil, W + 2 * pad - 2 * dil))
        self._check(self.L.pn_conv2d_forward_dil(self.ctx.handle, self._ptr(x), self._ptr(w), self._ptr(self.p.get(name + ".bias")), self._ptr(y), N, Cin, H, W, Cout,
                                                 ks, stride, pad, dil, 0, self._s()), "pn_conv2d_forward_dil")
        self.A["x:" + name] = x
        return y

    def _conv_bwd(self, name, dy, ks, stride=1, pad=0, dx=None, accumulate=False, need_dx=True, dil=1):
        if self._x3 and ks == 1 and stride == 1 and pad == 0:
            x = self.A["x:" + name]
            w = self.p[name + ".weight"]
            N, Cin, H, W = x.shape
            Cout = w.shape[0]
            self._check(self.L.pn_conv1x1_x3_wgrad(self.ctx.handle, self._ptr(x), self._ptr(dy), self._ptr(self.g[name + ".weight"]), self._ptr(self.g.get(name + ".bias")),
                                                   N, Cin, H * W, Cout, self._s()), "pn_conv1x1_x3_wgrad")
            if not need_dx:
                return None
            if dx is None:
                dx = self._buf("dx:" + name, x.shape)
            self._check(self.L.pn_conv1x1_x3_dgrad(self.ctx.handle, self._ptr(dy), self._ptr(w), self._ptr(dx), N, Cin, H * W, Cout, 1 if accumulate else 0, self._s()),
                        "pn_conv1x1_x3_dgrad")
            return dx
        if dil == 1:
            return super()._conv_bwd(name, dy, ks, stride, pad, dx=dx, accumulate=accumulate, need_dx=need_dx)
        x = self.A["x:" + name]
        w = self.p[name + ".weight"]
        N, Cin, H, W = x.shape
        Cout = w.shape[0]
        self._check(self.L.pn_conv2d_wgrad_dil(self.ctx.handle, self._ptr(x), self._ptr(dy), self._ptr(self.g[name + ".weight"]), self._ptr(self.g.get(name + ".bias")),
                                               N, Cin, H, W, Cout, ks, stride, pad, dil, self._s()), "pn_conv2d_wgrad_dil")
        if not need_dx:
            return None
        if dx is None:
            dx = self._buf("dx:" + name, x.shape)
        self._check(self.L.pn_conv2d_dgrad_dil(self.ctx.handle, self._ptr(dy), self._ptr(w), self._ptr(dx), N, Cin, H, W, Cout, ks, pad, dil, 1 if accumulate else 0,
                                               self._s()), "pn_conv2d_dgrad_dil")
        return dx

    # ---- composite modules ----
    def _block(self, p, x, stride=1, dil=1):
        """Bottleneck (resnet.py:61-104): 1x1, 3x3 (carries the stride and the dilation, padding = dilation), 1x1 to 4 x planes"""
        a1 = self._bn(p + ".bn1", self._conv(p + ".conv1", x, 1, 1, 0), ACT_RELU)
        a2 = self._bn(p + ".bn2", self._conv(p + ".conv2", a1, 3, stride, dil, dil), ACT_RELU)
        c3 = self._conv(p + ".conv3", a2, 1, 1, 0)
        idn = x
        if (p + ".downsample.0.weight") in self.p:
            idn = self._bn(p + ".downsample.1", self._conv(p + ".downsample.0", x, 1, stride, 0), ACT_NONE)
        self.A["geom:" + p] = (stride, dil)
        return self._bn(p + ".bn3", c3, ACT_RELU, res=idn)

    def _block_bwd(self, p, dout):
        stride, dil = self.A["geom:" + p]
        x = self.A["x:" + p + ".conv1"]
        dx = self._buf("dx:" + p, x.shape)
        if (p + ".downsample.0.weight") in self.p:
            didn = self._buf("di:" + p, dout.shape)
            dc3 = self._bn_bwd(p + ".bn3", dout, dres=didn)
            dcd = self._bn_bwd(p + ".downsample.1", didn)
            self._conv_bwd(p + ".downsample.0", dcd, 1, stride, 0, dx=dx, accumulate=False)
        else:
            dc3 = self._bn_bwd(p + ".bn3", dout, dres=dx)              # identity path: dx = g
        da2 = self._conv_bwd(p + ".conv3", dc3, 1, 1, 0)
        da1 = self._conv_bwd(p + ".conv2", self._bn_bwd(p + ".bn2", da2), 3, stride, dil, dil=dil)
        self._conv_bwd(p + ".conv1", self._bn_bwd(p + ".bn1", da1), 1, 1, 0, dx=dx, accumulate=True)
        return dx

    def _head(self, p, x):
        """the three heads of model.py:5-142: (conv 3x3 + bias, BN, ReLU) x 4, then the output convolution"""
        for i in (1, 2, 3, 4):
            x = self._bn("%s.bn%d" % (p, i), self._conv("%s.conv%d" % (p, i), x, 3, 1, 1), ACT_RELU)
        return self._conv(p + ".output", x, 3, 1, 1)

    def _head_bwd(self, p, dv, dx, accumulate):
        d = self._conv_bwd(p + ".output", dv, 3, 1, 1)
        for i in (4, 3, 2, 1):
            dc = self._bn_bwd("%s.bn%d" % (p, i), d)
            if i > 1:
                d = self._conv_bwd("%s.conv%d" % (p, i), dc, 3, 1, 1)
            else:
                self._conv_bwd("%s.conv%d" % (p, i), dc, 3, 1, 1, dx=dx, accumulate=accumulate)

    def _block_names(self, layer):
        n = 0
        while ("Backbone.model.%s.%d.conv1.weight" % (layer, n)) in self.p:
            n += 1
        return ["Backbone.model.%s.%d" % (layer, i) for i in range(n)]

    def anchors(self, h, w):
        """[h w 16, 2] float32 (y, x) on the device: the array post_process / A2J_loss hold for an h x w map at stride 16"""
        a = self._anchors.get((h, w))
        if a is None:
            a = self._anchors[(h, w)] = torch.from_numpy(shift([h, w], 16, generate_anchors())).float().to(self.device)
        return a

    # ---- the step ----
    def forward_backward(self, img, label):
        """img [N, 1, H, W], label [N, P, 3] (y, x, z).  Fills self.flat_g (this replica's gradient of Cls + reg_loss_factor Reg) and
        self.loss_terms [2] (LOSS_NAMES); updates the BN running statistics."""
        for t, n in ((img, "img"), (label, "label")):
            _lib.require_cuda_tensor(t, n)
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.PopnetError("popnet_amd.train_a2j: %s must be a contiguous float32 tensor" % n)
        if img.dim() != 4 or img.shape[1] != 1:
            raise _lib.PopnetError("popnet_amd.train_a2j: img must be [N, 1, H, W], got %s" % (tuple(img.shape),))
        N, _, H, W = img.shape
        if N > MAX_BATCH:
            raise _lib.PopnetError("popnet_amd.train_a2j: at most %d crops per replica (pn_bn_train_* takes N * C <= 65535 and layer4 has 2048 channels), "
                                   "got %d; use data-parallel replicas for a larger batch" % (MAX_BATCH, N))
        if H % 16 or W % 16:
            raise _lib.PopnetError("popnet_amd.train_a2j: input size must be a multiple of 16, got %d x %d" % (H, W))
        h, w = H // 16, W // 16
        if N * h * w == 1:
            raise _lib.PopnetError("popnet_amd.train_a2j: one %d x %d crop leaves one value per channel: BatchNorm has no batch statistics" % (H, W))
        A, P = self.num_anchors, self.num_classes
        if tuple(label.shape) != (N, P, 3):
            raise _lib.PopnetError("popnet_amd.train_a2j: label must be [%d, %d, 3]" % (N, P))
        self.A = {}
        L, ctx, s = self.L, self.ctx.handle, self._s()
        self._check(L.pn_train_pack_refresh(ctx, s), "pn_train_pack_refresh")
        # forward (model.py:152-186).  conv1.weight stays [64, 3, 7, 7]: the depth channel three times (model.py:155-156)
        x3c = self._buf("img3", (N, 3, H, W))
        x3c.copy_(img.expand(N, 3, H, W))
        pre = "Backbone.model."
        a = self._bn(pre + "bn1", self._conv(pre + "conv1", x3c, 7, 2, 3), ACT_RELU)
        a = self._maxpool("stem", a, 3, 2, 1)
        blocks = []
        for layer, stride, dil in LAYERS:
            for i, p in enumerate(self._block_names(layer)):
                a = self._block(p, a, stride if i == 0 else 1, 1 if i == 0 else dil)
                blocks.append(p)
            if layer == "layer3":
                x3 = a
        x4 = a
        cls, reg, dep = self._head(HEADS[0], x3), self._head(HEADS[1], x4), self._head(HEADS[2], x4)
        dcls, dreg, ddep = self._buf("dv:cls", cls.shape), self._buf("dv:reg", reg.shape), self._buf("dv:dep", dep.shape)
        self.head_grads = (dcls, dreg, ddep)
        self._check(L.pn_a2j_loss(ctx, self._ptr(cls), self._ptr(reg), self._ptr(dep), N, h, w, A, P, self._ptr(self.anchors(h, w)), self._ptr(label),
                                  self.spatial_factor, self._ptr(self._scale), self._ptr(self.loss_terms), self._ptr(dcls), self._ptr(dreg), self._ptr(ddep), s),
                    "pn_a2j_loss")
        # backward: x4 feeds two heads, x3 the classification head and layer4 -- those data gradients accumulate
        dx4 = self._buf("dx4", x4.shape)
        self._head_bwd(HEADS[1], dreg, dx4, accumulate=False)
        self._head_bwd(HEADS[2], ddep, dx4, accumulate=True)
        d = dx4
        n3 = len(self._block_names("layer4"))
        for p in reversed(blocks[-n3:]):
            d = self._block_bwd(p, d)
        self._head_bwd(HEADS[0], dcls, d, accumulate=True)
        for p in reversed(blocks[:-n3]):
            d = self._block_bwd(p, d)
        d = self._maxpool_bwd("stem", d)
        self._conv_bwd(pre + "conv1", self._bn_bwd(pre + "bn1", d), 7, 2, 3, need_dx=False)
        for k in self.tracked:
            self.tracked[k] += 1
        return self.loss_terms

    def apply(self):
        """Average the gradient over the replicas (one all-reduce of the flat buffer) and take the Adam step (pn_adam, step counter self.steps + 1)."""
        if self.world > 1:
            self.reduce_flat_gradient(self.flat_g, self.world, self.group)
        self._check(self.L.pn_adam(self.ctx.handle, self._ptr(self.flat_p), self._ptr(self.flat_g), self._ptr(self.flat_m), self._ptr(self.flat_v), self.flat_p.numel(),
                                   self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.steps + 1, 1.0 / self.world, self._s()), "pn_adam")
        self.steps += 1

    def step(self, img, label):
        """-> device tensor [2] of loss terms (LOSS_NAMES); the trainer's loss is terms[0] + reg_loss_factor terms[1].  Asynchronous."""
        terms = self.forward_backward(img, label)
        self.apply()
        return terms

    def conv1x1_shapes(self, H, W):
        """[(name, Cin, HW, Cout)] of the stride-1 1x1 convolutions of one step on H x W crops: the calls precision="bf16x3" sends to
        pn_conv1x1_x3_forward / _dgrad / _wgrad (conv1, conv3 and a stride-1 downsample of every bottleneck)."""
        out = []
        h, w = -(-H // 4), -(-W // 4)
        for layer, stride, _ in LAYERS:
            for i, p in enumerate(self._block_names(layer)):
                st = stride if i == 0 else 1
                ho, wo = -(-h // st), -(-w // st)
                for n, hw in ((".conv1", h * w), (".conv3", ho * wo)) + (((".downsample.0", h * w),) if st == 1 and (p + ".downsample.0.weight") in self.p else ()):
                    wt = self.p[p + n + ".weight"]
                    out.append((p + n, wt.shape[1], hw, wt.shape[0]))
                h, w = ho, wo
        return out

    def flops_per_step(self, N, H, W):
        """Algorithmic FLOPs of one step (2 per multiply-add): every convolution's forward and weight gradient, and the data gradient of every
        convolution but the first; BatchNorm, pooling and the loss are not counted."""
        total = 0.0

        def conv(name, h, w, stride, first=False):
            wt = self.p[name + ".weight"]
            ho, wo = -(-h // stride), -(-w // stride)
            nonlocal total
            total += 2.0 * N * ho * wo * wt.numel() * (2 if first else 3)
            return ho, wo
        h, w = conv("Backbone.model.conv1", H, W, 2, first=True)
        h, w = -(-h // 2), -(-w // 2)
        for layer, stride, _ in LAYERS:
            for i, p in enumerate(self._block_names(layer)):
                st = stride if i == 0 else 1
                conv(p + ".conv1", h, w, 1)
                if (p + ".downsample.0.weight") in self.p:
                    conv(p + ".downsample.0", h, w, st)
                h, w = conv(p + ".conv2", h, w, st)
                conv(p + ".conv3", h, w, 1)
        for head in HEADS:
            for n in ("conv1", "conv2", "conv3", "conv4", "output"):
                conv("%s.%s" % (head, n), h, w, 1)
        return total

