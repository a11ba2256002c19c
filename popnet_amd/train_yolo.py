"""One training step of YoloPoseNet on the GPU.

Host-side mirror of the per-batch body of the reference trainer
  third_party_methods/train_yolo_posenet_kdh3d_mpaug.py:157-192 (CR)   model(img) -> yolo_loss_fgweight[_poseweight] -> backward -> SGD
  third_party_methods/lib/network/yolo_posenet.py:137-158              the module in train mode (BatchNorm on batch statistics)
  third_party_methods/lib/network/losses.py:397-466                    the loss
  torch.optim.SGD(lr 1.0, momentum 0.9, nesterov=True)                 the trainer's optimiser
on the fp32 NCHW primitives of csrc/train.hip (convolutions, BatchNorm, Nesterov SGD) and the YoloPoseNet ones of csrc/train_yolo.hip
(strided data gradient, max pooling, the cast + loss + gradient of the head).  popnet_amd.train.TrainEngine supplies the flat parameter /
gradient / momentum buffers, the per-layer plumbing, the data-parallel exchange and the checkpoint format; this class adds YoloPoseNet's
call order.  model0.layer3.* is carried unchanged: the reference builds it but never runs it, so SGD never moves it.
"""
import ctypes as C

import torch

from . import _lib
from .train import ACT_LEAKY, ACT_NONE, ACT_RELU, TrainEngine

LOSS_NAMES = ["loss_prior", "loss_bbox", "loss_obj", "loss_selfpose"]
ANCHORS = [(6., 3.), (12., 6.)]


class YoloTrainEngine(TrainEngine):
    """state_dict: reference-format (optionally `module.`-prefixed) YoloPoseNet(15, input_dim=1) checkpoint.
    rarity_weight: True = yolo_loss_fgweight_poseweight (the trainer's default, --rarity-weight 1), False = yolo_loss_fgweight."""

    def __init__(self, state_dict, device="cuda:0", lr=1.0, momentum=0.9, weight_decay=0.0, process_group=None, world_size=1, precision="fp32",
                 rarity_weight=True, num_parts=15, anchors=ANCHORS):
        if precision != "fp32":
            raise ValueError("YoloTrainEngine computes in fp32 only, got precision %r" % (precision,))
        # the NCHW engine of TrainEngine: every product an exact fp32 FMA chain
        super().__init__(state_dict, device=device, lr=lr, momentum=momentum, weight_decay=weight_decay, process_group=process_group,
                         world_size=world_size, precision="fp32-nchw")
        self.precision = "fp32"
        self.rarity_weight = bool(rarity_weight)
        self.num_parts, self.anchors = int(num_parts), [tuple(a) for a in anchors]
        self.n_out = len(self.anchors) * (5 + 3 * self.num_parts)
        if tuple(self.p["model2_4.0.weight"].shape[:2]) != (self.n_out, 128):
            raise _lib.PopnetError("popnet_amd.train_yolo: model2_4.0.weight is %s, expected [%d, 128, 3, 3] for %d anchors and %d joints"
                                   % (tuple(self.p["model2_4.0.weight"].shape), self.n_out, len(self.anchors), self.num_parts))
        # model0.layer3 never runs: its BatchNorm statistics and counters stay as loaded (carried in self.extra)
        self.stats = {k: v for k, v in self.stats.items() if not k.startswith("model0.layer3")}
        self.tracked = {k: v for k, v in self.tracked.items() if not k.startswith("model0.layer3")}
        self.loss_terms = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.out = None        # the cast module output of the last step [N, A(5+3J), H/16, W/16]

    @classmethod
    def from_module(cls, module, **kw):
        """From a popnet_amd.network.yolo_posenet.YoloPoseNet (or the reference's own module); module.load_state_dict(engine.state_dict())
        hands the trained weights back to the inference path."""
        kw.setdefault("num_parts", module.num_parts)
        kw.setdefault("anchors", [tuple(float(v) for v in a) for a in module.anchors])
        return cls(module.state_dict(), **kw)

    def _trainer(self, N, H, W):
        raise _lib.PopnetError("popnet_amd.train_yolo: YoloPoseNet has no planes engine")

    def capture(self, *a, **k):
        raise _lib.PopnetError("popnet_amd.train_yolo: the YoloPoseNet step is not captured as a hipGraph; call step()")

    def _block(self, p, x, stride=1):
        """BasicBlock of resnet34 (conv1 and the 1x1 downsample carry the stride)"""
        a1 = self._bn(p + ".bn1", self._conv(p + ".conv1", x, 3, stride, 1), ACT_RELU)
        c2 = self._conv(p + ".conv2", a1, 3, 1, 1)
        idn = x
        if (p + ".downsample.0.weight") in self.p:
            idn = self._bn(p + ".downsample.1", self._conv(p + ".downsample.0", x, 1, stride, 0), ACT_NONE)
        self.A["stride:" + p] = stride
        return self._bn(p + ".bn2", c2, ACT_RELU, res=idn)

    def _block_bwd(self, p, dout):
        stride = self.A["stride:" + p]
        x = self.A["x:" + p + ".conv1"]
        dx = self._buf("dx:" + p, x.shape)
        if (p + ".downsample.0.weight") in self.p:
            didn = self._buf("di:" + p, dout.shape)
            dc2 = self._bn_bwd(p + ".bn2", dout, dres=didn)
            dcd = self._bn_bwd(p + ".downsample.1", didn)
            self._conv_bwd(p + ".downsample.0", dcd, 1, stride, 0, dx=dx, accumulate=False)
        else:
            dc2 = self._bn_bwd(p + ".bn2", dout, dres=dx)              # identity path: dx = g
        da1 = self._conv_bwd(p + ".conv2", dc2, 3, 1, 1)
        dc1 = self._bn_bwd(p + ".bn1", da1)
        self._conv_bwd(p + ".conv1", dc1, 3, stride, 1, dx=dx, accumulate=True)
        return dx

    def _layer_names(self, layer):
        n = 0
        while ("model0.%s.%d.conv1.weight" % (layer, n)) in self.p:
            n += 1
        return ["model0.%s.%d" % (layer, i) for i in range(n)]

    # ---- the step ----
    def forward_backward(self, img, prior_map, mask_conf, mask_coord, weight_map=None):
        """Fills self.flat_g (this replica's gradient of loss_prior) and self.loss_terms [4] (LOSS_NAMES); updates the BN running statistics;
        self.out holds the cast module output.  weight_map is required when rarity_weight is True and ignored otherwise."""
        if self.rarity_weight and weight_map is None:
            raise _lib.PopnetError("popnet_amd.train_yolo: rarity_weight=True needs prior_weight_map")
        batch = [(img, "img"), (prior_map, "prior_map"), (mask_conf, "prior_mask_conf"), (mask_coord, "prior_mask_coord")]
        if self.rarity_weight:
            batch.append((weight_map, "prior_weight_map"))
        for t, n in batch:
            _lib.require_cuda_tensor(t, n)
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.PopnetError("popnet_amd.train_yolo: %s must be a contiguous float32 tensor" % n)
        N, _, H, W = img.shape
        if H % 16 or W % 16:
            raise _lib.PopnetError("popnet_amd.train_yolo: input size must be a multiple of 16")
        A, h, w = len(self.anchors), H // 16, W // 16
        if tuple(prior_map.shape) != (N, self.n_out, h, w):
            raise _lib.PopnetError("popnet_amd.train_yolo: prior_map must be [%d, %d, %d, %d]" % (N, self.n_out, h, w))
        for t, n in batch[2:]:
            if tuple(t.shape) != (N, A, h, w):
                raise _lib.PopnetError("popnet_amd.train_yolo: %s must be [%d, %d, %d, %d]" % (n, N, A, h, w))
        self.A = {}
        L, ctx, s = self.L, self.ctx.handle, self._s()
        self._check(L.pn_train_pack_refresh(ctx, s), "pn_train_pack_refresh")       # every cached weight pack, one launch (whatever changed the weights)
        # forward (yolo_posenet.py:43-54, 137-158)
        a = self._bn("model0.bn1", self._conv("model0.conv1", img, 7, 2, 3), ACT_RELU)
        a = self._maxpool("stem", a, 3, 2, 1)
        l1, l2 = self._layer_names("layer1"), self._layer_names("layer2")
        for p in l1:
            a = self._block(p, a)
        for i, p in enumerate(l2):
            a = self._block(p, a, 2 if i == 0 else 1)
        a = self._stage("model1", a)                                     # conv BN LeakyReLU x 4 + the bare conv 12
        a = self._bn("model2_1.1", self._conv("model2_1.0", a, 3, 1, 1), ACT_LEAKY)
        a = self._maxpool("model2_1", a, 2, 2, 0)
        a = self._bn("model2_2.1", self._conv("model2_2.0", a, 3, 1, 1), ACT_LEAKY)
        a = self._bn("model2_3.1", self._conv("model2_3.0", a, 3, 1, 1), ACT_LEAKY)
        v = self._conv("model2_4.0", a, 3, 1, 1)
        out = self.out = self._buf("out", v.shape)
        dv = self._buf("dv", v.shape)
        self._check(L.pn_yolo_loss(ctx, self._ptr(v), self._ptr(prior_map), self._ptr(mask_conf), self._ptr(mask_coord),
                                   self._ptr(weight_map) if self.rarity_weight else None, N, A, self.num_parts, h, w, self._ptr(out),
                                   self._ptr(self.loss_terms), self._ptr(dv), s), "pn_yolo_loss")
        # backward
        d = self._conv_bwd("model2_4.0", dv, 3, 1, 1)
        d = self._conv_bwd("model2_3.0", self._bn_bwd("model2_3.1", d), 3, 1, 1)
        d = self._conv_bwd("model2_2.0", self._bn_bwd("model2_2.1", d), 3, 1, 1)
        d = self._maxpool_bwd("model2_1", d)
        d = self._conv_bwd("model2_1.0", self._bn_bwd("model2_1.1", d), 3, 1, 1)
        dm = self._buf("dmodel1", self.A["x:model1.0"].shape)
        self._stage_bwd("model1", d, dm, accumulate=False)
        d = dm
        for p in reversed(l2):
            d = self._block_bwd(p, d)
        for p in reversed(l1):
            d = self._block_bwd(p, d)
        d = self._maxpool_bwd("stem", d)
        self._conv_bwd("model0.conv1", self._bn_bwd("model0.bn1", d), 7, 2, 3, need_dx=False)
        for k in self.tracked:
            self.tracked[k] += 1
        return self.loss_terms

    def step(self, img, prior_map, mask_conf, mask_coord, weight_map=None):
        """-> device tensor [4] of loss terms (LOSS_NAMES); loss_prior is the total.  Asynchronous."""
        terms = self.forward_backward(img, prior_map, mask_conf, mask_coord, weight_map)
        self.apply()
        return terms

    def flops_per_step(self, N, H, W):
        """Algorithmic FLOPs of one step (2 per multiply-add): every convolution's forward and weight gradient, and the data gradient of every
        convolution but the first; BatchNorm, pooling and the loss are not counted."""
        total = 0.0
        h, w = H, W
        shapes = []

        def conv(name, ks, stride, pad):
            nonlocal h, w
            wt = self.p[name + ".weight"]
            Ho, Wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
            shapes.append((name, 2.0 * N * Ho * Wo * wt.shape[0] * wt.shape[1] * ks * ks))
            return Ho, Wo
        h, w = conv("model0.conv1", 7, 2, 3)
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        for layer in ("layer1", "layer2"):
            for i, p in enumerate(self._layer_names(layer)):
                st = 2 if (layer == "layer2" and i == 0) else 1
                if (p + ".downsample.0.weight") in self.p:
                    conv(p + ".downsample.0", 1, st, 0)
                h, w = conv(p + ".conv1", 3, st, 1)
                conv(p + ".conv2", 3, 1, 1)
        for i in (0, 3, 6, 9, 12):
            conv("model1.%d" % i, 3, 1, 1)
        conv("model2_1.0", 3, 1, 1)
        h, w = h // 2, w // 2
        for name in ("model2_2.0", "model2_3.0", "model2_4.0"):
            conv(name, 3, 1, 1)
        for name, f in shapes:
            total += f * (2 if name == "model0.conv1" else 3)
        return total
