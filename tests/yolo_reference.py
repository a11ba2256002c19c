"""Plain-torch CPU restatement of YoloPoseNet in train mode and of its prior losses (fp32 or fp64, autograd for the gradients).

Written from the module's structure, not from its code: model0 = 7x7/2 convolution, BatchNorm, ReLU, MaxPool2d(3, 2, 1), resnet34's
layer1 (3 BasicBlocks, 64) and layer2 (4 BasicBlocks, 128, the first at stride 2 with a 1x1/2 downsample) -- layer3 is never run;
model1 = four (3x3 conv + bias, BatchNorm, LeakyReLU(0.1)) and a bare 3x3 conv; model2_1 = conv, BN, LeakyReLU, MaxPool2d(2, 2);
model2_2 / model2_3 = conv, BN, LeakyReLU; model2_4 = conv to A (5 + 3J) channels; then the per-anchor casts (xy (s - 0.5) 2,
wh 2 s, conf s, joints (s - 0.5) 4 of s = sigmoid).  BatchNorm uses batch statistics and updates the running ones (momentum 0.1).
The losses: coord / obj / selfpose mean squared errors with the masks as weights (plain) or multiplied into both sides and the
pose weight map as weight (pose-weighted); x 4 for coord, x 3J for selfpose; loss_prior their sum.
The mask-forced form (forward(..., forced=...)): every ReLU / LeakyReLU takes its branch from a given mask instead of the sign of its own
pre-activation (where(m, z, slope z): derivative 1 where m is set, slope elsewhere) and every max pool takes its value and routes its gradient
through a given flat index per window (gather) instead of its own argmax.  With the masks and indices of a GPU step it computes, in fp64, the
step that GPU run took: what is left between the two is arithmetic, not which side of zero a pre-activation landed on.
Also the seeded prior targets of the training goldens (tests/golden/make_golden_yolo.py imports them from here).
"""
import numpy as np
import torch
import torch.nn.functional as F

NUM_JOINTS = 15
ANCHORS = [(6., 3.), (12., 6.)]


def yolo_case_targets(seed=41, B=3, H=96, W=128, A=2, J=NUM_JOINTS):
    """Seeded prior targets for a [B, 1, H, W] batch: prior_map [B, A(5+3J), H/16, W/16], masks and weight map [B, A, H/16, W/16]."""
    rng = np.random.default_rng(seed)
    h, w = H // 16, W // 16
    prior = rng.uniform(-1, 1, (B, A * (5 + 3 * J), h, w)).astype(np.float32)
    coord = (rng.uniform(0, 1, (B, A, h, w)) < 0.25).astype(np.float32)
    conf = (0.1 + 0.9 * coord).astype(np.float32)
    weight = rng.uniform(0.5, 2.0, (B, A, h, w)).astype(np.float32)
    return prior, conf, coord, weight


def _params(sd, dtype, requires_grad=True):
    out = {}
    for k, v in sd.items():
        if k.startswith("module."):
            k = k[len("module."):]
        if k.startswith("model0.layer3") or k.endswith("num_batches_tracked"):
            continue
        t = v.detach().clone().to(dtype)
        if not (k.endswith("running_mean") or k.endswith("running_var")):
            t.requires_grad_(requires_grad)
        out[k] = t
    return out


def forward(P, x, num_parts=NUM_JOINTS, anchors=ANCHORS, forced=None, record=None):
    """P: {name: tensor} (parameters with requires_grad, running statistics updated in place) -> cast output [B, A(5+3J), H/16, W/16].
    Masks and indices are keyed like YoloTrainEngine's: "bn:<BatchNorm name>" -> bool [B, C, H, W] (the activation after that BatchNorm
    passes z, else takes slope z), "mp:stem" / "mp:model2_1" -> int [B, C, Ho, Wo] (flat index into the pool's input plane).
    forced: the mask-forced form (module docstring) with these; record: a dict that receives this evaluation's own (z > 0, argmax)."""
    def conv(a, n, stride=1, pad=None):
        w = P[n + ".weight"]
        return F.conv2d(a, w, P.get(n + ".bias"), stride, w.shape[-1] // 2 if pad is None else pad)

    def bn(a, n):
        return F.batch_norm(a, P[n + ".running_mean"], P[n + ".running_var"], P[n + ".weight"], P[n + ".bias"], True, 0.1, 1e-5)

    def act(z, n, slope):
        if record is not None:
            record["bn:" + n] = (z > 0).detach()
        if forced is None:
            return F.relu(z) if slope == 0 else F.leaky_relu(z, slope)
        return torch.where(forced["bn:" + n].to(torch.bool), z, z * slope)

    def pool(a, n, k, stride, pad):
        if forced is None and record is None:
            return F.max_pool2d(a, k, stride, pad)
        y, idx = F.max_pool2d(a, k, stride, pad, return_indices=True)
        if record is not None:
            record["mp:" + n] = idx
        if forced is None:
            return y
        i = forced["mp:" + n].to(torch.long)
        return a.flatten(2).gather(2, i.flatten(2)).view(i.shape)

    def block(a, p, stride):
        y = act(bn(conv(a, p + ".conv1", stride), p + ".bn1"), p + ".bn1", 0)
        y = bn(conv(y, p + ".conv2"), p + ".bn2")
        idn = bn(conv(a, p + ".downsample.0", stride, 0), p + ".downsample.1") if (p + ".downsample.0.weight") in P else a
        return act(y + idn, p + ".bn2", 0)

    a = pool(act(bn(conv(x, "model0.conv1", 2, 3), "model0.bn1"), "model0.bn1", 0), "stem", 3, 2, 1)
    for layer, n, first_stride in (("layer1", 3, 1), ("layer2", 4, 2)):
        for i in range(n):
            a = block(a, "model0.%s.%d" % (layer, i), first_stride if i == 0 else 1)
    for i in (0, 3, 6, 9):
        a = act(bn(conv(a, "model1.%d" % i), "model1.%d" % (i + 1)), "model1.%d" % (i + 1), 0.1)
    a = conv(a, "model1.12")
    a = pool(act(bn(conv(a, "model2_1.0"), "model2_1.1"), "model2_1.1", 0.1), "model2_1", 2, 2, 0)
    for m in ("model2_2", "model2_3"):
        a = act(bn(conv(a, m + ".0"), m + ".1"), m + ".1", 0.1)
    v = conv(a, "model2_4.0")
    B, _, h, w = v.shape
    s = v.view(B, len(anchors), 5 + 3 * num_parts, h, w).sigmoid()
    out = torch.cat([(s[:, :, :2] - 0.5) * 2, s[:, :, 2:4] * 2, s[:, :, 4:5], (s[:, :, 5:] - 0.5) * 4], 2)
    return out.view(v.shape)


def loss_terms(out, prior, conf, coord, weight=None, num_joints=NUM_JOINTS, num_anchors=2):
    """-> tensor [4]: loss_prior, loss_bbox, loss_obj, loss_selfpose (pose-weighted when weight is given)."""
    B, _, h, w = out.shape
    o, t = out.reshape(B, num_anchors, -1, h, w), prior.reshape(B, num_anchors, -1, h, w)
    mc, mf = coord.unsqueeze(2), conf.unsqueeze(2)
    wm = None if weight is None else weight.unsqueeze(2)

    def err(sl, m):
        if wm is None:
            return ((o[:, :, sl] - t[:, :, sl]) ** 2 * m).mean()
        return ((o[:, :, sl] * m - t[:, :, sl] * m) ** 2 * wm).mean()
    c = err(slice(0, 4), mc) * 4
    ob = err(slice(4, 5), mf)
    sp = err(slice(5, None), mc) * (3 * num_joints)
    return torch.stack([c + ob + sp, c, ob, sp])


def train_step(sd, img, prior, conf, coord, weight=None, dtype=torch.float32, forced=None, record=None):
    """One forward + loss + backward on the CPU -> {"terms": ndarray [4], "grads": {name: tensor}, "out": tensor, "stats": {name: tensor}}.
    forced / record: as in forward()."""
    P = _params(sd, dtype)
    x = torch.as_tensor(img).to(dtype)
    cast = [None if a is None else torch.as_tensor(a).to(dtype) for a in (prior, conf, coord, weight)]
    out = forward(P, x, forced=forced, record=record)
    terms = loss_terms(out, *cast)
    terms[0].backward()
    grads = {k: v.grad.detach().clone() for k, v in P.items() if v.requires_grad}
    stats = {k: v.detach().clone() for k, v in P.items() if not v.requires_grad}
    return {"terms": terms.detach().numpy().copy(), "grads": grads, "out": out.detach(), "stats": stats}
