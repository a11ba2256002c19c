"""Plain-torch CPU restatement of one rtpose_light3d(15, 14, 2, input_dim=1) training step (fp32 or fp64, autograd for the gradients).

Written from the module's structure: model0 = 7x7/2 convolution (no bias), BatchNorm, ReLU, two BasicBlocks(64) (3x3 conv, BN, ReLU, 3x3 conv,
BN, + input, ReLU), AvgPool2d(3, 2, 1), a BasicBlock(64 -> 128) whose shortcut is a 1x1 convolution + BN, a 1x1 convolution(128) + BN + ReLU,
AvgPool2d(3, 2, 1) -> feat; two stages of three branches (paf 28, heat 16, z 15 channels), each four (conv + bias, BatchNorm,
LeakyReLU(0.1)) and a bare conv; the casts (sigmoid - 0.5) * 4 for paf and z, sigmoid for heat; stage 2 reads cat[paf1, heat1, z1, feat].
BatchNorm uses batch statistics and updates the running ones (momentum 0.1, unbiased variance).  The loss is the sum over both stages of
mse(paf) + mse(heat) + mean((z - z_gt)^2 (0.1 + 0.9 fg)).  The average pools have no data-dependent choice, so the only masks are the ReLU /
LeakyReLU ones.

The mask-forced form (forward(..., forced=...)): every ReLU / LeakyReLU takes its branch from a given mask instead of the sign of its own
pre-activation (where(m, z, slope z): derivative 1 where m is set, slope elsewhere).  With the masks of a GPU step (its stored activation > 0)
it computes, in fp64, the step that GPU run took: what is left between the two is arithmetic, not which side of zero a pre-activation
landed on.  Masks are keyed "bn:<name of the BatchNorm in front of the activation>" (a BasicBlock's output activation: its bn2), bool
[B, C, H, W].
"""
import torch
import torch.nn.functional as F

STAGES = ("model1_1", "model1_2", "model1_3", "model2_1", "model2_2", "model2_3")


def _params(sd, dtype):
    out = {}
    for k, v in sd.items():
        if k.startswith("module."):
            k = k[len("module."):]
        if k.startswith("model0.layer3") or k.endswith("num_batches_tracked"):
            continue
        t = v.detach().clone().to(dtype)
        if not (k.endswith("running_mean") or k.endswith("running_var")):
            t.requires_grad_(True)
        out[k] = t
    return out


def mask_keys():
    """Every activation of the step, in forward order."""
    keys = ["bn:model0.bn1"]
    for p in ("model0.layer1.0", "model0.layer1.1", "model0.layer2.0"):
        keys += ["bn:%s.bn1" % p, "bn:%s.bn2" % p]
    keys.append("bn:model0.bn2")
    for s in STAGES:
        keys += ["bn:%s.%d" % (s, i) for i in (1, 4, 7, 10)]
    return keys


def forward(P, x, forced=None, record=None):
    """P: {name: tensor} (running statistics updated in place) -> [paf1, heat1, z1, paf2, heat2, z2] after their casts."""
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

    def block(a, p):
        y = act(bn(conv(a, p + ".conv1"), p + ".bn1"), p + ".bn1", 0)
        y = bn(conv(y, p + ".conv2"), p + ".bn2")
        idn = bn(conv(a, p + ".downsample.0", 1, 0), p + ".downsample.1") if (p + ".downsample.0.weight") in P else a
        return act(y + idn, p + ".bn2", 0)

    def stage(a, p):
        for i in (0, 3, 6, 9):
            a = act(bn(conv(a, "%s.%d" % (p, i)), "%s.%d" % (p, i + 1)), "%s.%d" % (p, i + 1), 0.1)
        return conv(a, p + ".12")

    a = act(bn(conv(x, "model0.conv1", 2, 3), "model0.bn1"), "model0.bn1", 0)
    a = block(block(a, "model0.layer1.0"), "model0.layer1.1")
    a = F.avg_pool2d(a, 3, 2, 1)
    a = block(a, "model0.layer2.0")
    a = act(bn(conv(a, "model0.conv2"), "model0.bn2"), "model0.bn2", 0)
    feat = F.avg_pool2d(a, 3, 2, 1)
    out = [(stage(feat, "model1_1").sigmoid() - 0.5) * 4, stage(feat, "model1_2").sigmoid(), (stage(feat, "model1_3").sigmoid() - 0.5) * 4]
    cat = torch.cat(out + [feat], 1)
    return out + [(stage(cat, "model2_1").sigmoid() - 0.5) * 4, stage(cat, "model2_2").sigmoid(), (stage(cat, "model2_3").sigmoid() - 0.5) * 4]


def loss_terms(saved, heat_gt, paf_gt, z_gt, fg_mask):
    """-> tensor [6]: (paf, heat, z) of stage 1, then of stage 2."""
    w = 0.1 + 0.9 * fg_mask
    terms = []
    for j in range(2):
        terms += [((saved[3 * j] - paf_gt) ** 2).mean(), ((saved[3 * j + 1] - heat_gt) ** 2).mean(), ((saved[3 * j + 2] - z_gt) ** 2 * w).mean()]
    return torch.stack(terms)


def train_step(sd, img, heat_gt, paf_gt, z_gt, fg_mask, dtype=torch.float32, forced=None, record=None):
    """One forward + loss + backward on the CPU -> {"terms": ndarray [6], "grads": {name: tensor}, "stats": {name: tensor}, "saved": [...]}."""
    P = _params(sd, dtype)
    x, heat_gt, paf_gt, z_gt, fg_mask = (torch.as_tensor(a).to(dtype) for a in (img, heat_gt, paf_gt, z_gt, fg_mask))
    saved = forward(P, x, forced=forced, record=record)
    terms = loss_terms(saved, heat_gt, paf_gt, z_gt, fg_mask)
    terms.sum().backward()
    grads = {k: v.grad.detach().clone() for k, v in P.items() if v.requires_grad}
    stats = {k: v.detach().clone() for k, v in P.items() if not v.requires_grad}
    return {"terms": terms.detach().numpy().copy(), "grads": grads, "stats": stats, "saved": [s.detach() for s in saved]}
