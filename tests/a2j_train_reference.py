"""Plain-torch statement of what the A2J training path computes, written for the tests (CPU, fp64 or fp32; no HIP code involved):

  forward_train   A2J_model.forward in train mode (third_party_methods/A2J_experiments/model.py:152-186, resnet.py Bottleneck): the depth
                  channel expanded to three, ResNet-50 with conv2 of layer4.1 / layer4.2 at dilation 2, three heads, BatchNorm on batch
                  statistics (running statistics updated in the state dict it is given), the heads in the reference's [B, K, P] layout
  a2j_loss        A2J_loss.forward (anchor.py:84-154), with switches that inject the faults the tests must be able to see
  adam_step       torch.optim.Adam's update (L2 weight decay) on arrays
  dilated_conv    F.conv2d with dilation, and its two gradients
  smooth_l1       the loss's element function
  loss_fp64       a2j_loss and its gradients in fp64 on NCHW (or flat) head maps, with the per-element error bound of an fp32 evaluation
"""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = (("layer1", 3, 1, 1), ("layer2", 4, 2, 1), ("layer3", 6, 2, 1), ("layer4", 3, 1, 2))      # name, blocks, stride of block 0, dilation of blocks >= 1
HEADS = ("classificationModel", "regressionModel", "DepthRegressionModel")
U = 2.0 ** -24


def smooth_l1(d):
    return torch.where(d <= 1, 0.5 * d * d, d - 0.5)


def _bn(x, sd, name, momentum=0.1, eps=1e-5):
    """train-mode BatchNorm2d; updates sd[name + '.running_*'] / num_batches_tracked in place like the module"""
    rm, rv = sd[name + ".running_mean"], sd[name + ".running_var"]
    y = F.batch_norm(x, rm, rv, sd[name + ".weight"], sd[name + ".bias"], True, momentum, eps)
    if name + ".num_batches_tracked" in sd:
        sd[name + ".num_batches_tracked"] += 1
    return y


def forward_train(sd, x, num_anchors=16, num_classes=15):
    """sd: state dict of tensors in x's dtype (parameters may require grad; BatchNorm buffers are updated in place).  x [B, 1, H, W].
    -> (cls [B, K, P], reg [B, K, P, 2], dep [B, K, P]), (raw NCHW maps of the three heads)"""
    B, _, H, W = x.shape
    pre = "Backbone.model."
    a = F.conv2d(x.expand(B, 3, H, W), sd[pre + "conv1.weight"], stride=2, padding=3)
    a = F.max_pool2d(F.relu(_bn(a, sd, pre + "bn1")), 3, 2, 1)
    feats = {}
    for lname, blocks, stride, dil in LAYERS:
        for i in range(blocks):
            n = "%s%s.%d." % (pre, lname, i)
            s, d = (stride, 1) if i == 0 else (1, dil)
            y = F.relu(_bn(F.conv2d(a, sd[n + "conv1.weight"]), sd, n + "bn1"))
            y = F.relu(_bn(F.conv2d(y, sd[n + "conv2.weight"], stride=s, padding=d, dilation=d), sd, n + "bn2"))
            y = _bn(F.conv2d(y, sd[n + "conv3.weight"]), sd, n + "bn3")
            idn = a
            if n + "downsample.0.weight" in sd:
                idn = _bn(F.conv2d(a, sd[n + "downsample.0.weight"], stride=s), sd, n + "downsample.1")
            a = F.relu(y + idn)
        feats[lname] = a
    raw = []
    for hname, feat in zip(HEADS, (feats["layer3"], feats["layer4"], feats["layer4"])):
        y = feat
        for i in (1, 2, 3, 4):
            y = F.conv2d(y, sd["%s.conv%d.weight" % (hname, i)], sd["%s.conv%d.bias" % (hname, i)], padding=1)
            y = F.relu(_bn(y, sd, "%s.bn%d" % (hname, i)))
        raw.append(F.conv2d(y, sd[hname + ".output.weight"], sd[hname + ".output.bias"], padding=1))
    h, w = H // 16, W // 16
    A, P = num_anchors, num_classes
    cls = raw[0].permute(0, 3, 2, 1).reshape(B, w, h, A, P).reshape(B, -1, P)
    reg = raw[1].permute(0, 3, 2, 1).reshape(B, w, h, A, P, 2).reshape(B, -1, P, 2)
    dep = raw[2].permute(0, 3, 2, 1).reshape(B, w, h, A, P).reshape(B, -1, P)
    return (cls, reg, dep), raw


def a2j_loss(heads, labels, anchors, spatial_factor, fault=None):
    """heads in the reference's layout, labels [B, P, 3], anchors [K, 2] -> (Cls [1], Reg [1]).
    fault: None, or one of the mistakes a test of the loss must notice: "smooth_depth" (the smooth form of the depth term, which the
    reference computes and then does not use), "swap_xy" (anchors' columns exchanged), "no_spatial_factor"."""
    cls, reg, dep = heads
    if fault == "swap_xy":
        anchors = anchors.flip(1)
    sf = 1.0 if fault == "no_spatial_factor" else spatial_factor
    w = torch.softmax(cls, 1)                                            # [B, K, P]
    gt_xy, gt_z = labels[:, :, :2], labels[:, :, 2]
    a_xy = (w.unsqueeze(3) * anchors[None, :, None, :]).sum(1)           # [B, P, 2]
    r_xy = (w.unsqueeze(3) * (anchors[None, :, None, :] + reg)).sum(1)
    z = (w * dep).sum(1)                                                 # [B, P]
    c = smooth_l1((gt_xy - a_xy).abs()).mean((1, 2))
    r = smooth_l1((gt_xy - r_xy).abs()).mean((1, 2)) * sf
    dz = (gt_z - z).abs()
    if fault == "smooth_depth":
        r = r + torch.where(dz <= 3, 0.5 * (1 / 3) * dz * dz, dz - 0.5 / (1 / 3)).mean(1)
    else:
        r = r + dz.mean(1)
    return c.mean(0, keepdim=True), r.mean(0, keepdim=True)


def nchw_to_reference(raw, A, P, two=False):
    """[B, A P (2), h, w] -> [B, K, P (, 2)], K = (x h + y) A + a"""
    B, _, h, w = raw.shape
    t = raw.permute(0, 3, 2, 1)
    return t.reshape(B, w, h, A, P, 2).reshape(B, -1, P, 2) if two else t.reshape(B, w, h, A, P).reshape(B, -1, P)


def reference_to_nchw(t, h, w, A):
    """the inverse of nchw_to_reference"""
    B, P = t.shape[0], t.shape[2]
    if t.dim() == 4:
        return t.reshape(B, w, h, A * P * 2).permute(0, 3, 2, 1).contiguous()
    return t.reshape(B, w, h, A * P).permute(0, 3, 2, 1).contiguous()


def adam_step(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, grad_scale=1.0):
    """numpy arrays in any float dtype -> (p, m, v) after step t >= 1, in that dtype's arithmetic"""
    g = grad_scale * g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    step = lr / (1 - b1 ** t)
    p = p - step * (m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps))
    return p, m, v


def dilated_conv(x, w, b, pad, dil, dy=None):
    """fp64 F.conv2d(x, w, b, padding=pad, dilation=dil) -> y, and with dy also (dx, dw, db)"""
    x = x.double().requires_grad_(dy is not None)
    w = w.double().requires_grad_(dy is not None)
    y = F.conv2d(x, w, None if b is None else b.double(), padding=pad, dilation=dil)
    if dy is None:
        return y.detach()
    dx, dw = torch.autograd.grad(y, (x, w), dy.double())
    return y.detach(), dx, dw, dy.double().sum((0, 2, 3))


def loss_fp64(cls, reg, dep, geom, anchors, labels, sf, scale):
    """fp64: terms, the gradients in the inputs' layout, and the per-element error bounds derived below"""
    B, h, w, A, P = geom
    raw = [t.double().requires_grad_() for t in (cls, reg, dep)]
    if h:
        heads = (nchw_to_reference(raw[0], A, P), nchw_to_reference(raw[1], A, P, two=True), nchw_to_reference(raw[2], A, P))
    else:
        heads = raw
    an, lab = anchors.double(), labels.double()
    c, r = a2j_loss(heads, lab, an, sf)
    grads = torch.autograd.grad(scale[0] * c + scale[1] * r, raw)
    # ---- the bound.  K = anchors per (crop, joint), u = 2^-24, eps = K u.
    # A prediction is V = N / D with N = sum_k e_k v_k, D = sum_k e_k, e_k = exp(cls_k - max).  A K-term fp32 sum in any order is within
    # K u sum|addends| of the exact sum of its addends; an addend e_k v_k itself carries e_k's error: the rounding of cls_k - max (|cls_k - max| u
    # relative in e_k), expf (2 ulp) and one product -- (3 + |cls_k - max|) u, which is <= K u on every case here (asserted), so
    #   dN <= 2 eps sum|e_k v_k|,  dD <= 2 eps D,  and through the division  dV <= dN / D + |V| dD / D + u |V| = 2 eps (sum_k w_k |v_k| + |V|) + u |V|.
    # The smooth L1 and |.| are 1-Lipschitz: an element of a term moves by at most dV (+ u-level roundings of gt - V and of the few products),
    # and a term is a weighted mean of its elements.
    with torch.no_grad():
        K = heads[0].shape[1]
        eps = K * U
        assert float((heads[0].max(1, keepdim=True)[0] - heads[0]).max()) + 3 <= K
        wk = torch.softmax(heads[0], 1)                                       # [B, K, P]
        va = an[None, :, None, :].expand(B, K, P, 2)
        vr = va + heads[1]
        vals = torch.cat([va, vr, heads[2].unsqueeze(3)], 3)                  # [B, K, P, 5]: anchor y x, anchor + reg y x, depth
        V = (wk.unsqueeze(3) * vals).sum(1)                                   # [B, P, 5]
        dV = 2 * eps * ((wk.unsqueeze(3) * vals.abs()).sum(1) + V.abs()) + U * V.abs()
        gt = torch.cat([lab[:, :, :2], lab[:, :, :2], lab[:, :, 2:]], 2)
        d = gt - V
        dV = dV + 4 * U * (gt.abs() + V.abs())                                # gt - V and the element function's own roundings
        coef = torch.tensor([1 / (2.0 * P * B)] * 2 + [sf / (2.0 * P * B)] * 2 + [1.0 / (P * B)], dtype=torch.float64)
        t_allow = torch.stack([(dV[:, :, :2] * coef[:2]).sum(), (dV[:, :, 2:] * coef[2:]).sum()]) + 8 * U * torch.stack([c, r]).reshape(2).abs()
        # gradients: g_i = s c_i f'(d_i) (f' is 1-Lipschitz; the sign of the depth term is exact while |d_z| > dV: asserted), w_k = e_k / D within 3 eps w_k,
        #   d cls_k = w_k sum_i g_i (v_ik - V_i),  d reg_k = w_k g_R,  d dep_k = w_k g_z
        assert bool((d[:, :, 4].abs() > dV[:, :, 4]).all() | (d[:, :, 4] == 0).all())
        sc = torch.tensor([scale[0]] * 2 + [scale[1]] * 3, dtype=torch.float64) * coef
        fp = torch.where(d.abs() <= 1, -d, -torch.sign(d))
        fp[:, :, 4] = -torch.sign(d[:, :, 4])
        g = sc * fp                                                           # [B, P, 5]
        dg = sc.abs() * dV
        dg[:, :, 4] = 0
        dev = (vals - V.unsqueeze(1)).abs()                                   # [B, K, P, 5]
        a_cls = wk * ((dg.unsqueeze(1) * dev).sum(3) + (g.abs() * dV).unsqueeze(1).sum(3) + (3 * eps + 8 * U) * (g.abs().unsqueeze(1) * dev).sum(3))
        a_reg = wk.unsqueeze(3) * (dg[:, :, 2:4].unsqueeze(1) + (3 * eps + 4 * U) * g[:, :, 2:4].abs().unsqueeze(1))
        a_dep = wk * (3 * eps + 4 * U) * g[:, :, 4].abs().unsqueeze(1)
        if h:
            a_cls, a_reg, a_dep = reference_to_nchw(a_cls, h, w, A), reference_to_nchw(a_reg, h, w, A), reference_to_nchw(a_dep, h, w, A)
    return torch.stack([c, r]).reshape(2).detach(), grads, t_allow, (a_cls, a_reg, a_dep)
