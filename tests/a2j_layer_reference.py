"""fp64 host reference of one step of a compiled A2J net: tests/layer_reference.py plus what this net adds.

* Dilation: a convolution that pn_net_step_info reports with "dil": 2 (layer4 blocks 1 and 2, conv2) is
  F.conv2d(..., dilation=2, padding=2): taps at 0 and +-2.  The products, their count and the allowance rule are those of
  layer_reference.conv_ref -- only where the taps land changes -- so conv_ref runs unchanged with the convolution it calls replaced.
* The stem: ResNetBackBone.forward feeds three identical channels, net_pack.hip::pack_stem sums the [64, 3, 7, 7] weights over Cin in
  double, multiplies by the BatchNorm scale and rounds to float32: the same single-channel stem as the other nets with
  model0.conv1.weight = sum over Cin (kept in double) and model0.bn1 = Backbone.model.bn1.

dil_of(conv) -> int overrides the dilation the reference uses (the sensitivity tests: dilation 1 everywhere, or block 0 / block 1
swapped, must fail against the real kernels).
"""
import torch
import torch.nn.functional as F

import layer_reference as LR


class _DilatedF:
    """Stands in for torch.nn.functional inside layer_reference.conv_ref: padding ks // 2 becomes dil * (ks // 2)."""
    def __init__(self, dil):
        self.dil = dil

    def conv2d(self, a, w, stride=1, padding=0):
        return F.conv2d(a, w, stride=stride, padding=padding * self.dil, dilation=self.dil)

    def __getattr__(self, name):
        return getattr(F, name)


def stem_state_dict(sd):
    """The reference state dict plus the single-channel stem names layer_reference.stem_weights reads."""
    out = dict(sd)
    out["model0.conv1.weight"] = sd["Backbone.model.conv1.weight"].double().sum(1, keepdim=True)
    for leaf in ("weight", "bias", "running_mean", "running_var"):
        out["model0.bn1." + leaf] = sd["Backbone.model.bn1." + leaf]
    return out


def reported_dil(conv):
    return int(conv.get("dil", 1))


def step_reference(step, net, sd, read, x, dil_of=reported_dil):
    """Checks of one step of an A2J net; sd = stem_state_dict(reference state dict)."""
    if step["type"] != "conv":
        return LR.step_reference(step, net, sd, read, x)
    dils = {dil_of(c) for c in step["convs"]}
    assert len(dils) == 1, "a launch shares one dilation"
    dil = dils.pop()
    if dil == 1:
        return LR.step_reference(step, net, sd, read, x)
    saved = LR.F
    LR.F = _DilatedF(dil)
    try:
        return LR.step_reference(step, net, sd, read, x)
    finally:
        LR.F = saved


def swapped_block_dil(conv):
    """layer4 with the dilation on block 0 instead of block 1 (block 2 keeps it)."""
    if conv["w"] == "Backbone.model.layer4.0.conv2":
        return 2
    if conv["w"] == "Backbone.model.layer4.1.conv2":
        return 1
    return reported_dil(conv)
