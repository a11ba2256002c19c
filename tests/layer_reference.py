"""fp64 host reference of one step of a compiled net (pn_net_step_info), with a per-element error allowance.

The reference computes, in float64 on the CPU, exactly the operation the kernels define on the operands they
actually read -- so a kernel may sum in any order, tile any way, and still pass, while a wrong operand moves the
result by far more than the allowance.  How the kernels define their operands (read from the packing / launch code):

* Folded weights (net_pack.hip::prepare_conv): s = gamma / sqrt(var + 1e-5) in double, w_f = float32(w * s) with
  the product in double.  bf16 packs RNE(w_f); bf16x3 packs W_hi = RNE(w_f) and W_lo = RNE(float32(w_f - W_hi)) and
  the K loop reads [x_hi | x_lo | x_hi] against [W_hi | W_hi | W_lo]: x_hi W_hi + x_lo W_hi + x_hi W_lo, with NO
  x_lo W_lo term.  fp32 packs w_f.  The bias is float32((b - mean) * s + beta) (b = 0 without a conv bias); a conv
  without BatchNorm uses float32(b).
* Epilogue (conv_common.h for conv_mfma_kernel / conv3_kernel / conv4_kernel; bb64*_kernel.h): acc + bias, then + residual
  (bf16x3: + hi, then + lo), then the activation: ReLU, LeakyReLU v * 0.1f (the float32 constant), sigmoid
  1 / (1 + expf(-v)) and its casts (rtpose heads: (s - 0.5) * 4 and s; YOLO head: by channel within an anchor of
  5 + 3J channels, (s - 0.5) * 2, s * 2, s, (s - 0.5) * 4).  Then the store: bf16 RNE, or the two planes
  hi = RNE(v), lo = RNE(v - hi); fp32 buffers and the NCHW heads store v.
* Special cases:
  - 1x1 tails (net_pack.hip::pack_tail, conv3_kernel.h TAIL == 1): the 128-channel tile after its activation is rounded
    to bf16 in LDS; the tail reads it against raw RNE(w) (no BatchNorm) plus float32(bias).
  - embed3: a 1x1 stride-2 convolution packed as the centre tap of a 3x3 one: the same products plus exact zeros.
  - stage-2 input-channel map: buffer channel i carries reference channel cin_map[i]; -1 (the pad channels) has
    zero weights.
  - bb64 / bb64x3: the first conv's output (bias, ReLU) is rounded to bf16 (bf16x3: two planes) in LDS and read by
    the second conv, whose residual is the first conv's input.
  - stems (conv_misc.hip): bf16 rounds the fp32 image to x_hi = RNE(x), bf16x3 also keeps x_lo = RNE(x - x_hi);
    weights float32(w * s) split as above; bias float32((0 - mean) * s + beta); ReLU.  fp32: an fmaf chain.
    stem7x7_pool_kernel takes the MaxPool2d(3, 2, 1) of the bf16-rounded stem output.  The multi-channel stem is
    the fp32 pn_conv2d_forward followed by nchw_relu_to_nhwc (ReLU, then the store).
  - pools (pool_kernel): AvgPool2d(3, 2, 1, count_include_pad) as an fp32 sum of the nine taps (hi + lo in
    bf16x3), then / 9.0f; max pools take the max, which is exact.  The fused pool tail (conv3_kernel.h TAIL == 2)
    does the same on the conv's stored-format values.

Allowance: |gpu - r| <= half_ulp_store(|r| + delta) + delta.  delta bounds fp32 rounding before the store:
  n * 2^-24 * S, S = sum of |every product and addend| (a second fp64 convolution of |w| and |x|), n = the number
  of terms (products + bias + residual planes).  This is the worst-case bound of ANY fp32 summation order of n
  terms (each term passes at most n - 1 roundings), so it holds for every K-loop order, tiling or MFMA-internal
  order and does not need to know any of them.  It is not tightened further: the MFMA's internal order of its 32
  products is not specified, and with the bf16 store's half ulp (2^-9 relative) on top it is still far below one
  k-step of the K loop (32 products), which is what the sensitivity tests check it rejects.
  Activations: LeakyReLU adds one rounding; the sigmoid casts are 1/4-Lipschitz in v and add 9 fp32 ulps of the
  result for expf, the add, the division and the subtraction, times the cast's scale.
  Intermediates the GPU never stores (tail tile, bb64 intermediate, fused pools) carry their own full allowance
  e into the next operation: + conv(e, |W|) (+ 2^-7 conv(|x|, |W_lo|) in bf16x3, for the split of an uncertain
  value); the max pool of an intermediate is within the max of e over the window.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIG_PM2, ACT_SIG, ACT_YOLO = 0, 1, 2, 3, 4, 5
LEAKY = float(np.float32(0.1))


# ---- number formats ---------------------------------------------------------------------------
def rne_bf16(t):
    """float tensor -> float64 tensor holding RNE(bf16) of its float32 value."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def f32(t):
    return t.to(torch.float32).to(torch.float64)


def half_ulp(a, fmt):
    """Half a unit in the last place of the stored format at magnitude a (float64 tensor >= 0)."""
    _, e = torch.frexp(a)
    shift = {"bf16": 9, "x3": 17, "fp32": 25}[fmt]        # bf16x3: the lo plane's half ulp at |v - hi| <= half_ulp_bf16(v)
    h = torch.ldexp(torch.ones_like(a), (e - shift).to(torch.float64))
    return torch.where(a > 0, h, torch.zeros_like(a))


class Act:
    """An activation the next operation reads: v = its exact value, hi = its bf16x3 hi plane, e = uncertainty
    (0 for a value read back from the GPU; the allowance of an intermediate the GPU kept on chip)."""
    def __init__(self, v, hi=None, e=None):
        self.v, self.hi = v, hi
        self.e = torch.zeros_like(v) if e is None else e

    def sub(self, c0, n):
        return Act(self.v[:, c0:c0 + n], None if self.hi is None else self.hi[:, c0:c0 + n], self.e[:, c0:c0 + n])


def intermediate(r, allow, fmt):
    """The on-chip stored-format value of a reference result r held to allowance `allow`."""
    hi = rne_bf16(r) if fmt == "x3" else None
    return Act(r, hi, allow)


# ---- operands -----------------------------------------------------------------------------------
def fold(sd, wname, bn, cout, use_bias=True):
    scale = np.ones(cout)
    b = sd.get(wname + ".bias") if use_bias else None
    shift = np.zeros(cout) if b is None else b.double().numpy().copy()
    if bn:
        g, be = sd[bn + ".weight"].double().numpy(), sd[bn + ".bias"].double().numpy()
        mu, var = sd[bn + ".running_mean"].double().numpy(), sd[bn + ".running_var"].double().numpy()
        scale = g / np.sqrt(var + 1e-5)
        shift = (shift - mu) * scale + be
    return torch.from_numpy(scale), f32(torch.from_numpy(shift))


def conv_weights(sd, c, prec, cin_used):
    """Folded weights of conv spec c as the kernels hold them, laid out over the cin_used buffer channels it reads:
    [W] (bf16 / fp32) or [W_hi, W_lo] (bf16x3), float64 [cout, cin_used, k, k]; and the float32 bias."""
    w = sd[c["w"] + ".weight"].double()
    cout, cin_ref = w.shape[0], w.shape[1]
    scale, bias = fold(sd, c["w"], c["bn"], cout)
    wf = f32(w * scale.view(-1, 1, 1, 1))
    cmap = c["cin_map"] or list(range(cin_ref))
    W = torch.zeros((cout, cin_used) + tuple(wf.shape[2:]), dtype=torch.float64)
    for i, m in enumerate(cmap[:cin_used]):
        if m >= 0:
            W[:, i] = wf[:, m]
    used = sum(1 for m in cmap[:cin_used] if m >= 0)
    if prec == "fp32":
        return [W], bias, used
    hi = rne_bf16(W)
    if prec == "bf16":
        return [hi], bias, used
    return [hi, rne_bf16(f32(W - hi))], bias, used


def apply_act(pre, delta, act, naf=0):
    """(r, delta) after the activation."""
    if act == ACT_NONE:
        return pre, delta
    if act == ACT_RELU:
        return pre.clamp_min(0), delta
    if act == ACT_LEAKY:
        r = torch.where(pre > 0, pre, pre * LEAKY)
        return r, delta + U * (r.abs() + delta)
    s = torch.sigmoid(pre)
    if act == ACT_SIG:
        return s, 0.25 * delta + 9 * U
    if act == ACT_SIG_PM2:
        return (s - 0.5) * 4, 4 * (0.25 * delta + 9 * U)
    assert act == ACT_YOLO
    f = (torch.arange(pre.shape[1]) % naf).view(1, -1, 1, 1)
    r = torch.where(f < 2, (s - 0.5) * 2, torch.where(f < 4, s * 2, torch.where(f == 4, s, (s - 0.5) * 4)))
    scale = torch.where(f < 4, 2.0, torch.where(f == 4, 1.0, 4.0)).to(torch.float64)
    return r, scale * (0.25 * delta + 9 * U)


def conv_ref(x, W, bias, used, ks, stride, act, res=None, naf=0, x3_res=False):
    """x: Act over the channels W covers.  Returns (r, delta): the exact result of the kernel's operation on its
    operands after the activation, and the bound on its fp32 error before the store."""
    pad = ks // 2
    conv = lambda a, w: F.conv2d(a, w, stride=stride, padding=pad)
    xa = x.v.abs() + x.e
    if len(W) == 1:
        pre = conv(x.v, W[0])
        S = conv(xa, W[0].abs())
        E = conv(x.e, W[0].abs())
        n = used * W[0].shape[2] * W[0].shape[3]
    else:
        hi = x.hi if x.hi is not None else rne_bf16(x.v)
        pre = conv(x.v, W[0]) + conv(hi, W[1])                       # x_hi W_hi + x_lo W_hi + x_hi W_lo
        S = conv(hi.abs() + (x.v - hi).abs() + x.e, W[0].abs()) + conv(hi.abs(), W[1].abs())
        E = conv(x.e, W[0].abs() + W[1].abs())
        if bool((x.e > 0).any()):                                    # an on-chip value: its hi plane may be one bf16 ulp off
            E = E + 2.0 ** -7 * conv(xa, W[1].abs())
        n = 3 * used * W[0].shape[2] * W[0].shape[3]
    b = bias.view(1, -1, 1, 1)
    pre = pre + b
    S = S + b.abs()
    n += 1
    if res is not None:
        pre = pre + res
        S = S + res.abs()
        n += 2 if x3_res else 1
    return apply_act(pre, n * U * S + E, act, naf)


def avgpool_ref(x):
    """AvgPool2d(3, 2, 1, count_include_pad) of Act x: (r, delta)."""
    r = F.avg_pool2d(x.v, 3, 2, 1, count_include_pad=True)
    S = 9 * F.avg_pool2d(x.v.abs() + x.e, 3, 2, 1, count_include_pad=True)
    E = F.avg_pool2d(x.e, 3, 2, 1, count_include_pad=True)
    d = 8 * U * S / 9 + E
    return r, d + U * (r.abs() + d)


def maxpool_ref(x, mode):
    k, s, p = (3, 2, 1) if mode == 1 else (2, 2, 0)
    return F.max_pool2d(x.v, k, s, p), F.max_pool2d(x.e, k, s, p)


def allowance(r, delta, fmt):
    return delta + half_ulp(r.abs() + delta, fmt)


# ---- steps ----------------------------------------------------------------------------------------
class Check:
    """One compared output: GPU location (("buf", index, coff) or ("nchw", slot)) and the reference."""
    def __init__(self, name, where, r, allow):
        self.name, self.where, self.r, self.allow = name, where, r, allow


def stem_weights(sd, prec, cin):
    w = sd["model0.conv1.weight"].double()
    scale, _ = fold(sd, "model0.conv1", "model0.bn1", 64, use_bias=False)
    _, bias = fold(sd, "model0.conv1", "model0.bn1", 64, use_bias=False)
    wf = f32(w * scale.view(-1, 1, 1, 1))
    if prec == "fp32" or cin > 1:
        return [wf], bias
    hi = rne_bf16(wf)
    return ([hi], bias) if prec == "bf16" else ([hi, rne_bf16(f32(wf - hi))], bias)


def step_reference(step, net, sd, read, x, naf=0):
    """Checks of one step.  read(buf) -> Act of the whole buffer before the step (selected frames); x: the fp32
    input frames (float64 [F, Cin, H, W]).  net: pn_net_step_info(-1)."""
    prec = net["prec"]
    fmt = "x3" if prec == "bf16x3" else prec
    out = []
    if step["type"] == "stem":
        cin = step["cin"]
        W, bias = stem_weights(sd, prec, cin)
        if prec == "fp32" or cin > 1:
            xin = Act(x)
        else:
            hi = rne_bf16(x)
            xin = Act(hi if prec == "bf16" else hi + rne_bf16(f32(x - hi)), hi)
        r, d = conv_ref(xin, W, bias, cin, 7, 2, ACT_RELU)
        if step["pool_buf"] >= 0:
            rp, ep = maxpool_ref(intermediate(r, allowance(r, d, fmt), fmt), 1)
            out.append(Check("stem+maxpool", ("buf", step["pool_buf"], 0), rp, ep))
        else:
            out.append(Check("stem", ("buf", step["out_buf"], 0), r, allowance(r, d, fmt)))
        return out
    if step["type"] == "pool":
        xin = read(step["in_buf"]).sub(0, step["C"])
        if step["mode"] == 0:
            r, d = avgpool_ref(xin)
        else:
            r, d = maxpool_ref(xin, step["mode"])
        out.append(Check("pool%d" % step["mode"], ("buf", step["out_buf"], step["out_coff"]), r, allowance(r, d, fmt)))
        return out
    convs = step["convs"]
    if step["type"] == "bblock":
        a, b = convs
        xa = read(a["in_buf"]).sub(0, 64)
        W, bias, used = conv_weights(sd, a, prec, 64)
        r, d = conv_ref(xa, W, bias, used, 3, 1, ACT_RELU)
        mid = intermediate(r, allowance(r, d, fmt), fmt)
        W, bias, used = conv_weights(sd, b, prec, 64)
        r, d = conv_ref(mid, W, bias, used, 3, 1, ACT_RELU, res=xa.v, x3_res=fmt == "x3")
        out.append(Check(b["w"], ("buf", b["out_buf"], b["out_coff"]), r, allowance(r, d, fmt)))
        return out
    for c in convs:
        buf = read(c["in_buf"])
        cin_used = len(c["cin_map"]) if c["cin_map"] else sd[c["w"] + ".weight"].shape[1]
        if fmt == "x3":
            cin_used = min(max(cin_used, 0), buf.v.shape[1])
        xin = buf.sub(c["in_coff"], cin_used)
        W, bias, used = conv_weights(sd, c, prec, cin_used)
        res = read(c["res_buf"]).v[:, c["res_coff"]:c["res_coff"] + c["cout"]] if c["res_buf"] >= 0 else None
        r, d = conv_ref(xin, W, bias, used, c["ks"], c["stride"], c["act"], res=res, naf=naf, x3_res=fmt == "x3")
        if c["tail"] is not None:
            t = c["tail"]
            mid = intermediate(r, allowance(r, d, "bf16"), "bf16")
            wt = rne_bf16(sd[t["w"] + ".weight"].double())
            bt = sd.get(t["w"] + ".bias")
            bt = f32(bt.double()) if bt is not None else torch.zeros(t["cout"], dtype=torch.float64)
            r, d = conv_ref(mid, [wt], bt, wt.shape[1], 1, 1, t["act"], naf=naf)
            c = dict(c, w=t["w"], out_buf=t["out_buf"], out_coff=t["out_coff"], nchw_slot=t["nchw_slot"])
        elif c["pool"] is not None:
            r, d = avgpool_ref(intermediate(r, allowance(r, d, fmt), fmt))
            c = dict(c, out_buf=c["pool"]["out_buf"], out_coff=c["pool"]["out_coff"], nchw_slot=-1)
        if c["out_buf"] >= 0:
            out.append(Check(c["w"], ("buf", c["out_buf"], c["out_coff"]), r, allowance(r, d, fmt)))
        if c["nchw_slot"] >= 0:
            out.append(Check(c["w"] + " (nchw)", ("nchw", c["nchw_slot"]), r, allowance(r, d, "fp32")))
    return out


# ---- comparison -----------------------------------------------------------------------------------
def compare(gpu, r, allow, frames=None, worst_n=8):
    """gpu, r, allow: [F, C, H, W].  Returns a report dict: worst |gpu - r| / allowance, how many elements
    exceed it, and where the worst ones are (frame, channel, row, column)."""
    gpu = torch.as_tensor(gpu).to(torch.float64)
    assert gpu.shape == r.shape, (tuple(gpu.shape), tuple(r.shape))
    d = (gpu - r).abs()
    ratio = torch.where(allow > 0, d / allow.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    ratio = torch.where(torch.isfinite(gpu), ratio, torch.full_like(d, float("inf")))
    bad = ratio > 1
    flat = ratio.flatten()
    k = min(worst_n, flat.numel())
    top = torch.topk(flat, k).indices if k else []
    where = []
    for i in top:
        f, ch, y, xx = np.unravel_index(int(i), tuple(ratio.shape))
        if ratio[f, ch, y, xx] <= 1:
            break
        where.append((int(frames[f]) if frames is not None else int(f), int(ch), int(y), int(xx), float(ratio[f, ch, y, xx])))
    return {"worst": float(flat.max()) if flat.numel() else 0.0, "n_bad": int(bad.sum()), "where": where}
