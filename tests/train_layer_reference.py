"""fp64 host reference of every op of the planes training step (pn_trainer_op_info), with a per-element error allowance.

As tests/layer_reference.py does for the inference nets: the reference computes, in float64 on the CPU, exactly the operation the kernels
define on the operands they actually read, so a kernel may sum in any order and still pass while a wrong operand (tap, halo row, channel,
constant) moves the result by far more than the allowance.  U = 2^-24.  "store" = the stored format's half ulp (bf16x3: of the lo plane,
2^-17 relative; fp32 engine: 2^-25 relative), added by layer_reference.allowance.  The definitions, read from trainx.hip /
trainx_kernels.h / trainx_wgrad.h / train.hip:

* conv (forward and dgrad; conv3_kernel / conv4_kernel / conv_mfma_kernel on device-built packs, tx::pack_rows_kernel): weights come from
  the live fp32 parameter w [Cout][Cin][k][k].  bf16x3: W_hi = RNE(w), W_lo = RNE(w - W_hi), products x_hi W_hi + x_lo W_hi + x_hi W_lo
  (no lo * lo term); fp32: exact fp32 products.  The dgrad pack is W'[ci][co][ky][kx] = w[co][ci][k-1-ky][k-1-kx].  A layer that reads the
  stage-2 input sees this engine's channel order [feat 0..127 | paf 128..155 | heat 156..171 | z 172..186 | pad 187..191] of the
  reference's cat[paf, heat, z, feat]: plane channel i carries reference channel CAT_MAP[i]; the 5 pad channels (-1) have zero weights
  (forward: zero k columns; dgrad: zero rows, so the pad channels of the gradient are written as zeros).  Epilogue: + float32 bias (forward
  of a layer with a bias; none in a dgrad), + residual (hi, then lo), activation (none, or the heads' sigmoid casts), store.  Heads also
  write NCHW f32 and, in stage 1, channels [CAT_OFF, CAT_OFF + C) of the stage-2 input; every other channel of that tensor is unchanged.
  Allowance: layer_reference.conv_ref, delta = n U S over n = (3 | 1) * used channels * k * k + bias + residual planes terms; + store.
* bn_fwd (reduce_kernel<0>, bn_finish_kernel, bn_apply_kernel): each thread adds x and x * x of its pixels in fp32 (chain of
  m = ceil(ppb / PL) pixels, PL = 256 / (C / 8) pixel lanes), the rest in double.  mean = s / n; var = max(ss / n - mean^2, 0);
  invstd = 1 / sqrt(var + eps); scale = gamma invstd; shift = beta - mean scale, each rounded to float32 from double; running_mean' =
  (1 - momentum) running_mean + momentum mean, running_var' the same with var n / (n - 1) (momentum = float32(0.1), eps = float32(1e-5)).
  Bounds: |d s| <= m U sum|x|; |d ss| <= (m + 1) U sum x^2 (one more rounding for the square); carried through the formulas above to first
  order plus the exact second-order terms, invstd by evaluating it at var -+ d var; + the float32 rounding of each result.
  Apply: y = act(x scale + shift [+ res]) in fp32 with the GPU's own scale / shift, LeakyReLU as y * 0.1f: delta = n U (|x scale| + |shift|
  + |res|) with n = 2 (+ 1 residual) (+ 1 LeakyReLU); + store.
* bn_bwd (reduce_kernel<1>, bn_bwd_finish_kernel, bn_bwd_apply_kernel): g = dy where the activation passed, else dy * slope (0 | 0.1f);
  xhat = (x - mean) * invstd in fp32; dbeta = sum g; dgamma = sum g xhat; k1 = gamma * invstd (one fp32 product); k2 = dbeta / n;
  k3 = dgamma / n; dx = k1 (g - k2 - xhat k3); dres = g.  The reference takes the mask from the STORED forward output (y > 0).  Where no
  residual went in, the kernels recompute the sign from x * scale + shift: mask_disagreements() counts the elements whose dx matches the
  other branch -- expected 0.  Bounds: sum g: (m + 1) U sum|g|; sum g xhat: (m + 4) U sum|g xhat| (the subtraction, two products and the
  LeakyReLU product are each correctly rounded: relative U each); k2 / k3 from those / n; dx: 7 U |k1| (|g| + |k2| + |xhat k3|); dres:
  U |g| for LeakyReLU, exact otherwise; + store / float32 rounding.
* dbias (reduce_kernel<2>, sum_finish_kernel): db[c] = sum dy[c], c < cout: m U sum|dy| + float32 rounding.
* add: fp32 sum of the inputs in order: (k - 1) U sum|terms| + store.
* pool_fwd: layer_reference.avgpool_ref (nine-tap fp32 sum / 9.0f, count_include_pad).  pool_bwd (avgpool_bwd_kernel): dx[iy][ix] = (sum of
  the <= 4 dy whose window holds it) / 9.0f -- always 9, whatever the number of valid taps: 3 U S / 9 + U |r| + store.
* heads (head_kernel, loss_finish_kernel): o = the head's stored NCHW f32 output; s = o * 0.25f + 0.5f (paf, z) or o (heat); d = o - t;
  w = float32(0.1f + 0.9f fg) (z) or 1; loss = sum (d d w) / numel, products in fp32 (relative 4 U), the sum in double, rounded to float32;
  dv = (2 d w inv_numel + dextra) * (4 | 1) * (1 - s) s with inv_numel = float32(1 / numel) and dextra channel CAT_OFF + c of the stage-2
  input gradient (stage 1; none in stage 2).  Bounds: |d s| <= 2 U, |d (1 - s)| <= 3 U, the bracket 4 U (|2 d w inv_numel| + |dextra|), two
  more products: 2 U |dv|; + store.  Channels >= C of dv stay zero.
* wgrad (wgrad_stream_kernel | wgrad_f32_kernel, wgrad_reduce_kernel): dW[co][ci][ky][kx] = sum dy[n, y, x, co] x[n, y + ky - p, x + kx - p,
  ci], products dy_hi x_hi + dy_lo x_hi + dy_hi x_lo (fp32 engine: exact), scattered to the reference's channel order through CAT_MAP (the
  pad channels have no element in the gradient buffer; nothing outside the layer's own tensor changes).  Chain depth: a block adds
  rows_per_block rows of <= Wt pixels (x 3 products in bf16x3) into an accumulator in fp32 in some order, then wgrad_reduce_kernel adds
  ceil(Sr / 16) slices per lane and 16 lane sums: every term passes at most depth = rows_per_block Wt (3 | 1) + ceil(Sr / 16) + 16
  roundings, so |error| <= depth U S + float32 rounding (S = sum of |products|, bounded from above by sum (|dy_hi| + |dy_lo|) (|x_hi| + |x_lo|)).  (The any-order bound n U S over all B H W pixels is 2.4 %
  of S at the bench shape.)
* stem_fwd (tstem_fwd_kernel): 7x7 stride-2 pad-3 convolution of the fp32 image with the fp32 weights, exact fp32 products in both
  precisions, no bias: 50 U S + store.  stem_wgrad (tstem_wgrad_kernel<BN = 1>): the stem's BatchNorm backward (as bn_bwd, the sign
  recomputed from x * scale + shift; the reference takes it from the stored activation) is applied per element, rounded to the stored
  format, and multiplied with the image in exact fp32: slices of pps pixels, then the slices in order (train.hip::pn_stem_wgrad_planes:
  slices = min(1024, ceil(P / 1024)), pps = ceil(P / slices) rounded up to 32): depth = pps + slices; the allowance of the per-element
  gradient (it is never stored, so the reference carries it) goes through the sum: + sum e |img|.
* pack: checked through the convolutions that read the packs.
"""
import numpy as np
import torch
import torch.nn.functional as F

import layer_reference as LR
from layer_reference import U, Act, f32, rne_bf16

HEAD_C = (28, 16, 15)
CAT_OFF = (128, 156, 172)
CAT_PLANE = 192
CAT_MAP = [59 + i for i in range(128)] + list(range(28)) + [28 + i for i in range(16)] + [44 + i for i in range(15)] + [-1] * 5
# the configurations of tests/test_gpu_train_layers.py (name, B, H, W); the CPU tests of this module use their map sizes
SHAPES = [("bench", 32, 224, 224),          # the bench shape: the stage levels take the conv4 plan (exactly at its 448-block threshold)
          ("b1_ragged", 1, 104, 136),       # B = 1; maps 52x68 -> 26x34 -> 13x17: ragged strips, odd pooled maps, no conv4
          ("ragged", 3, 72, 40)]            # maps 36x20 -> 18x10 -> 9x5: half-empty tiles
MOMENTUM = float(np.float32(0.1))
EPS = float(np.float32(1e-5))


def fmt_of(prec):
    return "x3" if prec == "bf16x3" else "fp32"


def split_act(v, prec):
    """float64 values -> the Act a planes tensor holding them carries (bf16x3: hi + lo as Lay<bf>::st splits)."""
    v = f32(v)
    if prec != "bf16x3":
        return Act(v)
    hi = rne_bf16(v)
    return Act(hi + rne_bf16(f32(v - hi)), hi)


def _round32(r, d):
    """allowance of a float32 result whose exact value is within d of r."""
    return d + LR.half_ulp(r.abs() + d, "fp32")


# ---- conv ---------------------------------------------------------------------------------------------
def conv_weights(w, p, prec, kplane):
    """The pack of problem p as the kernels hold it: [W] or [W_hi, W_lo], float64 [rows, kplane, k, k], and the k channels in use."""
    w = f32(w)
    cout, cin, k, _ = w.shape
    cmap = CAT_MAP if p["cat"] else list(range(cin))
    rows = p["rows"]
    W = torch.zeros((rows, kplane, k, k), dtype=torch.float64)
    if not p["dgrad"]:
        idx = [(i, m) for i, m in enumerate(cmap[:kplane]) if m >= 0]
        W[:cout, [i for i, _ in idx]] = w[:, [m for _, m in idx]]
        used = len(idx)
    else:
        wr = w.flip(2, 3).transpose(0, 1)                   # [cin, cout, k, k], taps rotated by 180 degrees
        idx = [(i, m) for i, m in enumerate(cmap[:rows]) if m >= 0]
        W[[i for i, _ in idx], :cout] = wr[[m for _, m in idx]]
        used = cout
    if prec != "bf16x3":
        return [W], used
    hi = rne_bf16(W)
    return [hi, rne_bf16(f32(W - hi))], used


def conv_ref(p, prec, w, bias, x, res=None):
    """(r, delta) of convolution problem p on Act x (all kplane channels) [+ Act res]; bias: float tensor [cout] or None."""
    W, used = conv_weights(w, p, prec, x.v.shape[1])
    b = torch.zeros(p["rows"], dtype=torch.float64)
    if bias is not None and p["bias"]:
        b[:bias.numel()] = f32(bias)
    return LR.conv_ref(x, W, b, used, p["ks"], 1, p["act"], res=None if res is None else res.v, x3_res=prec == "bf16x3")


# ---- BatchNorm ----------------------------------------------------------------------------------------
def chain(p):
    """Pixels one thread of reduce_kernel adds in fp32."""
    PL = 256 // (p["C"] // 8)
    return -(-p["ppb"] // PL)


def bn_stats_ref(x, gamma, beta, rm, rv, m):
    """x: float64 [B, C, H, W] (all frames).  -> {name: (r, allowance)} for mean, invstd, scale, shift, running_mean, running_var."""
    n = x.shape[0] * x.shape[2] * x.shape[3]
    gamma, beta, rm, rv = f32(gamma), f32(beta), f32(rm), f32(rv)
    s, ss, sa = x.sum((0, 2, 3)), (x * x).sum((0, 2, 3)), x.abs().sum((0, 2, 3))
    mean, dm = s / n, m * U * sa / n
    dss = (m + 1) * U * ss / n
    var_raw = ss / n - mean * mean
    dv = dss + 2 * mean.abs() * dm + dm * dm
    var = var_raw.clamp_min(0)
    inv = lambda v: 1.0 / torch.sqrt(v + EPS)
    istd = inv(var)
    dis = torch.maximum(inv((var - dv).clamp_min(0)) - istd, istd - inv(var + dv))
    sc = gamma * istd
    dsc = gamma.abs() * dis
    sh = beta - mean * sc
    dsh = mean.abs() * dsc + sc.abs() * dm + dm * dsc
    unb = var * n / (n - 1.0) if n > 1 else var
    out = {"mean": (mean, dm), "invstd": (istd, dis), "scale": (sc, dsc), "shift": (sh, dsh),
           "running_mean": ((1.0 - MOMENTUM) * rm + MOMENTUM * mean, MOMENTUM * dm),
           "running_var": ((1.0 - MOMENTUM) * rv + MOMENTUM * unb, MOMENTUM * dv * (n / (n - 1.0) if n > 1 else 1.0))}
    return {k: (r, _round32(r, d)) for k, (r, d) in out.items()}


def bn_apply_ref(x, scale, shift, res, act):
    """(r, delta) of y = act(x * scale + shift [+ res]); scale / shift: the float32 vectors the apply kernel read."""
    sc, sf = f32(scale).view(1, -1, 1, 1), f32(shift).view(1, -1, 1, 1)
    pre = x.v * sc + sf
    S = (x.v * sc).abs() + sf.abs()
    n = 2
    if res is not None:
        pre, S, n = pre + res.v, S + res.v.abs(), n + 1
    return LR.apply_act(pre, n * U * S, act)


def bn_g(dy, mask, act):
    if act == 0:
        return dy
    return torch.where(mask, dy, dy * (LR.LEAKY if act == 2 else 0.0))


def bn_bwd_sums_ref(x, dy, mask, mean, invstd, gamma, act, m):
    """All frames.  -> {name: (r, allowance)} for dbeta, dgamma, k1, k2, k3."""
    n = x.shape[0] * x.shape[2] * x.shape[3]
    mu, istd = f32(mean).view(1, -1, 1, 1), f32(invstd).view(1, -1, 1, 1)
    g = bn_g(dy, mask, act)
    t = g * ((x - mu) * istd)
    s, sx = g.sum((0, 2, 3)), t.sum((0, 2, 3))
    ds, dsx = (m + 1) * U * g.abs().sum((0, 2, 3)), (m + 4) * U * t.abs().sum((0, 2, 3))
    k1 = f32(gamma) * f32(invstd)
    out = {"dbeta": (s, ds), "dgamma": (sx, dsx), "k1": (k1, torch.zeros_like(k1)), "k2": (s / n, ds / n), "k3": (sx / n, dsx / n)}
    return {k: (r, _round32(r, d)) for k, (r, d) in out.items()}


def bn_bwd_apply_ref(x, dy, mask, mean, invstd, k1, k2, k3, act):
    """-> (dx r, dx delta, dres r, dres delta) with the GPU's own per-channel vectors."""
    v = lambda a: f32(a).view(1, -1, 1, 1)
    g = bn_g(dy, mask, act)
    xh = (x - v(mean)) * v(invstd)
    r = v(k1) * (g - v(k2) - xh * v(k3))
    d = 7 * U * v(k1).abs() * (g.abs() + v(k2).abs() + (xh * v(k3)).abs())
    return r, d, g, (U * g.abs() if act == 2 else torch.zeros_like(g))


def mask_disagreements(gpu_dx, x, dy, mask, mean, invstd, k1, k2, k3, act, fmt):
    """Elements whose dx is outside the allowance for the stored output's branch and inside it for the other branch."""
    if act == 0:
        return 0
    r, d, _, _ = bn_bwd_apply_ref(x, dy, mask, mean, invstd, k1, k2, k3, act)
    bad = (gpu_dx - r).abs() > LR.allowance(r, d, fmt)
    if not bool(bad.any()):
        return 0
    ro, do, _, _ = bn_bwd_apply_ref(x, dy, ~mask, mean, invstd, k1, k2, k3, act)
    other = (gpu_dx - ro).abs() <= LR.allowance(ro, do, fmt)
    return int((bad & other).sum())


def dbias_ref(dy, cout, m):
    s = dy[:, :cout].sum((0, 2, 3))
    return s, _round32(s, m * U * dy[:, :cout].abs().sum((0, 2, 3)))


# ---- element-wise -------------------------------------------------------------------------------------
def add_ref(ins):
    r, S = sum(ins), sum(a.abs() for a in ins)
    return r, (len(ins) - 1) * U * S


def pool_bwd_ref(dy, H, W):
    C = dy.shape[1]
    w = torch.ones((C, 1, 3, 3), dtype=torch.float64)
    op = (H - (2 * dy.shape[2] - 1), W - (2 * dy.shape[3] - 1))
    tr = lambda a: F.conv_transpose2d(a, w, stride=2, padding=1, output_padding=op, groups=C)
    r = tr(dy) / 9.0
    return r, 3 * U * tr(dy.abs()) / 9.0 + U * r.abs()


def heads_ref(o, target, fg, dextra, kind):
    """o, target [, fg, dextra]: float64 [B, C, h, w].  -> (dv r, dv delta, loss r, loss allowance)."""
    o, target = f32(o), f32(target)
    numel = o.numel()
    inv = float(np.float32(1.0 / numel))
    s = o * 0.25 + 0.5 if kind else o
    d = o - target
    w = f32(float(np.float32(0.1)) + float(np.float32(0.9)) * f32(fg)) if fg is not None else torch.ones_like(o)
    e = d * d * w
    loss = e.sum() / numel
    a = 2 * d * w * inv
    de = dextra if dextra is not None else torch.zeros_like(o)
    g = a + de
    k = 4.0 if kind else 1.0
    r = g * k * (1 - s) * s
    dg = 4 * U * (a.abs() + de.abs())
    delta = k * (dg * ((1 - s) * s).abs() + g.abs() * (3 * U) * s.abs() + g.abs() * (1 - s).abs() * (2 * U)) + 2 * U * r.abs()
    return r, delta, loss, _round32(loss, 5 * U * loss.abs())


# ---- weight gradients -----------------------------------------------------------------------------------
def _cw(dy, x, ks):
    """sum over (n, y, x) of dy[n, co, y, x] * x[n, ci, y + ky - p, x + kx - p] -> [co, ci, ks, ks] (one GEMM per tap)."""
    p = ks // 2
    xp = F.pad(x, (p, p, p, p))
    H, W = dy.shape[2], dy.shape[3]
    a = dy.permute(1, 0, 2, 3).reshape(dy.shape[1], -1)
    out = torch.empty((dy.shape[1], x.shape[1], ks, ks), dtype=torch.float64)
    for ky in range(ks):
        for kx in range(ks):
            out[:, :, ky, kx] = a @ xp[:, :, ky:ky + H, kx:kx + W].permute(1, 0, 2, 3).reshape(x.shape[1], -1).t()
    return out


def wgrad_depth(op, prec):
    return op["rows_per_block"] * op["Wt"] * (3 if prec == "bf16x3" else 1) + -(-op["Sr"] // 16) + 16


def wgrad_ref(op, prec, x, dy):
    """x, dy: Acts over all frames and all plane channels.  -> (r, allowance), float64 [cout, cin, ks, ks] in the reference's channel order."""
    cout, cin, ks = op["cout"], op["cin"], op["ks"]
    sel = [CAT_MAP.index(c) for c in range(cin)] if op["cat"] else list(range(cin))
    xv, dv = x.v[:, sel], dy.v[:, :cout]
    if prec == "bf16x3":
        xh, dh = x.hi[:, sel], dy.hi[:, :cout]
        r = _cw(dv, xh, ks) + _cw(dh, xv - xh, ks)
        S = _cw(dh.abs() + (dv - dh).abs(), xh.abs() + (xv - xh).abs(), ks)        # (one pass: the lo * lo magnitudes ride along, 2^-18 of S too much)
    else:
        r, S = _cw(dv, xv, ks), _cw(dv.abs(), xv.abs(), ks)
    return r, _round32(r, wgrad_depth(op, prec) * U * S)


def stem_fwd_ref(img, w):
    return LR.conv_ref(Act(f32(img)), [f32(w)], torch.zeros(w.shape[0], dtype=torch.float64), 1, 7, 2, LR.ACT_NONE)


def stem_depth(P):
    slices = max(1, min(1024, -(-P // 1024)))
    pps = -(-(-(-P // slices)) // 32) * 32
    return pps + -(-P // pps)


def _cw_stem(dy, img):
    """dW[co][0][ky][kx] = sum dy[n, co, y, x] img[n, 0, 2 y + ky - 3, 2 x + kx - 3]"""
    cols = F.unfold(img, 7, padding=3, stride=2)                           # [B, 49, Ho * Wo]
    return torch.einsum("bcp,bkp->ck", dy.flatten(2), cols).view(dy.shape[1], 1, 7, 7)


def stem_wgrad_ref(img, x, dA, mask, mean, invstd, k1, k2, k3, prec):
    """The default path: BatchNorm backward (ReLU) inside the weight gradient.  All frames."""
    fmt = fmt_of(prec)
    img = f32(img)
    r, d, _, _ = bn_bwd_apply_ref(x, dA, mask, mean, invstd, k1, k2, k3, 1)
    e = LR.allowance(r, d, fmt)
    dw, S = _cw_stem(r, img), _cw_stem(r.abs() + e, img.abs())
    P = x.shape[0] * x.shape[2] * x.shape[3]
    return dw, _round32(dw, stem_depth(P) * U * S + _cw_stem(e, img.abs()))


# ---- exact integer probes -------------------------------------------------------------------------------
def integer_operand(shape, seed):
    """Integers in [-3, 3] (float64): every hi / lo split is exact (lo = 0) and every fp32 sum of their products is exact below 2^24."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=g).to(torch.float64)


def integer_limits(B, H, W):
    """Largest |value| an integer probe can produce at input size B x H x W: a 3x3 convolution over 256 channels (+ a bias and a residual in [-3, 3]) and a
    weight gradient over the largest map.  Must stay below 2^16 (exact as hi + lo planes) resp. 2^24 (exact in fp32)."""
    return 9 * 256 * 9 + 3 + 3, 9 * B * (H // 2) * (W // 2)
