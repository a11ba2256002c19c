"""fp64 host reference of every primitive the NCHW training engines launch (csrc/train.hip, csrc/train_yolo.hip), with a per-element allowance.

As tests/layer_reference.py and tests/train_layer_reference.py do for the inference nets and the planes trainer: the reference computes, in
float64 on the CPU, exactly the operation a kernel defines on the operands it actually reads, so a kernel may sum in any order and still pass
while a wrong operand (tap, halo row, channel, constant, product term) moves the result by far more than the allowance.  U = 2^-24; "store"
= the float32 half ulp (2^-25 relative), added by layer_reference.allowance.  Which kernel a call runs, its tile geometry and its slices come
from pn_train_conv_plan_info / pn_train_reduce_slices (plan() / reduce_slices() below), i.e. from the launch code's own decision.  The
definitions, read from the kernels:

* conv forward (pn_conv2d_forward: tconv_fwd_kernel<1|3|7>, tconv3_tile_kernel, tconv3_tile_x3_kernel, tconv3_tile_x3w_kernel):
  y[n, co, oy, ox] (+)= bias[co] + sum x[n, ci, oy s + ky - p, ox s + kx - p] w[co, ci, ky, kx], zero outside the map.  The fp32 kernels
  (every 1x1, 7x7 and strided call, 3x3 with Cin < 16 or a tile geometry the planner refuses, and all of them in fp32 precision) use exact
  fp32 products.  The two x3 kernels (3x3, stride 1, Cin >= 32, PN_PREC_BF16X3) split BOTH fp32 operands, x_hi = RNE_bf16(x), x_lo =
  RNE_bf16(fp32(x - x_hi)) (t_split8; weights the same way in wpack3_x3_kernel / wpack_all_kernel) and keep x_hi w_hi + x_hi w_lo + x_lo w_hi:
  NO lo * lo term.  The bias is added once, to the accumulator; with accumulate the previous y is added after it.  Allowance: any summation
  order, n U S with n = (3 | 1) Cin k k + bias + accumulate terms and S = sum of |every product and addend|; + store.
* conv dgrad (pn_conv2d_dgrad, stride 1): dx[n, ci, iy, ix] (+)= sum dy[n, co, iy + p - ky, ix + p - kx] w[co, ci, ky, kx].  3x3 with
  Cout >= 16 runs the SAME tile kernels as a forward convolution of dy with padding 2 - p on a pack built with flip = 1:
  W'[ci][co][tap] = w[co][ci][8 - tap] (transposed, taps rotated by 180 degrees; "the packing is the rotation"); every other shape rotates
  with wflip_kernel (Wt[ci][co][k-1-ky][k-1-kx]) and calls pn_conv2d_forward with padding k - 1 - p.  x3: dy is the split "x" operand.
  n = (3 | 1) Cout k k + accumulate.
* conv dgrad, strided (pn_conv2d_dgrad_strided, dgrad_strided_kernel<1|3>): the same sum at stride s, one fp32 fmaf chain per input pixel
  over (co outer, the valid taps row-major); n = the number of taps that hit the pixel x Cout + accumulate.  Always fp32.
* conv wgrad (pn_conv2d_wgrad: tconv_wgrad_kernel<1|3|7>, tconv3_wgrad_tile_kernel, tconv3_wgrad_x3_kernel / _x3pp / _x3v, then
  wgrad_reduce_kernel): dw[co, ci, ky, kx] = sum over (n, oy, ox) dy[n, co, oy, ox] x[n, ci, oy s + ky - p, ox s + kx - p].  The three x3
  kernels split x and dy as above and keep dy_hi x_hi + dy_hi x_lo + dy_lo x_hi.  A block adds the pixels of its slice in fp32 in some order
  (per_slice tiles of R x TW pixels, or per_slice pixels for the generic kernel), then wgrad_reduce_kernel adds the slices in order:
  depth = pixels per slice x (3 | 1) + slices, |error| <= depth U S + float32 rounding.  dbias[co] = sum dy (chan_reduce_kernel<2> in DOUBLE
  over t_slices slices, sums_finish_kernel): P 2^-53 sum|dy| + float32 rounding.
* dilated 3x3 convolutions (pn_conv2d_forward_dil / _dgrad_dil / _wgrad_dil: tconv_fwd_kernel<3, 0, true>, tconv_wgrad_kernel<3, true>; fp32,
  stride 1): the three definitions above with the taps dil apart, x[n, ci, oy + ky dil - p, ox + kx dil - p].  The data gradient is the
  forward kernel on dy with the wflip_kernel weights at padding 2 dil - p.  n and S as for the undilated fp32 arm (a tap in the padding
  contributes nothing to S).  The weight gradient's slices are t_wgrad_pixel_slices(N Ho Wo, 9 Cin, Cout), the generic path's
  (dil_wgrad_plan()): depth = pixels per slice + slices.  dil = 1 forwards to the undilated entry.
* BatchNorm forward (pn_bn_train_forward: chan_reduce_kernel<0>, bn_apply_kernel): sum x and sum x^2 in double (slices, then the slices in
  order, in double); mean = s / n; var = max(ss / n - mean^2, 0); save_mean = float32(mean), save_invstd = float32(1 / sqrt(var + eps));
  running_mean' = float32((1 - m) running_mean + m mean), running_var' the same with var n / (n - 1) (m = float32(0.1), eps = float32(1e-5),
  both promoted to double).  y = act(fma(fp32((x - save_mean) * save_invstd), gamma, beta) [+ res]), ReLU or LeakyReLU as v * 0.1f.
  Bounds: train_layer_reference.bn_stats_ref with a chain of n 2^-29 fp32-equivalents (= n 2^-53); apply: (3 + res) U (|t| + |beta| + |res|)
  with the GPU's own save_mean / save_invstd, + LeakyReLU's product, + store.
* BatchNorm backward (pn_bn_train_backward: chan_reduce_kernel<1>, bn_bwd_apply_kernel): g = dy where the activation passed, else dy * (0 |
  0.1f).  The mask is `out > 0` of the stored forward output where the forward had a residual (the engines pass out only then), and otherwise
  RECOMPUTED from x with the forward's own expression t_bn_affine (out = NULL); the reference always takes it from the stored output, and
  mask_disagreements() counts elements whose dx fits the other branch -- expected 0.  sum_g = sum g, sum_gx = sum g * fp32(x - mean) in
  double; dbeta = float32(sum_g); dgamma = float32(sum_gx * invstd); mg = dbeta * float32(1 / n); k2 = float32(sum_gx) * float32(1 / n) *
  invstd * invstd; dx = (g - mg - fp32(x - mean) * k2) * invstd * gamma; dres (=|+=) g.  Bounds: sums U sum|.| per fp32 factor (LeakyReLU
  product, x - mean) + n 2^-53; dx: |invstd gamma| (e_g + |x - mean| e_k2 + 5 U (|g| + |mg| + |(x - mean) k2|)) + 2 U |dx| with the GPU's own
  dbeta and e_k2 from the reference's sum_gx; dres: e_g (+ U |sum| when accumulating); + store.
* average pool (pn_avgpool3s2_*): forward = layer_reference.avgpool_ref (sum of the valid taps in fp32, then / 9.0f -- ALWAYS 9, whatever the
  number of valid taps); backward = train_layer_reference.pool_bwd_ref (sum of the <= 4 dy whose window holds the pixel, / 9.0f).
* max pool (pn_maxpool_*): the window clipped to the plane in row-major order, a pixel replaces the maximum when v > max or v is NaN: the
  FIRST maximum wins a tie, the LAST NaN of a window wins (torch CPU max_pool2d_with_indices).  y and idx exact.  Backward: dx[p] = fp32 sum
  in output row-major order of the dy whose idx is p: (terms - 1) U S + store.
* heads (pn_head_forward / _backward): s = 1 / (1 + expf(-v)); out = kind ? (s - 0.5f) * 4 : s, written with an image stride of out_ld
  channels; loss = float32(sum_double(fp32(d d w)) / numel), d = out - target, w = 0.1f + fg * 0.9f.  Backward reads the STORED s:
  dv = (2 (o - t) w inv_numel + dextra) * (4 | 1) * (1 - s) * s, inv_numel = float32(1 / numel).  Bounds: sigmoid and casts as
  layer_reference.apply_act; loss 7 U relative (three roundings in d d w, two in w, d itself) + float32; dv: see heads_bwd_ref.
* pn_slice_copy: dst[n, c, p] (=|+=) src[n, c, p] between channel slices of leading dimensions src_ld / dst_ld; exact, or one rounding.
* pn_yolo_loss: s = sigmoid(v) in fp32, casts by channel k = c % (5 + 3J) in fp32; element errors, gradients and sums in double from the
  float32 out / s (see train_yolo.hip).  Reference = yolo_reference.loss_terms's definition, per element.
* pn_sgd_nesterov: d = g * gscale (+ wd * p); b = first ? d : mu * buf + d; buf = b; p = p - lr * (d + mu * b), fp32, contraction off.
* pn_train_pack_refresh (wpack_all_kernel): the packs above, rebuilt from the live parameters; checked through the convolutions that read
  the packs after a parameter change.
"""
import ctypes as C
import json

import numpy as np
import torch
import torch.nn.functional as F

import layer_reference as LR
import train_layer_reference as TL
from layer_reference import U, allowance, compare, f32, rne_bf16                      # noqa: F401  (re-exported for the tests)
from train_layer_reference import dbias_ref, integer_limits, integer_operand, pool_bwd_ref   # noqa: F401

EPS, MOMENTUM = TL.EPS, TL.MOMENTUM
WHICH = {"forward": 0, "dgrad": 1, "dgrad_strided": 2, "wgrad": 3}
X3_KERNELS = ("tconv3_tile_x3_kernel", "tconv3_tile_x3w_kernel", "tconv3_wgrad_x3_kernel", "tconv3_wgrad_x3pp_kernel", "tconv3_wgrad_x3v_kernel")


# ---- the launch code's own plan ---------------------------------------------------------------------------
_PLAN_CTX = {}


def plan_context(x3):
    """A device-less pn_ctx carrying the precision: pn_train_conv_plan_info launches nothing."""
    from popnet_amd import _lib
    L = _lib.lib()
    h = _PLAN_CTX.get(bool(x3))
    if h is None:
        h = _PLAN_CTX[bool(x3)] = L.pn_create(-1)
        assert L.pn_train_set_precision(h, _lib.PN_PREC_BF16X3 if x3 else _lib.PN_PREC_F32) == 0
    return h


def plan(handle, which, N, Cin, H, W, Cout, ks, stride, pad):
    """pn_train_conv_plan_info as a dict; which: "forward", "dgrad", "dgrad_strided", "wgrad"."""
    from popnet_amd import _lib
    buf = C.create_string_buffer(1024)
    rc = _lib.lib().pn_train_conv_plan_info(handle, WHICH[which], N, Cin, H, W, Cout, ks, stride, pad, buf, len(buf))
    if rc != 0:
        raise ValueError("pn_train_conv_plan_info(%s, %r) -> %d" % (which, (N, Cin, H, W, Cout, ks, stride, pad), rc))
    return json.loads(buf.value.decode())


def reduce_slices(handle, N, Cc, HW):
    from popnet_amd import _lib
    return _lib.lib().pn_train_reduce_slices(handle, N, Cc, HW)


def is_x3(label):
    return label in X3_KERNELS


def wgrad_depth(p):
    """Roundings a term of a weight gradient passes at most: the pixels of one slice (x 3 products in a split kernel), then the slices."""
    pix = p["per_slice"] * (p["R"] * p["TW"] if p["per_slice_unit"] == "tiles" else 1)
    return pix * (3 if is_x3(p["kernel"]) else 1) + p["slices"]


def _round32(r, d):
    return d + LR.half_ulp(r.abs() + d, "fp32")


def split(v):
    """float64 tensor of float32 values -> (hi, lo) as t_split8 / wpack3_x3_kernel split them."""
    v = f32(v)
    hi = rne_bf16(v)
    return hi, rne_bf16(f32(v - hi))


# ---- convolutions -------------------------------------------------------------------------------------------
def conv_fwd_ref(x, w, bias, prev, stride, pad, x3, dilation=1):
    """-> (r, allowance).  x [N, Cin, H, W], w [Cout, Cin, k, k], bias [Cout] or None, prev = the y accumulated into or None.
    dilation: the spacing of the taps (pn_conv2d_forward_dil: x[oy + ky dil - p, ox + kx dil - p])."""
    x, w = f32(x), f32(w)
    conv = lambda a, b: F.conv2d(a, b, stride=stride, padding=pad, dilation=dilation)      # noqa: E731
    n = w.shape[1] * w.shape[2] * w.shape[3]
    if x3:
        xh, xl = split(x)
        wh, wl = split(w)
        r = conv(xh + xl, wh) + conv(xh, wl)
        S = conv(xh.abs() + xl.abs(), wh.abs()) + conv(xh.abs(), wl.abs())
        n *= 3
    else:
        r, S = conv(x, w), conv(x.abs(), w.abs())
    if bias is not None:
        b = f32(bias).view(1, -1, 1, 1)
        r, S, n = r + b, S + b.abs(), n + 1
    if prev is not None:
        r, S, n = r + f32(prev), S + f32(prev).abs(), n + 1
    return r, allowance(r, n * U * S, "fp32")


def conv_dgrad_ref(dy, w, prev, shape, stride, pad, x3, dilation=1):
    """-> (r, allowance) of dx [shape]; stride > 1: the strided primitive (always fp32).  dilation: the forward convolution's tap spacing."""
    dy, w = f32(dy), f32(w)
    N, Cin, H, W = shape
    ke = dilation * (w.shape[2] - 1) + 1                          # the extent of the dilated window
    op = (H + 2 * pad - ke - (dy.shape[2] - 1) * stride, W + 2 * pad - ke - (dy.shape[3] - 1) * stride)
    tr = lambda a, b: F.conv_transpose2d(a, b, stride=stride, padding=pad, output_padding=op, dilation=dilation)      # noqa: E731
    if x3:
        dh, dl = split(dy)
        wh, wl = split(w)
        r = tr(dh + dl, wh) + tr(dh, wl)
        S = tr(dh.abs() + dl.abs(), wh.abs()) + tr(dh.abs(), wl.abs())
        n = 3 * tr(torch.ones_like(dy), torch.ones_like(w))
    else:
        r, S = tr(dy, w), tr(dy.abs(), w.abs())
        n = tr(torch.ones_like(dy), torch.ones_like(w))           # the taps that hit each pixel x Cout
    assert tuple(r.shape) == tuple(shape), (tuple(r.shape), shape)
    if prev is not None:
        r, S, n = r + f32(prev), S + f32(prev).abs(), n + 1
    return r, allowance(r, n * U * S, "fp32")


def _cw(dy, x, ks, stride, pad, dilation=1):
    """sum over (n, oy, ox) of dy[n, co, oy, ox] x[n, ci, oy s + ky d - p, ox s + kx d - p] -> [co, ci, ks, ks]"""
    cols = F.unfold(x, ks, dilation=dilation, padding=pad, stride=stride)    # [N, Cin k k, Ho Wo]
    return torch.einsum("ncp,nkp->ck", dy.flatten(2), cols).view(dy.shape[1], x.shape[1], ks, ks)


def conv_wgrad_ref(x, dy, ks, stride, pad, p, dilation=1):
    """p: plan(..., "wgrad", ...) -- for a dilated call dil_wgrad_plan(...).  -> (r, allowance) of dw"""
    x, dy = f32(x), f32(dy)
    if is_x3(p["kernel"]):
        xh, xl = split(x)
        dh, dl = split(dy)
        r = _cw(dh + dl, xh, ks, stride, pad, dilation) + _cw(dh, xl, ks, stride, pad, dilation)
        S = _cw(dh.abs() + dl.abs(), xh.abs(), ks, stride, pad, dilation) + _cw(dh.abs(), xl.abs(), ks, stride, pad, dilation)
    else:
        r, S = _cw(dy, x, ks, stride, pad, dilation), _cw(dy.abs(), x.abs(), ks, stride, pad, dilation)
    return r, _round32(r, wgrad_depth(p) * U * S)


def dil_wgrad_plan(handle, N, Cin, Ho, Wo, Cout):
    """The slices of pn_conv2d_wgrad_dil for an output of N x Ho x Wo pixels.  The dilated entry is not described by pn_train_conv_plan_info;
    it calls t_wgrad_pixel_slices(P = N Ho Wo, Kdim = 9 Cin, Cout) exactly as pn_conv2d_wgrad's generic path does, and the slices depend on
    nothing else.  So the plan is read from an undilated call the planner sends down the generic path with the same P, Kdim and Cout:
    3x3, stride 2, pad 1 on a (2 Ho - 1) x (2 Wo - 1) map, whose output is Ho x Wo."""
    p = plan(handle, "wgrad", N, Cin, 2 * Ho - 1, 2 * Wo - 1, Cout, 3, 2, 1)
    assert p["kernel"] == "tconv_wgrad_kernel<3>" and p["per_slice_unit"] == "pixels" and (p["Ho"], p["Wo"]) == (Ho, Wo), p
    return p


def double_chain(count):
    """A double-precision sum of `count` terms, as a chain length in units of U (train_layer_reference's m): count 2^-53 = (count 2^-29) U."""
    return count * 2.0 ** -29


def conv_dbias_ref(dy):
    dy = f32(dy)
    return dbias_ref(dy, dy.shape[1], double_chain(dy.shape[0] * dy.shape[2] * dy.shape[3]))


# ---- BatchNorm ------------------------------------------------------------------------------------------------
def bn_stats_ref(x, rm, rv):
    """-> {mean, invstd, running_mean, running_var: (r, allowance)}"""
    x = f32(x)
    n = x.shape[0] * x.shape[2] * x.shape[3]
    z = torch.zeros(x.shape[1], dtype=torch.float64)
    out = TL.bn_stats_ref(x, z + 1, z, rm, rv, double_chain(n))
    return {k: out[k] for k in ("mean", "invstd", "running_mean", "running_var")}


def _v(a):
    return f32(a).view(1, -1, 1, 1)


def bn_apply_ref(x, mean, invstd, gamma, beta, res, act):
    """mean / invstd: the float32 vectors the kernel published.  -> (r, allowance)"""
    x = f32(x)
    t = (x - _v(mean)) * _v(invstd) * _v(gamma)
    pre, S, n = t + _v(beta), t.abs() + _v(beta).abs(), 3
    if res is not None:
        pre, S, n = pre + f32(res), S + f32(res).abs(), n + 1
    r, d = LR.apply_act(pre, n * U * S, act)
    return r, allowance(r, d, "fp32")


def bn_bwd_ref(x, dy, mask, mean, invstd, gamma, act, gpu_dbeta, dres_prev=None):
    """mask: out > 0 of the stored forward output (ignored for act 0).  gpu_dbeta: the dbeta the kernel wrote (dx is built from it).
    -> {"dbeta", "dgamma", "dx", "dres": (r, allowance)}"""
    x, dy = f32(x), f32(dy)
    n = x.shape[0] * x.shape[2] * x.shape[3]
    g = TL.bn_g(dy, mask, act)
    eg = U * g.abs() if act == 2 else torch.zeros_like(g)             # dy * 0.1f
    xm = x - _v(mean)
    tiny = 2.0 ** -53 * n
    sg, sgx = g.sum((0, 2, 3)), (g * xm).sum((0, 2, 3))
    dsg = eg.sum((0, 2, 3)) + tiny * g.abs().sum((0, 2, 3))
    dsgx = ((eg + U * g.abs()) * xm.abs()).sum((0, 2, 3)) + tiny * (g * xm).abs().sum((0, 2, 3))
    istd, ga = f32(invstd), f32(gamma)
    out = {"dbeta": (sg, _round32(sg, dsg)), "dgamma": (sgx * istd, _round32(sgx * istd, dsgx * istd))}
    invc = float(np.float32(1.0 / n))
    mg = _v(gpu_dbeta) * invc
    k2 = _v(sgx * invc * istd * istd)
    ek2 = _v(_round32(sgx, dsgx) * invc * istd * istd) + 3 * U * k2.abs()
    k1 = _v(istd * ga)
    r = (g - mg - xm * k2) * k1
    d = k1.abs() * (eg + xm.abs() * ek2 + 5 * U * (g.abs() + mg.abs() + (xm * k2).abs())) + 2 * U * r.abs()
    out["dx"] = (r, allowance(r, d, "fp32"))
    rr = g if dres_prev is None else g + f32(dres_prev)
    out["dres"] = (rr, allowance(rr, eg, "fp32") if dres_prev is not None or act == 2 else eg)
    return out


def mask_disagreements(gpu_dx, x, dy, mask, mean, invstd, gamma, act, gpu_dbeta):
    """Elements whose dx is outside the allowance for the stored output's branch and inside it for the other branch."""
    if act == 0:
        return 0
    r, a = bn_bwd_ref(x, dy, mask, mean, invstd, gamma, act, gpu_dbeta)["dx"]
    bad = (gpu_dx - r).abs() > a
    if not bool(bad.any()):
        return 0
    g = TL.bn_g(f32(dy), mask, act)
    go = TL.bn_g(f32(dy), ~mask, act)
    ro = r + (go - g) * _v(f32(invstd) * f32(gamma))                     # the other branch of that element alone (the sums stay)
    return int((bad & ((gpu_dx - ro).abs() <= a + U * ro.abs())).sum())


# ---- pools ----------------------------------------------------------------------------------------------------
def avgpool_fwd_ref(x):
    r, d = LR.avgpool_ref(LR.Act(f32(x)))
    return r, allowance(r, d, "fp32")


def avgpool_bwd_ref(dy, H, W):
    r, d = pool_bwd_ref(f32(dy), H, W)
    return r, allowance(r, d, "fp32")


def maxpool_fwd_ref(x, k, stride, pad):
    """(y, idx): torch's CPU pool -- first maximum of the row-major window, the last NaN"""
    return F.max_pool2d(x.to(torch.float32), k, stride, pad, return_indices=True)


def maxpool_bwd_ref(dy, idx, H, W):
    dy = f32(dy)
    N, Cc = dy.shape[:2]
    i = idx.to(torch.long).flatten(2)
    z = torch.zeros((N, Cc, H * W), dtype=torch.float64)
    r = z.clone().scatter_add_(2, i, dy.flatten(2)).view(N, Cc, H, W)
    S = z.clone().scatter_add_(2, i, dy.flatten(2).abs()).view(N, Cc, H, W)
    cnt = z.clone().scatter_add_(2, i, torch.ones_like(dy.flatten(2))).view(N, Cc, H, W)
    return r, allowance(r, (cnt - 1).clamp_min(0) * U * S, "fp32")


# ---- heads, copies, optimiser -----------------------------------------------------------------------------------
def head_fwd_ref(v, kind):
    """-> (s r, s allowance, out r, out allowance)"""
    v = f32(v)
    s, ds = LR.apply_act(v, torch.zeros_like(v), LR.ACT_SIG)
    o, do = LR.apply_act(v, torch.zeros_like(v), LR.ACT_SIG_PM2 if kind else LR.ACT_SIG)
    return s, allowance(s, ds, "fp32"), o, allowance(o, do, "fp32")


def head_loss_ref(out, target, fg):
    """out: the float32 values the kernel stored.  -> (loss, allowance)"""
    out, target = f32(out), f32(target)
    w = float(np.float32(0.1)) + f32(fg) * float(np.float32(0.9)) if fg is not None else torch.ones_like(out)
    loss = ((out - target) ** 2 * w).sum() / out.numel()
    return loss, _round32(loss, 7 * U * loss.abs())


def heads_bwd_ref(s, target, fg, dextra, kind):
    """s: the stored sigmoid.  -> (dv r, allowance)"""
    s, target = f32(s), f32(target)
    inv = float(np.float32(1.0 / s.numel()))
    o = (s - 0.5) * 4 if kind else s
    eo = 4 * U * (s - 0.5).abs() if kind else torch.zeros_like(s)
    w = float(np.float32(0.1)) + f32(fg) * float(np.float32(0.9)) if fg is not None else torch.ones_like(s)
    d = o - target
    a = 2 * d * w * inv
    ea = 2 * w * inv * (eo + U * d.abs()) + 4 * U * a.abs()           # d, the two roundings of w, two products
    g, eg = a, ea
    if dextra is not None:
        g = a + f32(dextra)
        eg = ea + U * g.abs()
    kk = 4.0 if kind else 1.0
    r = g * kk * (1 - s) * s
    delta = kk * ((1 - s) * s).abs() * eg + 3 * U * r.abs()               # 1 - s, two products
    return r, allowance(r, delta, "fp32")


def slice_copy_ref(src, prev):
    r = f32(src) if prev is None else f32(src) + f32(prev)
    return r, (torch.zeros_like(r) if prev is None else allowance(r, torch.zeros_like(r), "fp32"))


def sgd_ref(p, g, buf, lr, mu, wd, first, gscale):
    """-> {"p", "buf": (r, allowance)}"""
    p, g, buf = f32(p), f32(g), f32(buf)
    lr, mu, wd, gscale = (float(np.float32(a)) for a in (lr, mu, wd, gscale))
    d = g * gscale
    ed = U * d.abs()
    if wd != 0:
        d = d + wd * p
        ed = ed + U * (wd * p).abs() + U * d.abs()
    if first:
        b, eb = d, ed
    else:
        b = mu * buf + d
        eb = ed + U * (mu * buf).abs() + U * b.abs()
    t = d + mu * b
    et = ed + mu * eb + U * (mu * b).abs() + U * t.abs()
    r = p - lr * t
    er = lr * et + U * (lr * t).abs()
    return {"p": (r, allowance(r, er, "fp32")), "buf": (b, allowance(b, eb, "fp32"))}


# ---- YOLO head casts + loss ---------------------------------------------------------------------------------------
def yolo_loss_ref(v, prior, conf, coord, weight, A, J):
    """-> {"out", "dv": (r, allowance), "terms": (r [4], allowance [4])}; the loss as yolo_reference.loss_terms defines it, per element."""
    v, prior = f32(v), f32(prior)
    B, _, h, w = v.shape
    Fk = 5 + 3 * J
    k = (torch.arange(A * Fk) % Fk).view(1, -1, 1, 1)
    s = torch.sigmoid(v)
    es = 9 * U                                                                   # layer_reference.apply_act: expf, add, divide
    o, do = LR.apply_act(v, torch.zeros_like(v), LR.ACT_YOLO, naf=Fk)
    fac = torch.where(k < 4, 2.0, torch.where(k == 4, 1.0, 4.0)).to(torch.float64).expand_as(v)
    ex = lambda m: f32(m).unsqueeze(2).expand(B, A, Fk, h, w).reshape(v.shape)        # noqa: E731
    m = torch.where(k == 4, ex(conf), ex(coord))
    M = float(B * A * h * w)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)                             # noqa: E731
    sc = torch.where(k < 4, t64(4.0 / (M * 4.0)), torch.where(k == 4, t64(1.0 / M), t64((3.0 * J) / (M * 3.0 * J)))).expand_as(v)
    if weight is not None:
        wt = ex(weight)
        d = o * m - prior * m
        e = d * d * wt
        dlo = 2 * d * wt * m
        ddlo = 2 * wt * m * m                                                    # d dlo / d o
    else:
        d = o - prior
        e = d * d * m
        dlo = 2 * d * m
        ddlo = 2 * m
    dv = dlo * sc * fac * s * (1 - s)
    edv = (ddlo * do).abs() * sc * fac * (s * (1 - s)) + (dlo * sc * fac * (1 - 2 * s)).abs() * es
    terms, eterms = [], []
    for sel in (k < 4, k == 4, k > 4):
        sel = sel.expand_as(v)
        t = (e * sel * sc).sum()
        terms.append(t)
        eterms.append(_round32(t, ((dlo.abs() * do) * sel * sc).sum()))
    tot = terms[0] + terms[1] + terms[2]
    et = eterms[0] + eterms[1] + eterms[2]
    terms, eterms = torch.stack([tot] + terms), torch.stack([et + 2 * U * tot.abs()] + eterms)
    return {"out": (o, allowance(o, do, "fp32")), "dv": (dv, allowance(dv, edv, "fp32")), "terms": (terms, eterms)}
