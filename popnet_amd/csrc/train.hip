// The NCHW training engine ("fp32-nchw", "bf16x3-nchw"): fp32, NCHW (the layout of the reference's tensors), one C-ABI entry per
// differentiable primitive of rtpose_light3d in train mode (BASELINE configs[4]).  The host side (popnet_amd/train.py)
// strings them together in the order autograd would.
//   conv forward / data gradient / weight gradient   implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains), or split-bf16 MFMA
//       nn.Conv2d of tpm/lib/network/rtpose_light3d.py:31-40,144-146,232-246 and its autograd
//       kernels: train_conv_kernels.h (forward, data gradient, weight packs, the planes engine's stem forward),
//                train_wgrad_kernels.h (weight gradient and its slice reduction, the planes engine's stem weight gradient),
//                train_conv_common.h (what those two share with conv1x1_x3_kernels.h, and the weight-pack formats)
//   train-mode BatchNorm2d (+ residual add + ReLU / LeakyReLU(0.1)) forward and backward      rtpose_light3d.py:52-70,147,244
//   AvgPool2d(3, 2, 1) forward / backward                                                     rtpose_light3d.py:152,158
//   sigmoid heads + rtpose_light3d_loss_fgweight forward and gradient                         rtpose_light3d.py:335-337, losses.py:65-106
//   SGD with Nesterov momentum                                                                train_rtpose_light3d_kdh3d_mpaug.py:313-316
// This file: the pack cache, the tile geometries, the element-wise kernels, the workspace, the planners (one function per entry decides
// kernel and geometry) and every extern "C" entry.
// Roofline: the three GEMM-shaped kernels are MFMA-bound (fp32-input matrix peak 157 TFLOP/s), everything else HBM-bound.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "pn_internal.h"
#include "train_conv_kernels.h"
#include "train_wgrad_kernels.h"

static int t_ws(pn_ctx *ctx, size_t bytes, void **out);
// The pack buffer of (w, shape, flip, kind), t_pack_bytes large: the context's scratch when the cache is off (packed by the caller on every call),
// else the cached entry -- *fresh tells the caller whether this step's refresh has already filled it.
static int t_pack_get(pn_ctx *ctx, const float *w, int Cout, int Cin, int flip, PnPackKind kind, hipStream_t s, void **buf, bool *fresh) {
    *fresh = false;
    const size_t bytes = t_pack_bytes(kind, Cout, Cin);
    if (!ctx->train_pack_cache) return t_ws(ctx, bytes, buf);
    for (auto &e : ctx->train_packs)
        if (e.w == w && e.Cout == Cout && e.Cin == Cin && e.flip == flip && e.kind == kind) {
            *buf = e.buf; *fresh = e.fresh; e.fresh = true;           // (a stale entry is packed by the caller right now)
            return PN_OK;
        }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cap);
    if (cap != hipStreamCaptureStatusNone)
        return pn_set_error(ctx, PN_ERR_STATE, "pn_train_pack_cache: a convolution met weights that were never packed while the stream is capturing (run one eager step first)");
    pn_ctx::PackEntry e;
    e.w = w; e.Cout = Cout; e.Cin = Cin; e.flip = flip; e.kind = kind; e.bytes = bytes; e.fresh = true; e.buf = nullptr;
    PN_HIP_CHECK(ctx, hipMalloc(&e.buf, bytes));
    ctx->train_packs.push_back(e);
    *buf = e.buf;
    return PN_OK;
}

static bool t_tile_geometry_x3w(int Ho, int Wo, int N, int Cout, bool every_shape, TTile *g) {     // 256-slot tiles; only when they still fill the chip
    g->tiles_x = (Wo + 63) / 64;
    g->TW = (Wo + g->tiles_x - 1) / g->tiles_x;
    g->R = 256 / g->TW;
    if (g->R > Ho) g->R = Ho;
    if (g->R < 1) g->R = 1;
    g->tiles_y = (Ho + g->R - 1) / g->R;
    g->HC = g->TW + 2;
    g->HR = g->R + 2;
    g->NI = 0;
    g->CHP = 0;
    const long blocks = (long)N * g->tiles_x * g->tiles_y * ((Cout + 63) / 64);
    const long slots = (long)g->R * g->TW;
    if (every_shape) return g->HR * g->HC <= 400;      // PnSwitches::train_x3_wide (tests): the wide kernel on every shape it can hold
    return g->HR * g->HC <= 400 && blocks >= 448 && slots >= 192;
}

static bool t_tile_geometry_x3(int Ho, int Wo, TTile *g) {       // tiles of at most 64 columns: the halo tile stays under 320 pixels
    g->tiles_x = (Wo + 63) / 64;
    g->TW = (Wo + g->tiles_x - 1) / g->tiles_x;
    g->R = 128 / g->TW;
    if (g->R > Ho) g->R = Ho;
    if (g->R < 1) g->R = 1;
    g->tiles_y = (Ho + g->R - 1) / g->R;
    g->HC = g->TW + 2;
    g->HR = g->R + 2;
    g->NI = 0;
    g->CHP = 0;
    return g->HR * g->HC <= 320;
}

// geometry of the vectorised variant: the x3pp tiles, the row layout described above; false = the shape stays on x3pp
static bool t_tile_geometry_wx3v(const TConv &c, TTileW *g, int *ppi, int *npieces) {
    if (c.pad != 1 || c.Ho != c.H || c.Wo != c.W || (c.W & 3)) return false;
    g->tiles_x = (c.Wo + 63) / 64;
    if (c.Wo % g->tiles_x) return false;
    g->TW = c.Wo / g->tiles_x;
    if (g->TW & 3) return false;
    g->SW = (g->TW + 7) / 8 * 8;
    g->R = 128 / g->SW;
    if (g->R > c.Ho) g->R = c.Ho;
    if (g->R < 1) return false;
    g->tiles_y = (c.Ho + g->R - 1) / g->R;
    g->HP = g->SW + 8;
    g->HR = g->R + 2;
    g->CHB = 16 + g->HR * g->HP * 2;
    // (channel stride 496 / 528 B: a sweep of + 0 .. 128 B found no faster mapping of the fragment reads onto the banks, a multiple of 256 B twice as slow: profiles/r05_notes.txt)
    *ppi = g->TW / 4 + 2;
    *npieces = TXW_CI * g->HR * *ppi;
    if (g->HR > 63 || *npieces > 256 * TXV_NPI) return false;
    const size_t sets = (size_t)2 * 2 * TXW_CI * g->CHB;
    return sets <= 158 * 1024;                              // (the launch asks for at least the 72 KB the accumulator hand-over at the end needs)
}

static bool t_tile_geometry_wx3(int Ho, int Wo, TTileW *g) {
    g->tiles_x = (Wo + 63) / 64;
    g->TW = (Wo + g->tiles_x - 1) / g->tiles_x;
    g->SW = (g->TW + 7) / 8 * 8;
    g->R = 128 / g->SW;
    if (g->R > Ho) g->R = Ho;
    if (g->R < 1) g->R = 1;
    g->tiles_y = (Ho + g->R - 1) / g->R;
    g->HP = g->SW + 8;
    g->HR = g->R + 2;
    g->CHB = g->HR * g->HP * 2 + 16;          // + 16: the dword after the last aligned group; 16 n + 16 keeps 16-byte alignment
    return g->SW <= 64 && 2 * 64 * TXW_YP + 2 * TXW_CI * g->CHB <= 78 * 1024;      // two blocks per CU
}

static int t_tile_lds_ok(pn_ctx *ctx) {       // the tile kernels use up to 76 KB of dynamic LDS: lift the 64 KB default once per context (= per device)
    bool &done = ctx->train_lds_attr;
    if (!done) {
        PN_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)tconv3_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        PN_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)tconv3_wgrad_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        PN_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)tconv3_tile_x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        PN_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)tconv3_wgrad_x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        PN_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)tconv3_tile_x3w_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        PN_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)tconv3_wgrad_x3pp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        PN_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)tconv3_wgrad_x3v_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        done = true;
    }
    return PN_OK;
}

static bool t_tile_geometry(int Ho, int Wo, int mod, TTile *g) {
    g->TW = Wo < 128 ? Wo : 128;
    g->R = 128 / g->TW;
    if (g->R > Ho) g->R = Ho;
    if (g->R < 1) g->R = 1;
    g->tiles_x = (Wo + g->TW - 1) / g->TW;
    g->tiles_y = (Ho + g->R - 1) / g->R;
    g->HC = g->TW + 2;
    g->HR = g->R + 2;
    const int n = g->HR * g->HC;
    g->NI = (n + 255) / 256;
    g->CHP = (n + 63) / 64 * 64 + mod;        // = mod (mod 64)
    if (g->CHP - 64 >= n) g->CHP -= 64;
    return g->NI <= TT_MAXNI;
}

// ---------------------------------------------------------------------------------------------------------------------
// Reductions per channel over (N, HW): grid (C, slices) partial sums in double, then a one-block-per-channel finish.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double t_block_sum(double v, double *sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += sh[i];
    return s;      // valid on thread 0
}

// MODE 0: sum x, sum x^2 (BN statistics).  MODE 1: sum g, sum g * (x - mean) with g = dy * act'(out) (BN backward).
// MODE 2: sum dy (bias gradient).
// BatchNorm's affine map, ONE definition for the forward and for the mask the backward recomputes from x (explicit fma: the
// three kernels that evaluate it must round identically)
__device__ __forceinline__ float t_bn_affine(float x, float mean, float invstd, float gamma, float beta) {
    return __fmaf_rn((x - mean) * invstd, gamma, beta);
}

// V = 4: four consecutive pixels per thread and 16-byte loads (HW and the slice length multiples of 4); V = 1 otherwise
template <int MODE, int V>
__global__ __launch_bounds__(256) void chan_reduce_kernel(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ out,
                                                           const float *__restrict__ mean, const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, int act, int N, int C, int HW, int slices,
                                                           double *__restrict__ partial) {
    __shared__ double sh[4];
    const int ch = blockIdx.x, sl = blockIdx.y;
    const long total = (long)N * HW;
    long per = (total + slices - 1) / slices;
    per = (per + V - 1) / V * V;
    const long beg = sl * per, end = min(beg + per, total);
    const float mu = MODE == 1 ? mean[ch] : 0.f;
    // out == nullptr (no residual in the forward): the activation mask is recomputed from x with the forward's own expression
    const bool remask = MODE == 1 && !out && act != PN_ACT_NONE;
    const float a_s = remask ? invstd[ch] : 0.f, a_g = remask ? gamma[ch] : 0.f, a_b = remask ? beta[ch] : 0.f;
    double s0 = 0.0, s1 = 0.0;
    // (image, pixel) walked without a division per element
    long i = beg + (long)threadIdx.x * V;
    int n = (int)(i / HW), p = (int)(i - (long)n * HW);
    for (; i < end; i += 256 * V) {
        const size_t off = ((size_t)n * C + ch) * HW + p;
        float xv[V], gv[V], ov[V];
        if (V == 4) {
            if (MODE != 2) *reinterpret_cast<float4 *>(xv) = *reinterpret_cast<const float4 *>(x + off);
            if (MODE != 0) *reinterpret_cast<float4 *>(gv) = *reinterpret_cast<const float4 *>(dy + off);
            if (MODE == 1 && act != PN_ACT_NONE && out) *reinterpret_cast<float4 *>(ov) = *reinterpret_cast<const float4 *>(out + off);
        } else {
            if (MODE != 2) xv[0] = x[off];
            if (MODE != 0) gv[0] = dy[off];
            if (MODE == 1 && act != PN_ACT_NONE && out) ov[0] = out[off];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (MODE == 0) {
                const double v = xv[k];
                s0 += v; s1 += v * v;
            } else if (MODE == 1) {
                float g = gv[k];
                if (act != PN_ACT_NONE) {
                    const float o = out ? ov[k] : t_bn_affine(xv[k], mu, a_s, a_g, a_b);
                    if (act == PN_ACT_RELU) g = o > 0.f ? g : 0.f;
                    else g = o > 0.f ? g : g * 0.1f;
                }
                s0 += g; s1 += (double)g * (double)(xv[k] - mu);
            } else {
                s0 += gv[k];
            }
        }
        p += 256 * V;
        while (p >= HW) { p -= HW; ++n; }
    }
    const double r0 = t_block_sum(s0, sh);
    const double r1 = t_block_sum(s1, sh);
    if (threadIdx.x == 0) {
        partial[((size_t)ch * slices + sl) * 2] = r0;
        partial[((size_t)ch * slices + sl) * 2 + 1] = r1;
    }
}

// launches the reduction with 16-byte loads when the layout allows it
template <int MODE>
static void t_chan_reduce(hipStream_t s, const float *x, const float *dy, const float *out, const float *mean, const float *invstd, const float *gamma,
                          const float *beta, int act, int N, int C, int HW, int slices, double *partial) {
    const bool v4 = (HW & 3) == 0 && ((((size_t)x) | ((size_t)dy) | ((size_t)out)) & 15) == 0;
    if (v4)
        hipLaunchKernelGGL((chan_reduce_kernel<MODE, 4>), dim3((unsigned)C, (unsigned)slices), dim3(256), 0, s, x, dy, out, mean, invstd, gamma, beta, act, N, C, HW, slices, partial);
    else
        hipLaunchKernelGGL((chan_reduce_kernel<MODE, 1>), dim3((unsigned)C, (unsigned)slices), dim3(256), 0, s, x, dy, out, mean, invstd, gamma, beta, act, N, C, HW, slices, partial);
}

// sum of a channel's `slices` partial pairs in slice order, eight pairs' loads in flight (the plain loop waited for every pair: a dependent chain of
// up to 256 round trips in front of every block of the apply kernels); same additions in the same order
__device__ __forceinline__ void t_sum_partials(const double *__restrict__ p, int slices, double &s, double &ss) {
    int k = 0;
    for (; k + 8 <= slices; k += 8) {
        double a[8], b[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { a[j] = p[(k + j) * 2]; b[j] = p[(k + j) * 2 + 1]; }
#pragma unroll
        for (int j = 0; j < 8; ++j) { s += a[j]; ss += b[j]; }
    }
    for (; k < slices; ++k) { s += p[k * 2]; ss += p[k * 2 + 1]; }
}

__global__ void sums_finish_kernel(const double *__restrict__ partial, int C, int slices, float *__restrict__ out0, float *__restrict__ out1,
                                   const float *__restrict__ invstd) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= C) return;
    double s = 0.0, ss = 0.0;
    t_sum_partials(partial + (size_t)ch * slices * 2, slices, s, ss);
    if (out0) out0[ch] = (float)s;                                     // d beta / d bias
    if (out1) out1[ch] = (float)(invstd ? ss * (double)invstd[ch] : ss);   // d gamma = sum g (x - mean) * invstd
}

// V = 4: four consecutive pixels per thread as one 16-byte access (HW a multiple of 4: every map of the network); V = 1 otherwise
// Round 4: the statistics are FINISHED here (bn_stats_finish_kernel's arithmetic, same order, in every thread of the block: `slices` <= 256
// partial pairs of the block's channel) instead of in a launch of their own -- 33 launches of one 64-thread block each per training step less;
// the block of image 0 / pixel group 0 publishes mean / invstd for the backward pass and updates the running statistics.
template <int V>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                const double *__restrict__ partial, int slices, double count, float eps, float momentum,
                                float *__restrict__ save_mean, float *__restrict__ save_invstd, float *__restrict__ running_mean, float *__restrict__ running_var,
                                const float *__restrict__ res, int act, int C, int HW, float *__restrict__ y) {
    const int p = (blockIdx.x * blockDim.x + threadIdx.x) * V;
    const int ch = blockIdx.y % C;
    double s = 0.0, ss = 0.0;
    t_sum_partials(partial + (size_t)ch * slices * 2, slices, s, ss);
    const double dmean = s / count;
    double var = ss / count - dmean * dmean;
    if (var < 0.0) var = 0.0;
    const float mu = (float)dmean, is = (float)(1.0 / sqrt(var + (double)eps));
    if (blockIdx.x == 0 && (int)blockIdx.y == ch && threadIdx.x == 0) {
        save_mean[ch] = mu;
        save_invstd[ch] = is;
        if (running_mean) running_mean[ch] = (float)((1.0 - momentum) * running_mean[ch] + momentum * dmean);
        if (running_var) running_var[ch] = (float)((1.0 - momentum) * running_var[ch] + momentum * var * (count / (count - 1.0)));
    }
    if (p >= HW) return;
    const size_t i = (size_t)blockIdx.y * HW + p;
    const float ga = gamma[ch], be = beta[ch];
    float xv[V], rv[V], o[V];
    if (V == 4) {
        *reinterpret_cast<float4 *>(xv) = *reinterpret_cast<const float4 *>(x + i);
        if (res) *reinterpret_cast<float4 *>(rv) = *reinterpret_cast<const float4 *>(res + i);
    } else {
        xv[0] = x[i];
        if (res) rv[0] = res[i];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        float v = t_bn_affine(xv[k], mu, is, ga, be);
        if (res) v += rv[k];
        if (act == PN_ACT_RELU) v = v > 0.f ? v : 0.f;
        else if (act == PN_ACT_LEAKY) v = v > 0.f ? v : v * 0.1f;
        o[k] = v;
    }
    if (V == 4) *reinterpret_cast<float4 *>(y + i) = *reinterpret_cast<const float4 *>(o);
    else y[i] = o[0];
}

// dx = gamma * invstd * (g - sum_g / n - (x - mean) * invstd^2 * sum_gx / n);  dres (+)= g   (identity path of a BasicBlock)
// grid (ceil(HW / (256 V)), N * C): the channel is uniform per block, no division per element
// Round 4: the two channel sums are finished here (bn_bwd_finish_kernel's arithmetic: slice-order double sums rounded to float) by every
// thread of the block; the block of image 0 / pixel group 0 writes d beta and d gamma.
template <int V>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ out,
                                    const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean, const float *__restrict__ invstd,
                                    const double *__restrict__ partial, int slices, float *__restrict__ dbeta, float *__restrict__ dgamma,
                                    int act, int C, int HW, float inv_count,
                                    float *__restrict__ dx, float *__restrict__ dres, int dres_accumulate) {
    const int p = (blockIdx.x * blockDim.x + threadIdx.x) * V;
    const int ch = blockIdx.y % C;
    double s = 0.0, ss = 0.0;
    t_sum_partials(partial + (size_t)ch * slices * 2, slices, s, ss);
    const float sum_g = (float)s, sum_gx = (float)ss;
    if (blockIdx.x == 0 && (int)blockIdx.y == ch && threadIdx.x == 0) {
        dbeta[ch] = sum_g;
        dgamma[ch] = (float)(ss * (double)invstd[ch]);
    }
    if (p >= HW) return;
    const size_t i = (size_t)blockIdx.y * HW + p;
    const float is = invstd[ch], mu = mean[ch], ga = gamma[ch];
    const float be = (act != PN_ACT_NONE && !out) ? beta[ch] : 0.f;
    const float mg = sum_g * inv_count, k2 = sum_gx * inv_count * is * is;
    float xv[V], gv[V], ov[V], dv[V], rv[V];
    if (V == 4) {
        *reinterpret_cast<float4 *>(xv) = *reinterpret_cast<const float4 *>(x + i);
        *reinterpret_cast<float4 *>(gv) = *reinterpret_cast<const float4 *>(dy + i);
        if (act != PN_ACT_NONE && out) *reinterpret_cast<float4 *>(ov) = *reinterpret_cast<const float4 *>(out + i);
        if (dres && dres_accumulate) *reinterpret_cast<float4 *>(rv) = *reinterpret_cast<const float4 *>(dres + i);
    } else {
        xv[0] = x[i];
        gv[0] = dy[i];
        if (act != PN_ACT_NONE && out) ov[0] = out[i];
        if (dres && dres_accumulate) rv[0] = dres[i];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        float g = gv[k];
        if (act != PN_ACT_NONE) {
            const float o = out ? ov[k] : t_bn_affine(xv[k], mu, is, ga, be);      // the forward's own expression (bn_apply_kernel)
            if (act == PN_ACT_RELU) g = o > 0.f ? g : 0.f;
            else g = o > 0.f ? g : g * 0.1f;
        }
        dv[k] = (g - mg - (xv[k] - mu) * k2) * is * ga;
        gv[k] = (dres && dres_accumulate) ? rv[k] + g : g;
    }
    if (V == 4) {
        *reinterpret_cast<float4 *>(dx + i) = *reinterpret_cast<const float4 *>(dv);
        if (dres) *reinterpret_cast<float4 *>(dres + i) = *reinterpret_cast<const float4 *>(gv);
    } else {
        dx[i] = dv[0];
        if (dres) dres[i] = gv[0];
    }
}

// AvgPool2d(3, stride 2, padding 1), count_include_pad = True
// (grid.y = plane, 32-bit pixel arithmetic: the flat 64-bit index cost three 64-bit divisions per element -- round 5)
__global__ void avgpool_fwd_kernel(const float *__restrict__ x, int H, int W, int Ho, int Wo, size_t total, float *__restrict__ y) {
    const int pp = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (pp >= Ho * Wo) return;
    const int oy = pp / Wo, ox = pp - oy * Wo;
    const size_t planes = total / ((size_t)Ho * Wo);
    for (size_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {       // grid.y = min(planes, 65535): any plane count
        const size_t i = plane * Ho * Wo + pp;
        const float *xp = x + plane * H * W;
        float s = 0.f;
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
                if (iy >= 0 && iy < H && ix >= 0 && ix < W) s += xp[(size_t)iy * W + ix];
            }
        y[i] = s / 9.f;
    }
}

__global__ void avgpool_bwd_kernel(const float *__restrict__ dy, int H, int W, int Ho, int Wo, size_t total, float *__restrict__ dx) {
    const int pp = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (pp >= H * W) return;
    const int iy = pp / W, ix = pp - iy * W;
    const size_t planes = total / ((size_t)H * W);
    for (size_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const size_t i = plane * H * W + pp;
        const float *dp = dy + plane * Ho * Wo;
        float s = 0.f;
        for (int oy = (iy >> 1); oy <= ((iy + 1) >> 1); ++oy)         // outputs whose window [2oy-1, 2oy+1] holds iy
            for (int ox = (ix >> 1); ox <= ((ix + 1) >> 1); ++ox)
                if (oy < Ho && ox < Wo) s += dp[(size_t)oy * Wo + ox];
        dx[i] = s / 9.f;
    }
}

// Heads: s = sigmoid(v); out = kind ? (s - 0.5) * 4 : s  (rtpose_light3d.py:335-337), written into a channel slice of the
// stage-2 input when out_ld > C (torch.cat, :339); loss partials sum w (out - t)^2 per block.
__global__ __launch_bounds__(256) void head_fwd_kernel(const float *__restrict__ v, const float *__restrict__ target, const float *__restrict__ fg, int kind,
                                                       int C, int HW, size_t total, float *__restrict__ s_out, float *__restrict__ out, int out_ld,
                                                       double *__restrict__ partial) {
    __shared__ double sh[4];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double e = 0.0;
    if (i < total) {
        const float s = 1.f / (1.f + expf(-v[i]));
        const float o = kind ? (s - 0.5f) * 4.f : s;
        s_out[i] = s;
        const size_t n = i / ((size_t)C * HW), rem = i - n * (size_t)C * HW;
        out[n * (size_t)out_ld * HW + rem] = o;
        const float d = o - target[i];
        const float w = fg ? 0.1f + fg[i] * 0.9f : 1.f;
        e = (double)(d * d * w);
    }
    const double r = t_block_sum(e, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

__global__ __launch_bounds__(256) void loss_finish_kernel(const double *__restrict__ partial, int nblocks, double numel, float *__restrict__ loss) {
    __shared__ double sh[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) s += partial[i];
    const double r = t_block_sum(s, sh);
    if (threadIdx.x == 0) *loss = (float)(r / numel);
}

// dv = (2 w (out - t) / numel + dextra) * (kind ? 4 : 1) * s (1 - s)
__global__ void head_bwd_kernel(const float *__restrict__ s_in, const float *__restrict__ target, const float *__restrict__ fg, const float *__restrict__ dextra,
                                int dextra_ld, int kind, int C, int HW, size_t total, float inv_numel, float *__restrict__ dv) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float s = s_in[i];
    const float o = kind ? (s - 0.5f) * 4.f : s;
    const float w = fg ? 0.1f + fg[i] * 0.9f : 1.f;
    float g = 2.f * (o - target[i]) * w * inv_numel;
    if (dextra) {
        const size_t n = i / ((size_t)C * HW), rem = i - n * (size_t)C * HW;
        g += dextra[n * (size_t)dextra_ld * HW + rem];
    }
    if (kind) g *= 4.f;
    dv[i] = g * (1.f - s) * s;
}

// torch.optim.SGD(momentum, nesterov=True, dampening 0, weight decay wd): buf = first ? g : mu buf + g; p -= lr (g + mu buf)
__global__ void sgd_nesterov_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ buf, size_t n, float lr, float mu, float wd,
                                    int first, float gscale) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float d = g[i] * gscale;
    if (wd != 0.f) d += wd * p[i];
    const float b = first ? d : mu * buf[i] + d;
    buf[i] = b;
    p[i] -= lr * (d + mu * b);
}

// copy a [N, C, HW] tensor into / out of a channel slice of a [N, ld, HW] tensor (torch.cat and its gradient)
__global__ void slice_copy_kernel(const float *__restrict__ src, int src_ld, float *__restrict__ dst, int dst_ld, int C, int HW, size_t total, int accumulate) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t n = i / ((size_t)C * HW), rem = i - n * (size_t)C * HW;
    const float v = src[n * (size_t)src_ld * HW + rem];
    float *d = dst + n * (size_t)dst_ld * HW + rem;
    *d = accumulate ? *d + v : v;
}

static int t_ws(pn_ctx *ctx, size_t bytes, void **out) {
    if (bytes > ctx->train_ws_bytes) {
        if (ctx->train_ws) {
            if (ctx->train_ws_keep) {
                // pn_train_ws_keep: a captured hipGraph still points into the old block -- retire it (freed with the ctx)
                // instead of freeing it; the graph keeps replaying on the old block, eager calls use the new one
                ctx->train_ws_retired.push_back(ctx->train_ws);
            } else {
                PN_HIP_CHECK(ctx, hipDeviceSynchronize());
                (void)hipFree(ctx->train_ws);
            }
            ctx->train_ws = nullptr;
            ctx->train_ws_bytes = 0;
        }
        const size_t want = bytes + bytes / 4;
        PN_HIP_CHECK(ctx, hipMalloc(&ctx->train_ws, want));
        ctx->train_ws_bytes = want;
    }
    *out = ctx->train_ws;
    return PN_OK;
}

int pn_train_ws(pn_ctx *ctx, size_t bytes, void **out) { return t_ws(ctx, bytes, out); }

static int t_slices(long total, int C) {       // slices per channel so that the reduction fills the chip
    long s = (1024 + C - 1) / C;
    const long cap = (total + 4095) / 4096;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    if (s > 256) s = 256;
    return (int)s;
}

// ---- dispatch decisions ------------------------------------------------------------------------------------------------
// ONE function per entry decides which kernel a shape runs on and with what geometry; the launch code below and
// pn_train_conv_plan_info (diagnostics, tests) both call it, so the description cannot drift from the launch.
enum { TK_GENERIC = 0, TK_TILE, TK_TILE_X3, TK_TILE_X3W };                      // forward / data gradient
enum { TKW_GENERIC = 0, TKW_TILE, TKW_X3, TKW_X3PP, TKW_X3V };                  // weight gradient

struct TTilePlan {
    int kernel;     // TK_*
    TTile g;        // geometry of the chosen tile kernel (unset for TK_GENERIC)
};

// a 3x3 stride-1 convolution of K input channels to M output channels on an Ho x Wo map (the data gradient calls it with K = Cout, M = Cin)
static TTilePlan t_plan_tile3(const pn_ctx *ctx, int N, int K, int M, int Ho, int Wo) {
    TTilePlan p = TTilePlan();
    p.kernel = TK_GENERIC;
    if (K < 16 || !t_tile_geometry(Ho, Wo, 16, &p.g)) return p;
    p.kernel = TK_TILE;
    TTile gx;
    if (ctx->train_x3 && K >= 32 && t_tile_geometry_x3(Ho, Wo, &gx)) {
        p.kernel = TK_TILE_X3;
        p.g = gx;
        TTile gw2;
        if (t_tile_geometry_x3w(Ho, Wo, N, M, pn_read_switches().train_x3_wide, &gw2)) {
            p.kernel = TK_TILE_X3W;
            p.g = gw2;
        }
    }
    return p;
}

static TTilePlan t_plan_forward(const pn_ctx *ctx, int N, int Cin, int Cout, int Ho, int Wo, int ks, int stride, int pad) {
    if (ks == 3 && stride == 1 && pad <= 2) return t_plan_tile3(ctx, N, Cin, Cout, Ho, Wo);
    TTilePlan p = TTilePlan();
    p.kernel = TK_GENERIC;
    return p;
}

static TTilePlan t_plan_dgrad(const pn_ctx *ctx, int N, int Cin, int H, int W, int Cout, int ks) {
    if (ks == 3) return t_plan_tile3(ctx, N, Cout, Cin, H, W);
    TTilePlan p = TTilePlan();
    p.kernel = TK_GENERIC;      // rotated weights (wflip_kernel), then pn_conv2d_forward's own plan
    return p;
}

// What the chosen weight-gradient kernel launches with.
struct TWgradPlan {
    int kernel;                 // TKW_*
    TTile g;                    // TKW_TILE
    TTileW gw;                  // TKW_X3, TKW_X3PP, TKW_X3V (x3v: the tiles of x3pp, its own row layout)
    int ppi, npieces;           // TKW_X3V
    int col_blocks;             // grid.x: blocks of 64 k columns (generic), of 16 / TXW_CI input channels (tile kernels)
    int tiles;                  // tile kernels: tiles of the chosen kernel's grid
    long slices, per_slice;     // grid.z, and the tiles (generic: pixels) of a slice
    long ws_slices;             // slices the partial-sum buffer is sized for: the larger of the fp32 tile kernel's and the chosen kernel's
                                // (captured graphs and retired blocks depend on when the workspace grows)
    size_t lds;                 // dynamic LDS bytes of the launch
    int csl;                    // slices of the bias-gradient reduction (t_slices)
};

// The generic weight gradient's slices of pps pixels (whole 32-pixel chunks): enough (column block, cout block) x slice blocks to fill the chip,
// at least 1024 pixels per slice.  pn_stem_wgrad_planes launches with the same rule: the same partial sums in the same order.
static void t_wgrad_pixel_slices(long P, int Kdim, int Cout, long *slices, long *pps) {
    const int tiles = ((Kdim + 63) / 64) * ((Cout + 63) / 64);
    long s = (1024 + tiles - 1) / tiles;
    const long cap = (P + 1023) / 1024;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    long per = (P + s - 1) / s;
    per = (per + TW_RC - 1) / TW_RC * TW_RC;
    *slices = (P + per - 1) / per;
    *pps = per;
}

// Enough slices for `target` blocks when a slice is `groups` blocks, at least min_tiles tiles per slice, then rebalanced: no slice is empty.
// *slices = 0: there are fewer than min_tiles tiles.
static void t_fill_chip(int target, int groups, int tiles, int min_tiles, long *slices, long *per_slice) {
    int S = (target + groups - 1) / groups;
    if (S > tiles / min_tiles) S = tiles / min_tiles;
    *slices = *per_slice = 0;
    if (S < 1) return;
    const int per = (tiles + S - 1) / S;
    *slices = (tiles + per - 1) / per;
    *per_slice = per;
}

// c: the convolution with Ho, Wo, Kdim, P filled in
static TWgradPlan t_plan_wgrad(const pn_ctx *ctx, const TConv &c, int ks) {
    TWgradPlan p = TWgradPlan();
    const int N = c.N, Cin = c.Cin, Cout = c.Cout, cout_blocks = (Cout + 63) / 64;
    p.csl = t_slices(c.P, Cout);
    if (!(ks == 3 && c.stride == 1 && c.pad <= 2 && Cin >= 16 && t_tile_geometry(c.Ho, c.Wo, 4, &p.g))) {
        p.kernel = TKW_GENERIC;
        p.col_blocks = (c.Kdim + 63) / 64;
        t_wgrad_pixel_slices(c.P, c.Kdim, Cout, &p.slices, &p.per_slice);
        p.ws_slices = p.slices;
        return p;
    }
    p.kernel = TKW_TILE;
    p.col_blocks = (Cin + 15) / 16;
    p.tiles = N * p.g.tiles_x * p.g.tiles_y;
    t_fill_chip(512, p.col_blocks * cout_blocks, p.tiles, 1, &p.slices, &p.per_slice);      // two blocks per CU: 512 fill the chip
    p.lds = (size_t)(128 * TT_YP + p.g.HR * p.g.HC * TT_HP + 128) * sizeof(float);
    p.ws_slices = p.slices;
    if (!(ctx->train_x3 && t_tile_geometry_wx3(c.Ho, c.Wo, &p.gw))) return p;
    // the split-bf16 variants: their own tile grid
    p.col_blocks = (Cin + TXW_CI - 1) / TXW_CI;
    p.tiles = N * p.gw.tiles_x * p.gw.tiles_y;
    const int groups = p.col_blocks * cout_blocks;
    const size_t setb = (size_t)2 * 64 * TXW_YP + (size_t)2 * TXW_CI * p.gw.CHB;
    // ping-pong variant: one 8-wave block per CU, at least two tiles per block, or the second wave group has nothing to do -- and only if the LDS sets fit
    t_fill_chip(256, groups, p.tiles, 2, &p.slices, &p.per_slice);
    if (p.slices >= 1 && 2 * setb <= 158 * 1024 && 2 * setb >= 73728) {
        p.kernel = TKW_X3PP;
        p.lds = 2 * setb;
        // the same tiles and slices as x3pp (bit-identical partial sums), one round trip of staging per tile
        TTileW gv;
        if (!pn_read_switches().train_wgrad_novec && t_tile_geometry_wx3v(c, &gv, &p.ppi, &p.npieces) && gv.tiles_x == p.gw.tiles_x &&
            gv.tiles_y == p.gw.tiles_y && gv.R == p.gw.R && gv.TW == p.gw.TW) {
            p.kernel = TKW_X3V;
            p.gw = gv;
            p.lds = std::max<size_t>((size_t)2 * 2 * TXW_CI * gv.CHB, (size_t)72 * 256 * 4);
        }
    } else {
        p.kernel = TKW_X3;
        t_fill_chip(512, groups, p.tiles, 1, &p.slices, &p.per_slice);      // two blocks per CU: 512 fill the chip; fewer slices = less partial-sum traffic
        p.lds = setb;
    }
    p.ws_slices = std::max(p.ws_slices, p.slices);
    return p;
}

static const char *t_fwd_label(int kernel, int ks) {
    switch (kernel) {
    case TK_TILE: return "tconv3_tile_kernel";
    case TK_TILE_X3: return "tconv3_tile_x3_kernel";
    case TK_TILE_X3W: return "tconv3_tile_x3w_kernel";
    default: return ks == 1 ? "tconv_fwd_kernel<1>" : ks == 3 ? "tconv_fwd_kernel<3>" : "tconv_fwd_kernel<7>";
    }
}

static const char *t_wgrad_label(int kernel, int ks) {
    switch (kernel) {
    case TKW_TILE: return "tconv3_wgrad_tile_kernel";
    case TKW_X3: return "tconv3_wgrad_x3_kernel";
    case TKW_X3PP: return "tconv3_wgrad_x3pp_kernel";
    case TKW_X3V: return "tconv3_wgrad_x3v_kernel";
    default: return ks == 1 ? "tconv_wgrad_kernel<1>" : ks == 3 ? "tconv_wgrad_kernel<3>" : "tconv_wgrad_kernel<7>";
    }
}

// The shape of a convolution (the pointers are the caller's), range-checked; `who` names the entry in the error message.
static int t_conv_desc(pn_ctx *ctx, TConv *c, const char *who, int N, int Cin, int H, int W, int Cout, int ks, int stride, int pad, int accumulate) {
    c->N = N; c->Cin = Cin; c->H = H; c->W = W; c->Cout = Cout; c->stride = stride; c->pad = pad; c->accumulate = accumulate;
    c->Ho = (H + 2 * pad - ks) / stride + 1;
    c->Wo = (W + 2 * pad - ks) / stride + 1;
    c->Kdim = Cin * ks * ks;
    const long P = (long)N * c->Ho * c->Wo;
    if (c->Ho < 1 || c->Wo < 1 || P > 0x7fffffffL) return pn_set_error(ctx, PN_ERR_INVALID, "%s: size out of range", who);
    c->P = (int)P;
    return PN_OK;
}

// The second-generation 3x3 kernels (TK_TILE, TK_TILE_X3, TK_TILE_X3W) on convolution c: weights w_dev packed to the kernel's order
// (flip: the data gradient's rotated, transposed weights -- the packing IS the rotation; the pack's shape is c's own Cout x Cin), then halo tiles.
static int t_launch_tile3(pn_ctx *ctx, const TTilePlan &plan, const TConv &c, const float *w_dev, int flip, hipStream_t s) {
    const TTile &g = plan.g;
    const PnPackKind kind = plan.kernel == TK_TILE ? PN_PACK_TILE3 : PN_PACK_TILE3_X3;
    void *ws = nullptr;
    bool fresh = false;
    int rc;
    if ((rc = t_tile_lds_ok(ctx)) != PN_OK) return rc;
    const dim3 grid((unsigned)(c.N * g.tiles_x * g.tiles_y), (unsigned)((c.Cout + 63) / 64));
    if ((rc = t_pack_get(ctx, w_dev, c.Cout, c.Cin, flip, kind, s, &ws, &fresh)) != PN_OK) return rc;
    const dim3 pack_grid(t_pack_blocks(kind, c.Cout, c.Cin));
    if (plan.kernel == TK_TILE) {
        if (!fresh) hipLaunchKernelGGL(wpack3_kernel, pack_grid, dim3(256), 0, s, w_dev, (float *)ws, c.Cout, c.Cin, flip);
        const size_t lds = (size_t)(144 * TT_AP + 16 * g.CHP) * sizeof(float);
        hipLaunchKernelGGL(tconv3_tile_kernel, grid, dim3(256), lds, s, c, g, (const float *)ws);
    } else {
        if (!fresh) hipLaunchKernelGGL(wpack3_x3_kernel, pack_grid, dim3(256), 0, s, w_dev, (__bf16 *)ws, c.Cout, c.Cin, flip);
        if (plan.kernel == TK_TILE_X3W) {
            const size_t ldsw2 = (size_t)2 * TXW2_A_BYTES + (size_t)2 * g.HR * g.HC * TXW2_PITCH;
            hipLaunchKernelGGL(tconv3_tile_x3w_kernel, grid, dim3(256), ldsw2, s, c, g, (const __bf16 *)ws);
        } else {
            const size_t ldsx = (size_t)2 * TX_A_BYTES + (size_t)2 * g.HR * g.HC * TX_PITCH;
            hipLaunchKernelGGL(tconv3_tile_x3_kernel, grid, dim3(256), ldsx, s, c, g, (const __bf16 *)ws);
        }
    }
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

extern "C" {

int pn_train_ws_keep(pn_ctx *ctx, int keep) {
    PN_CTX_CHECK
    ctx->train_ws_keep = keep != 0;
    return PN_OK;
}

int pn_train_pack_cache(pn_ctx *ctx, int enable) {
    PN_CTX_CHECK
    if (!enable && ctx->train_pack_cache) {
        PN_HIP_CHECK(ctx, hipDeviceSynchronize());
        for (auto &e : ctx->train_packs) (void)hipFree(e.buf);
        ctx->train_packs.clear();
        if (ctx->train_pack_table) (void)hipFree(ctx->train_pack_table);
        ctx->train_pack_table = nullptr;
        ctx->train_pack_table_entries = 0;
        ctx->train_pack_table_cap = 0;
    }
    ctx->train_pack_cache = enable != 0;
    return PN_OK;
}

int pn_train_pack_refresh(pn_ctx *ctx, void *hip_stream) {
    PN_CTX_CHECK
    if (!ctx->train_pack_cache || ctx->train_packs.empty()) return PN_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t n = ctx->train_packs.size();
    if (ctx->train_pack_table_entries != n) {
        // the list has grown since the table was uploaded (the engine's first steps): rebuild it -- never under a capture
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s, &cap);
        if (cap != hipStreamCaptureStatusNone)
            return pn_set_error(ctx, PN_ERR_STATE, "pn_train_pack_refresh: the pack list changed since the last eager step; run one eager step before capturing");
        std::vector<TPackDesc> host(n);
        unsigned blocks = 0;
        for (size_t i = 0; i < n; ++i) {
            const auto &e = ctx->train_packs[i];
            host[i] = TPackDesc{e.w, e.buf, e.Cout, e.Cin, e.flip, e.kind, blocks, 0u};
            blocks += t_pack_blocks(e.kind, e.Cout, e.Cin);
        }
        PN_HIP_CHECK(ctx, hipStreamSynchronize(s));
        // The table is APPEND-ONLY in a fixed-capacity block: a captured step graph bakes (table pointer, entry count, grid) into its
        // wpack_all_kernel node, and an eager step of another resolution after capture() adds (w, Cout, Cin, flip, kind) keys.  Entries
        // 0 .. n_old - 1 keep their bytes and their block offsets, so the replayed node stays valid (the table used to be
        // freed and reallocated here -- a replay then read freed memory).  Beyond the capacity the old block is retired, not freed,
        // while a graph may point at it (pn_train_ws_keep), exactly like train_ws.
        if (n > ctx->train_pack_table_cap) {
            size_t cap = std::max<size_t>(256, ctx->train_pack_table_cap * 2);
            while (cap < n) cap *= 2;
            if (ctx->train_pack_table) {
                if (ctx->train_ws_keep) ctx->train_ws_retired.push_back(ctx->train_pack_table);
                else (void)hipFree(ctx->train_pack_table);
                ctx->train_pack_table = nullptr;
            }
            PN_HIP_CHECK(ctx, hipMalloc(&ctx->train_pack_table, cap * sizeof(TPackDesc)));
            ctx->train_pack_table_cap = cap;
        }
        PN_HIP_CHECK(ctx, hipMemcpy(ctx->train_pack_table, host.data(), n * sizeof(TPackDesc), hipMemcpyHostToDevice));
        ctx->train_pack_table_entries = n;
        ctx->train_pack_blocks = blocks;
    }
    hipLaunchKernelGGL(wpack_all_kernel, dim3(ctx->train_pack_blocks), dim3(256), 0, s, (const TPackDesc *)ctx->train_pack_table, (int)n);
    PN_HIP_CHECK(ctx, hipGetLastError());
    for (auto &e : ctx->train_packs) e.fresh = true;
    return PN_OK;
}

int pn_train_set_precision(pn_ctx *ctx, int precision) {
    if (!ctx) return PN_ERR_INVALID;          // a host-side switch: a context without a device takes it too (pn_train_conv_plan_info on a CPU-only host)
    if (precision != PN_PREC_F32 && precision != PN_PREC_BF16X3)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_train_set_precision: PN_PREC_F32 or PN_PREC_BF16X3");
    ctx->train_x3 = precision == PN_PREC_BF16X3;
    return PN_OK;
}

int pn_conv2d_forward(pn_ctx *ctx, const float *x_dev, const float *w_dev, const float *bias_dev, float *y_dev, int N, int Cin, int H, int W,
                      int Cout, int ks, int stride, int pad, int accumulate, void *hip_stream) {
    PN_CTX_CHECK
    if (!x_dev || !w_dev || !y_dev || N < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1 || stride < 1 || pad < 0 || (ks != 1 && ks != 3 && ks != 7))
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv2d_forward: bad arguments (kernel sizes 1, 3, 7)");
    TConv c;
    c.x = x_dev; c.w = w_dev; c.bias = bias_dev; c.y = y_dev;
    if (int rc = t_conv_desc(ctx, &c, "pn_conv2d_forward", N, Cin, H, W, Cout, ks, stride, pad, accumulate)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const TTilePlan plan = t_plan_forward(ctx, N, Cin, Cout, c.Ho, c.Wo, ks, stride, pad);
    if (plan.kernel != TK_GENERIC) return t_launch_tile3(ctx, plan, c, w_dev, 0, s);
    dim3 grid((unsigned)(((long)c.P + 127) / 128), (unsigned)((Cout + 63) / 64)), block(256);
    if (ks == 1) hipLaunchKernelGGL(tconv_fwd_kernel<1>, grid, block, 0, s, c);
    else if (ks == 3) hipLaunchKernelGGL(tconv_fwd_kernel<3>, grid, block, 0, s, c);
    else hipLaunchKernelGGL(tconv_fwd_kernel<7>, grid, block, 0, s, c);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_conv2d_dgrad(pn_ctx *ctx, const float *dy_dev, const float *w_dev, float *dx_dev, int N, int Cin, int H, int W, int Cout, int ks, int pad,
                    int accumulate, void *hip_stream) {
    PN_CTX_CHECK
    if (!dy_dev || !w_dev || !dx_dev || (ks != 1 && ks != 3 && ks != 7) || pad > ks - 1)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv2d_dgrad: bad arguments (stride 1 only)");
    const int Ho = H + 2 * pad - ks + 1, Wo = W + 2 * pad - ks + 1;
    hipStream_t s = (hipStream_t)hip_stream;
    const TTilePlan plan = t_plan_dgrad(ctx, N, Cin, H, W, Cout, ks);
    if (plan.kernel != TK_GENERIC) {
        // dX = conv(dY, rotated transposed weights, padding 2 - pad) on the halo-tile kernel
        TConv c;
        c.x = dy_dev; c.w = nullptr; c.bias = nullptr; c.y = dx_dev;
        c.N = N; c.Cin = Cout; c.H = Ho; c.W = Wo; c.Cout = Cin; c.stride = 1; c.pad = 2 - pad; c.accumulate = accumulate;
        c.Ho = H; c.Wo = W; c.Kdim = Cout * 9; c.P = N * H * W;
        return t_launch_tile3(ctx, plan, c, w_dev, 1, s);
    }
    const size_t wn = (size_t)Cout * Cin * ks * ks;
    void *ws = nullptr;
    if (int rc = t_ws(ctx, wn * sizeof(float), &ws)) return rc;
    hipLaunchKernelGGL(wflip_kernel, dim3((unsigned)((wn + 255) / 256)), dim3(256), 0, s, w_dev, (float *)ws, Cout, Cin, ks);
    // dX = conv(dY [N, Cout, Ho, Wo], Wt [Cin, Cout, ks, ks], padding ks - 1 - pad)
    return pn_conv2d_forward(ctx, dy_dev, (const float *)ws, nullptr, dx_dev, N, Cout, Ho, Wo, Cin, ks, 1, ks - 1 - pad, accumulate, hip_stream);
}

int pn_conv2d_wgrad(pn_ctx *ctx, const float *x_dev, const float *dy_dev, float *dw_dev, float *dbias_dev, int N, int Cin, int H, int W, int Cout,
                    int ks, int stride, int pad, void *hip_stream) {
    PN_CTX_CHECK
    if (!x_dev || !dy_dev || !dw_dev || N < 1 || (ks != 1 && ks != 3 && ks != 7) || stride < 1)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv2d_wgrad: bad arguments");
    TConv c;
    c.x = x_dev; c.w = nullptr; c.bias = nullptr; c.y = (float *)dy_dev;
    if (int rc = t_conv_desc(ctx, &c, "pn_conv2d_wgrad", N, Cin, H, W, Cout, ks, stride, pad, 0)) return rc;
    const TWgradPlan plan = t_plan_wgrad(ctx, c, ks);
    const bool tiled = plan.kernel != TKW_GENERIC;
    const size_t wn = (size_t)Cout * c.Kdim;
    hipStream_t s = (hipStream_t)hip_stream;
    // workspace: the partial sums (sized for the largest grid any of the tile kernels may be launched with), then the bias gradient's partials
    // 16-byte aligned behind them (the byte count of the generic path has never been rounded up: when the workspace grows stays as it is)
    const size_t part_bytes = wn * (size_t)plan.ws_slices * sizeof(float), part_off = (part_bytes + 15) & ~(size_t)15;
    void *ws = nullptr;
    if (int rc = t_ws(ctx, (tiled ? part_off : part_bytes) + 16 + (size_t)Cout * plan.csl * 2 * sizeof(double), &ws)) return rc;
    if (tiled)
        if (int rc = t_tile_lds_ok(ctx)) return rc;
    float *partial = (float *)ws;
    const int slices = (int)plan.slices, per = (int)plan.per_slice;
    const dim3 grid((unsigned)plan.col_blocks, (unsigned)((Cout + 63) / 64), (unsigned)slices);
    switch (plan.kernel) {
    case TKW_X3V: hipLaunchKernelGGL(tconv3_wgrad_x3v_kernel, grid, dim3(512), plan.lds, s, c, plan.gw, partial, per, plan.tiles, plan.ppi, plan.npieces); break;
    case TKW_X3PP: hipLaunchKernelGGL(tconv3_wgrad_x3pp_kernel, grid, dim3(512), plan.lds, s, c, plan.gw, partial, per, plan.tiles); break;
    case TKW_X3: hipLaunchKernelGGL(tconv3_wgrad_x3_kernel, grid, dim3(256), plan.lds, s, c, plan.gw, partial, per, plan.tiles); break;
    case TKW_TILE: hipLaunchKernelGGL(tconv3_wgrad_tile_kernel, grid, dim3(256), plan.lds, s, c, plan.g, partial, per, plan.tiles); break;
    default:
        if (ks == 1) hipLaunchKernelGGL(tconv_wgrad_kernel<1>, grid, dim3(256), 0, s, c, partial, per);
        else if (ks == 3) hipLaunchKernelGGL(tconv_wgrad_kernel<3>, grid, dim3(256), 0, s, c, partial, per);
        else hipLaunchKernelGGL(tconv_wgrad_kernel<7>, grid, dim3(256), 0, s, c, partial, per);
    }
    t_wgrad_reduce(s, partial, dw_dev, wn, slices);
    if (dbias_dev) {
        double *part = (double *)((char *)ws + part_off);
        t_chan_reduce<2>(s, nullptr, dy_dev, nullptr, nullptr, nullptr, nullptr, nullptr, 0, N, Cout, c.Ho * c.Wo, plan.csl, part);
        hipLaunchKernelGGL(sums_finish_kernel, dim3((unsigned)((Cout + 63) / 64)), dim3(64), 0, s, (const double *)part, Cout, plan.csl, dbias_dev, nullptr, nullptr);
    }
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

// ---- dilated 3x3 convolutions (A2J_model's layer4.1 / layer4.2 conv2; the contract is in popnet_hip.h next to pn_a2j_loss) --------------
// The gather kernels with the taps `dil` apart: tconv_fwd_kernel<3, 0, true> (forward; on the rotated pack with padding 2 dil - pad, the data
// gradient) and tconv_wgrad_kernel<3, true>, with the grids, slices and reductions of the undilated generic path.  dil == 1 IS the undilated entry.
static int t_dil_desc(pn_ctx *ctx, TConv *c, const char *who, int N, int Cin, int H, int W, int Cout, int ks, int stride, int pad, int dil, int accumulate) {
    if (N < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1 || ks != 3 || stride != 1 || dil < 1 || pad < 0 || pad > 2 * dil)
        return pn_set_error(ctx, PN_ERR_INVALID, "%s: bad arguments (kernel 3, stride 1, dil >= 1, 0 <= pad <= 2 dil)", who);
    c->N = N; c->Cin = Cin; c->H = H; c->W = W; c->Cout = Cout; c->stride = 1; c->pad = pad; c->accumulate = accumulate; c->dil = dil;
    c->Ho = H + 2 * pad - 2 * dil;
    c->Wo = W + 2 * pad - 2 * dil;
    c->Kdim = Cin * 9;
    const long P = (long)N * c->Ho * c->Wo;
    if (c->Ho < 1 || c->Wo < 1 || P > 0x7fffffffL || (long)Cin * H * W > 0x7fffffffL || (long)Cout * c->Ho * c->Wo > 0x7fffffffL)
        return pn_set_error(ctx, PN_ERR_INVALID, "%s: size out of range", who);
    c->P = (int)P;
    return PN_OK;
}

int pn_conv2d_forward_dil(pn_ctx *ctx, const float *x_dev, const float *w_dev, const float *bias_dev, float *y_dev, int N, int Cin, int H, int W,
                          int Cout, int ks, int stride, int pad, int dil, int accumulate, void *hip_stream) {
    PN_CTX_CHECK
    if (!x_dev || !w_dev || !y_dev) return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv2d_forward_dil: null tensor");
    TConv c;
    c.x = x_dev; c.w = w_dev; c.bias = bias_dev; c.y = y_dev;
    if (int rc = t_dil_desc(ctx, &c, "pn_conv2d_forward_dil", N, Cin, H, W, Cout, ks, stride, pad, dil, accumulate)) return rc;
    if (dil == 1) return pn_conv2d_forward(ctx, x_dev, w_dev, bias_dev, y_dev, N, Cin, H, W, Cout, ks, stride, pad, accumulate, hip_stream);
    const dim3 grid((unsigned)(((long)c.P + 127) / 128), (unsigned)((Cout + 63) / 64));
    hipLaunchKernelGGL((tconv_fwd_kernel<3, 0, true>), grid, dim3(256), 0, (hipStream_t)hip_stream, c);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_conv2d_dgrad_dil(pn_ctx *ctx, const float *dy_dev, const float *w_dev, float *dx_dev, int N, int Cin, int H, int W, int Cout, int ks, int pad,
                        int dil, int accumulate, void *hip_stream) {
    PN_CTX_CHECK
    if (!dy_dev || !w_dev || !dx_dev) return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv2d_dgrad_dil: null tensor");
    TConv f;        // the forward convolution this is the gradient of: range checks and the shape of dy
    if (int rc = t_dil_desc(ctx, &f, "pn_conv2d_dgrad_dil", N, Cin, H, W, Cout, ks, 1, pad, dil, accumulate)) return rc;
    if (dil == 1) return pn_conv2d_dgrad(ctx, dy_dev, w_dev, dx_dev, N, Cin, H, W, Cout, ks, pad, accumulate, hip_stream);
    const size_t wn = (size_t)Cout * Cin * 9;
    void *ws = nullptr;
    if (int rc = t_ws(ctx, wn * sizeof(float), &ws)) return rc;
    hipLaunchKernelGGL(wflip_kernel, dim3((unsigned)((wn + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, w_dev, (float *)ws, Cout, Cin, 3);
    // dX = conv(dY [N, Cout, Ho, Wo], Wt [Cin, Cout, 3, 3], padding 2 dil - pad, the same dilation): Ho + 2 (2 dil - pad) - 2 dil = H
    return pn_conv2d_forward_dil(ctx, dy_dev, (const float *)ws, nullptr, dx_dev, N, Cout, f.Ho, f.Wo, Cin, 3, 1, 2 * dil - pad, dil, accumulate, hip_stream);
}

int pn_conv2d_wgrad_dil(pn_ctx *ctx, const float *x_dev, const float *dy_dev, float *dw_dev, float *dbias_dev, int N, int Cin, int H, int W, int Cout,
                        int ks, int stride, int pad, int dil, void *hip_stream) {
    PN_CTX_CHECK
    if (!x_dev || !dy_dev || !dw_dev) return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv2d_wgrad_dil: null tensor");
    TConv c;
    c.x = x_dev; c.w = nullptr; c.bias = nullptr; c.y = (float *)dy_dev;
    if (int rc = t_dil_desc(ctx, &c, "pn_conv2d_wgrad_dil", N, Cin, H, W, Cout, ks, stride, pad, dil, 0)) return rc;
    if (dil == 1) return pn_conv2d_wgrad(ctx, x_dev, dy_dev, dw_dev, dbias_dev, N, Cin, H, W, Cout, ks, stride, pad, hip_stream);
    // pn_conv2d_wgrad's generic path: pixel slices, partial sums reduced in slice order, the bias gradient's partials behind them
    long slices, pps;
    t_wgrad_pixel_slices(c.P, c.Kdim, Cout, &slices, &pps);
    const int csl = t_slices(c.P, Cout);
    const size_t wn = (size_t)Cout * c.Kdim;
    const size_t part_off = (wn * (size_t)slices * sizeof(float) + 15) & ~(size_t)15;
    void *ws = nullptr;
    if (int rc = t_ws(ctx, part_off + 16 + (size_t)Cout * csl * 2 * sizeof(double), &ws)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const dim3 grid((unsigned)((c.Kdim + 63) / 64), (unsigned)((Cout + 63) / 64), (unsigned)slices);
    hipLaunchKernelGGL((tconv_wgrad_kernel<3, true>), grid, dim3(256), 0, s, c, (float *)ws, (int)pps);
    t_wgrad_reduce(s, (const float *)ws, dw_dev, wn, (int)slices);
    if (dbias_dev) {
        double *part = (double *)((char *)ws + part_off);
        t_chan_reduce<2>(s, nullptr, dy_dev, nullptr, nullptr, nullptr, nullptr, nullptr, 0, N, Cout, c.Ho * c.Wo, csl, part);
        hipLaunchKernelGGL(sums_finish_kernel, dim3((unsigned)((Cout + 63) / 64)), dim3(64), 0, s, (const double *)part, Cout, csl, dbias_dev, nullptr, nullptr);
    }
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

}   // extern "C"
// ---- what conv1x1_x3.hip shares with the entries above (internal, not part of the C ABI) -----------------------------------------------
int pn_train_pack_get(pn_ctx *ctx, const float *w, int Cout, int Cin, int flip, PnPackKind kind, hipStream_t s, void **buf, bool *fresh) {
    return t_pack_get(ctx, w, Cout, Cin, flip, kind, s, buf, fresh);
}

void pn_train_wgrad_reduce(hipStream_t s, const float *partial, float *dw_dev, size_t wn, int slices) { t_wgrad_reduce(s, partial, dw_dev, wn, slices); }

// dbias[co] = sum dy over (n, pixel): pn_conv2d_wgrad's bias gradient -- chan_reduce_kernel<2> in double over csl slices into part, then sums_finish_kernel
void pn_train_dbias(hipStream_t s, const float *dy_dev, float *dbias_dev, int N, int Cout, int HW, int csl, double *part) {
    t_chan_reduce<2>(s, nullptr, dy_dev, nullptr, nullptr, nullptr, nullptr, nullptr, 0, N, Cout, HW, csl, part);
    hipLaunchKernelGGL(sums_finish_kernel, dim3((unsigned)((Cout + 63) / 64)), dim3(64), 0, s, (const double *)part, Cout, csl, dbias_dev, nullptr, nullptr);
}

// ---- the planes training engine's stem (trainx.hip; internal, not part of the C ABI) --------------------------------------------------
// model0.conv1 (rtpose_light3d.py:144: 7x7 / 2, Cin = 1) with its output / its output gradient as a planes tensor (TConv::pl): the kernels,
// grids, slices and summation order of pn_conv2d_forward / pn_conv2d_wgrad's generic path, without the NCHW f32 hand-over tensor.
static int t_stem_conv(pn_ctx *ctx, TConv *c, const float *x_dev, void *planes, int cs, int split, int N, int Cin, int H, int W, int Cout, int ks, int stride, int pad) {
    if (!x_dev || !planes || N < 1 || Cin < 1 || ks != 7 || stride < 1 || pad < 0 || Cout < 8 || (Cout & 7) || cs < Cout || (cs & 7) || (split & 7))
        return pn_set_error(ctx, PN_ERR_INVALID, "planes stem: bad arguments (7x7, Cout and strides multiples of 8)");
    c->x = x_dev; c->w = nullptr; c->bias = nullptr; c->y = nullptr;
    if (int rc = t_conv_desc(ctx, c, "planes stem", N, Cin, H, W, Cout, ks, stride, pad, 0)) return rc;
    c->pl = planes; c->pl_cs = cs; c->pl_split = split;
    return PN_OK;
}

int pn_stem_forward_planes(pn_ctx *ctx, const float *x_dev, const float *w_dev, void *y_planes, int cs, int split, int f32, int N, int Cin, int H, int W, int Cout,
                           int ks, int stride, int pad, int gather, hipStream_t s) {
    PN_CTX_CHECK
    TConv c;
    if (int rc = t_stem_conv(ctx, &c, x_dev, y_planes, cs, split, N, Cin, H, W, Cout, ks, stride, pad)) return rc;
    if (!w_dev) return pn_set_error(ctx, PN_ERR_INVALID, "pn_stem_forward_planes: no weights");
    c.w = w_dev;
    if (!gather && Cin == 1 && Cout == 64 && stride == 2 && pad == 3) {         // the input patch in LDS (tstem_fwd_kernel)
        const int tiles_x = (c.Wo + 15) / 16, tiles_y = (c.Ho + 7) / 8;
        const long ntiles = (long)N * tiles_x * tiles_y;
        // blocks per CU, one-stream traces of the step: 1: 49.1, 2: 41.5, 3: 42.8, 4: 45.0, 6: 48.3, 12: 62.2 us (three are resident at 148 registers; every block
        // loads the 52 weight registers once)
        const unsigned blocks = (unsigned)std::min<long>(ntiles, (long)ctx->num_cus * 2);
        if (f32) hipLaunchKernelGGL(tstem_fwd_kernel<1>, dim3(blocks), dim3(256), 0, s, c, tiles_x, tiles_y, (int)ntiles);
        else hipLaunchKernelGGL(tstem_fwd_kernel<0>, dim3(blocks), dim3(256), 0, s, c, tiles_x, tiles_y, (int)ntiles);
        PN_HIP_CHECK(ctx, hipGetLastError());
        return PN_OK;
    }
    dim3 grid((unsigned)((c.P + 127) / 128), (unsigned)((Cout + 63) / 64)), block(256);
    if (f32) hipLaunchKernelGGL((tconv_fwd_kernel<7, 2>), grid, block, 0, s, c);
    else hipLaunchKernelGGL((tconv_fwd_kernel<7, 1>), grid, block, 0, s, c);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_stem_wgrad_planes(pn_ctx *ctx, const float *x_dev, const void *dy_planes, int cs, int split, int f32, const PnStemBn *bn, float *dw_dev, int N, int Cin, int H,
                         int W, int Cout, int ks, int stride, int pad, int depth, hipStream_t s) {
    PN_CTX_CHECK
    TConv c;
    if (int rc = t_stem_conv(ctx, &c, x_dev, (void *)dy_planes, cs, split, N, Cin, H, W, Cout, ks, stride, pad)) return rc;
    if (!dw_dev) return pn_set_error(ctx, PN_ERR_INVALID, "pn_stem_wgrad_planes: no output");
    long slices, pps;
    t_wgrad_pixel_slices(c.P, c.Kdim, Cout, &slices, &pps);
    const size_t wn = (size_t)Cout * c.Kdim;
    void *ws = nullptr;
    if (int rc = t_ws(ctx, wn * slices * sizeof(float) + 16, &ws)) return rc;
    dim3 grid((unsigned)((c.Kdim + 63) / 64), (unsigned)((Cout + 63) / 64), (unsigned)slices), block(512);
    TStemBn b = TStemBn();
    if (bn) {
        if (!bn->x || !bn->mean || !bn->invstd || !bn->k1 || !bn->k2 || !bn->k3 || !bn->scale || !bn->shift || (bn->x_cs & 7) || (bn->x_split & 7))
            return pn_set_error(ctx, PN_ERR_INVALID, "pn_stem_wgrad_planes: incomplete BatchNorm description");
        b.x = bn->x; b.x_cs = bn->x_cs; b.x_split = bn->x_split; b.mean = bn->mean; b.invstd = bn->invstd; b.k1 = bn->k1; b.k2 = bn->k2; b.k3 = bn->k3;
        b.scale = bn->scale; b.shift = bn->shift; b.act = bn->act;
    }
    float *wsf = (float *)ws;
    const int pp = (int)pps;
#define TSTEM_LAUNCH(F, B, D) hipLaunchKernelGGL((tstem_wgrad_kernel<7, F, B, D>), grid, block, 0, s, c, b, wsf, pp)
    if (depth <= 1) {        // (one chunk in flight: tconv_wgrad_kernel's schedule, for A/B runs)
        if (f32) { if (bn) TSTEM_LAUNCH(1, 1, 1); else TSTEM_LAUNCH(1, 0, 1); }
        else { if (bn) TSTEM_LAUNCH(0, 1, 1); else TSTEM_LAUNCH(0, 0, 1); }
    } else if (depth < 4) {
        if (f32) { if (bn) TSTEM_LAUNCH(1, 1, 2); else TSTEM_LAUNCH(1, 0, 2); }
        else { if (bn) TSTEM_LAUNCH(0, 1, 2); else TSTEM_LAUNCH(0, 0, 2); }
    } else {
        if (f32) { if (bn) TSTEM_LAUNCH(1, 1, 4); else TSTEM_LAUNCH(1, 0, 4); }
        else { if (bn) TSTEM_LAUNCH(0, 1, 4); else TSTEM_LAUNCH(0, 0, 4); }
    }
#undef TSTEM_LAUNCH
    t_wgrad_reduce(s, (const float *)ws, dw_dev, wn, (int)slices);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

extern "C" {
int pn_bn_train_forward(pn_ctx *ctx, const float *x_dev, const float *gamma_dev, const float *beta_dev, const float *res_dev, float *y_dev,
                        float *save_mean_dev, float *save_invstd_dev, float *running_mean_dev, float *running_var_dev, float momentum, float eps,
                        int act, int N, int C, int HW, void *hip_stream) {
    PN_CTX_CHECK
    if (!x_dev || !gamma_dev || !beta_dev || !y_dev || !save_mean_dev || !save_invstd_dev || N < 1 || C < 1 || HW < 1 || (long)N * HW < 2)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_bn_train_forward: bad arguments");
    if ((long)N * C > 65535) return pn_set_error(ctx, PN_ERR_INVALID, "pn_bn_train_forward: N * C out of range");        // (grid.y of the apply kernel) refused before anything is launched
    const long cnt = (long)N * HW;
    const int sl = t_slices(cnt, C);
    void *ws = nullptr;
    int rc = t_ws(ctx, (size_t)C * sl * 2 * sizeof(double), &ws);
    if (rc != PN_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    t_chan_reduce<0>(s, x_dev, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, N, C, HW, sl, (double *)ws);
    const bool v4 = (HW & 3) == 0 && ((((size_t)x_dev) | ((size_t)y_dev) | ((size_t)res_dev)) & 15) == 0;
    if (v4)
        hipLaunchKernelGGL(bn_apply_kernel<4>, dim3((unsigned)((HW / 4 + 255) / 256), (unsigned)(N * C)), dim3(256), 0, s, x_dev, gamma_dev, beta_dev, (const double *)ws, sl,
                           (double)cnt, eps, momentum, save_mean_dev, save_invstd_dev, running_mean_dev, running_var_dev, res_dev, act, C, HW, y_dev);
    else
        hipLaunchKernelGGL(bn_apply_kernel<1>, dim3((unsigned)((HW + 255) / 256), (unsigned)(N * C)), dim3(256), 0, s, x_dev, gamma_dev, beta_dev, (const double *)ws, sl,
                           (double)cnt, eps, momentum, save_mean_dev, save_invstd_dev, running_mean_dev, running_var_dev, res_dev, act, C, HW, y_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_bn_train_backward(pn_ctx *ctx, const float *x_dev, const float *dy_dev, const float *out_dev, const float *gamma_dev, const float *beta_dev,
                         const float *save_mean_dev, const float *save_invstd_dev, int act, int N, int C, int HW, float *dx_dev, float *dgamma_dev, float *dbeta_dev,
                         float *dres_dev, int dres_accumulate, void *hip_stream) {
    PN_CTX_CHECK
    if (!x_dev || !dy_dev || !gamma_dev || !save_mean_dev || !save_invstd_dev || !dx_dev || !dgamma_dev || !dbeta_dev || (act != PN_ACT_NONE && !out_dev && !beta_dev))
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_bn_train_backward: bad arguments (an activation needs out, or beta to recompute its mask)");
    if (N < 1 || C < 1 || HW < 1 || (long)N * C > 65535)        // (grid.y of the apply kernel) refused before anything is launched
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_bn_train_backward: N * C out of range");
    const long cnt = (long)N * HW;
    const int sl = t_slices(cnt, C);
    void *ws = nullptr;
    int rc = t_ws(ctx, (size_t)C * sl * 2 * sizeof(double), &ws);
    if (rc != PN_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    t_chan_reduce<1>(s, x_dev, dy_dev, out_dev, save_mean_dev, save_invstd_dev, gamma_dev, beta_dev, act, N, C, HW, sl, (double *)ws);
    // d beta = sum g, d gamma = sum g (x - mean) * invstd: finished inside the apply kernel
    const bool v4 = (HW & 3) == 0 && ((((size_t)x_dev) | ((size_t)dy_dev) | ((size_t)out_dev) | ((size_t)dx_dev) | ((size_t)dres_dev)) & 15) == 0;
    if (v4)
        hipLaunchKernelGGL(bn_bwd_apply_kernel<4>, dim3((unsigned)((HW / 4 + 255) / 256), (unsigned)(N * C)), dim3(256), 0, s, x_dev, dy_dev, out_dev, gamma_dev, beta_dev,
                           save_mean_dev, save_invstd_dev, (const double *)ws, sl, dbeta_dev, dgamma_dev, act, C, HW, (float)(1.0 / (double)cnt), dx_dev, dres_dev, dres_accumulate);
    else
        hipLaunchKernelGGL(bn_bwd_apply_kernel<1>, dim3((unsigned)((HW + 255) / 256), (unsigned)(N * C)), dim3(256), 0, s, x_dev, dy_dev, out_dev, gamma_dev, beta_dev,
                           save_mean_dev, save_invstd_dev, (const double *)ws, sl, dbeta_dev, dgamma_dev, act, C, HW, (float)(1.0 / (double)cnt), dx_dev, dres_dev, dres_accumulate);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_avgpool3s2_forward(pn_ctx *ctx, const float *x_dev, float *y_dev, int planes, int H, int W, void *hip_stream) {
    PN_CTX_CHECK
    if (!x_dev || !y_dev || planes < 1 || H < 1 || W < 1) return pn_set_error(ctx, PN_ERR_INVALID, "pn_avgpool3s2_forward: bad arguments");
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    const size_t total = (size_t)planes * Ho * Wo;
    hipLaunchKernelGGL(avgpool_fwd_kernel, dim3((unsigned)((Ho * Wo + 255) / 256), (unsigned)std::min(planes, 65535)), dim3(256), 0, (hipStream_t)hip_stream, x_dev, H, W, Ho, Wo, total, y_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_avgpool3s2_backward(pn_ctx *ctx, const float *dy_dev, float *dx_dev, int planes, int H, int W, void *hip_stream) {
    PN_CTX_CHECK
    if (!dy_dev || !dx_dev || planes < 1 || H < 1 || W < 1) return pn_set_error(ctx, PN_ERR_INVALID, "pn_avgpool3s2_backward: bad arguments");
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    const size_t total = (size_t)planes * H * W;
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3((unsigned)((H * W + 255) / 256), (unsigned)std::min(planes, 65535)), dim3(256), 0, (hipStream_t)hip_stream, dy_dev, H, W, Ho, Wo, total, dx_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_head_forward(pn_ctx *ctx, const float *v_dev, const float *target_dev, const float *fg_dev, int kind, int N, int C, int HW, float *s_dev,
                    float *out_dev, int out_ld, float *loss_dev, void *hip_stream) {
    PN_CTX_CHECK
    if (!v_dev || !target_dev || !s_dev || !out_dev || !loss_dev || out_ld < C || N < 1) return pn_set_error(ctx, PN_ERR_INVALID, "pn_head_forward: bad arguments");
    const size_t total = (size_t)N * C * HW;
    const unsigned nb = (unsigned)((total + 255) / 256);
    void *ws = nullptr;
    int rc = t_ws(ctx, (size_t)nb * sizeof(double), &ws);
    if (rc != PN_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(head_fwd_kernel, dim3(nb), dim3(256), 0, s, v_dev, target_dev, fg_dev, kind, C, HW, total, s_dev, out_dev, out_ld, (double *)ws);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, s, (const double *)ws, (int)nb, (double)total, loss_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_head_backward(pn_ctx *ctx, const float *s_dev, const float *target_dev, const float *fg_dev, const float *dextra_dev, int dextra_ld, int kind,
                     int N, int C, int HW, float *dv_dev, void *hip_stream) {
    PN_CTX_CHECK
    if (!s_dev || !target_dev || !dv_dev || (dextra_dev && dextra_ld < C)) return pn_set_error(ctx, PN_ERR_INVALID, "pn_head_backward: bad arguments");
    const size_t total = (size_t)N * C * HW;
    hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, s_dev, target_dev, fg_dev, dextra_dev,
                       dextra_ld, kind, C, HW, total, (float)(1.0 / (double)total), dv_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_slice_copy(pn_ctx *ctx, const float *src_dev, int src_ld, float *dst_dev, int dst_ld, int N, int C, int HW, int accumulate, void *hip_stream) {
    PN_CTX_CHECK
    if (!src_dev || !dst_dev || src_ld < C || dst_ld < C) return pn_set_error(ctx, PN_ERR_INVALID, "pn_slice_copy: bad arguments");
    const size_t total = (size_t)N * C * HW;
    hipLaunchKernelGGL(slice_copy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, src_dev, src_ld, dst_dev, dst_ld, C, HW,
                       total, accumulate);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_sgd_nesterov(pn_ctx *ctx, float *param_dev, const float *grad_dev, float *momentum_buf_dev, size_t n, float lr, float momentum, float weight_decay,
                    int first_step, float grad_scale, void *hip_stream) {
    PN_CTX_CHECK
    if (!param_dev || !grad_dev || !momentum_buf_dev) return pn_set_error(ctx, PN_ERR_INVALID, "pn_sgd_nesterov: bad arguments");
    if (n == 0) return PN_OK;
    for (auto &e : ctx->train_packs) e.fresh = false;         // the weights move: cached packs are stale until the next pn_train_pack_refresh (or per-call pack)
    hipLaunchKernelGGL(sgd_nesterov_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, param_dev, grad_dev, momentum_buf_dev, n,
                       lr, momentum, weight_decay, first_step, grad_scale);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_train_conv_plan_info(pn_ctx *ctx, int which, int N, int Cin, int H, int W, int Cout, int ks, int stride, int pad, char *out, size_t cap) {
    if (!ctx) return PN_ERR_INVALID;
    if (!out || N < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1 || stride < 1 || pad < 0 || (ks != 1 && ks != 3 && ks != 7) || which < PN_PLAN_FORWARD || which > PN_PLAN_WGRAD)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_train_conv_plan_info: bad arguments");
    if (which == PN_PLAN_DGRAD) stride = 1;
    TConv c;
    if (int rc = t_conv_desc(ctx, &c, "pn_train_conv_plan_info", N, Cin, H, W, Cout, ks, stride, pad, 0)) return rc;
    const int Ho = c.Ho, Wo = c.Wo;
    static const char *names[] = {"forward", "dgrad", "dgrad_strided", "wgrad"};
    char buf[1024];
    int n = snprintf(buf, sizeof buf, "{\"which\":\"%s\",\"x3\":%d,\"Ho\":%d,\"Wo\":%d", names[which], ctx->train_x3 ? 1 : 0, Ho, Wo);
    auto tile = [&](const char *label, const char *pack, int TW, int R, int tx, int ty, unsigned g0, unsigned g1, unsigned g2) {
        n += snprintf(buf + n, sizeof buf - n, ",\"kernel\":\"%s\",\"pack\":\"%s\",\"TW\":%d,\"R\":%d,\"tiles_x\":%d,\"tiles_y\":%d,\"grid\":[%u,%u,%u]", label, pack, TW, R, tx, ty, g0,
                      g1, g2);
    };
    if (which == PN_PLAN_FORWARD || which == PN_PLAN_DGRAD) {
        const bool dg = which == PN_PLAN_DGRAD;
        if (dg && pad > ks - 1) return pn_set_error(ctx, PN_ERR_INVALID, "pn_train_conv_plan_info: pad out of range for a data gradient");
        // the data gradient is a forward convolution of dy (Cout channels, Ho x Wo) to the H x W input map
        TTilePlan p = dg ? t_plan_dgrad(ctx, N, Cin, H, W, Cout, ks) : t_plan_forward(ctx, N, Cin, Cout, Ho, Wo, ks, stride, pad);
        const int M = dg ? Cin : Cout, oh = dg ? H : Ho, ow = dg ? W : Wo;
        // pn_conv2d_dgrad's fall-back: wflip_kernel, then pn_conv2d_forward(N, Cout, Ho, Wo -> Cin, stride 1, pad ks - 1 - pad)
        if (dg && p.kernel == TK_GENERIC) p = t_plan_forward(ctx, N, Cout, Cin, H, W, ks, 1, ks - 1 - pad);
        if (p.kernel == TK_GENERIC)
            tile(t_fwd_label(p.kernel, ks), dg ? "wflip_kernel" : "", 0, 0, 0, 0, (unsigned)(((long)N * oh * ow + 127) / 128), (unsigned)((M + 63) / 64), 1u);
        else
            tile(t_fwd_label(p.kernel, ks), p.kernel == TK_TILE ? "wpack3_kernel" : "wpack3_x3_kernel", p.g.TW, p.g.R, p.g.tiles_x, p.g.tiles_y,
                 (unsigned)(N * p.g.tiles_x * p.g.tiles_y), (unsigned)((M + 63) / 64), 1u);
    } else if (which == PN_PLAN_DGRAD_STRIDED) {
        unsigned g0 = 0, g1 = 0;
        const char *label = pn_dgrad_strided_plan(N, Cin, H, W, ks, &g0, &g1);
        if (!label || pad > ks - 1) return pn_set_error(ctx, PN_ERR_INVALID, "pn_train_conv_plan_info: pn_conv2d_dgrad_strided takes kernel 1 or 3, pad < kernel");
        tile(label, "", 0, 0, 0, 0, g0, g1, 1u);
    } else {
        const TWgradPlan p = t_plan_wgrad(ctx, c, ks);
        const char *label = t_wgrad_label(p.kernel, ks);
        const unsigned g0 = (unsigned)p.col_blocks, g1 = (unsigned)((Cout + 63) / 64), g2 = (unsigned)p.slices;
        if (p.kernel == TKW_GENERIC) tile(label, "", 0, 0, 0, 0, g0, g1, g2);
        else if (p.kernel == TKW_TILE) tile(label, "", p.g.TW, p.g.R, p.g.tiles_x, p.g.tiles_y, g0, g1, g2);
        else tile(label, "", p.gw.TW, p.gw.R, p.gw.tiles_x, p.gw.tiles_y, g0, g1, g2);
        n += snprintf(buf + n, sizeof buf - n, ",\"slices\":%d,\"per_slice\":%ld,\"per_slice_unit\":\"%s\",\"t_slices\":%d", (int)p.slices, p.per_slice,
                      p.kernel == TKW_GENERIC ? "pixels" : "tiles", p.csl);
    }
    n += snprintf(buf + n, sizeof buf - n, "}");
    if ((size_t)n + 1 > cap) return pn_set_error(ctx, PN_ERR_INVALID, "pn_train_conv_plan_info: %d bytes needed", n + 1);
    memcpy(out, buf, (size_t)n + 1);
    return PN_OK;
}

// slices of the per-channel reductions (BatchNorm statistics and gradients, bias gradient) over N * HW elements of C channels
int pn_train_reduce_slices(pn_ctx *ctx, int N, int C, int HW) {
    if (!ctx || N < 1 || C < 1 || HW < 1) return PN_ERR_INVALID;
    return t_slices((long)N * HW, C);
}

}  // extern "C"
