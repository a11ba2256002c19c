// Device kernels of the NHWC training engine (trainx.hip): everything between the convolutions of one training step of
// rtpose_light3d on tensors stored as two bf16 planes [hi | lo] (value = hi + lo, 16 significant bits), channel-minor.
//
// Reference arithmetic being replaced (tpm/ = third_party_methods/):
//   nn.BatchNorm2d in train mode + (residual) + ReLU / LeakyReLU(0.1)     tpm/lib/network/rtpose_light3d.py:48-72,222-246
//   nn.AvgPool2d(3, 2, 1) and its gradient                                 tpm/lib/network/rtpose_light3d.py:152,158
//   sigmoid range casts + rtpose_light3d_loss_fgweight and its gradient    tpm/lib/network/rtpose_light3d.py:335-337 ; tpm/lib/network/losses.py:65-106
// Layout: a tensor is [B][H][W][2 * plane] bf16, plane a multiple of 64 (pad channels hold zeros and are never written);
// every kernel moves 16-byte vectors of 8 channels.  No atomics: channel reductions write per-block partials that a finish
// kernel adds in a fixed order (deterministic, like train.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pn_internal.h"

namespace tx {

typedef __bf16 bf;
typedef __attribute__((ext_vector_type(8))) __bf16 bf8;
typedef __attribute__((ext_vector_type(4))) float f4;

__device__ __forceinline__ void ld8(const bf *p, float (&v)[8]) {
    const bf8 a = *reinterpret_cast<const bf8 *>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)a[i];
}
// value = hi plane + lo plane
__device__ __forceinline__ void ld8x(const bf *p, int split, float (&v)[8]) {
    const bf8 a = *reinterpret_cast<const bf8 *>(p), b = *reinterpret_cast<const bf8 *>(p + split);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)a[i] + (float)b[i];
}
__device__ __forceinline__ void st8x(bf *p, int split, const float (&v)[8]) {
    bf8 h, l;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bf hi = (bf)v[i];
        h[i] = hi;
        l[i] = (bf)(v[i] - (float)hi);
    }
    *reinterpret_cast<bf8 *>(p) = h;
    *reinterpret_cast<bf8 *>(p + split) = l;
}

// Two storage forms share every kernel below (template parameter T):
//   T = bf     planes [hi | lo]: value = hi + lo, `split` channels apart, channel stride 2 * plane      (precision "bf16x3")
//   T = float  one fp32 plane, `split` unused, channel stride = plane                                    (precision "fp32", round 6)
template <typename T> struct Lay;
template <> struct Lay<bf> {
    static __device__ __forceinline__ void ld(const bf *p, int split, float (&v)[8]) { ld8x(p, split, v); }
    static __device__ __forceinline__ void ldhi(const bf *p, float (&v)[8]) { ld8(p, v); }          // sign / magnitude class only
    static __device__ __forceinline__ void st(bf *p, int split, const float (&v)[8]) { st8x(p, split, v); }
    static __device__ __forceinline__ float ld1(const bf *p, int split) { return (float)p[0] + (float)p[split]; }
    static __device__ __forceinline__ void st1(bf *p, int split, float v) { const bf h = (bf)v; p[0] = h; p[split] = (bf)(v - (float)h); }
};
template <> struct Lay<float> {
    static __device__ __forceinline__ void ld(const float *p, int, float (&v)[8]) {
        *reinterpret_cast<f4 *>(v) = *reinterpret_cast<const f4 *>(p);
        *reinterpret_cast<f4 *>(v + 4) = *reinterpret_cast<const f4 *>(p + 4);
    }
    static __device__ __forceinline__ void ldhi(const float *p, float (&v)[8]) { ld(p, 0, v); }
    static __device__ __forceinline__ void st(float *p, int, const float (&v)[8]) {
        *reinterpret_cast<f4 *>(p) = *reinterpret_cast<const f4 *>(v);
        *reinterpret_cast<f4 *>(p + 4) = *reinterpret_cast<const f4 *>(v + 4);
    }
    static __device__ __forceinline__ float ld1(const float *p, int) { return p[0]; }
    static __device__ __forceinline__ void st1(float *p, int, float v) { p[0] = v; }
};

// ---- per-channel reductions over the pixels of a planes tensor --------------------------------------------------------------
// MODE 0: s0 = sum x, s1 = sum x^2                       (BatchNorm batch statistics)
// MODE 1: s0 = sum g, s1 = sum g * xhat                  (BatchNorm backward: g = dy * act'(y), xhat = (x - mean) * invstd)
// MODE 2: s0 = sum x                                     (bias gradient)
// Block = 256 threads = (C / 8 channel groups) x (256 / (C / 8) pixel lanes); block b owns pixels [b * ppb, (b + 1) * ppb).
// partial[(c * nblk + block) * 2 + {0, 1}] (double).
// Independent tensors of a level (the three branches of a stage) share a launch: blockIdx.y = problem.
template <typename A> struct Multi { A a[3]; };

struct RedArgs {
    const void *x; int x_cs, x_split;        // MODE 0 / 2: the tensor; MODE 1: the convolution output (pre-BN)
    const void *dy; int dy_cs, dy_split;     // MODE 1: gradient w.r.t. the activation output
    const void *y; int y_cs;                   // MODE 1: activation output, hi plane (sign only); nullptr = recompute the sign from x (scale / shift)
    const float *mean, *invstd;              // MODE 1
    const float *scale, *shift;              // MODE 1, y == nullptr: the forward's affine (y = x * scale + shift, no residual)
    int act;                                 // MODE 1: 0 none, 1 ReLU, 2 LeakyReLU(0.1)
    int C; long npix; int ppb, nblk;
    double *partial;
};

template <int MODE, typename T>
__global__ __launch_bounds__(256) void reduce_kernel(Multi<RedArgs> mm) {
    __shared__ float sh[2][256][9];
    const RedArgs &a = mm.a[blockIdx.y];
    if ((int)blockIdx.x >= a.nblk) return;
    const int G = a.C >> 3, PL = 256 / G;
    const int cg = threadIdx.x % G, pl = threadIdx.x / G;
    const long p0 = (long)blockIdx.x * a.ppb, p1 = min(p0 + a.ppb, a.npix);
    float s0[8], s1[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s0[i] = s1[i] = 0.f;
    float mu[8], is[8], sc[8], sf[8];
    if (MODE == 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) { mu[i] = a.mean[cg * 8 + i]; is[i] = a.invstd[cg * 8 + i]; }
        if (a.act && !a.y) {
#pragma unroll
            for (int i = 0; i < 8; ++i) { sc[i] = a.scale[cg * 8 + i]; sf[i] = a.shift[cg * 8 + i]; }
        }
    }
    if (pl < PL)
        for (long p = p0 + pl; p < p1; p += PL) {
            float x[8];
            Lay<T>::ld((const T *)a.x + p * a.x_cs + cg * 8, a.x_split, x);
            if (MODE == 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) { s0[i] += x[i]; s1[i] += x[i] * x[i]; }
            } else if (MODE == 2) {
#pragma unroll
                for (int i = 0; i < 8; ++i) s0[i] += x[i];
            } else {
                float g[8];
                Lay<T>::ld((const T *)a.dy + p * a.dy_cs + cg * 8, a.dy_split, g);
                if (a.act) {
                    float y[8];
                    if (a.y) Lay<T>::ldhi((const T *)a.y + p * a.y_cs + cg * 8, y);
                    else {                                   // no residual: the forward's own expression on the same operands gives the same sign
#pragma unroll
                        for (int i = 0; i < 8; ++i) y[i] = x[i] * sc[i] + sf[i];
                    }
                    const float neg = a.act == 2 ? 0.1f : 0.f;
#pragma unroll
                    for (int i = 0; i < 8; ++i) g[i] = y[i] > 0.f ? g[i] : g[i] * neg;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) { s0[i] += g[i]; s1[i] += g[i] * ((x[i] - mu[i]) * is[i]); }
            }
        }
#pragma unroll
    for (int i = 0; i < 8; ++i) { sh[0][threadIdx.x][i] = s0[i]; sh[1][threadIdx.x][i] = s1[i]; }
    __syncthreads();
    // thread (which, channel) adds the PL pixel lanes of its channel in order
    for (int o = threadIdx.x; o < 2 * a.C; o += 256) {
        const int which = o / a.C, c = o % a.C;
        double s = 0.0;
        for (int l = 0; l < PL; ++l) s += (double)sh[which][l * G + (c >> 3)][c & 7];
        a.partial[((size_t)c * a.nblk + blockIdx.x) * 2 + which] = s;       // [channel][block][2]: a finish wave reads its channel's partials as consecutive KBs
    }
}

// BatchNorm forward finish: partial sums -> mean / invstd / running statistics, and the per-channel affine of the apply pass.
struct BnFinArgs {
    const double *partial; int nblk, C; double n;       // n = pixels per channel
    const float *gamma, *beta;
    float *mean, *invstd, *scale, *shift;               // scale = gamma * invstd, shift = beta - mean * scale
    float *running_mean, *running_var;                  // updated in place (momentum, unbiased variance) when given
    float momentum, eps;
};
// one WAVE per channel: lanes stride over the partial blocks (independent loads in flight), then a fixed-order butterfly -- deterministic
__device__ __forceinline__ void wave_sum2(const double *__restrict__ partial, int nblk, int C, int c, double &s0, double &s1) {
    const int lane = threadIdx.x & 63;
    s0 = 0.0; s1 = 0.0;
    (void)C;
    const double *pc = partial + (size_t)c * nblk * 2;             // (round 6, late: was [block][channel][2] -- every lane of every load in a line of its own)
    for (int b = lane; b < nblk; b += 64) { const double2 v = *reinterpret_cast<const double2 *>(pc + 2 * b); s0 += v.x; s1 += v.y; }
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off, 64); s1 += __shfl_down(s1, off, 64); }
}
__global__ __launch_bounds__(256) void bn_finish_kernel(Multi<BnFinArgs> mm) {
    const BnFinArgs &a = mm.a[blockIdx.y];
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= a.C) return;
    double s, ss;
    wave_sum2(a.partial, a.nblk, a.C, c, s, ss);
    if (threadIdx.x & 63) return;
    const double m = s / a.n;
    double var = ss / a.n - m * m;
    if (var < 0.0) var = 0.0;
    const double is = 1.0 / sqrt(var + (double)a.eps);
    a.mean[c] = (float)m;
    a.invstd[c] = (float)is;
    const double sc = (double)a.gamma[c] * is;
    a.scale[c] = (float)sc;
    a.shift[c] = (float)((double)a.beta[c] - m * sc);
    if (a.running_mean) {
        const double unb = a.n > 1.0 ? var * a.n / (a.n - 1.0) : var;
        a.running_mean[c] = (float)((1.0 - a.momentum) * (double)a.running_mean[c] + (double)a.momentum * m);
        a.running_var[c] = (float)((1.0 - a.momentum) * (double)a.running_var[c] + (double)a.momentum * unb);
    }
}

// BatchNorm backward finish: dgamma = sum g xhat, dbeta = sum g (into the flat gradient), and the three per-channel constants
// of dx = k1 (g - k2 - xhat k3)
struct BnBwdFinArgs {
    const double *partial; int nblk, C; double n;
    const float *gamma, *invstd;
    float *dgamma, *dbeta, *k1, *k2, *k3;
};
__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(Multi<BnBwdFinArgs> mm) {
    const BnBwdFinArgs &a = mm.a[blockIdx.y];
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= a.C) return;
    double s, sx;
    wave_sum2(a.partial, a.nblk, a.C, c, s, sx);
    if (threadIdx.x & 63) return;
    a.dbeta[c] = (float)s;
    a.dgamma[c] = (float)sx;
    a.k1[c] = a.gamma[c] * a.invstd[c];
    a.k2[c] = (float)(s / a.n);
    a.k3[c] = (float)(sx / a.n);
}

// channel sums -> out[c] (bias gradients), c < Cvalid
__global__ __launch_bounds__(256) void sum_finish_kernel(const double *__restrict__ partial, int nblk, int C, int Cvalid, float *__restrict__ out) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= Cvalid) return;
    double s, unused;
    wave_sum2(partial, nblk, C, c, s, unused);
    if ((threadIdx.x & 63) == 0) out[c] = (float)s;
}

// ---- BatchNorm apply: y = act(x * scale + shift [+ res]) ------------------------------------------------------------------
struct BnApplyArgs {
    const void *x; int x_cs, x_split;
    const void *res; int res_cs, res_split;  // residual or nullptr
    void *y; int y_cs, y_split;
    const float *scale, *shift;
    int act, C; long npix;
};
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(Multi<BnApplyArgs> mm) {
    const BnApplyArgs &a = mm.a[blockIdx.y];
    const int G = a.C >> 3;
    const long total = a.npix * G;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long p = i / G;
        const int cg = (int)(i - p * G);
        float x[8], sc[8], sf[8];
        Lay<T>::ld((const T *)a.x + p * a.x_cs + cg * 8, a.x_split, x);
        *reinterpret_cast<f4 *>(sc) = *reinterpret_cast<const f4 *>(a.scale + cg * 8);
        *reinterpret_cast<f4 *>(sc + 4) = *reinterpret_cast<const f4 *>(a.scale + cg * 8 + 4);
        *reinterpret_cast<f4 *>(sf) = *reinterpret_cast<const f4 *>(a.shift + cg * 8);
        *reinterpret_cast<f4 *>(sf + 4) = *reinterpret_cast<const f4 *>(a.shift + cg * 8 + 4);
        float y[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) y[k] = x[k] * sc[k] + sf[k];
        if (a.res) {
            float r[8];
            Lay<T>::ld((const T *)a.res + p * a.res_cs + cg * 8, a.res_split, r);
#pragma unroll
            for (int k = 0; k < 8; ++k) y[k] += r[k];
        }
        if (a.act == 1) {
#pragma unroll
            for (int k = 0; k < 8; ++k) y[k] = y[k] > 0.f ? y[k] : 0.f;
        } else if (a.act == 2) {
#pragma unroll
            for (int k = 0; k < 8; ++k) y[k] = y[k] > 0.f ? y[k] : y[k] * 0.1f;
        }
        Lay<T>::st((T *)a.y + p * a.y_cs + cg * 8, a.y_split, y);
    }
}

// ---- BatchNorm backward apply: g = dy act'(y); dx = k1 (g - k2 - xhat k3); dres = g ------------------------------------------
struct BnBwdApplyArgs {
    const void *x; int x_cs, x_split;
    const void *dy; int dy_cs, dy_split;
    const void *y; int y_cs;                 // nullptr = recompute the sign from x (scale / shift), as in reduce_kernel<1>
    const float *mean, *invstd, *k1, *k2, *k3, *scale, *shift;
    void *dx; int dx_cs, dx_split;
    void *dres; int dres_cs, dres_split;       // gradient of the residual input (= g) or nullptr
    int act, C; long npix;
};
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(Multi<BnBwdApplyArgs> mm) {
    const BnBwdApplyArgs &a = mm.a[blockIdx.y];
    const int G = a.C >> 3;
    const long total = a.npix * G;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long p = i / G;
        const int cg = (int)(i - p * G);
        float x[8], g[8];
        Lay<T>::ld((const T *)a.x + p * a.x_cs + cg * 8, a.x_split, x);
        Lay<T>::ld((const T *)a.dy + p * a.dy_cs + cg * 8, a.dy_split, g);
        if (a.act) {
            float y[8];
            if (a.y) Lay<T>::ldhi((const T *)a.y + p * a.y_cs + cg * 8, y);
            else {
#pragma unroll
                for (int k = 0; k < 8; ++k) y[k] = x[k] * a.scale[cg * 8 + k] + a.shift[cg * 8 + k];
            }
            const float neg = a.act == 2 ? 0.1f : 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) g[k] = y[k] > 0.f ? g[k] : g[k] * neg;
        }
        float d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = cg * 8 + k;
            const float xh = (x[k] - a.mean[c]) * a.invstd[c];
            d[k] = a.k1[c] * (g[k] - a.k2[c] - xh * a.k3[c]);
        }
        Lay<T>::st((T *)a.dx + p * a.dx_cs + cg * 8, a.dx_split, d);
        if (a.dres) Lay<T>::st((T *)a.dres + p * a.dres_cs + cg * 8, a.dres_split, g);
    }
}

// ---- AvgPool2d(3, 2, 1) backward (count_include_pad): dx[iy, ix] = sum of dy over the windows that hold it / 9 -----------------
template <typename T>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const T *__restrict__ dy, int dy_cs, int dy_split, T *__restrict__ dx, int dx_cs, int dx_split,
                                                          int B, int H, int W, int Ho, int Wo, int C) {
    const int G = C >> 3;
    const long total = (long)B * H * W * G;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int cg = (int)(i % G);
        long p = i / G;
        const int ix = (int)(p % W);
        p /= W;
        const int iy = (int)(p % H), b = (int)(p / H);
        float s[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = 0.f;
        for (int oy = iy >> 1; oy <= ((iy + 1) >> 1); ++oy)
            for (int ox = ix >> 1; ox <= ((ix + 1) >> 1); ++ox)
                if (oy < Ho && ox < Wo) {
                    float v[8];
                    Lay<T>::ld(dy + ((long)(b * Ho + oy) * Wo + ox) * dy_cs + cg * 8, dy_split, v);
#pragma unroll
                    for (int k = 0; k < 8; ++k) s[k] += v[k];
                }
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = s[k] / 9.f;
        Lay<T>::st(dx + ((long)(b * H + iy) * W + ix) * dx_cs + cg * 8, dx_split, s);
    }
}

// ---- sum of up to four planes tensors (gradients meeting at a fan-out) ----------------------------------------------------------
struct AddArgs {
    const void *in[4]; int cs[4], split[4]; int n;
    void *out; int out_cs, out_split;
    int C; long npix;
};
template <typename T>
__global__ __launch_bounds__(256) void add_kernel(AddArgs a) {
    const int G = a.C >> 3;
    const long total = a.npix * G;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long p = i / G;
        const int cg = (int)(i - p * G);
        float s[8];
        Lay<T>::ld((const T *)a.in[0] + p * a.cs[0] + cg * 8, a.split[0], s);
        for (int k = 1; k < a.n; ++k) {
            float v[8];
            Lay<T>::ld((const T *)a.in[k] + p * a.cs[k] + cg * 8, a.split[k], v);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += v[j];
        }
        Lay<T>::st((T *)a.out + p * a.out_cs + cg * 8, a.out_split, s);
    }
}

// ---- heads: loss and its gradient from the activated output ------------------------------------------------------------------------
// out [B][C][HW] f32 = s (kind 0) or (s - 0.5) * 4 (kind 1), s = sigmoid(v), as the convolution epilogue wrote it (PN_ACT_SIG / PN_ACT_SIG_PM2).
//   loss partial = sum w (out - t)^2,  w = 0.1 + 0.9 fg (fg != nullptr) else 1                     losses.py:65-90
//   dv = (2 w (out - t) / numel + dextra) * (kind ? 4 : 1) * s (1 - s)                          -> planes [B][HW][2 * dv_plane], channels >= C stay zero
// dextra: channel slice of a planes tensor (the gradient that reaches a stage-1 head through the stage-2 input) or nullptr.
struct HeadArgs {
    const float *out, *target, *fg;
    const void *dextra; int de_cs, de_split;
    void *dv; int dv_cs, dv_split;
    int kind, C, HW; long total; float inv_numel;
    double *partial;
};
template <typename T>
__global__ __launch_bounds__(256) void head_kernel(Multi<HeadArgs> mm) {        // blockIdx.y = head (paf, heat, z)
    __shared__ double sh[4];
    const HeadArgs &a = mm.a[blockIdx.y];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if ((long)blockIdx.x * 256 >= a.total) return;
    double e = 0.0;
    if (i < a.total) {
        const float o = a.out[i];
        const float s = a.kind ? o * 0.25f + 0.5f : o;
        const long n = i / ((long)a.C * a.HW), rem = i - n * (long)a.C * a.HW;
        const int c = (int)(rem / a.HW), p = (int)(rem - (long)c * a.HW);
        const float d = o - a.target[i];
        const float w = a.fg ? 0.1f + a.fg[i] * 0.9f : 1.f;
        e = (double)(d * d * w);
        float g = 2.f * d * w * a.inv_numel;
        const long pix = n * a.HW + p;
        if (a.dextra) g += Lay<T>::ld1((const T *)a.dextra + pix * a.de_cs + c, a.de_split);
        if (a.kind) g *= 4.f;
        const float dv = g * (1.f - s) * s;
        Lay<T>::st1((T *)a.dv + pix * a.dv_cs + c, a.dv_split, dv);
    }
    // block sum (double): wave shuffles, then four partials through LDS
    for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) a.partial[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
struct LossFinArgs { const double *partial; int nblocks; double numel; float *loss; };
__global__ __launch_bounds__(256) void loss_finish_kernel(Multi<LossFinArgs> mm) {
    __shared__ double sh[4];
    const double *partial = mm.a[blockIdx.x].partial;
    const int nblocks = mm.a[blockIdx.x].nblocks;
    const double numel = mm.a[blockIdx.x].numel;
    float *loss = mm.a[blockIdx.x].loss;
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) s += partial[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *loss = (float)((sh[0] + sh[1] + sh[2] + sh[3]) / numel);
}

// ---- layout hand-over at the stem (the 7x7 Cin = 1 convolution keeps train.hip's NCHW f32 kernels) and for the legacy weight gradient ----
// NCHW f32 [B][C][HW] -> planes [B][HW][2 * plane]: 64-pixel x 64-channel tiles through LDS (coalesced on both sides)
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_planes_kernel(const float *__restrict__ in, T *__restrict__ out, int C, int HW, int out_cs, int out_split) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z, c0 = blockIdx.y * 64, p0 = blockIdx.x * 64;
    for (int k = threadIdx.x; k < 64 * 64; k += 256) {
        const int c = k >> 6, p = k & 63;
        tile[c][p] = (c0 + c < C && p0 + p < HW) ? in[((size_t)b * C + c0 + c) * HW + p0 + p] : 0.f;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 64 * 8; k += 256) {
        const int p = k >> 3, cg = k & 7;
        if (p0 + p >= HW || c0 + cg * 8 >= C) continue;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = tile[cg * 8 + j][p];
        Lay<T>::st(out + ((size_t)b * HW + p0 + p) * out_cs + c0 + cg * 8, out_split, v);
    }
}
// planes -> NCHW f32 [B][Cout][HW]; channel c of the output is channel map[c] of the planes tensor (map == nullptr: c)
template <typename T>
__global__ __launch_bounds__(256) void planes_to_nchw_kernel(const T *__restrict__ in, int in_cs, int in_split, float *__restrict__ out, int Cout, int HW,
                                                             const int *__restrict__ map) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z, c0 = blockIdx.y * 64, p0 = blockIdx.x * 64;
    if (!map) {
        for (int k = threadIdx.x; k < 64 * 8; k += 256) {
            const int p = k >> 3, cg = k & 7;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;
            if (p0 + p < HW && c0 + cg * 8 < Cout) Lay<T>::ld(in + ((size_t)b * HW + p0 + p) * in_cs + c0 + cg * 8, in_split, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) tile[cg * 8 + j][p] = v[j];
        }
    } else {
        for (int k = threadIdx.x; k < 64 * 64; k += 256) {
            const int p = k >> 6, c = k & 63;
            float v = 0.f;
            if (p0 + p < HW && c0 + c < Cout) {
                v = Lay<T>::ld1(in + ((size_t)b * HW + p0 + p) * in_cs + map[c0 + c], in_split);
            }
            tile[c][p] = v;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 64 * 64; k += 256) {
        const int c = k >> 6, p = k & 63;
        if (c0 + c < Cout && p0 + p < HW) out[((size_t)b * Cout + c0 + c) * HW + p0 + p] = tile[c][p];
    }
}

// ---- weight packs: fp32 parameters -> split-bf16 MFMA fragments, every convolution of the step in ONE launch ----------------------
// A pack is what net.hip::prepare_conv builds on the host for an inference net, rebuilt on the device from the live parameters:
//   rows x k, k = three plane passes [x_hi | x_lo | x_hi] against [W_hi | W_hi | W_lo]; layouts of conv3_kernel / conv_mfma_kernel
//   ([cout tile][k-step][lane][8]) and conv4_kernel ([cout block][k-step + 3 spare][8 tiles][lane][8]).
// transpose = 1 is the data-gradient pack: rows = input channels, k = output channels, taps rotated by 180 degrees.
struct PackDesc {
    const float *w; void *dst;
    int f32;                 // 1: fp32 pack of the generic fp32 kernel ([cout tile][k-step][2 halves][lane][4 floats]), one plane pass, no split
    int Cout, Cin, ks;
    int transpose, conv4, CT;
    int rows_valid;          // rows that exist (cout, or the input plane for a transposed pack)
    int kplane;              // channels of one plane of the k side
    int ksteps;              // 3 * kplane / 64 * ks * ks * 2
    const int *row_map;      // transposed pack: row -> reference input channel (nullptr = identity); -1 = zero row
    const int *k_map;        // forward pack: plane channel -> reference input channel (nullptr = identity); -1 = zero column
    unsigned first_group, ngroups;      // 16-byte groups of this pack in the launch (pack_kernel)
    unsigned first_unit, nunits;        // (row, 8 k-channels) units of this pack in the launch (pack_rows_kernel)
};

__global__ __launch_bounds__(256) void pack_kernel(const PackDesc *__restrict__ tab, int n, unsigned total_groups) {
    const unsigned gid = blockIdx.x * 256u + threadIdx.x;
    if (gid >= total_groups) return;
    int lo = 0, hi = n - 1;                         // the pack that holds this group
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].first_group <= gid) lo = mid; else hi = mid - 1;
    }
    const PackDesc d = tab[lo];
    const unsigned g = gid - d.first_group;
    const int KK = d.ks * d.ks;
    const int lane = (int)(g & 63u);
    int row, kstep;
    if (d.conv4) {
        const unsigned t = (g >> 6) & 7u, rest = g >> 9;
        kstep = (int)(rest % (unsigned)(d.ksteps + 3));
        const int cbk = (int)(rest / (unsigned)(d.ksteps + 3));
        if (kstep >= d.ksteps) return;              // spare k-steps stay zero
        row = cbk * 128 + pn_conv_row_channel((int)t, lane & 15, 4);
    } else {
        const unsigned frag = g >> 6;
        kstep = (int)(frag % (unsigned)d.ksteps);
        row = pn_conv_row_channel((int)(frag / (unsigned)d.ksteps), lane & 15, d.CT);
    }
    const int tap = kstep % KK, hs = kstep / KK;
    const int k0 = hs * 32 + 8 * (lane >> 4);
    bf8 o;
    float of[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int kidx = k0 + j, pl = kidx / d.kplane, i = kidx - pl * d.kplane;
        int co, ci, tw;
        if (!d.transpose) {
            co = row < d.rows_valid ? row : -1;
            ci = d.k_map ? d.k_map[i] : (i < d.Cin ? i : -1);
            tw = tap;
        } else {
            ci = row < d.rows_valid ? (d.row_map ? d.row_map[row] : (row < d.Cin ? row : -1)) : -1;
            co = i < d.Cout ? i : -1;
            tw = KK - 1 - tap;
        }
        float v = 0.f;
        if (co >= 0 && ci >= 0) v = d.w[((size_t)co * d.Cin + ci) * KK + tw];
        const bf h = (bf)v;
        o[j] = pl == 2 ? (bf)(v - (float)h) : h;
        of[j] = v;
    }
    if (d.f32) {
        float *fp = (float *)d.dst + (size_t)(g >> 6) * 512 + lane * 4;
        *reinterpret_cast<f4 *>(fp) = *reinterpret_cast<f4 *>(of);
        *reinterpret_cast<f4 *>(fp + 256) = *reinterpret_cast<f4 *>(of + 4);
    } else *reinterpret_cast<bf8 *>((bf *)d.dst + (size_t)g * 8) = o;
}

// The same packs, one thread per (row, 8 k-channels): the 8 x ks x ks parameters are read ONCE (a forward pack's are 288 contiguous bytes) and leave as
// the 3 x ks x ks groups that hold them -- every tap's k-step of the three plane passes [W_hi | W_hi | W_lo].  pack_kernel above gathers them per group:
// eight 4-byte loads 36 bytes apart for every one of the 27 groups (37 M gathers per step, 104 us beside the stem; this form: see profiles/r06_notes.txt).
// A wave = the 64 lanes of one fragment, so every (plane pass, tap) store of a wave is one contiguous KB.
template <int KK>
__device__ __forceinline__ void pack_rows_body(const PackDesc &d, unsigned u) {
    const int lane = (int)(u & 63u), r = lane & 15, igl = lane >> 4;
    const int hpp = d.kplane >> 5;                  // 32-channel halves per plane
    const unsigned rest = u >> 6;
    const int hh = (int)(rest % (unsigned)hpp), tile = (int)(rest / (unsigned)hpp);
    const int i0 = hh * 32 + igl * 8;
    int row;
    size_t gbase, gstride;
    if (d.conv4) {
        const int cbk = tile >> 3, t = tile & 7;
        row = cbk * 128 + pn_conv_row_channel(t, r, 4);
        gbase = ((size_t)cbk * (d.ksteps + 3) * 8 + t) * 64 + lane;
        gstride = 512;
    } else {
        row = pn_conv_row_channel(tile, r, d.CT);
        gbase = (size_t)tile * d.ksteps * 64 + lane;
        gstride = 64;
    }
    float v[8][KK];                                 // [k channel][tap of the PACK]
    if (!d.transpose) {
        const int co = row < d.rows_valid ? row : -1;
        if (co >= 0 && !d.k_map && i0 + 8 <= d.Cin) {
            const float *src = d.w + ((size_t)co * d.Cin + i0) * KK;
            if ((((size_t)src) & 15) == 0) {                  // (TrainEngine's flat buffers start every tensor on 16 bytes)
                float flat[8 * KK];
#pragma unroll
                for (int k = 0; k < 8 * KK / 4; ++k) *reinterpret_cast<f4 *>(flat + 4 * k) = *reinterpret_cast<const f4 *>(src + 4 * k);
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int t = 0; t < KK; ++t) v[j][t] = flat[j * KK + t];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int t = 0; t < KK; ++t) v[j][t] = src[j * KK + t];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = i0 + j;
                const int ci = d.k_map ? d.k_map[i] : (i < d.Cin ? i : -1);
                const bool ok = co >= 0 && ci >= 0;
                const float *src = d.w + (ok ? ((size_t)co * d.Cin + ci) * KK : 0);
#pragma unroll
                for (int t = 0; t < KK; ++t) { const float x = src[t]; v[j][t] = ok ? x : 0.f; }
            }
        }
    } else {
        const int ci = row < d.rows_valid ? (d.row_map ? d.row_map[row] : (row < d.Cin ? row : -1)) : -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int co = i0 + j < d.Cout ? i0 + j : -1;
            const bool ok = co >= 0 && ci >= 0;
            const float *src = d.w + (ok ? ((size_t)co * d.Cin + ci) * KK : 0);
#pragma unroll
            for (int t = 0; t < KK; ++t) { const float x = src[KK - 1 - t]; v[j][t] = ok ? x : 0.f; }      // taps rotated by 180 degrees
        }
    }
#pragma unroll
    for (int t = 0; t < KK; ++t) {
        const size_t g0 = gbase + (size_t)(hh * KK + t) * gstride;             // plane pass 0; pass pl: + pl * hpp * KK k-steps
        const size_t gpl = (size_t)hpp * KK * gstride;
        if (d.f32) {
            float *fp = (float *)d.dst + (g0 >> 6) * 512 + lane * 4;
            *reinterpret_cast<f4 *>(fp) = f4{v[0][t], v[1][t], v[2][t], v[3][t]};
            *reinterpret_cast<f4 *>(fp + 256) = f4{v[4][t], v[5][t], v[6][t], v[7][t]};
        } else {
            bf8 h, l;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bf hi = (bf)v[j][t];
                h[j] = hi;
                l[j] = (bf)(v[j][t] - (float)hi);
            }
            bf *o = (bf *)d.dst;
            *reinterpret_cast<bf8 *>(o + g0 * 8) = h;
            *reinterpret_cast<bf8 *>(o + (g0 + gpl) * 8) = h;
            *reinterpret_cast<bf8 *>(o + (g0 + 2 * gpl) * 8) = l;
        }
    }
}

__global__ __launch_bounds__(256) void pack_rows_kernel(const PackDesc *__restrict__ tab, int n, unsigned total_units) {
    const unsigned uid = blockIdx.x * 256u + threadIdx.x;
    if (uid >= total_units) return;
    int lo = 0, hi = n - 1;                         // the pack that holds this unit
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].first_unit <= uid) lo = mid; else hi = mid - 1;
    }
    const PackDesc d = tab[lo];
    if (d.ks == 3) pack_rows_body<9>(d, uid - d.first_unit);
    else pack_rows_body<1>(d, uid - d.first_unit);
}

// padded copies of the convolution biases (the epilogues read whole cout tiles)
struct BiasDesc { const float *src; float *dst; int n, npad; };
__global__ void bias_kernel(const BiasDesc *__restrict__ tab, int n) {
    const BiasDesc d = tab[blockIdx.x];
    (void)n;
    for (int i = threadIdx.x; i < d.npad; i += blockDim.x) d.dst[i] = i < d.n ? d.src[i] : 0.f;
}

}  // namespace tx
