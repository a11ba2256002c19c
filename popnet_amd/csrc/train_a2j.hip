// Training kernels of A2J_model (the second stage of the "Yolo-A2J" baseline) that the other two trainers never needed.  fp32 like the
// primitives of train.hip, asynchronous on the caller's stream, fixed summation orders (a repeated call gives the same bits), no float atomics.
//   pn_a2j_loss   A2J_loss.forward (third_party_methods/A2J_experiments/anchor.py:84-154) and its gradient on the three raw head maps
//   pn_adam       torch.optim.Adam with L2 weight decay on a flat buffer (train_a2j_mpaug_new.py:181)
// The dilated 3x3 convolutions of layer4.1 / layer4.2 (pn_conv2d_forward_dil / _dgrad_dil / _wgrad_dil) are instantiations of train.hip's
// gather kernels and live next to the entries they extend.
// Both kernels here are HBM-bound: the loss reads 4 K floats per (crop, joint) two or three times (the second and third pass from L2),
// Adam moves 7 floats per parameter.
#pragma clang fp contract(off)
#include <cmath>
#include "pn_internal.h"

namespace {

struct A2JLossArgs {
    const float *cls, *reg, *dep;      // NCHW maps (h > 0) or the reference's flat layout (h == 0)
    const float *anchors;              // [K, 2]
    const float *labels;               // [B, P, 3]
    const float *scale;                // device: (s_cls, s_reg)
    float *partial;                    // [B * P, 2]: this (crop, joint)'s share of Cls and of Reg before the batch mean
    float *dcls, *dreg, *ddep;         // all three or none
    int B, h, w, A, P, K;
    float spatial_factor;
};

// One item j < K of a (crop b, joint p): where its logit, its two offsets and its depth lie, and which anchor it is.
//   NCHW: j = a * h w + y w + x (lanes along the contiguous x), anchor k = (x h + y) A + a, channel a P + p (reg: (a P + p) 2 + c)
//   flat: j = k, [B, K, P] / [B, K, P, 2]
struct A2JItem { size_t c, r0, r1; int k; };
__device__ __forceinline__ A2JItem a2j_item(const A2JLossArgs &a, int b, int p, int j) {
    A2JItem it;
    if (a.h == 0) {
        it.k = j;
        it.c = ((size_t)b * a.K + j) * a.P + p;
        it.r0 = 2 * it.c;
        it.r1 = it.r0 + 1;
        return it;
    }
    const int hw = a.h * a.w;
    const int an = j / hw, pix = j - an * hw, y = pix / a.w, x = pix - y * a.w;
    it.k = (x * a.h + y) * a.A + an;
    const size_t ch = (size_t)b * a.A * a.P + (size_t)an * a.P + p;
    it.c = ch * hw + pix;
    it.r0 = 2 * ch * hw + pix;
    it.r1 = it.r0 + hw;
    return it;
}

// sum over the 256 threads of a block in a fixed tree (lanes by xor shuffles, then the four waves), the result in every thread
__device__ __forceinline__ float a2j_block_sum(float v, float *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// smooth L1 (beta 1) of u = |d|, and the derivative of that loss with respect to the PREDICTION (d = gt - prediction); 0 at d == 0
__device__ __forceinline__ float a2j_sl1(float u) { return u <= 1.f ? 0.5f * u * u : u - 0.5f; }
__device__ __forceinline__ float a2j_dsl1(float d) { return fabsf(d) <= 1.f ? -d : (d > 0.f ? -1.f : 1.f); }
__device__ __forceinline__ float a2j_dabs(float d) { return d > 0.f ? -1.f : (d < 0.f ? 1.f : 0.f); }

// grid (P, B), 256 threads: one workgroup per (crop, joint).
__global__ __launch_bounds__(256) void a2j_loss_kernel(A2JLossArgs a) {
    __shared__ float red[4];
    const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int K = a.K;
    // pass 1: the maximum logit
    float m = -INFINITY;
    for (int j = tid; j < K; j += 256) m = fmaxf(m, a.cls[a2j_item(a, b, p, j).c]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    // pass 2: sum e, sum e anchor, sum e (anchor + reg), sum e dep
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = tid; j < K; j += 256) {
        const A2JItem it = a2j_item(a, b, p, j);
        const float e = expf(a.cls[it.c] - m);
        const float ay = a.anchors[2 * it.k], ax = a.anchors[2 * it.k + 1];
        s[0] += e;
        s[1] += e * ay;
        s[2] += e * ax;
        s[3] += e * (ay + a.reg[it.r0]);
        s[4] += e * (ax + a.reg[it.r1]);
        s[5] += e * a.dep[it.c];
    }
    float t[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) t[i] = a2j_block_sum(s[i], red);
    const float Ay = t[1] / t[0], Ax = t[2] / t[0], Ry = t[3] / t[0], Rx = t[4] / t[0], D = t[5] / t[0];
    const float *gt = a.labels + ((size_t)b * a.P + p) * 3;
    const float day = gt[0] - Ay, dax = gt[1] - Ax, dry = gt[0] - Ry, drx = gt[1] - Rx, dz = gt[2] - D;
    if (tid == 0) {
        const float inv2p = 1.f / (2.f * (float)a.P);
        float *o = a.partial + ((size_t)b * a.P + p) * 2;
        o[0] = (a2j_sl1(fabsf(day)) + a2j_sl1(fabsf(dax))) * inv2p;
        o[1] = (a2j_sl1(fabsf(dry)) + a2j_sl1(fabsf(drx))) * inv2p * a.spatial_factor + fabsf(dz) / (float)a.P;
    }
    if (!a.dcls) return;
    // pass 3: d (s_cls Cls + s_reg Reg) / d (cls, reg, dep).  With w_k = e_k / sum e and a prediction V = sum w_k v_k:  dV / d cls_k = w_k (v_k - V).
    const float s_cls = a.scale[0], s_reg = a.scale[1];
    const float nb = (float)a.B * (float)a.P;
    const float c_cls = s_cls / (2.f * nb), c_reg = s_reg * a.spatial_factor / (2.f * nb), c_dep = s_reg / nb;
    const float gAy = c_cls * a2j_dsl1(day), gAx = c_cls * a2j_dsl1(dax);
    const float gRy = c_reg * a2j_dsl1(dry), gRx = c_reg * a2j_dsl1(drx), gD = c_dep * a2j_dabs(dz);
    for (int j = tid; j < K; j += 256) {
        const A2JItem it = a2j_item(a, b, p, j);
        const float wk = expf(a.cls[it.c] - m) / t[0];
        const float ay = a.anchors[2 * it.k], ax = a.anchors[2 * it.k + 1];
        const float acc = gAy * (ay - Ay) + gAx * (ax - Ax) + gRy * (ay + a.reg[it.r0] - Ry) + gRx * (ax + a.reg[it.r1] - Rx) + gD * (a.dep[it.c] - D);
        a.dcls[it.c] = wk * acc;
        a.dreg[it.r0] = wk * gRy;
        a.dreg[it.r1] = wk * gRx;
        a.ddep[it.c] = wk * gD;
    }
}

// terms[i] = (sum over the B P partials, in index order per thread and a fixed tree across the block, in double) / B
__global__ __launch_bounds__(256) void a2j_loss_finish_kernel(const float *__restrict__ partial, int n, double inv_b, float *__restrict__ terms) {
    __shared__ double sh[2][4];
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { s0 += (double)partial[2 * i]; s1 += (double)partial[2 * i + 1]; }
    for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s0; sh[1][threadIdx.x >> 6] = s1; }
    __syncthreads();
    if (threadIdx.x < 2) terms[threadIdx.x] = (float)(((sh[threadIdx.x][0] + sh[threadIdx.x][1]) + (sh[threadIdx.x][2] + sh[threadIdx.x][3])) * inv_b);
}

// torch.optim.Adam (amsgrad off, L2 weight decay):  g = gscale g + wd p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;
// p -= step m / (sqrt(v) / bc2s + eps)   with step = lr / (1 - b1^t), bc2s = sqrt(1 - b2^t) from the host.
// The element arithmetic runs in double and p, m, v are rounded to float once each: the launch moves 28 bytes per element and stays HBM-bound
// with ~40 double operations per element, and the result is within half an ulp of the formula evaluated exactly on the stored float state.
struct AdamArgs { double b1, omb1, b2, omb2, step, bc2s, eps, wd, gscale; };
__device__ __forceinline__ void adam_one(float &p, float gf, float &m, float &v, const AdamArgs &a) {
    const double g = (double)gf * a.gscale + a.wd * (double)p;
    const double mn = a.b1 * (double)m + a.omb1 * g;
    const double vn = a.b2 * (double)v + a.omb2 * g * g;
    p = (float)((double)p - a.step * (mn / (sqrt(vn) / a.bc2s + a.eps)));
    m = (float)mn;
    v = (float)vn;
}

// thread i < n4: elements 4 i .. 4 i + 3 as 16-byte accesses (the caller checked the alignment); thread n4 + j: tail element 4 n4 + j
__global__ __launch_bounds__(256) void adam_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, size_t n4, size_t n,
                                                   AdamArgs a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        float4 pv = reinterpret_cast<float4 *>(p)[i], mv = reinterpret_cast<float4 *>(m)[i], vv = reinterpret_cast<float4 *>(v)[i];
        const float4 gv = reinterpret_cast<const float4 *>(g)[i];
        adam_one(pv.x, gv.x, mv.x, vv.x, a);
        adam_one(pv.y, gv.y, mv.y, vv.y, a);
        adam_one(pv.z, gv.z, mv.z, vv.z, a);
        adam_one(pv.w, gv.w, mv.w, vv.w, a);
        reinterpret_cast<float4 *>(p)[i] = pv;
        reinterpret_cast<float4 *>(m)[i] = mv;
        reinterpret_cast<float4 *>(v)[i] = vv;
        return;
    }
    const size_t e = 4 * n4 + (i - n4);
    if (e >= n) return;
    adam_one(p[e], g[e], m[e], v[e], a);
}

}  // namespace

extern "C" {

int pn_a2j_loss(pn_ctx *ctx, const float *cls_dev, const float *reg_dev, const float *dep_dev, int B, int h, int w, int A, int P, const float *anchors_dev,
                const float *labels_dev, float spatial_factor, const float *scale_dev, float *terms_dev, float *dcls_dev, float *dreg_dev, float *ddep_dev,
                void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (!cls_dev || !reg_dev || !dep_dev || !anchors_dev || !labels_dev || !terms_dev || B < 1 || h < 0 || w < 1 || A < 1 || P < 1 || (h == 0 && A != 1))
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_loss: bad arguments (the flat layout is h = 0, w = K, A = 1)");
    const int ng = (dcls_dev != nullptr) + (dreg_dev != nullptr) + (ddep_dev != nullptr);
    if (ng != 0 && ng != 3) return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_loss: all three gradient pointers or none");
    if (ng == 3 && !scale_dev) return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_loss: the gradient needs (s_cls, s_reg)");
    const long K = h ? (long)h * w * A : (long)w;
    if (K * P * 2 >= (1L << 31) || B > 65535 || P > 65535) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "pn_a2j_loss: %ld anchors x %d joints x %d crops", K, P, B);
    void *ws = nullptr;
    if (int rc = pn_train_ws(ctx, (size_t)B * P * 2 * sizeof(float), &ws)) return rc;
    A2JLossArgs a;
    a.cls = cls_dev; a.reg = reg_dev; a.dep = dep_dev; a.anchors = anchors_dev; a.labels = labels_dev; a.scale = scale_dev; a.partial = (float *)ws;
    a.dcls = dcls_dev; a.dreg = dreg_dev; a.ddep = ddep_dev;
    a.B = B; a.h = h; a.w = w; a.A = A; a.P = P; a.K = (int)K; a.spatial_factor = spatial_factor;
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(a2j_loss_kernel, dim3((unsigned)P, (unsigned)B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(a2j_loss_finish_kernel, dim3(1), dim3(256), 0, s, (const float *)ws, B * P, 1.0 / (double)B, terms_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_adam(pn_ctx *ctx, float *param_dev, const float *grad_dev, float *exp_avg_dev, float *exp_avg_sq_dev, size_t n, double lr, double beta1, double beta2,
            double eps, double weight_decay, int t, double grad_scale, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (!param_dev || !grad_dev || !exp_avg_dev || !exp_avg_sq_dev || t < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_adam: bad arguments (t >= 1, betas in [0, 1))");
    if (n == 0) return PN_OK;
    for (auto &e : ctx->train_packs) e.fresh = false;         // the weights move: cached packs are stale, as after pn_sgd_nesterov
    AdamArgs a;
    a.b1 = beta1; a.omb1 = 1.0 - beta1; a.b2 = beta2; a.omb2 = 1.0 - beta2; a.eps = eps; a.wd = weight_decay; a.gscale = grad_scale;
    a.step = lr / (1.0 - std::pow(beta1, (double)t));
    a.bc2s = std::sqrt(1.0 - std::pow(beta2, (double)t));
    const bool aligned = ((((size_t)param_dev) | ((size_t)grad_dev) | ((size_t)exp_avg_dev) | ((size_t)exp_avg_sq_dev)) & 15) == 0;
    const size_t n4 = aligned ? n / 4 : 0, threads = n4 + (n - 4 * n4);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, param_dev, grad_dev, exp_avg_dev, exp_avg_sq_dev, n4,
                       n, a);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

}  // extern "C"
