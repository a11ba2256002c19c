// Training kernels of YoloPoseNet ("Yolo-Pose+") that rtpose_light3d never needed.  fp32 NCHW like the primitives of train.hip,
// asynchronous on the caller's stream, fixed summation orders (a repeated call gives the same bits), no float atomics.
//   pn_conv2d_dgrad_strided   data gradient of a strided convolution (layer2.0.conv1 3x3 / layer2.0.downsample.0 1x1, stride 2;
//                             tpm/lib/network/resnet.py BasicBlock): a gather over the taps that hit each input pixel
//   pn_maxpool_forward / _backward   nn.MaxPool2d(3, 2, 1) after the stem and nn.MaxPool2d(2, 2) in model2_1
//                             (tpm/lib/network/yolo_posenet.py:36,111-114) with PyTorch CPU max_pool2d_with_indices' tie / NaN rules
//   pn_yolo_loss              the per-slice sigmoid casts (yolo_posenet.py:146-156) + yolo_loss_fgweight / _poseweight
//                             (tpm/lib/network/losses.py:397-466) forward and gradient, two-pass deterministic reduction
//   pn_build_prior_targets    build_prior_targets + bbox_ious (tpm/lib/datasets/datasets_kdh3d_mpaug.py:353-417,505-533, CR)
//                             in float64, stored as float32 (the dataset's .astype(np.float32))
// All of these are HBM- or latency-bound and small next to the convolutions of the step.
#pragma clang fp contract(off)
#include <cmath>
#include "pn_internal.h"

// ---- strided data gradient --------------------------------------------------------------------------------------------------------
// dx[n, ci, iy, ix] (+)= sum over co (outer), then the taps (ky, kx) in row-major order whose output pixel
// oy = (iy + pad - ky) / stride, ox = (ix + pad - kx) / stride is integral and inside [0, Ho) x [0, Wo), of dy[n, co, oy, ox] * w[co, ci, ky, kx]
// -- one fmaf chain per input pixel.  grid.y walks the N * Cin planes (so ci and the weight row are uniform across a block).
template <int KS>
__global__ __launch_bounds__(256) void dgrad_strided_kernel(const float *__restrict__ dy, const float *__restrict__ w, float *__restrict__ dx, int N, int Cin,
                                                            int H, int W, int Cout, int Ho, int Wo, int stride, int pad, int accumulate) {
    const int pp = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (pp >= H * W) return;
    const int iy = pp / W, ix = pp - iy * W;
    int toff[KS * KS], doff[KS * KS], nt = 0;           // valid taps: weight offset inside [ci] of one co, dy offset inside one plane
    for (int ky = 0; ky < KS; ++ky) {
        const int ty = iy + pad - ky;
        if (ty < 0 || ty % stride) continue;
        const int oy = ty / stride;
        if (oy >= Ho) continue;
        for (int kx = 0; kx < KS; ++kx) {
            const int tx = ix + pad - kx;
            if (tx < 0 || tx % stride) continue;
            const int ox = tx / stride;
            if (ox >= Wo) continue;
            toff[nt] = ky * KS + kx;
            doff[nt] = oy * Wo + ox;
            ++nt;
        }
    }
    const size_t planes = (size_t)N * Cin;
    const size_t oplane = (size_t)Ho * Wo;
    for (size_t plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const size_t n = plane / Cin;
        const int ci = (int)(plane - n * Cin);
        const float *dyn = dy + n * Cout * oplane;
        const float *wc = w + (size_t)ci * KS * KS;
        float acc = 0.f;
        for (int co = 0; co < Cout; ++co) {
            const float *dp = dyn + (size_t)co * oplane;
            const float *wp = wc + (size_t)co * Cin * KS * KS;
            for (int t = 0; t < nt; ++t) acc = fmaf(dp[doff[t]], wp[toff[t]], acc);
        }
        float *o = dx + plane * H * W + pp;
        *o = accumulate ? *o + acc : acc;
    }
}

// ---- max pooling ------------------------------------------------------------------------------------------------------------------
// PyTorch CPU max_pool2d_with_indices (aten/src/ATen/native/cpu/MaxPoolKernel.cpp, cpu_max_pool): the window is clipped to the
// plane, maxindex starts at its first pixel and maxval at -inf; a pixel replaces the maximum when `val > maxval || isnan(val)`
// (row-major window order): the first maximum wins a tie, the LAST NaN of a window wins.
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float *__restrict__ x, float *__restrict__ y, int *__restrict__ idx, int planes, int H, int W,
                                                          int Ho, int Wo, int k, int stride, int pad) {
    const int pp = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (pp >= Ho * Wo) return;
    const int oy = pp / Wo, ox = pp - oy * Wo;
    const int y0 = max(oy * stride - pad, 0), y1 = min(oy * stride - pad + k, H);
    const int x0 = max(ox * stride - pad, 0), x1 = min(ox * stride - pad + k, W);
    for (size_t plane = blockIdx.y; plane < (size_t)planes; plane += gridDim.y) {
        const float *xp = x + plane * H * W;
        int mi = y0 * W + x0;
        float mv = -INFINITY;
        for (int iy = y0; iy < y1; ++iy)
            for (int ix = x0; ix < x1; ++ix) {
                const float v = xp[iy * W + ix];
                if (v > mv || isnan(v)) {
                    mv = v;
                    mi = iy * W + ix;
                }
            }
        y[plane * Ho * Wo + pp] = mv;
        idx[plane * Ho * Wo + pp] = mi;
    }
}

// dx[p] = sum, in output row-major order, of dy[o] over the outputs o whose argmax is p (PyTorch's CPU scatter visits the outputs
// in that order and adds into a zeroed dx: the same additions in the same order)
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float *__restrict__ dy, const int *__restrict__ idx, float *__restrict__ dx, int planes, int H, int W,
                                                          int Ho, int Wo, int k, int stride, int pad) {
    const int pp = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (pp >= H * W) return;
    const int iy = pp / W, ix = pp - iy * W;
    // outputs whose window [o * stride - pad, o * stride - pad + k) holds the pixel
    const int oy0 = iy + pad - k + 1 > 0 ? (iy + pad - k + 1 + stride - 1) / stride : 0, oy1 = min((iy + pad) / stride, Ho - 1);
    const int ox0 = ix + pad - k + 1 > 0 ? (ix + pad - k + 1 + stride - 1) / stride : 0, ox1 = min((ix + pad) / stride, Wo - 1);
    for (size_t plane = blockIdx.y; plane < (size_t)planes; plane += gridDim.y) {
        const float *dp = dy + plane * Ho * Wo;
        const int *ip = idx + plane * Ho * Wo;
        float s = 0.f;
        for (int oy = oy0; oy <= oy1; ++oy)
            for (int ox = ox0; ox <= ox1; ++ox)
                if (ip[oy * Wo + ox] == pp) s += dp[oy * Wo + ox];
        dx[plane * H * W + pp] = s;
    }
}

// ---- YOLO head casts + loss -------------------------------------------------------------------------------------------------------
// Channel c of v [N, A (5 + 3J), h, w] is feature k = c % (5 + 3J) of anchor a = c / (5 + 3J):
//   k 0, 1: (sigmoid - 0.5) * 2    k 2, 3: sigmoid * 2    k 4: sigmoid    k >= 5: (sigmoid - 0.5) * 4
// loss terms (M = N A h w cells, m = mask_coord for k != 4 and mask_conf for k == 4, W = weight_map):
//   plain      coord = mean_{M x 4}((o - t)^2 m) * 4,   obj = mean_M((o - t)^2 m),   selfpose = mean_{M x 3J}((o - t)^2 m) * 3J
//   weighted   the same with (o m - t m)^2 W in place of (o - t)^2 m
// Element errors and gradients in double; per-block partial sums (three terms) then one finishing block: a fixed order.
struct YoloLossArgs {
    const float *v, *prior, *mconf, *mcoord, *wmap;
    float *out, *dv;
    double *partial;
    int A, F, HW;
    size_t total;
    double sc[3];        // multiplier / element count of the three terms (coord, obj, selfpose)
};

__device__ __forceinline__ double y_block_sum(double v, double *sh) {
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

__global__ __launch_bounds__(256) void yolo_loss_kernel(YoloLossArgs a) {
    __shared__ double sh[4];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double e[3] = {0.0, 0.0, 0.0};
    if (i < a.total) {
        const size_t cell = i / a.HW, p = i - cell * a.HW;               // cell = n * A F + c
        const int c = (int)(cell % (size_t)(a.A * a.F));
        const size_t n = cell / (size_t)(a.A * a.F);
        const int an = c / a.F, k = c - an * a.F;
        const size_t mi = (n * a.A + an) * a.HW + p;
        const float s = 1.f / (1.f + expf(-a.v[i]));
        float o;
        double dfac;
        int term;
        if (k < 2) { o = (s - 0.5f) * 2.f; dfac = 2.0; term = 0; }
        else if (k < 4) { o = s * 2.f; dfac = 2.0; term = 0; }
        else if (k == 4) { o = s; dfac = 1.0; term = 1; }
        else { o = (s - 0.5f) * 4.f; dfac = 4.0; term = 2; }
        a.out[i] = o;
        const double m = (double)(term == 1 ? a.mconf[mi] : a.mcoord[mi]);
        const double t = (double)a.prior[i];
        double dlo;                                                       // d (element error) / d o
        if (a.wmap) {
            const double wt = (double)a.wmap[mi];
            const double d = (double)o * m - t * m;
            e[term] = d * d * wt;
            dlo = 2.0 * d * wt * m;
        } else {
            const double d = (double)o - t;
            e[term] = d * d * m;
            dlo = 2.0 * d * m;
        }
        a.dv[i] = (float)(dlo * a.sc[term] * dfac * (double)s * (1.0 - (double)s));
    }
    for (int t = 0; t < 3; ++t) {
        const double r = y_block_sum(e[t], sh);
        if (threadIdx.x == 0) a.partial[(size_t)blockIdx.x * 3 + t] = r;
    }
}

// terms[0..3] = loss_prior, loss_bbox (coord), loss_obj, loss_selfpose
__global__ __launch_bounds__(256) void yolo_loss_finish_kernel(const double *__restrict__ partial, int nblocks, double sc0, double sc1, double sc2,
                                                               float *__restrict__ terms) {
    __shared__ double sh[4];
    double r[3];
    for (int t = 0; t < 3; ++t) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += 256) s += partial[(size_t)b * 3 + t];
        r[t] = y_block_sum(s, sh);
    }
    if (threadIdx.x == 0) {
        const float coord = (float)(r[0] * sc0), obj = (float)(r[1] * sc1), self = (float)(r[2] * sc2);
        terms[0] = coord + obj + self;        // loss_prior = loss_coord + loss_obj + loss_selfpose (float32, in that order)
        terms[1] = coord;
        terms[2] = obj;
        terms[3] = self;
    }
}

// ---- prior targets ----------------------------------------------------------------------------------------------------------------
__global__ void prior_init_kernel(float *__restrict__ prior, float *__restrict__ mconf, float *__restrict__ mcoord, float *__restrict__ wmap, size_t nprior,
                                  size_t nmask, float noobj) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nprior) prior[i] = 0.f;
    if (i < nmask) {
        mconf[i] = noobj;
        mcoord[i] = 0.f;
        wmap[i] = 1.f;
    }
}

__device__ __forceinline__ double np_min(double a, double b) { return (isnan(a) || isnan(b)) ? NAN : (a < b ? a : b); }
__device__ __forceinline__ double np_max(double a, double b) { return (isnan(a) || isnan(b)) ? NAN : (a > b ? a : b); }

// one thread per frame, persons in list order: where two persons share a cell the later one overwrites, as the reference's loop does
__global__ void prior_build_kernel(const double *__restrict__ boxes, const float *__restrict__ kp2d, const double *__restrict__ kpz, const double *__restrict__ pw,
                                   const int *__restrict__ n_persons, int B, int P, pn_yolo_target_cfg cfg, int gh, int gw, float *__restrict__ prior,
                                   float *__restrict__ mconf, float *__restrict__ mcoord, float *__restrict__ wmap) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= B) return;
    const int A = cfg.num_anchors, J = cfg.num_joints, F = 5 + 3 * J;
    const double sp = (double)cfg.stride_prior;
    const size_t HW = (size_t)gh * gw;
    const int np = min(max(n_persons[b], 0), P);
    for (int i = 0; i < np; ++i) {
        const double *bx = boxes + ((size_t)b * P + i) * 4;
        const double cx = (bx[0] + bx[2]) / 2.0 / sp, cy = (bx[1] + bx[3]) / 2.0 / sp;
        const double bw = (bx[2] - bx[0]) / sp, bh = (bx[3] - bx[1]) / sp;
        // bbox_ious([0, 0, bw, bh], [0, 0, aw, ah]) and the first argmax
        int best = 0;
        double bestv = 0.0;
        for (int an = 0; an < A; ++an) {
            const double aw = cfg.anchors[an][0], ah = cfg.anchors[an][1];
            const double b1x1 = 0.0 - bw / 2.0, b1y1 = 0.0 - bh / 2.0, b1x2 = 0.0 + bw / 2.0, b1y2 = 0.0 + bh / 2.0;
            const double b2x1 = 0.0 - aw / 2.0, b2y1 = 0.0 - ah / 2.0, b2x2 = 0.0 + aw / 2.0, b2y2 = 0.0 + ah / 2.0;
            double dxo = np_min(b1x2, b2x2) - np_max(b1x1, b2x1);
            double dyo = np_min(b1y2, b2y2) - np_max(b1y1, b2y1);
            if (dxo < 0) dxo = 0;
            if (dyo < 0) dyo = 0;
            const double inter = dxo * dyo;
            const double a1 = (b1x2 - b1x1) * (b1y2 - b1y1), a2 = (b2x2 - b2x1) * (b2y2 - b2y1);
            const double iou = inter / ((a1 + a2) - inter);
            if (an == 0) {
                bestv = iou;
            } else if (!isnan(bestv) && (iou > bestv || isnan(iou))) {        // np.argmax: first maximum, a NaN is the maximum
                best = an;
                bestv = iou;
            }
        }
        const double tx = trunc(cx), ty = trunc(cy);                            // int(), then min(size - 1, max(0, .)); a NaN centre (which
        const int gi = !(tx >= 0.0) ? 0 : (tx > (double)(gw - 1) ? gw - 1 : (int)tx);     // int() refuses) lands in cell 0, never outside
        const int gj = !(ty >= 0.0) ? 0 : (ty > (double)(gh - 1) ? gh - 1 : (int)ty);
        const double aw = cfg.anchors[best][0], ah = cfg.anchors[best][1];
        const size_t cellm = ((size_t)b * A + best) * HW + (size_t)gj * gw + gi;
        mconf[cellm] = (float)cfg.object_scale;
        mcoord[cellm] = 1.f;
        for (int an = 0; an < A; ++an) wmap[((size_t)b * A + an) * HW + (size_t)gj * gw + gi] = (float)pw[(size_t)b * P + i];
        float *pm = prior + ((size_t)b * A * F + (size_t)best * F) * HW + (size_t)gj * gw + gi;
        pm[0 * HW] = (float)(cx - gi);
        pm[1 * HW] = (float)(cy - gj);
        pm[2 * HW] = (float)(bw / aw);
        pm[3 * HW] = (float)(bh / ah);
        pm[4 * HW] = 1.f;
        const float *kp = kp2d + ((size_t)b * P + i) * J * 2;
        const double *kz = kpz + ((size_t)b * P + i) * J;
        for (int j = 0; j < J; ++j) {
            pm[(size_t)(5 + j) * HW] = (float)(((double)kp[2 * j] / sp - gi) / (aw / 2.0));
            pm[(size_t)(5 + J + j) * HW] = (float)(((double)kp[2 * j + 1] / sp - gj) / (ah / 2.0));
            pm[(size_t)(5 + 2 * J + j) * HW] = (float)((kz[j] - cfg.depth_mean) / cfg.depth_std);
        }
    }
}

// pn_conv2d_dgrad_strided's dispatch: kernel label and grid (nullptr: a kernel size it does not take); shared with pn_train_conv_plan_info
const char *pn_dgrad_strided_plan(int N, int Cin, int H, int W, int ks, unsigned *grid_x, unsigned *grid_y) {
    if (ks != 1 && ks != 3) return nullptr;
    *grid_x = (unsigned)((H * W + 255) / 256);
    *grid_y = (unsigned)std::min(N * Cin, 65535);
    return ks == 3 ? "dgrad_strided_kernel<3>" : "dgrad_strided_kernel<1>";
}

extern "C" {

int pn_conv2d_dgrad_strided(pn_ctx *ctx, const float *dy_dev, const float *w_dev, float *dx_dev, int N, int Cin, int H, int W, int Cout, int ks, int stride,
                            int pad, int accumulate, void *hip_stream) {
    PN_CTX_CHECK
    if (!dy_dev || !w_dev || !dx_dev || (ks != 1 && ks != 3) || stride < 1 || pad < 0 || pad > ks - 1 || N < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv2d_dgrad_strided: bad arguments (kernel 1 or 3, stride >= 1, 0 <= pad < kernel)");
    const int Ho = (H + 2 * pad - ks) / stride + 1, Wo = (W + 2 * pad - ks) / stride + 1;
    if (Ho < 1 || Wo < 1) return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv2d_dgrad_strided: empty output");
    unsigned gx = 0, gy = 0;
    (void)pn_dgrad_strided_plan(N, Cin, H, W, ks, &gx, &gy);
    const dim3 grid(gx, gy);
    hipStream_t s = (hipStream_t)hip_stream;
    if (ks == 3)
        hipLaunchKernelGGL(dgrad_strided_kernel<3>, grid, dim3(256), 0, s, dy_dev, w_dev, dx_dev, N, Cin, H, W, Cout, Ho, Wo, stride, pad, accumulate);
    else
        hipLaunchKernelGGL(dgrad_strided_kernel<1>, grid, dim3(256), 0, s, dy_dev, w_dev, dx_dev, N, Cin, H, W, Cout, Ho, Wo, stride, pad, accumulate);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

static int y_pool_geom(int H, int W, int k, int stride, int pad, int *Ho, int *Wo) {
    if (H < 1 || W < 1 || k < 1 || stride < 1 || pad < 0 || 2 * pad > k) return 0;      // torch: pad at most half the kernel
    *Ho = (H + 2 * pad - k) / stride + 1;
    *Wo = (W + 2 * pad - k) / stride + 1;
    return *Ho >= 1 && *Wo >= 1;
}

int pn_maxpool_forward(pn_ctx *ctx, const float *x_dev, float *y_dev, int *idx_dev, int planes, int H, int W, int k, int stride, int pad, void *hip_stream) {
    PN_CTX_CHECK
    int Ho, Wo;
    if (!x_dev || !y_dev || !idx_dev || planes < 1 || !y_pool_geom(H, W, k, stride, pad, &Ho, &Wo))
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_maxpool_forward: bad arguments");
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3((unsigned)((Ho * Wo + 255) / 256), (unsigned)std::min(planes, 65535)), dim3(256), 0, (hipStream_t)hip_stream,
                       x_dev, y_dev, idx_dev, planes, H, W, Ho, Wo, k, stride, pad);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_maxpool_backward(pn_ctx *ctx, const float *dy_dev, const int *idx_dev, float *dx_dev, int planes, int H, int W, int k, int stride, int pad, void *hip_stream) {
    PN_CTX_CHECK
    int Ho, Wo;
    if (!dy_dev || !idx_dev || !dx_dev || planes < 1 || !y_pool_geom(H, W, k, stride, pad, &Ho, &Wo))
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_maxpool_backward: bad arguments");
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)((H * W + 255) / 256), (unsigned)std::min(planes, 65535)), dim3(256), 0, (hipStream_t)hip_stream,
                       dy_dev, idx_dev, dx_dev, planes, H, W, Ho, Wo, k, stride, pad);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_yolo_loss(pn_ctx *ctx, const float *v_dev, const float *prior_map_dev, const float *mask_conf_dev, const float *mask_coord_dev, const float *weight_map_dev,
                 int N, int A, int J, int h, int w, float *out_dev, float *terms_dev, float *dv_dev, void *hip_stream) {
    PN_CTX_CHECK
    if (!v_dev || !prior_map_dev || !mask_conf_dev || !mask_coord_dev || !out_dev || !terms_dev || !dv_dev || N < 1 || A < 1 || J < 1 || h < 1 || w < 1)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_yolo_loss: bad arguments");
    YoloLossArgs a;
    a.v = v_dev; a.prior = prior_map_dev; a.mconf = mask_conf_dev; a.mcoord = mask_coord_dev; a.wmap = weight_map_dev;
    a.out = out_dev; a.dv = dv_dev;
    a.A = A; a.F = 5 + 3 * J; a.HW = h * w;
    a.total = (size_t)N * A * a.F * a.HW;
    const double M = (double)N * A * h * w;
    a.sc[0] = 4.0 / (M * 4.0);                        // WeightedMSELoss(...) * 4 over M x 4 elements
    a.sc[1] = 1.0 / M;
    a.sc[2] = (3.0 * J) / (M * 3.0 * J);              // WeightedMSELoss(...) * 3 J over M x 3J elements
    const unsigned nb = (unsigned)((a.total + 255) / 256);
    void *ws = nullptr;
    int rc = pn_train_ws(ctx, (size_t)nb * 3 * sizeof(double), &ws);
    if (rc != PN_OK) return rc;
    a.partial = (double *)ws;
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(yolo_loss_kernel, dim3(nb), dim3(256), 0, s, a);
    hipLaunchKernelGGL(yolo_loss_finish_kernel, dim3(1), dim3(256), 0, s, (const double *)ws, (int)nb, a.sc[0], a.sc[1], a.sc[2], terms_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

void pn_yolo_target_cfg_default(pn_yolo_target_cfg *cfg) {
    if (!cfg) return;
    cfg->input_x = 224; cfg->input_y = 224; cfg->stride_prior = 16; cfg->num_joints = PN_NUM_JOINTS; cfg->num_anchors = 2;
    for (int a = 0; a < PN_YOLO_MAX_ANCHORS; ++a) cfg->anchors[a][0] = cfg->anchors[a][1] = 0.0;
    cfg->anchors[0][0] = 6.0; cfg->anchors[0][1] = 3.0; cfg->anchors[1][0] = 12.0; cfg->anchors[1][1] = 6.0;
    cfg->noobject_scale = 0.1; cfg->object_scale = 1.0; cfg->depth_mean = 3.0; cfg->depth_std = 2.0;
}

int pn_build_prior_targets(pn_ctx *ctx, const double *boxes_dev, const float *kp2d_dev, const double *kp_z_dev, const double *pose_weight_dev,
                           const int *n_persons_dev, int B, int Pmax, const pn_yolo_target_cfg *cfg, float *prior_map_dev, float *mask_conf_dev,
                           float *mask_coord_dev, float *weight_map_dev, void *hip_stream) {
    PN_CTX_CHECK
    if (!cfg || !n_persons_dev || !prior_map_dev || !mask_conf_dev || !mask_coord_dev || !weight_map_dev || B < 1 || Pmax < 0 ||
        (Pmax > 0 && (!boxes_dev || !kp2d_dev || !kp_z_dev || !pose_weight_dev)) || cfg->stride_prior < 1 || cfg->num_joints < 1 ||
        cfg->num_anchors < 1 || cfg->num_anchors > PN_YOLO_MAX_ANCHORS || cfg->input_x < cfg->stride_prior || cfg->input_y < cfg->stride_prior)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_build_prior_targets: bad arguments");
    const int gh = cfg->input_y / cfg->stride_prior, gw = cfg->input_x / cfg->stride_prior;       // int(input / stride_prior)
    const size_t nmask = (size_t)B * cfg->num_anchors * gh * gw;
    const size_t nprior = nmask * (5 + 3 * cfg->num_joints);
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(prior_init_kernel, dim3((unsigned)((nprior + 255) / 256)), dim3(256), 0, s, prior_map_dev, mask_conf_dev, mask_coord_dev, weight_map_dev,
                       nprior, nmask, (float)cfg->noobject_scale);
    if (Pmax > 0)
        hipLaunchKernelGGL(prior_build_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, boxes_dev, kp2d_dev, kp_z_dev, pose_weight_dev, n_persons_dev, B, Pmax,
                           *cfg, gh, gw, prior_map_dev, mask_conf_dev, mask_coord_dev, weight_map_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

}  // extern "C"
