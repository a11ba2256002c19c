// Depth-ablation arms of the MP-3DHP evaluation (pn_ablation_pred_raw, pn_ablation_perfect_2d, pn_depth_probe): the per-joint read-outs of
// tpm/evaluate/evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py:197-299 that replace the depth of a joint by the "raw depth" -- the
// un-normalised network input at one pixel -- and / or its 2D location by the ground truth.  The pre-processed [B,1,S,S] tensor need not
// exist (pn_rtpose_forward_frames never writes it): a pixel is re-derived from the raw frame with pn_preprocess's arithmetic
// (preproc_pixel.h), then un-normalised as the script does (:183-185, `img *= std; img += mean` on float32), and back-projected in
// float64 in the order of joint_readout (parse_device.h).
#include "pn_internal.h"
#include "preproc_pixel.h"

namespace {

constexpr int J_ = PN_NUM_JOINTS;
constexpr int Z_C = PN_NUM_LIMBS + 1;      // channels of the pose-depth map; joint j reads channel j (joint2chn is the identity)

// img224[dy, dx] of the script: fl32(fl32(norm * std) + mean), two float32 roundings, no fused multiply-add
template <typename TIN>
__device__ __forceinline__ float raw_pixel(const TIN *__restrict__ img, int H, int W, int dy, int dx, double scale_x, double scale_y,
                                           float dmax, float mean, float stdv) {
#pragma clang fp contract(off)
    float v = pn_preproc_pixel(img, H, W, dy, dx, scale_x, scale_y, dmax, mean, stdv);
    v = v * stdv;
    v = v + mean;
    return v;
}

// (x2 - cx) * d / fx, (y2 - cy) * d / fy, d  (:258-262, :268-272, :284-298)
__device__ __forceinline__ void back_project(double x2, double y2, double d, const pn_parse_cfg &cfg, double *__restrict__ out3) {
#pragma clang fp contract(off)
    out3[0] = (x2 - cfg.cx) * d / cfg.fx;
    out3[1] = (y2 - cfg.cy) * d / cfg.fy;
    out3[2] = d;
}

// PN_DEPTH_NET: the buffer IS the network input [B,1,S,S] float32 (H == W == S), already clamped and normalised -- the scripts that compose
// or augment their frames have no raw frame to re-derive a pixel from (evaluation_rtpose_light3d_kdh3d_mpaug_ablation.py:206-207).  The tag
// type selects the overload below in the same three kernels; the un-normalisation is the same two roundings.
struct NetIn { float v; };

__device__ __forceinline__ float raw_pixel(const NetIn *__restrict__ img, int H, int W, int dy, int dx, double, double, float, float mean, float stdv) {
#pragma clang fp contract(off)
    float v = img[(size_t)dy * W + dx].v;
    v = v * stdv;
    v = v + mean;
    return v;
}

// grid = B, block = 256: thread t -> (person, joint) rows of one record
template <typename TIN>
__global__ __launch_bounds__(256) void ablation_pred_raw_kernel(const TIN *__restrict__ depth, int H, int W, double scale_x, double scale_y,
                                                                float dmax, pn_parse_cfg cfg, const pn_pose_frame *__restrict__ frames,
                                                                double *__restrict__ out) {
    const int b = blockIdx.x;
    const pn_pose_frame &F = frames[b];
    const TIN *img = depth + (size_t)b * H * W;
    const int S = cfg.input_size;
    const int np = min(max(F.n_persons, 0), PN_MAX_PERSONS);
    double *ob = out + (size_t)b * PN_MAX_PERSONS * J_ * 3;
    for (int t = threadIdx.x; t < PN_MAX_PERSONS * J_; t += 256) {
        const int o = t / J_, j = t - o * J_;
        double *o3 = ob + (size_t)t * 3;
        if (o >= np) {
            o3[0] = 0.0; o3[1] = 0.0; o3[2] = 0.0;
            continue;
        }
        const int id = F.person_joint[o][j];
        double x2 = -1.0, y2 = -1.0, raw = -1.0;
        if (id >= 0 && id < PN_MAX_PEAKS) {
            // img[b][0][int(joint[1]), int(joint[0])] (:216); the peak of a record lies inside the S x S frame, the clamp only keeps a
            // hand-made record from naming a pixel that does not exist
            const int px = min(max((int)F.peak_x[id], 0), S - 1), py = min(max((int)F.peak_y[id], 0), S - 1);
            raw = (double)raw_pixel(img, H, W, py, px, scale_x, scale_y, dmax, cfg.depth_mean, cfg.depth_std);
            x2 = F.joints_2d[o][j][0];
            y2 = F.joints_2d[o][j][1];
        }
        back_project(x2, y2, raw, cfg, o3);
    }
}

// grid = (ceil(Gmax * J / 256), B), block = 256: thread -> (GT person, joint)
template <typename TIN>
__global__ __launch_bounds__(256) void ablation_perfect_2d_kernel(const TIN *__restrict__ depth, int H, int W, double scale_x, double scale_y,
                                                                  float dmax, const float *__restrict__ z, int h, int w, pn_parse_cfg cfg,
                                                                  const double *__restrict__ gt_2d, const int *__restrict__ gt_count, int Gmax,
                                                                  double *__restrict__ out_map, double *__restrict__ out_raw) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Gmax * J_) return;
    const int g = t / J_, j = t - g * J_;
    const size_t row = ((size_t)b * Gmax + g) * J_ + j;
    double *om = out_map + row * 3, *orw = out_raw + row * 3;
    if (g >= min(max(gt_count[b], 0), Gmax)) {
        om[0] = 0.0; om[1] = 0.0; om[2] = 0.0;
        orw[0] = 0.0; orw[1] = 0.0; orw[2] = 0.0;
        return;
    }
    const double gx = gt_2d[row * 2], gy = gt_2d[row * 2 + 1];
    const int S = cfg.input_size;
    const double dS = (double)S, dD = (double)cfg.downsample;
    // int(gx / w_org * input_size / DOWNSAMPLE), float64 left to right, truncation toward zero, clamp to the map (:227-232)
    int mx = (int)(gx / (double)cfg.w_org * dS / dD), my = (int)(gy / (double)cfg.h_org * dS / dD);
    mx = min(max(mx, 0), w - 1);
    my = min(max(my, 0), h - 1);
    float d = z[(((size_t)b * Z_C + j) * h + my) * w + mx] * cfg.depth_std;      // posedepth *= std; += mean on float32 (:179-180)
    d = d + cfg.depth_mean;
    // int(gx / w_org * input_size) clamped to the frame (:238-240)
    int px = (int)(gx / (double)cfg.w_org * dS), py = (int)(gy / (double)cfg.h_org * dS);
    px = min(max(px, 0), S - 1);
    py = min(max(py, 0), S - 1);
    const float raw = raw_pixel(depth + (size_t)b * H * W, H, W, py, px, scale_x, scale_y, dmax, cfg.depth_mean, cfg.depth_std);
    back_project(gx, gy, (double)d, cfg, om);
    back_project(gx, gy, (double)raw, cfg, orw);
}

// one thread per point
template <typename TIN>
__global__ __launch_bounds__(256) void depth_probe_kernel(const TIN *__restrict__ depth, int B, int H, int W, int S, double scale_x, double scale_y,
                                                          float dmax, float mean, float stdv, const int *__restrict__ pts, int n,
                                                          float *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = pts[3 * i], y = pts[3 * i + 1], x = pts[3 * i + 2];
    if (b < 0 || b >= B || y < 0 || y >= S || x < 0 || x >= S) return;      // the host refused these before the launch
    out[i] = raw_pixel(depth + (size_t)b * H * W, H, W, y, x, scale_x, scale_y, dmax, mean, stdv);
}

// the arguments every entry shares: frames, their size against the S x S network input, the parse configuration
int check_frames(pn_ctx *ctx, const char *who, const void *depth_dev, int depth_dtype, int B, int H, int W, int S) {
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if ((B > 0 && !depth_dev) || B < 0 || H < 2 || W < 2 || S < 1 || (size_t)S * S > 0x7fffffffu || B > 65535)
        return pn_set_error(ctx, PN_ERR_INVALID, "%s: bad arguments", who);
    if (depth_dtype != PN_DEPTH_F16 && depth_dtype != PN_DEPTH_F32 && depth_dtype != PN_DEPTH_NET)
        return pn_set_error(ctx, PN_ERR_INVALID, "%s: unknown depth dtype %d", who, depth_dtype);
    if (depth_dtype == PN_DEPTH_NET) {   // nothing is resized: the 2x refusal below does not apply
        if (H != S || W != S)
            return pn_set_error(ctx, PN_ERR_INVALID, "%s: a network input (PN_DEPTH_NET) is %dx%d, the buffer is %dx%d", who, S, S, W, H);
        return PN_OK;
    }
    if (W == 2 * S && H == 2 * S)   // as pn_preprocess: the pixel would be INTER_AREA's, which is not built
        return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "%s: %dx%d -> %d is an exact 2x decimation, where cv2.resize(INTER_LINEAR) runs INTER_AREA instead: not built", who, W, H, S);
    return PN_OK;
}

int check_cfg(pn_ctx *ctx, const char *who, const pn_parse_cfg *cfg) {
    if (!cfg || cfg->input_size < 1 || cfg->downsample < 1 || cfg->w_org < 1 || cfg->h_org < 1)
        return pn_set_error(ctx, PN_ERR_INVALID, "%s: bad configuration", who);
    return PN_OK;
}

}  // namespace

#define ABL_LAUNCH(kernel, grid, ...)                                                                               \
    do {                                                                                                            \
        if (depth_dtype == PN_DEPTH_F16)                                                                            \
            hipLaunchKernelGGL(kernel<_Float16>, grid, dim3(256), 0, s, (const _Float16 *)depth_dev, __VA_ARGS__);  \
        else if (depth_dtype == PN_DEPTH_NET)                                                                       \
            hipLaunchKernelGGL(kernel<NetIn>, grid, dim3(256), 0, s, (const NetIn *)depth_dev, __VA_ARGS__);        \
        else                                                                                                        \
            hipLaunchKernelGGL(kernel<float>, grid, dim3(256), 0, s, (const float *)depth_dev, __VA_ARGS__);        \
    } while (0)

extern "C" int pn_ablation_pred_raw(pn_ctx *ctx, const void *depth_dev, int depth_dtype, int B, int H, int W, float depth_max,
                                    const pn_parse_cfg *cfg, const pn_pose_frame *frames_dev, double *out_dev, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    int rc = check_cfg(ctx, "pn_ablation_pred_raw", cfg);
    if (rc != PN_OK) return rc;
    rc = check_frames(ctx, "pn_ablation_pred_raw", depth_dev, depth_dtype, B, H, W, cfg->input_size);
    if (rc != PN_OK) return rc;
    if (!frames_dev || !out_dev || B < 1) return pn_set_error(ctx, PN_ERR_INVALID, "pn_ablation_pred_raw: bad arguments");
    const int S = cfg->input_size;
    const double scale_x = 1.0 / ((double)S / (double)W), scale_y = 1.0 / ((double)S / (double)H);   // as pn_preprocess
    hipStream_t s = (hipStream_t)hip_stream;
    ABL_LAUNCH(ablation_pred_raw_kernel, dim3((unsigned)B), H, W, scale_x, scale_y, depth_max, *cfg, frames_dev, out_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

extern "C" int pn_ablation_perfect_2d(pn_ctx *ctx, const void *depth_dev, int depth_dtype, int B, int H, int W, float depth_max,
                                      const float *z_dev, int h, int w, const pn_parse_cfg *cfg, const double *gt_2d_dev,
                                      const int *gt_count_dev, int Gmax, double *out_map_dev, double *out_raw_dev, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    int rc = check_cfg(ctx, "pn_ablation_perfect_2d", cfg);
    if (rc != PN_OK) return rc;
    rc = check_frames(ctx, "pn_ablation_perfect_2d", depth_dev, depth_dtype, B, H, W, cfg->input_size);
    if (rc != PN_OK) return rc;
    if (Gmax < 0 || Gmax > 0x7fffffff / (J_ * 256)) return pn_set_error(ctx, PN_ERR_INVALID, "pn_ablation_perfect_2d: Gmax %d out of range", Gmax);
    if (B == 0 || Gmax == 0) return PN_OK;
    if (!z_dev || !gt_2d_dev || !gt_count_dev || !out_map_dev || !out_raw_dev)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_ablation_perfect_2d: bad arguments");
    const int S = cfg->input_size;
    // the script clamps the cell to int(input_size / DOWNSAMPLE) - 1 on both axes (:231-232): the map must be that square
    if (h != S / cfg->downsample || w != S / cfg->downsample || h < 1)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_ablation_perfect_2d: map %dx%d is not input_size / downsample = %d / %d", h, w, S, cfg->downsample);
    const double scale_x = 1.0 / ((double)S / (double)W), scale_y = 1.0 / ((double)S / (double)H);
    hipStream_t s = (hipStream_t)hip_stream;
    ABL_LAUNCH(ablation_perfect_2d_kernel, dim3((unsigned)((Gmax * J_ + 255) / 256), (unsigned)B), H, W, scale_x, scale_y, depth_max, z_dev, h, w,
               *cfg, gt_2d_dev, gt_count_dev, Gmax, out_map_dev, out_raw_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

extern "C" int pn_depth_probe(pn_ctx *ctx, const void *depth_dev, int depth_dtype, int B, int H, int W, int S, float depth_max,
                              float depth_mean, float depth_std, const int *pts_dev, int n, float *out_dev, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    int rc = check_frames(ctx, "pn_depth_probe", depth_dev, depth_dtype, B, H, W, S);
    if (rc != PN_OK) return rc;
    if (B < 1 || n < 0 || (n > 0 && (!pts_dev || !out_dev))) return pn_set_error(ctx, PN_ERR_INVALID, "pn_depth_probe: bad arguments");
    if (n == 0) return PN_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    // a point outside the batch or the frame is an error, not a clamp: the points are read back and checked before anything is launched
    // (this is the second-pass / test entry, like pn_parse_paf_unbounded; it waits for the stream and cannot be captured)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (s && hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return pn_set_error(ctx, PN_ERR_STATE, "pn_depth_probe: the stream is being captured (the call checks its points on the host)");
    std::vector<int> pts((size_t)n * 3);
    PN_HIP_CHECK(ctx, hipMemcpyAsync(pts.data(), pts_dev, pts.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    PN_HIP_CHECK(ctx, hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        const int b = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], x = pts[3 * (size_t)i + 2];
        if (b < 0 || b >= B || y < 0 || y >= S || x < 0 || x >= S)
            return pn_set_error(ctx, PN_ERR_INVALID, "pn_depth_probe: point %d (frame %d, y %d, x %d) is outside %d frames of %dx%d", i, b, y, x, B, S, S);
    }
    const double scale_x = 1.0 / ((double)S / (double)W), scale_y = 1.0 / ((double)S / (double)H);
    ABL_LAUNCH(depth_probe_kernel, dim3((unsigned)((n + 255) / 256)), B, H, W, S, scale_x, scale_y, depth_max, depth_mean, depth_std, pts_dev, n,
               out_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}
