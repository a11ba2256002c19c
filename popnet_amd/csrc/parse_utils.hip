// Stand-alone utilities of the pose parse for the per-call Python API: pn_retrieve_depth and pn_pack_pose_frames.
#pragma clang fp contract(off)
#include "parse_device.h"

// ---------------------------------------------------------------------------------------------
// Stand-alone retrieve_depth_heat_weighted (tpm/lib/utils/common.py:272-293) for the per-call
// Python API: n centres on one (depthmap, heatmap) pair, one lane per centre.  Like the reference
// it clamps negative heat values IN PLACE in the caller's heat map before reading.
// ---------------------------------------------------------------------------------------------
__global__ void clamp_negative_kernel(float *__restrict__ hm, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && hm[i] < 0.f) hm[i] = 0.f;
}

__global__ void retrieve_depth_kernel(const float *__restrict__ dm, const float *__restrict__ hm, int h, int w,
                                      const int *__restrict__ centers, int n, int radius, float *__restrict__ out) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int cx0 = centers[2 * t], cy0 = centers[2 * t + 1];
    const int min_x = min(max(cx0 - radius, 0), w - 1), max_x = max(min(cx0 + radius, w - 1), 0);
    const int min_y = min(max(cy0 - radius, 0), h - 1), max_y = max(min(cy0 + radius, h - 1), 0);
    // np.sum over the [ny, nx] window: numpy pairwise summation (blocks of 8, then the tail)
    const int nx = max_x - min_x + 1, cnt = nx * (max_y - min_y + 1);
    if (cnt >= 128) {
        out[t] = __builtin_nanf("");      // windows of >= 128 cells are refused by the host wrapper
        return;
    }
    auto P = [&](int k) { int yy = min_y + k / nx, xx = min_x + k % nx; return dm[yy * w + xx] * (hm[yy * w + xx] + 0.000000001f); };
    auto Wt = [&](int k) { int yy = min_y + k / nx, xx = min_x + k % nx; return hm[yy * w + xx] + 0.000000001f; };
    const float sp = np_pairwise_sum<float>(cnt, P), sw = np_pairwise_sum<float>(cnt, Wt);
    out[t] = sp / sw;
}

// one thread per (frame, person slot, joint): float64 record -> float32 wire values
__global__ __launch_bounds__(256) void pack_pose_kernel(const pn_pose_frame *__restrict__ frames, int B, pn_pose_wire *__restrict__ wire) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int per = PN_WIRE_MAX_PERSONS * PN_NUM_JOINTS;
    if (i >= B * per) return;
    const int f = i / per, r = i - f * per, p = r / PN_NUM_JOINTS, j = r - p * PN_NUM_JOINTS;
    const pn_pose_frame &fr = frames[f];
    pn_pose_wire &w = wire[f];
    const int n = fr.n_persons;
    if (r == 0) {
        w.n_persons = n;
        w.status = fr.status | (n > PN_WIRE_MAX_PERSONS ? PN_FRAME_OVERFLOW_PERSONS : 0u);
    }
    const bool live = p < n;
    w.person_joint[p][j] = live ? (int16_t)fr.person_joint[p][j] : (int16_t)-1;
    w.vals[p][j][0] = live ? (float)fr.joints_2d[p][j][0] : 0.f;
    w.vals[p][j][1] = live ? (float)fr.joints_2d[p][j][1] : 0.f;
    w.vals[p][j][2] = live ? (float)fr.joints_3d[p][j][0] : 0.f;
    w.vals[p][j][3] = live ? (float)fr.joints_3d[p][j][1] : 0.f;
    w.vals[p][j][4] = live ? (float)fr.joints_3d[p][j][2] : 0.f;
    w.vals[p][j][5] = live ? (float)fr.part_conf[p][j] : 0.f;
}

extern "C" int pn_pack_pose_frames(pn_ctx *ctx, const pn_pose_frame *frames_dev, int B, pn_pose_wire *wire_dev, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    if (!frames_dev || !wire_dev || B < 1) return pn_set_error(ctx, PN_ERR_INVALID, "pn_pack_pose_frames: bad arguments");
    const int total = B * PN_WIRE_MAX_PERSONS * PN_NUM_JOINTS;
    hipLaunchKernelGGL(pack_pose_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, frames_dev, B, wire_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

extern "C" size_t pn_sizeof_pose_wire(void) { return sizeof(pn_pose_wire); }

extern "C" int pn_retrieve_depth(pn_ctx *ctx, const float *depthmap_dev, float *heatmap_dev, int h, int w,
                                 const int *centers_xy_dev, int n, int radius, float *out_dev, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (!depthmap_dev || !heatmap_dev || !centers_xy_dev || !out_dev || n < 1 || radius < 0)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_retrieve_depth: bad arguments");
    if ((2 * radius + 1) * (2 * radius + 1) >= 128)
        return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "pn_retrieve_depth: radius %d too large", radius);
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(clamp_negative_kernel, dim3((h * w + 255) / 256), dim3(256), 0, s, heatmap_dev, h * w);
    hipLaunchKernelGGL(retrieve_depth_kernel, dim3((n + 63) / 64), dim3(64), 0, s, depthmap_dev, (const float *)heatmap_dev,
                       h, w, centers_xy_dev, n, radius, out_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}
