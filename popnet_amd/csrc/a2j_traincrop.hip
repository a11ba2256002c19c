// A2J training crops: the crop-level augmentation of the reference's A2J trainers, one launch for a batch of crops.
//
// Replaces (third_party_methods/A2J_experiments/):
//   dataPreprocess   itop_train_64.py:220-295, train_a2j_base.py:236-317, train_a2j_bgaug_new.py:251-338   (the image half)
//   transform        itop_train_64.py:208-218 (== train_a2j_base.py:170-180)                                (cv2.warpAffine of the crop)
// The label half, the random draws and every integer of the geometry are host work (popnet_amd/a2j_crops.py): each crop carries a
// pn_a2j_crop_item, checked and uploaded by pn_a2j_train_crop; the kernel never re-derives a truncation.
//
// One thread per output pixel, a gather of one or four composed pixels.  With warp set the four taps of cv2.warpAffine(INTER_LINEAR,
// constant border 0) are computed with the fixed-point arithmetic of OpenCV 4.2's generic path -- the arithmetic of aug_rotated_pixel
// (augment.hip), restated here because its source is not an image in memory but the chain below:
//   one pixel of the NORMALISED crop = INTER_NEAREST index -> (padded lookup) -> the frame's pixel as float32 -> (ITOP depth window)
//                                      -> (v - mean) / std
// A tap outside the crop reads the border value 0, which is not normalised zero depth.  Every operation rounds where numpy rounds it:
// plain operators under the file-wide pragma, no fused multiply-add, like augment.hip.
#pragma clang fp contract(off)
#include <cmath>
#include <hip/hip_fp16.h>
#include "pn_internal.h"

namespace {

struct TrainCropArgs {
    const void *frames;
    const pn_a2j_crop_item *items;
    float *out;
    int32_t *flags;
    int f16, H, W, cw, ch;
    float mean, stdv;
};

// pixel (x, y) of the normalised crop, 0 <= x < cw, 0 <= y < ch
__device__ __forceinline__ float tc_crop_pixel(const TrainCropArgs &a, const pn_a2j_crop_item &it, int x, int y) {
    // INTER_NEAREST: min(floor(d * (1 / inv_scale)), ssize - 1), inv_scale = dsize / ssize, all in double
    const double inv_x = (double)a.cw / (double)it.sw, inv_y = (double)a.ch / (double)it.sh;
    const int sx = min((int)floor((double)x * (1.0 / inv_x)), it.sw - 1);
    const int sy = min((int)floor((double)y * (1.0 / inv_y)), it.sh - 1);
    int py = sy, px = sx;
    bool inside = true;
    if (it.padded) {      // start < i < end, strictly, int(i - start) in float32, and the crop's own size
        const float fi = (float)sy, fj = (float)sx;
        py = (int)(fi - it.start1); px = (int)(fj - it.start2);
        inside = it.start1 < fi && fi < it.end1 && it.start2 < fj && fj < it.end2 && py < it.ih && px < it.iw;
    }
    float v = 0.f;
    if (inside) {      // 0 <= py < ih, 0 <= px < iw and the clipped region lies in the frame (checked on the host): a valid address
        const size_t off = ((size_t)it.frame * a.H + (it.cy0 + py)) * a.W + (it.cx0 + px);
        v = a.f16 ? __half2float(((const __half *)a.frames)[off]) : ((const float *)a.frames)[off];
    }
    if (it.window) {
        if (v >= it.hi) v = it.fill;
        if (v <= it.lo) v = it.fill;
        v = (v - it.sub) * it.scale;
    }
    return (v - a.mean) / a.stdv;
}

// grid (ceil(cw * ch / 256), n)
__global__ __launch_bounds__(256) void a2j_train_crop_kernel(TrainCropArgs a) {
    const int row = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const pn_a2j_crop_item it = a.items[row];
    const int raise = (it.sh < 1 || it.sw < 1) ? 1 : 0;
    if (idx == 0 && a.flags) a.flags[row] = raise;
    if (idx >= a.cw * a.ch) return;
    float *op = a.out + (size_t)row * a.cw * a.ch + idx;
    if (raise) { *op = 0.f; return; }
    const int y = idx / a.cw, x = idx - y * a.cw;
    if (!it.warp) { *op = tc_crop_pixel(a, it, x, y); return; }
    // warpAffine: AB_BITS = 10, INTER_BITS = 5; cvRound = rint (half to even)
    const double *m = it.m;
    const int adelta = (int)rint(m[0] * (double)x * 1024.0);
    const int bdelta = (int)rint(m[3] * (double)x * 1024.0);
    const int X0 = (int)rint((m[1] * (double)y + m[2]) * 1024.0) + 16;
    const int Y0 = (int)rint((m[4] * (double)y + m[5]) * 1024.0) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    const int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767);      // saturate_cast<short>
    if (sx >= a.cw || sx + 1 < 0 || sy >= a.ch || sy + 1 < 0) { *op = 0.f; return; }
    const float fx = (float)(X & 31) * 0.03125f, fy = (float)(Y & 31) * 0.03125f;
    const float wx0 = 1.f - fx, wy0 = 1.f - fy;
    const bool x0 = sx >= 0, x1 = sx + 1 < a.cw, y0 = sy >= 0, y1 = sy + 1 < a.ch;
    const float v0 = (y0 && x0) ? tc_crop_pixel(a, it, sx, sy) : 0.f;
    const float v1 = (y0 && x1) ? tc_crop_pixel(a, it, sx + 1, sy) : 0.f;
    const float v2 = (y1 && x0) ? tc_crop_pixel(a, it, sx, sy + 1) : 0.f;
    const float v3 = (y1 && x1) ? tc_crop_pixel(a, it, sx + 1, sy + 1) : 0.f;
    *op = v0 * (wy0 * wx0) + v1 * (wy0 * fx) + v2 * (fy * wx0) + v3 * (fy * fx);      // left to right, every product and sum rounded
}

bool tc_item_ok(const pn_a2j_crop_item &it, int F, int H, int W) {
    bool ok = it.frame >= 0 && it.frame < F && (it.padded == 0 || it.padded == 1) && (it.window == 0 || it.window == 1) && (it.warp == 0 || it.warp == 1);
    ok = ok && it.cy0 >= 0 && it.cx0 >= 0 && it.ih >= 0 && it.iw >= 0 && (long)it.cy0 + it.ih <= H && (long)it.cx0 + it.iw <= W;
    ok = ok && it.sh <= 65535 && it.sw <= 65535;
    if (it.padded) {
        const float b[4] = {it.start1, it.start2, it.end1, it.end2};
        for (float v : b) ok = ok && std::isfinite(v);
        ok = ok && it.start1 >= 0.f && it.start2 >= 0.f;
    } else {
        ok = ok && it.sh == it.ih && it.sw == it.iw;
    }
    if (it.window) {
        const float s[5] = {it.hi, it.lo, it.fill, it.sub, it.scale};
        for (float v : s) ok = ok && std::isfinite(v);
    }
    if (it.warp)      // |m0 x 1024| <= 2^28 and |(m1 y + m2) 1024| <= 2^28 + 2^29 for x, y < 4096: the casts to int and their sum stay in range
        for (int k = 0; k < 6; ++k) ok = ok && std::isfinite(it.m[k]) && std::fabs(it.m[k]) <= (k == 2 || k == 5 ? 524288.0 : 64.0);
    return ok;
}

}  // namespace

extern "C" {

size_t pn_sizeof_a2j_crop_item(void) { return sizeof(pn_a2j_crop_item); }

int pn_a2j_train_crop(pn_ctx *ctx, const void *frames_dev, int depth_dtype, int F, int H, int W, const pn_a2j_crop_item *items_host,
                      pn_a2j_crop_item *items_dev, int n, const pn_a2j_cfg *cfg, float *out_dev, int32_t *flags_dev, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (!frames_dev || (n > 0 && (!items_host || !items_dev || !out_dev)) || !cfg || F < 1 || H < 1 || W < 1 || H > 32767 || W > 32767 || n < 0 ||
        (size_t)F * H * W >= ((size_t)1 << 40))
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_train_crop: bad arguments");
    if (depth_dtype != PN_DEPTH_F16 && depth_dtype != PN_DEPTH_F32) return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_train_crop: unknown depth dtype %d", depth_dtype);
    if (n > 65535) return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_train_crop: %d crops, more than 65535 in one call", n);
    if (cfg->crop_w < 1 || cfg->crop_h < 1 || cfg->crop_w > 4096 || cfg->crop_h > 4096)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_train_crop: crop %dx%d, a side is 1 .. 4096", cfg->crop_w, cfg->crop_h);
    if (!std::isfinite(cfg->mean) || !std::isfinite(cfg->std) || cfg->std == 0.f)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_train_crop: mean %g / std %g", (double)cfg->mean, (double)cfg->std);
    for (int i = 0; i < n; ++i)
        if (!tc_item_ok(items_host[i], F, H, W))
            return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_train_crop: item %d has inconsistent geometry or a non-finite matrix or scalar", i);
    if (n == 0) return PN_OK;
    // the kernel reads the records this call has just checked: one source of truth, uploaded in stream order
    PN_HIP_CHECK(ctx, hipMemcpyAsync(items_dev, items_host, (size_t)n * sizeof(pn_a2j_crop_item), hipMemcpyHostToDevice, (hipStream_t)hip_stream));
    TrainCropArgs a;
    a.frames = frames_dev; a.items = items_dev; a.out = out_dev; a.flags = flags_dev;
    a.f16 = depth_dtype == PN_DEPTH_F16; a.H = H; a.W = W; a.cw = cfg->crop_w; a.ch = cfg->crop_h;
    a.mean = cfg->mean; a.stdv = cfg->std;
    hipLaunchKernelGGL(a2j_train_crop_kernel, dim3((unsigned)((a.cw * a.ch + 255) / 256), (unsigned)n), dim3(256), 0, (hipStream_t)hip_stream, a);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

}  // extern "C"
