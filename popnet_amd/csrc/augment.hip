// Random training augmentation on the GPU: the image half of the reference's training transform
//   Compose([Cvt2ndarray, Rotate(cx, cy), RenderDepth(cx, cy, max_ratio), [Hflip,] Crop, Resize(S)])
//   tpm/lib/datasets/data_augmentation_2d3d.py:411-448 (Rotate), :283-350 (RenderDepth), :452-493 (Hflip, the ITOP trainers), :94-128 (Crop),
//   :497-522 (Resize)
// followed by the clamp and the normalisation of KDH3D_Keypoints.__getitem__ (pn_preprocess's convention), as ONE launch per batch.
// Every item carries its own geometry in a pn_augment_item record; all integer geometry (the int() truncations of RenderDepth and
// Crop, numpy's clamping of slice ends) is decided on the host (popnet_amd/targets.py) -- the kernel never re-derives a truncation.
//
// One thread per output pixel, a gather of up to 16 composed pixels: the 2 x 2 taps of cv2.resize(INTER_LINEAR), each of them one
// pixel of the render image = float32(a) * one pixel of the rotated frame (or 0 in RenderDepth's zero padding), each of those the
// 2 x 2 taps of cv2.warpAffine(INTER_LINEAR, constant border 0).  Every intermediate rounds where the chain rounds:
//   warpAffine (OpenCV 4.2 imgwarp.cpp, generic path)  fixed point AB_BITS = 10, INTER_BITS = 5: adelta / bdelta / X0 / Y0 are
//       cvRound (half to even) of double products, the weights are the float table products (1 - k/32 | k/32)^2 (exact), the
//       value is v0*w0 + v1*w1 + v2*w2 + v3*w3 in float32, left to right; taps outside the source read 0
//   RenderDepth   new_image *= a: one float32 multiply
//   Resize        preproc_pixel.h's arithmetic (the same axis terms), with the scale taken from the item's own size
// No fused multiply-add anywhere: plain operators under the file-wide pragma, like the other bit-exact kernels.  (The __fmul_rn /
// __fadd_rn helpers are plain x * y / x + y compiled BEFORE the pragma, with contraction allowed: inlined, the compiler fuses them.)
// Cost on the MI355X: profiles/augment_producer_timing.md.
#pragma clang fp contract(off)
#include <cmath>
#include "pn_internal.h"
#include "preproc_pixel.h"

// one pixel of cv2.warpAffine(frame, rot_mat, (W, H), INTER_LINEAR); m = the inverted matrix as warpAffine holds it
__device__ __forceinline__ float aug_rotated_pixel(const float *__restrict__ img, int H, int W, const double *m, int x, int y) {
    const int adelta = (int)rint(m[0] * (double)x * 1024.0);
    const int bdelta = (int)rint(m[3] * (double)x * 1024.0);
    const int X0 = (int)rint((m[1] * (double)y + m[2]) * 1024.0) + 16;
    const int Y0 = (int)rint((m[4] * (double)y + m[5]) * 1024.0) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    const int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767);      // saturate_cast<short>
    if (sx >= W || sx + 1 < 0 || sy >= H || sy + 1 < 0) return 0.f;
    const float fx = (float)(X & 31) * 0.03125f, fy = (float)(Y & 31) * 0.03125f;
    const float wx0 = 1.f - fx, wy0 = 1.f - fy;
    const bool x0 = sx >= 0, x1 = sx + 1 < W, y0 = sy >= 0, y1 = sy + 1 < H;
    const float v0 = (y0 && x0) ? img[(size_t)sy * W + sx] : 0.f;
    const float v1 = (y0 && x1) ? img[(size_t)sy * W + sx + 1] : 0.f;
    const float v2 = (y1 && x0) ? img[(size_t)(sy + 1) * W + sx] : 0.f;
    const float v3 = (y1 && x1) ? img[(size_t)(sy + 1) * W + sx + 1] : 0.f;
    return v0 * (wy0 * wx0) + v1 * (wy0 * fx) + v2 * (fy * wx0) + v3 * (fy * fx);      // left to right, every product and sum rounded
}

// one pixel of the image Resize sees: (x, y) in the cropped render image
__device__ __forceinline__ float aug_source_pixel(const float *__restrict__ img, int H, int W, const pn_augment_item &it, int x, int y) {
    const int cxr = x + it.crop_x0;                                                      // column of the render image Crop hands on
    const int rx = (it.hflip ? it.render_w - 1 - cxr : cxr) + it.render_x, ry = y + it.crop_y0 + it.render_y;      // position in the rotated frame (Hflip: np.flip(axis=1) of the render image)
    if (rx < 0 || rx >= W || ry < 0 || ry >= H) return 0.f;                              // RenderDepth's zero image around the pasted frame
    return aug_rotated_pixel(img, H, W, it.m, rx, ry) * it.scale;
}

__global__ __launch_bounds__(256) void augment_resize_kernel(const float *__restrict__ composed, const pn_augment_item *__restrict__ items, int H, int W,
                                                              float *__restrict__ out, int S, float dmax, float mean, float stdv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= S * S) return;
    const int dy = i / S, dx = i - dy * S;
    const pn_augment_item it = items[b];
    const float *img = composed + (size_t)b * H * W;
    const double scale_x = 1.0 / ((double)S / (double)it.src_w);       // as cv::resize computes them
    const double scale_y = 1.0 / ((double)S / (double)it.src_h);
    const PnAxisX ax = pn_preproc_axis_x(dx, scale_x, it.src_w);
    const PnAxisY ay = pn_preproc_axis_y(dy, scale_y, it.src_h);
    const float a0 = 1.f - ax.fx, a1 = ax.fx;
    float h0, h1;
    if (ax.sx + 1 >= it.src_w) {      // HResizeLinear tail: D = S[sx] * 1
        h0 = aug_source_pixel(img, H, W, it, ax.sx, ay.y0);
        h1 = aug_source_pixel(img, H, W, it, ax.sx, ay.y1);
    } else {
        h0 = aug_source_pixel(img, H, W, it, ax.sx, ay.y0) * a0 + aug_source_pixel(img, H, W, it, ax.sx + 1, ay.y0) * a1;
        h1 = aug_source_pixel(img, H, W, it, ax.sx, ay.y1) * a0 + aug_source_pixel(img, H, W, it, ax.sx + 1, ay.y1) * a1;
    }
    float v = h0 * (1.f - ay.fy) + h1 * ay.fy;
    if (v < 0.f) v = 0.f;
    if (v > dmax) v = dmax;
    out[(size_t)b * S * S + i] = (v - mean) / stdv;
}

extern "C" {

size_t pn_sizeof_augment_item(void) { return sizeof(pn_augment_item); }

int pn_augment_resize(pn_ctx *ctx, const float *composed_dev, const pn_augment_item *items_host, pn_augment_item *items_dev, int B, int H, int W,
                      float *out_dev, int S, float depth_max, float depth_mean, float depth_std, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (!composed_dev || !items_dev || !items_host || !out_dev || B < 1 || B > 65535 || H < 2 || W < 2 || H > 32767 || W > 32767 || S < 1 || S > 32767)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_augment_resize: bad arguments");
    for (int b = 0; b < B; ++b) {
        const pn_augment_item &it = items_host[b];
        bool ok = std::isfinite(it.scale) && it.render_w >= 1 && it.render_h >= 1 && it.render_w <= 65535 && it.render_h <= 65535;
        for (int k = 0; k < 6; ++k) ok = ok && std::isfinite(it.m[k]) && std::fabs(it.m[k]) < 1.0e6;
        ok = ok && it.render_x > -65536 && it.render_x < 65536 && it.render_y > -65536 && it.render_y < 65536;
        ok = ok && it.crop_x0 >= 0 && it.crop_x0 < it.crop_x1 && it.crop_x1 <= it.render_w && it.crop_y0 >= 0 && it.crop_y0 < it.crop_y1 && it.crop_y1 <= it.render_h;
        ok = ok && (it.hflip == 0 || it.hflip == 1);
        ok = ok && it.src_w == it.crop_x1 - it.crop_x0 && it.src_h == it.crop_y1 - it.crop_y0 && it.src_w >= 1 && it.src_h >= 1;
        if (!ok) return pn_set_error(ctx, PN_ERR_INVALID, "pn_augment_resize: item %d has inconsistent geometry", b);
        if (it.src_w == 2 * S && it.src_h == 2 * S)      // as pn_preprocess: cv::resize switches to INTER_AREA at exactly 2x decimation
            return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "pn_augment_resize: item %d: %dx%d -> %d is an exact 2x decimation, where cv2.resize(INTER_LINEAR) runs INTER_AREA instead: not built",
                                b, it.src_w, it.src_h, S);
    }
    // the kernel reads the records this call has just checked: one source of truth, uploaded in stream order
    PN_HIP_CHECK(ctx, hipMemcpyAsync(items_dev, items_host, (size_t)B * sizeof(pn_augment_item), hipMemcpyHostToDevice, (hipStream_t)hip_stream));
    dim3 grid((unsigned)((S * S + 255) / 256), (unsigned)B), block(256);
    hipLaunchKernelGGL(augment_resize_kernel, grid, block, 0, (hipStream_t)hip_stream, composed_dev, items_dev, H, W, out_dev, S, depth_max, depth_mean, depth_std);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

}  // extern "C"
