// Yolo-A2J second stage, everything around the network: the per-box crop and the anchor vote with its map back to the frame.
//
// Replaces (third_party_methods/A2J_experiments/):
//   dataPreprocess                 a2j_test_pred_box_new.py:268-313   -> a2j_crop_kernel
//   post_process.forward           anchor.py:57-82                    -> a2j_vote_kernel (f32 / bf16 heads), a2j_vote_x3_kernel ([hi | lo] heads of a bf16x3 net)
//   main(), result -> frame lists  a2j_test_pred_box_new.py:373-421   -> a2j_vote_kernel's epilogue
// The network itself (A2J_model, model.py:145-186) is a pn_net of kind PN_NET_A2J (net.hip::build_a2j).
#include <hip/hip_fp16.h>
#include "pn_internal.h"

namespace {

struct CropArgs {
    const void *frames;
    const float *rows;
    float *out;
    int32_t *flags;
    int f16, F, H, W, n, img_w, img_h, cw, ch;
    float mean, stdv, conf_min;
};

// One row's geometry, as dataPreprocess computes it (every float operation in fp32, as numpy does on the float32 box array).
struct CropGeom {
    int valid;                 // 0: all-zero crop
    int raise;                 // the reference raises here (empty image into cv2.resize)
    int padded;
    int cy0, cx0, ih, iw;      // the clipped region depth[cy0 : cy0 + ih, cx0 : cx0 + iw]
    int sh, sw;                // the image cv2.resize reads
    float start1, start2, end1, end2;
};

// A float that int() takes without overflow: finite and within [-(2^31 - 128), 2^31 - 128], the largest float below 2^31.  False for a NaN.
__device__ __forceinline__ bool fits_int(float v) { return v >= -2147483520.f && v <= 2147483520.f; }

// The rows are device data nobody has inspected (a decode's exp of a logit), so nothing is cast to int before plain comparisons have shown
// that it fits:
//   frame index not in [0, F) (a NaN included): the reference has no such frame to load and raises whatever the confidence: zeros, flag 1;
//   conf <= conf_min or NaN: zeros, flag 0, whatever the coordinates hold -- the script never reads them;
//   otherwise a coordinate, x1 - x0 or y1 - y0 that is NaN, infinite or past an int: the reference raises (int(nan), int(inf), a zero image
//   of an absurd size): zeros, flag 1.
// Why every address is then bounded: every value cast below lies in [-(2^31 - 128), 2^31 - 128], so each int() is the truncation it says.
// cy0 >= 0 and ih <= H - min(cy0, H) by the slice rule, so ih > 0 implies cy0 + ih <= H, and the same in x.  The kernel reads the frame only
// at (cy0 + py, cx0 + px) with 0 <= py < ih and 0 <= px < iw -- unpadded because sy <= sh - 1 = ih - 1, padded because the paste test
// demands start < i (so i - start > 0 truncates to py >= 0) and py < ih -- and fi is in [0, F).
__device__ CropGeom crop_geom(const float *r, const CropArgs &a) {
    CropGeom g;
    g.valid = 0; g.raise = 0; g.padded = 0; g.cy0 = g.cx0 = g.ih = g.iw = g.sh = g.sw = 0;
    g.start1 = g.start2 = g.end1 = g.end2 = 0.f;
    const float x0 = r[1], y0 = r[2], x1 = r[3], y1 = r[4], conf = r[5];
    if (!(r[0] >= 0.f && r[0] < (float)a.F) || (int)r[0] >= a.F) { g.raise = 1; return g; }      // (float)F may round up: the int test decides
    if (!(conf > a.conf_min)) return g;
    if (!(fits_int(x0) && fits_int(y0) && fits_int(x1) && fits_int(y1) && fits_int(__fsub_rn(x1, x0)) && fits_int(__fsub_rn(y1, y0)))) { g.raise = 1; return g; }
    const float nx0 = fmaxf(x0, 0.f), ny0 = fmaxf(y0, 0.f);
    const float nx1 = fminf(x1, (float)(a.W - 1)), ny1 = fminf(y1, (float)(a.H - 1));
    const int cx0 = (int)nx0, cy0 = (int)ny0, cx1 = (int)nx1, cy1 = (int)ny1;      // int(): truncation
    // depth[cy0:cy1, cx0:cx1] by Python's slice rules: a start past the frame or an end before the start is empty, a NEGATIVE end counts from
    // the far edge (cy1 >= -(2^31 - 128) and H > 0: the sum cannot overflow)
    g.cy0 = cy0; g.cx0 = cx0;
    g.ih = max((cy1 < 0 ? max(cy1 + a.H, 0) : min(cy1, a.H)) - min(cy0, a.H), 0);
    g.iw = max((cx1 < 0 ? max(cx1 + a.W, 0) : min(cx1, a.W)) - min(cx0, a.W), 0);
    g.padded = (x0 < 0.f || y0 < 0.f || x1 > (float)a.img_w || y1 > (float)a.img_h) ? 1 : 0;
    if (g.padded) {
        g.sh = (int)__fsub_rn(y1, y0); g.sw = (int)__fsub_rn(x1, x0);
        g.start1 = y0 < 0.f ? __fsub_rn(0.f, y0) : 0.f;
        g.start2 = x0 < 0.f ? __fsub_rn(0.f, x0) : 0.f;
        g.end1 = y1 > (float)a.img_h ? __fadd_rn((float)g.ih, g.start1) : (float)g.sh;
        g.end2 = x1 > (float)a.img_w ? __fadd_rn((float)g.iw, g.start2) : (float)g.sw;
    } else {
        g.sh = g.ih; g.sw = g.iw;
    }
    if (g.sh <= 0 || g.sw <= 0) { g.raise = 1; return g; }
    g.valid = 1;
    return g;
}

// grid (ceil(cw * ch / 256), n): one thread per output pixel
__global__ __launch_bounds__(256) void a2j_crop_kernel(CropArgs a) {
    const int row = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const float *r = a.rows + (size_t)row * 6;
    const CropGeom g = crop_geom(r, a);
    if (idx == 0 && a.flags) a.flags[row] = g.raise;
    if (idx >= a.cw * a.ch) return;
    float *op = a.out + (size_t)row * a.cw * a.ch + idx;
    if (!g.valid) { *op = 0.f; return; }
    const int oy = idx / a.cw, ox = idx - oy * a.cw;
    // INTER_NEAREST: min(floor(d * (1 / inv_scale)), ssize - 1), inv_scale = dsize / ssize, all in double
    const double inv_x = (double)a.cw / (double)g.sw, inv_y = (double)a.ch / (double)g.sh;
    const int sx = min((int)floor((double)ox * (1.0 / inv_x)), g.sw - 1);
    const int sy = min((int)floor((double)oy * (1.0 / inv_y)), g.sh - 1);
    int py = sy, px = sx;
    bool inside = true;
    if (g.padded) {      // start < i < end, strictly, and the crop's own size
        const float fi = (float)sy, fj = (float)sx;
        py = (int)__fsub_rn(fi, g.start1); px = (int)__fsub_rn(fj, g.start2);
        inside = g.start1 < fi && fi < g.end1 && g.start2 < fj && fj < g.end2 && py < g.ih && px < g.iw;
    }
    float v = 0.f;
    if (inside) {      // py < ih, px < iw and the clipped region lies in the frame: a valid address
        const size_t off = ((size_t)(int)r[0] * a.H + (g.cy0 + py)) * a.W + (g.cx0 + px);
        v = a.f16 ? __half2float(((const __half *)a.frames)[off]) : ((const float *)a.frames)[off];
    }
    *op = __fdiv_rn(__fsub_rn(v, a.mean), a.stdv);
}

struct VoteArgs {
    const void *cls, *reg, *dep;
    const float *anchors;
    float *votes;
    const float *rows;
    pn_a2j_record *recs;
    int bf16, B, h, w, A, P, K;
    float crop_w, crop_h, fx, fy, cx, cy;
};

__device__ __forceinline__ float ld(const void *p, size_t i, int bf16) {
    if (!bf16) return ((const float *)p)[i];
    return __uint_as_float((unsigned)((const unsigned short *)p)[i] << 16);
}

// The end of a vote, one thread per (crop b, joint p): t = (sum e, sum e (anchor_y + reg_y), sum e (anchor_x + reg_x), sum e dep) -> the voted joint and,
// with records, its map back to the frame
__device__ __forceinline__ void vote_finish(const VoteArgs &a, int b, int p, const float *t) {
    const int P = a.P;
    const float vy = t[1] / t[0], vx = t[2] / t[0], vz = t[3] / t[0];
    if (a.votes) {
        float *o = a.votes + ((size_t)b * P + p) * 3;
        o[0] = vy; o[1] = vx; o[2] = vz;
    }
    if (a.recs && p < PN_NUM_JOINTS) {      // a2j_test_pred_box_new.py:373-394, float32 as numpy computes it
        const float *r = a.rows + (size_t)b * 6;
        const float x = __fadd_rn(__fdiv_rn(__fmul_rn(vx, __fsub_rn(r[3], r[1])), a.crop_w), r[1]);
        const float y = __fadd_rn(__fdiv_rn(__fmul_rn(vy, __fsub_rn(r[4], r[2])), a.crop_h), r[2]);
        pn_a2j_record &R = a.recs[b];
        R.joint[p][0] = x; R.joint[p][1] = y;
        R.joint[p][2] = __fdiv_rn(__fmul_rn(__fsub_rn(x, a.cx), vz), a.fx);
        R.joint[p][3] = __fdiv_rn(__fmul_rn(__fsub_rn(y, a.cy), vz), a.fy);
        R.joint[p][4] = vz;
        if (p == 0) { R.conf = r[5]; R.frame = fits_int(r[0]) ? (int32_t)r[0] : -1; }      // no cast of a NaN or of a value past an int
    }
}

// blockDim 256, grid (P, B).  Anchor k of the reference's order lives in head row (k / A -> cell (column x = cell / h, row y = cell % h)), anchor k % A.
__global__ __launch_bounds__(256) void a2j_vote_kernel(VoteArgs a) {
    const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int K = a.K, A = a.A, P = a.P;
    __shared__ float red[4][4];
    auto row_of = [&](int k) -> size_t {      // element index of (anchor k, joint 0) within one crop's [.., A, P] head
        if (a.h == 0) return (size_t)k * P;
        const int cell = k / A, an = k - cell * A;
        const int x = cell / a.h, y = cell - x * a.h;
        return ((size_t)(y * a.w + x) * A + an) * P;
    };
    const size_t base = (size_t)b * K * P;
    // pass 1: max of the logits
    float m = -INFINITY;
    for (int k = tid; k < K; k += 256) m = fmaxf(m, ld(a.cls, base + row_of(k) + p, a.bf16));
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) red[tid >> 6][0] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
    __syncthreads();
    // pass 2: sum e, sum e (anchor + reg), sum e dep
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = tid; k < K; k += 256) {
        const size_t r = row_of(k);
        const float e = expf(ld(a.cls, base + r + p, a.bf16) - m);
        const float ry = ld(a.reg, 2 * (base + r + p), a.bf16), rx = ld(a.reg, 2 * (base + r + p) + 1, a.bf16);
        const float d = ld(a.dep, base + r + p, a.bf16);
        s[0] += e;
        s[1] += e * (a.anchors[2 * k] + ry);
        s[2] += e * (a.anchors[2 * k + 1] + rx);
        s[3] += e * d;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        for (int o = 32; o > 0; o >>= 1) s[i] += __shfl_xor(s[i], o);
        if ((tid & 63) == 0) red[tid >> 6][i] = s[i];
    }
    __syncthreads();
    if (tid != 0) return;
    float t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    vote_finish(a, b, p, t);
}

// ---- bf16x3 heads: the vote on [hi | lo] plane pairs ----------------------------------------------------------------------------------
// A head row (one map cell of one crop) is [hi: A * P (x 2) values | lo: the same], bf16; a value is (float)hi + (float)lo, exact in fp32 (|lo| is at
// most half a bf16 ulp of hi, so the sum has 16 significant bits).  One block per crop; a group of TPG = A * P / 8 threads walks the cells, thread t of a
// group owning the same 8 (anchor, joint) slots 8 t .. 8 t + 7 of every cell it visits: per cell it loads 16 B of cls.hi, 16 B of cls.lo, the same of
// dep and 2 x 32 B of reg -- the group's loads of a plane are one contiguous run, hi and lo runs back to back.  Pass 1: per-slot maxima in registers,
// reduced per joint through LDS.  Pass 2: e = expf(c - max) and the four sums per slot in registers, reduced per joint in a fixed order (groups, then
// the A anchors of the joint).  Softmax and sums are fp32 as in a2j_vote_kernel; only the summation order differs.
constexpr int VX3_THREADS = 512;

__device__ __forceinline__ void ld8_pair(const unsigned short *hi, int split, float *v) {
    const uint4 h = *reinterpret_cast<const uint4 *>(hi), l = *reinterpret_cast<const uint4 *>(hi + split);
    const unsigned hw[4] = {h.x, h.y, h.z, h.w}, lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(hw[i] << 16) + __uint_as_float(lw[i] << 16);
        v[2 * i + 1] = __uint_as_float(hw[i] & 0xffff0000u) + __uint_as_float(lw[i] & 0xffff0000u);
    }
}

// blockDim VX3_THREADS, grid (B), dynamic LDS (NG * TPG * 8 + P) floats; (A * P) % 8 == 0 and TPG <= VX3_THREADS (pn_a2j_vote checks both)
__global__ __launch_bounds__(VX3_THREADS) void a2j_vote_x3_kernel(VoteArgs a) {
    extern __shared__ float vsm[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int A = a.A, P = a.P, AP = A * P, h = a.h, w = a.w, cells = h * w;
    const int TPG = AP / 8, NG = VX3_THREADS / TPG;
    const int g = tid / TPG, t = tid - g * TPG, e0 = 8 * t;
    const bool on = g < NG;                                  // the threads behind the last whole group only take part in the barriers
    float *red = vsm, *smax = vsm + NG * AP;                 // red[group][slot], smax[joint]
    const unsigned short *cls = (const unsigned short *)a.cls + (size_t)b * cells * 2 * AP + e0;
    const unsigned short *dep = (const unsigned short *)a.dep + (size_t)b * cells * 2 * AP + e0;
    const unsigned short *reg = (const unsigned short *)a.reg + (size_t)b * cells * 4 * AP + 2 * e0;
    // pass 1: max of the logits of every slot this thread owns
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
    if (on)
        for (int cell = g; cell < cells; cell += NG) {
            float c[8];
            ld8_pair(cls + (size_t)cell * 2 * AP, AP, c);
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], c[j]);
        }
    if (on) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[g * AP + e0 + j] = m[j];
    }
    __syncthreads();
    if (tid < P) {
        float mm = -INFINITY;
        for (int gg = 0; gg < NG; ++gg)
            for (int an = 0; an < A; ++an) mm = fmaxf(mm, red[gg * AP + an * P + tid]);
        smax[tid] = mm;
    }
    __syncthreads();
    // pass 2: sum e, sum e (anchor + reg), sum e dep per slot
    float s[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) s[i][j] = 0.f;
    if (on) {
        float mj[8];
        int anj[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { anj[j] = (e0 + j) / P; mj[j] = smax[(e0 + j) - anj[j] * P]; }
        for (int cell = g; cell < cells; cell += NG) {
            const int y = cell / w, x = cell - y * w;
            const float *an0 = a.anchors + (size_t)(x * h + y) * A * 2;      // the reference's order: cells column by column
            float c[8], d[8], r[16];
            ld8_pair(cls + (size_t)cell * 2 * AP, AP, c);
            ld8_pair(dep + (size_t)cell * 2 * AP, AP, d);
            ld8_pair(reg + (size_t)cell * 4 * AP, 2 * AP, r);
            ld8_pair(reg + (size_t)cell * 4 * AP + 8, 2 * AP, r + 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float e = expf(c[j] - mj[j]);
                s[0][j] += e;
                s[1][j] += e * (an0[2 * anj[j]] + r[2 * j]);
                s[2][j] += e * (an0[2 * anj[j] + 1] + r[2 * j + 1]);
                s[3][j] += e * d[j];
            }
        }
    }
    float tsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        __syncthreads();                                     // red is free again
        if (on) {
#pragma unroll
            for (int j = 0; j < 8; ++j) red[g * AP + e0 + j] = s[i][j];
        }
        __syncthreads();
        if (tid < P) {
            float acc = 0.f;
            for (int an = 0; an < A; ++an) {
                float ga = 0.f;
                for (int gg = 0; gg < NG; ++gg) ga += red[gg * AP + an * P + tid];
                acc += ga;
            }
            tsum[i] = acc;
        }
    }
    if (tid < P) vote_finish(a, b, tid, tsum);
}

}  // namespace

extern "C" {

void pn_a2j_cfg_default(pn_a2j_cfg *c) {
    if (!c) return;
    c->img_w = 480; c->img_h = 512; c->crop_w = 288; c->crop_h = 288;
    c->mean = 3.f; c->std = 2.f; c->conf_min = 0.01f;
    c->fx = 504.1189880371094; c->fy = 504.042724609375; c->cx = 231.7421875; c->cy = 320.62640380859375;
}

size_t pn_sizeof_a2j_record(void) { return sizeof(pn_a2j_record); }

int pn_a2j_crop(pn_ctx *ctx, const void *frames_dev, int depth_dtype, int F, int H, int W, const float *rows_dev, int n, const pn_a2j_cfg *cfg,
                float *out_dev, int32_t *flags_dev, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    if (!frames_dev || !rows_dev || !cfg || !out_dev || F < 1 || H < 1 || W < 1 || n < 0)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_crop: bad arguments");
    if (depth_dtype != PN_DEPTH_F16 && depth_dtype != PN_DEPTH_F32) return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_crop: unknown depth dtype %d", depth_dtype);
    if (cfg->crop_w < 1 || cfg->crop_h < 1 || cfg->crop_w > 4096 || cfg->crop_h > 4096 || !(cfg->std != 0.f))
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_crop: crop %dx%d / std %g", cfg->crop_w, cfg->crop_h, (double)cfg->std);
    if ((size_t)F * H * W >= ((size_t)1 << 40) || n > 65535) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "pn_a2j_crop: more than 65535 rows in one call");
    if (n == 0) return PN_OK;
    CropArgs a;
    a.frames = frames_dev; a.rows = rows_dev; a.out = out_dev; a.flags = flags_dev;
    a.f16 = depth_dtype == PN_DEPTH_F16; a.F = F; a.H = H; a.W = W; a.n = n;
    a.img_w = cfg->img_w; a.img_h = cfg->img_h; a.cw = cfg->crop_w; a.ch = cfg->crop_h;
    a.mean = cfg->mean; a.stdv = cfg->std; a.conf_min = cfg->conf_min;
    hipLaunchKernelGGL(a2j_crop_kernel, dim3((a.cw * a.ch + 255) / 256, n), dim3(256), 0, (hipStream_t)hip_stream, a);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_a2j_vote(pn_ctx *ctx, const void *cls_dev, const void *reg_dev, const void *dep_dev, int precision, int B, int h, int w, int A, int P,
                const float *anchors_dev, float *votes_dev, const float *rows_dev, const pn_a2j_cfg *cfg, pn_a2j_record *records_dev, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    if (!cls_dev || !reg_dev || !dep_dev || !anchors_dev || B < 0 || h < 0 || w < 1 || A < 1 || P < 1 || (!votes_dev && !records_dev))
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_vote: bad arguments");
    if (precision != PN_PREC_F32 && precision != PN_PREC_BF16 && precision != PN_PREC_BF16X3) return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_vote: heads are f32, bf16 or bf16x3");
    if (h == 0 && precision != PN_PREC_F32) return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_vote: the [B, K, P] entry takes f32 tensors");
    if (records_dev && (!rows_dev || !cfg || P != PN_NUM_JOINTS)) return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_vote: records need the box rows, a configuration and %d joints", PN_NUM_JOINTS);
    const long K = h ? (long)h * w * A : (long)w;
    if (K < 1 || K * P * 2 >= (1L << 31) || B > 65535 || P > 65535) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "pn_a2j_vote: %ld anchors x %d joints", K, P);
    if (B == 0) return PN_OK;
    VoteArgs a;
    a.cls = cls_dev; a.reg = reg_dev; a.dep = dep_dev; a.anchors = anchors_dev; a.votes = votes_dev; a.rows = rows_dev; a.recs = records_dev;
    a.bf16 = precision == PN_PREC_BF16; a.B = B; a.h = h; a.w = w; a.A = A; a.P = P; a.K = (int)K;
    a.crop_w = cfg ? (float)cfg->crop_w : 1.f; a.crop_h = cfg ? (float)cfg->crop_h : 1.f;
    a.fx = cfg ? (float)cfg->fx : 1.f; a.fy = cfg ? (float)cfg->fy : 1.f; a.cx = cfg ? (float)cfg->cx : 0.f; a.cy = cfg ? (float)cfg->cy : 0.f;
    if (precision == PN_PREC_BF16X3) {
        // 16-byte pieces of a plane, a group of A * P / 8 threads per cell, one thread per joint at the end
        if ((A * P) % 8 || A * P / 8 > VX3_THREADS || P > VX3_THREADS)
            return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "pn_a2j_vote: bf16x3 head rows of %d x %d values (A x P must be a multiple of 8, at most %d; P at most %d)", A, P, 8 * VX3_THREADS, VX3_THREADS);
        const int groups = VX3_THREADS / (A * P / 8);
        hipLaunchKernelGGL(a2j_vote_x3_kernel, dim3(B), dim3(VX3_THREADS), ((size_t)groups * A * P + P) * sizeof(float), (hipStream_t)hip_stream, a);
    } else {
        hipLaunchKernelGGL(a2j_vote_kernel, dim3(P, B), dim3(256), 0, (hipStream_t)hip_stream, a);
    }
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

}  // extern "C"
