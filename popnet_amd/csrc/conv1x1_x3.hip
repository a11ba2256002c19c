// 1x1, stride-1, pad-0 training convolutions in split bf16 on the bf16 matrix cores: pn_conv1x1_x3_forward / _dgrad / _wgrad and
// pn_conv1x1_x3_plan_info (contract: include/popnet_hip.h; kernels and arithmetic: conv1x1_x3_kernels.h).  Entries of their OWN: the
// pn_conv2d_* entries keep sending every 1x1 call to the fp32 kernels whatever the precision, and only A2JTrainEngine(precision="bf16x3")
// calls these.  One planner per role decides kernel, grid and slices; the launch code and pn_conv1x1_x3_plan_info both call it.
// Weight packs ([hi | lo], and the transpose for the data gradient) live in the context's pack cache under the kind PN_PACK_C1_X3
// (pn_train_pack_refresh rebuilds them in its one launch, pn_adam / pn_sgd_nesterov mark them stale); with the cache off they are packed
// per call into the training scratch.
#include <cstdio>
#include "pn_internal.h"
#include "conv1x1_x3_kernels.h"

struct C1Plan {
    const char *kernel;
    unsigned grid[3];
    int chunks;                  // forward / dgrad: k chunks of 32; wgrad: pixel chunks in all
    int cpi, per, slices, csl;   // wgrad: chunks per image, chunks per slice, slices, the bias gradient's slices
    bool aligned;                // wgrad: rows start 16-byte aligned in aligned tensors (HW % 4 == 0)
};

// forward (M = Cout, K = Cin) and data gradient (M = Cin, K = Cout)
static bool c1_plan_gemm(int N, int K, int HW, int M, C1Plan *p) {
    const long P = (long)N * HW;
    if (P > 0x7fffffffL - C1_BN || (long)K * HW > 0x7fffffffL || (long)M * HW > 0x7fffffffL) return false;
    *p = C1Plan{};
    p->kernel = "conv1x1_x3_kernel";
    p->grid[0] = (unsigned)((P + C1_BN - 1) / C1_BN);
    p->grid[1] = (unsigned)((M + C1_BM - 1) / C1_BM);
    p->grid[2] = 1;
    p->chunks = (K + C1_BK - 1) / C1_BK;
    return p->grid[1] <= 65535 && (long)p->grid[0] * p->grid[1] <= 0x7fffffffL;          // (t_logical_block computes the block count in an int)
}

// weight gradient: enough slices of whole 32-pixel chunks to fill the chip, at least C1_MIN_CHUNKS chunks each (the second launch reads every
// slice once per element: many short slices cost more there than they win here), rebalanced so that none is empty
#define C1_MIN_CHUNKS 16
static bool c1_plan_wgrad(pn_ctx *ctx, int N, int Cin, int HW, int Cout, C1Plan *p) {
    *p = C1Plan{};
    const long cpi = (HW + C1_BK - 1) / C1_BK, total = (long)N * cpi;
    if (total > 0x7fffffffL || (long)N * HW > 0x7fffffffL || (long)Cout * Cin > 0x7fffffffL) return false;
    const long tiles = (long)((Cin + C1_BN - 1) / C1_BN) * ((Cout + C1_BM - 1) / C1_BM);
    long s = (1024 + tiles - 1) / tiles;
    const long cap = (total + C1_MIN_CHUNKS - 1) / C1_MIN_CHUNKS;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    const long per = (total + s - 1) / s;
    p->aligned = (HW & 3) == 0;
    p->kernel = p->aligned ? "conv1x1_wgrad_x3_kernel<vec>" : "conv1x1_wgrad_x3_kernel<scalar>";
    p->cpi = (int)cpi;
    p->chunks = (int)total;
    p->per = (int)per;
    p->slices = (int)((total + per - 1) / per);
    p->csl = pn_train_reduce_slices(ctx, N, Cout, HW);
    p->grid[0] = (unsigned)((Cin + C1_BN - 1) / C1_BN);
    p->grid[1] = (unsigned)((Cout + C1_BM - 1) / C1_BM);
    p->grid[2] = (unsigned)p->slices;
    return p->grid[1] <= 65535 && p->grid[2] <= 65535 && (long)p->grid[0] * p->grid[1] * p->grid[2] <= 0x7fffffffL && p->csl >= 1;
}

// y[n][m][p] (+)= bias[m] + sum_k w'[m][k] x[n][k][p] with w' = w (flip 0, w is [M][K]) or its transpose (flip 1, w is [K][M])
static int c1_gemm(pn_ctx *ctx, const char *who, const float *x, const float *w, const float *bias, float *y, int N, int K, int HW, int M, int flip,
                   int accumulate, hipStream_t s) {
    C1Plan plan;
    if (!c1_plan_gemm(N, K, HW, M, &plan)) return pn_set_error(ctx, PN_ERR_INVALID, "%s: size out of range", who);
    void *wp = nullptr;
    bool fresh = false;
    if (int rc = pn_train_pack_get(ctx, w, M, K, flip, PN_PACK_C1_X3, s, &wp, &fresh)) return rc;
    if (!fresh) hipLaunchKernelGGL(conv1x1_wpack_x3_kernel, dim3(t_pack_blocks(PN_PACK_C1_X3, M, K)), dim3(256), 0, s, w, (__bf16 *)wp, M, K, flip);
    C1Gemm c;
    c.x = x; c.wp = (const __bf16 *)wp; c.bias = bias; c.y = y;
    c.N = N; c.K = K; c.HW = HW; c.M = M; c.accumulate = accumulate; c.P = N * HW;
    hipLaunchKernelGGL(conv1x1_x3_kernel, dim3(plan.grid[0], plan.grid[1]), dim3(256), 0, s, c);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

extern "C" {

int pn_conv1x1_x3_forward(pn_ctx *ctx, const float *x_dev, const float *w_dev, const float *bias_dev, float *y_dev, int N, int Cin, int HW, int Cout,
                          int accumulate, void *hip_stream) {
    PN_CTX_CHECK
    if (!x_dev || !w_dev || !y_dev || N < 1 || Cin < 1 || HW < 1 || Cout < 1)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv1x1_x3_forward: bad arguments");
    return c1_gemm(ctx, "pn_conv1x1_x3_forward", x_dev, w_dev, bias_dev, y_dev, N, Cin, HW, Cout, 0, accumulate, (hipStream_t)hip_stream);
}

int pn_conv1x1_x3_dgrad(pn_ctx *ctx, const float *dy_dev, const float *w_dev, float *dx_dev, int N, int Cin, int HW, int Cout, int accumulate,
                        void *hip_stream) {
    PN_CTX_CHECK
    if (!dy_dev || !w_dev || !dx_dev || N < 1 || Cin < 1 || HW < 1 || Cout < 1)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv1x1_x3_dgrad: bad arguments");
    return c1_gemm(ctx, "pn_conv1x1_x3_dgrad", dy_dev, w_dev, nullptr, dx_dev, N, Cout, HW, Cin, 1, accumulate, (hipStream_t)hip_stream);
}

int pn_conv1x1_x3_wgrad(pn_ctx *ctx, const float *x_dev, const float *dy_dev, float *dw_dev, float *dbias_dev, int N, int Cin, int HW, int Cout,
                        void *hip_stream) {
    PN_CTX_CHECK
    if (!x_dev || !dy_dev || !dw_dev || N < 1 || Cin < 1 || HW < 1 || Cout < 1)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv1x1_x3_wgrad: bad arguments");
    C1Plan plan;
    if (!c1_plan_wgrad(ctx, N, Cin, HW, Cout, &plan)) return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv1x1_x3_wgrad: size out of range");
    hipStream_t s = (hipStream_t)hip_stream;
    // scratch: the slices' partial sums, then (16-byte aligned) the bias gradient's double partials
    const size_t wn = (size_t)Cout * Cin;
    const size_t part_off = (wn * (size_t)plan.slices * sizeof(float) + 15) & ~(size_t)15;
    void *ws = nullptr;
    if (int rc = pn_train_ws(ctx, part_off + (size_t)Cout * plan.csl * 2 * sizeof(double), &ws)) return rc;
    C1Wgrad c;
    c.x = x_dev; c.dy = dy_dev; c.partial = (float *)ws;
    c.N = N; c.Cin = Cin; c.HW = HW; c.Cout = Cout; c.cpi = plan.cpi; c.total = plan.chunks; c.per = plan.per;
    const dim3 grid(plan.grid[0], plan.grid[1], plan.grid[2]);
    // 16-byte loads only where every whole group of a row is aligned: HW % 4 == 0 AND both tensors 16-byte aligned
    if (plan.aligned && ((((size_t)x_dev) | ((size_t)dy_dev)) & 15) == 0) hipLaunchKernelGGL(conv1x1_wgrad_x3_kernel<true>, grid, dim3(256), 0, s, c);
    else hipLaunchKernelGGL(conv1x1_wgrad_x3_kernel<false>, grid, dim3(256), 0, s, c);
    pn_train_wgrad_reduce(s, (const float *)ws, dw_dev, wn, plan.slices);       // (wn <= INT_MAX: c1_plan_wgrad)
    if (dbias_dev) pn_train_dbias(s, dy_dev, dbias_dev, N, Cout, HW, plan.csl, (double *)((char *)ws + part_off));
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

int pn_conv1x1_x3_plan_info(pn_ctx *ctx, int which, int N, int Cin, int HW, int Cout, char *out, size_t cap) {
    if (!ctx) return PN_ERR_INVALID;
    if (!out || N < 1 || Cin < 1 || HW < 1 || Cout < 1 || (which != PN_PLAN_FORWARD && which != PN_PLAN_DGRAD && which != PN_PLAN_WGRAD))
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv1x1_x3_plan_info: bad arguments");
    C1Plan p;
    int n;
    if (which == PN_PLAN_WGRAD) {
        if (!c1_plan_wgrad(ctx, N, Cin, HW, Cout, &p)) return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv1x1_x3_plan_info: size out of range");
        n = snprintf(out, cap,
                     "{\"kernel\": \"%s\", \"split\": true, \"BM\": %d, \"BN\": %d, \"BK\": %d, \"grid\": [%u, %u, %u], \"lds\": %d, \"slices\": %d, "
                     "\"per_slice\": %d, \"per_slice_unit\": \"pixels\", \"per_slice_chunks\": %d, \"chunks\": %d, \"chunks_per_image\": %d, "
                     "\"aligned\": %s, \"csl\": %d}",
                     p.kernel, C1_BM, C1_BN, C1_BK, p.grid[0], p.grid[1], p.grid[2], C1_LDS, p.slices, p.per * C1_BK, p.per, p.chunks, p.cpi,
                     p.aligned ? "true" : "false", p.csl);
    } else {
        const bool dg = which == PN_PLAN_DGRAD;
        const int M = dg ? Cin : Cout, K = dg ? Cout : Cin;
        if (!c1_plan_gemm(N, K, HW, M, &p)) return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv1x1_x3_plan_info: size out of range");
        n = snprintf(out, cap,
                     "{\"kernel\": \"%s\", \"split\": true, \"BM\": %d, \"BN\": %d, \"BK\": %d, \"grid\": [%u, %u, %u], \"lds\": %d, \"M\": %d, \"K\": %d, "
                     "\"P\": %ld, \"chunks\": %d, \"pack\": \"%s\"}",
                     p.kernel, C1_BM, C1_BN, C1_BK, p.grid[0], p.grid[1], p.grid[2], C1_LDS, M, K, (long)N * HW, p.chunks, dg ? "transposed" : "plain");
    }
    if (n < 0 || (size_t)n + 1 > cap) return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv1x1_x3_plan_info: %d bytes needed", n + 1);
    return PN_OK;
}

}   // extern "C"
