// Launch dispatch of the MFMA convolution (kernel template: conv_mfma_kernel.h).  The
// instantiations -- {3x3, 1x1} x {stride 1, 2} x LDS pitch class {16, 32, 64, 120 pixels} x tile
// configuration x {bf16, f32} -- are spread over conv_inst_*.hip so they compile in parallel; which of them exist
// is listed once, in conv_inst_table.h.
#include "pn_internal.h"
#include "conv_inst_table.h"

int pn_cfg_couts(int cfg) {
    switch (cfg) {
        case PN_CFG_C128: return 128;
        case PN_CFG_C64: return 64;
        case PN_CFG_C64W: return 64;
        case PN_CFG_C32: return 32;
        default: return 16;
    }
}


int pn_cfg_pixels(int cfg) { return cfg == PN_CFG_C128 ? 112 : (cfg == PN_CFG_C64W ? 224 : 128); }

size_t pn_conv_lds_bytes(int prec, int ks, int stride, int pitch, int R, int dil) {
    size_t pixb = prec == PN_PREC_BF16 ? 128 : 256;
    size_t rows = (size_t)(R - 1) * stride + (size_t)(ks - 1) * dil + 1;
    return rows * pitch * pixb;
}

// Is conv_mfma_kernel<prec, ks, stride, pitch, cfg> built?  The same rows as the dispatch below (conv_inst_table.h).
extern "C" int pn_conv_has_instance(int prec, int ks, int stride, int pitch, int cfg) {
    if (prec != PN_PREC_BF16 && prec != PN_PREC_F32) return 0;
#define PN_HAS_CASE(KS, ST, PITCH, CFG) \
    if (ks == KS && stride == ST && pitch == PITCH && cfg == CFG) return 1;
    PN_CONV_INSTANCES(PN_HAS_CASE)
#undef PN_HAS_CASE
    return 0;
}

// the dilation-2 rows of the table
int pn_conv_has_instance_d2(int prec, int ks, int stride, int pitch, int cfg) {
    if (prec != PN_PREC_BF16 && prec != PN_PREC_F32) return 0;
#define PN_HAS_CASE(KS, ST, PITCH, CFG) \
    if (ks == KS && stride == ST && pitch == PITCH && cfg == CFG) return 1;
    PN_CONV_INSTANCES_D2(PN_HAS_CASE)
#undef PN_HAS_CASE
    return 0;
}

int pn_launch_conv_part0(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_d2_part0(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_d2_part1(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_acc_part0(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_acc_part1(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_acc_part2(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_part1(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_part2(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_part3(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);

int pn_launch_conv(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream) {
    int rc;
    if (L.kern == 4) return pn_launch_conv4(ctx, L, stream);
    if (L.kern == 3) return pn_launch_conv3(ctx, L, stream);
    if (L.acc) {      // fp32 blocked accumulation: the same rows, instances of their own
        if (L.prec == PN_PREC_F32 && (L.dil == 1 || L.dil == 2)) {
            if ((rc = pn_launch_conv_acc_part0(ctx, L, stream)) != 1) return rc;
            if ((rc = pn_launch_conv_acc_part1(ctx, L, stream)) != 1) return rc;
            if ((rc = pn_launch_conv_acc_part2(ctx, L, stream)) != 1) return rc;
        }
        return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "no blocked-accumulation conv kernel for prec=%d ks=%d stride=%d dilation=%d pitch=%d cfg=%d", L.prec, L.ks, L.stride, L.dil, L.pitch, L.cfg);
    }
    if (L.dil != 1) {
        if (L.dil == 2 && (rc = pn_launch_conv_d2_part0(ctx, L, stream)) != 1) return rc;
        if (L.dil == 2 && (rc = pn_launch_conv_d2_part1(ctx, L, stream)) != 1) return rc;
        return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "no conv kernel for prec=%d ks=%d stride=%d dilation=%d pitch=%d cfg=%d", L.prec, L.ks, L.stride, L.dil, L.pitch, L.cfg);
    }
    if ((rc = pn_launch_conv_part0(ctx, L, stream)) != 1) return rc;
    if ((rc = pn_launch_conv_part1(ctx, L, stream)) != 1) return rc;
    if ((rc = pn_launch_conv_part2(ctx, L, stream)) != 1) return rc;
    if ((rc = pn_launch_conv_part3(ctx, L, stream)) != 1) return rc;
    return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "no conv kernel for prec=%d ks=%d stride=%d pitch=%d cfg=%d", L.prec, L.ks,
                        L.stride, L.pitch, L.cfg);
}

// host mirror of StageCfg (conv_mfma_kernel.h): largest halo tile (pixels) the register-prefetched
// staging path of this instantiation can hold; 0 = that instantiation stages with the plain loop.
int pn_conv_stage_maxpx(int prec, int ks, int stride, int pitch, int cfg) {
    if (cfg == PN_CFG_C64W) return 0;
    const int maxpx = stride != 1 ? 0 : (ks == 1 ? 128 : (pitch <= 32 ? 192 : (pitch <= 64 ? 288 : 360)));
    const int nch = prec == PN_PREC_BF16 ? 8 : 16;
    const int raw = (maxpx * nch + 255) / 256;
    return raw <= 12 ? maxpx : 0;
}
