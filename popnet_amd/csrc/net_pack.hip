// Reference state_dict -> host images: the BatchNorm fold and every weight pack of the inference nets (host code only, no HIP call).
// BatchNorm (eval, eps 1e-5) is folded into the preceding convolution: w' = w * g / sqrt(var + eps),  b' = (b - mean) * g / sqrt(var + eps) + beta.
#include <cmath>
#include "net_internal.h"

namespace pnnet {
namespace {
// Folded weight scale of `cout` output channels, and their folded bias as an f32 image of `pad` values.  bias_of: "<prefix>" of an optional
// "<prefix>.bias", or "" for no convolution bias; bn: BatchNorm prefix or "".
int fold_bn(pn_net *n, const std::string &bias_of, const std::string &bn, int cout, int pad, std::vector<double> &scale, int &bias_image) {
    pn_ctx *ctx = n->ctx;
    std::vector<double> shift(cout, 0.0);
    scale.assign(cout, 1.0);
    const HostTensor *bias = bias_of.empty() ? nullptr : find_t(n, bias_of + ".bias");
    if (bias && (int)bias->numel() != cout) return pn_set_error(ctx, PN_ERR_INVALID, "%s.bias: bad size", bias_of.c_str());
    for (int o = 0; o < cout; ++o) shift[o] = bias ? bias->data[o] : 0.0;
    if (!bn.empty()) {
        const HostTensor *g = find_t(n, bn + ".weight"), *be = find_t(n, bn + ".bias");
        const HostTensor *mu = find_t(n, bn + ".running_mean"), *var = find_t(n, bn + ".running_var");
        if (!g || !be || !mu || !var || (int)g->numel() != cout || (int)be->numel() != cout ||
            (int)mu->numel() != cout || (int)var->numel() != cout)
            return pn_set_error(ctx, PN_ERR_INVALID, "missing/ill-shaped BatchNorm tensors %s.*", bn.c_str());
        for (int o = 0; o < cout; ++o) {
            double s = (double)g->data[o] / std::sqrt((double)var->data[o] + 1e-5);
            scale[o] = s;
            shift[o] = (shift[o] - (double)mu->data[o]) * s + (double)be->data[o];
        }
    }
    std::vector<float> hb(pad, 0.f);
    for (int o = 0; o < cout; ++o) hb[o] = (float)shift[o];
    bias_image = add_image(n, hb.data(), hb.size() * 4);
    return PN_OK;
}

// bf16x3 splits a weight into hi = bf16(v) and lo = v - hi (rounded to bf16 when it is stored)
inline float split_part(float v, int lo) {
    const float hi = pn_bf16_to_f32(pn_f32_to_bf16(v));
    return lo ? v - hi : hi;
}

// One MFMA A-fragment (conv_mfma_kernel.h): 64 lanes x 8 values, lane l = row l & 15 of cout tile `tile` (rows permuted over the `ct` tiles a wave owns:
// pn_conv_row_channel), its values at packed input channels kbase + 8 (l >> 4) + j; weight(co, ci) is the folded value.  bf16: dst[lane][8]; f32: two halves of [lane][4].
template <class F> void write_frag(void *dst, bool f32, int tile, int ct, int kbase, F weight) {
    for (int lane = 0; lane < 64; ++lane) {
        const int co = pn_conv_row_channel(tile, lane & 15, ct), q = lane >> 4;
        for (int j = 0; j < 8; ++j) {
            const float v = weight(co, kbase + 8 * q + j);
            if (f32) ((float *)dst)[(size_t)(j >> 2) * 256 + lane * 4 + (j & 3)] = v;
            else ((uint16_t *)dst)[lane * 8 + j] = pn_f32_to_bf16(v);
        }
    }
}
}  // namespace

// Fold BN, permute/pad input channels, plan the launch (conv_plan.h), pack into MFMA A-fragment order.
int prepare_conv(pn_net *n, ConvSpec &cs) {
    pn_ctx *ctx = n->ctx;
    const HostTensor *w = find_t(n, cs.w + ".weight");
    if (!w || w->shape.size() != 4)
        return pn_set_error(ctx, PN_ERR_INVALID, "missing conv weight %s.weight", cs.w.c_str());
    const int cout = (int)w->shape[0], cin_ref = (int)w->shape[1], wks = (int)w->shape[2];
    const int ks = cs.embed3 ? 3 : wks;
    if ((cs.embed3 ? wks != 1 : wks != cs.ks) || (int)w->shape[3] != wks || ks != cs.ks)
        return pn_set_error(ctx, PN_ERR_INVALID, "%s.weight: kernel %dx%d, expected %d", cs.w.c_str(), wks, (int)w->shape[3], cs.embed3 ? 1 : cs.ks);
    cs.cout = cout;
    std::vector<int> map = cs.cin_map;
    if (map.empty()) {
        map.resize(cin_ref);
        for (int i = 0; i < cin_ref; ++i) map[i] = i;
    }
    for (int m : map)
        if (m >= cin_ref)
            return pn_set_error(ctx, PN_ERR_INVALID, "%s: input-channel map exceeds Cin=%d", cs.w.c_str(), cin_ref);
    std::vector<int> wsel;                        // bf16x3: which half of the split weight multiplies this input channel (0 = hi, 1 = lo)
    if (n->x3) {
        // the input is the WHOLE buffer, three planes of `plane` channels: [x_hi | x_lo | x_hi] against [W_hi | W_hi | W_lo]
        // = x_hi W_hi + x_lo W_hi + x_hi W_lo (the dropped x_lo W_lo term is 2^-16 of the product)
        const int pc = n->bufs[cs.in_buf].plane;
        if (cs.in_coff != 0 || (int)map.size() > pc)
            return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "%s: bf16x3 convolutions read whole buffers", cs.w.c_str());
        map.resize(pc, -1);
        std::vector<int> m3;
        for (int pl = 0; pl < 3; ++pl)
            for (int i = 0; i < pc; ++i) { m3.push_back(map[i]); wsel.push_back(pl == 2 ? 1 : 0); }
        map.swap(m3);
    }
    const int cin_pad = ((int)map.size() + 63) / 64 * 64;
    map.resize(cin_pad, -1);
    wsel.resize(cin_pad, 0);
    cs.cin_chunks = cin_pad / 64;

    const Buf &ib = n->bufs[cs.in_buf];
    pn_plan_conv_kernel(n->prec, n->max_batch, n->ctx->num_cus, ib.H, ib.W, cout, cs.cin_chunks, cs.wc_min, cs.nbuf_min, cs.k4_level, n->sw, cs);   // which kernel ...
    const int cout_pad = pn_conv_cout_pad(cs, cout);
    std::vector<double> scale;
    if (int rc = fold_bn(n, cs.w, cs.bn, cout, cout_pad, scale, cs.bias)) return rc;
    const int KK = ks * ks;
    const int ksteps = cs.cin_chunks * KK * 2;
    const size_t bytes = pn_conv_pack_bytes(n->prec, cs, cout_pad, ksteps);
    const bool f32 = n->prec != PN_PREC_BF16;
    const size_t frag_bytes = f32 ? 512 * 4 : 512 * 2;
    cs.wpack = add_image(n, nullptr, bytes);
    std::vector<unsigned char> &host = n->images[cs.wpack].host;      // packed in place
    host.assign(bytes, 0);
    // k order of every kernel: (64-channel chunk, 32-channel half, tap); k-step (half-chunk hh, tap) covers packed input channels hh * 32 ...
    auto pack = [&](size_t frag, int tile, int ct, int co0, int hh, int tap) {
        write_frag(host.data() + frag * frag_bytes, f32, tile, ct, hh * 32, [&](int co, int idx) -> float {      // folded weight of packed input channel idx
            const int ci = map[idx];
            co += co0;
            if (co >= cout || ci < 0) return 0.f;
            if (cs.embed3 && tap != 4) return 0.f;
            const float v = (float)((double)w->data[cs.embed3 ? (size_t)co * cin_ref + ci : ((size_t)co * cin_ref + ci) * (ks * ks) + tap] * scale[co]);
            return n->x3 ? split_part(v, wsel[idx]) : v;
        });
    };
    if (cs.kern == 4) {                           // conv4_kernel.h: [cout block of 128][k-step, the spare ones included][8 cout tiles]
        const size_t kstride4 = pn_conv_pack_frags(cs, 128, ksteps) / 8;
        for (int cbk = 0; cbk < cout_pad / 128; ++cbk)
            for (int hh = 0; hh < cs.cin_chunks * 2; ++hh)
                for (int tap = 0; tap < KK; ++tap)
                    for (int t = 0; t < 8; ++t) pack(((size_t)cbk * kstride4 + (size_t)hh * KK + tap) * 8 + t, t, 4, cbk * 128, hh, tap);
    } else {                                      // [cout tile][k-step]
        const int ct_per_wave = cs.kern == 3 ? 2 : pn_cfg_ct(cs.cfg);
        for (int ct = 0; ct < cout_pad / 16; ++ct)
            for (int hh = 0; hh < cs.cin_chunks * 2; ++hh)
                for (int tap = 0; tap < KK; ++tap) pack((size_t)ct * ksteps + (size_t)hh * KK + tap, ct, ct_per_wave, 0, hh, tap);
    }

    // geometry
    const int Ho = (ib.H + 2 * (ks / 2) - ks) / cs.stride + 1, Wo = (ib.W + 2 * (ks / 2) - ks) / cs.stride + 1;
    const char *why = "";
    if (int rc = pn_plan_conv_tiles(n->prec, ib.H, ib.W, cs, &why)) return pn_set_error(ctx, rc, "%s: %s", cs.w.c_str(), why);      // ... on what tiles
    cs.flops = 2.0 * Ho * Wo * (double)cout * cin_ref * (cs.embed3 ? 1 : KK);
    if (cs.out_buf >= 0) {
        const Buf &ob = n->bufs[cs.out_buf];
        if (ob.H != Ho || ob.W != Wo) return pn_set_error(ctx, PN_ERR_INVALID, "%s: output buffer is %dx%d, conv gives %dx%d", cs.w.c_str(), ob.H, ob.W, Ho, Wo);
    }
    return PN_OK;
}

// sum_cin > 1 (build_a2j): the weight is [64, sum_cin, 7, 7] and every input channel is the SAME image (ResNetBackBone.forward expands the depth
// crop to three identical channels, third_party_methods/A2J_experiments/model.py:155-156), so the convolution is the single-channel one with the
// weights summed over Cin -- in double, before the BatchNorm scale -- and runs the fused matrix-core stem.
int pack_stem(pn_net *n, Step &st, const std::string &conv, const std::string &bn, int sum_cin) {
    pn_ctx *ctx = n->ctx;
    const HostTensor *w = find_t(n, conv + ".weight");
    if (!w || w->shape.size() != 4 || w->shape[0] != 64 || w->shape[1] != (sum_cin > 1 ? sum_cin : n->input_dim) || w->shape[2] != 7 || w->shape[3] != 7)
        return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "%s.weight must be [64,%d,7,7] (input_dim = %d)", conv.c_str(), sum_cin > 1 ? sum_cin : n->input_dim, n->input_dim);
    std::vector<double> scale;
    if (int rc = fold_bn(n, "", bn, 64, 64, scale, st.stem_b)) return rc;      // the stems have no convolution bias
    if (n->input_dim != 1) {
        // multi-channel input (the reference constructors default to input_dim = 3, rtpose_light3d.py:250 / yolo_posenet.py:88): the folded
        // 7x7 convolution runs on the generic fp32 primitive (pn_conv2d_forward, any Cin), its NCHW map is handed to the NHWC layers by
        // nchw_relu_to_nhwc_kernel.  The depth path (input_dim = 1) keeps its fused matrix-core stem.
        const int cin = n->input_dim;
        std::vector<float> hw((size_t)64 * cin * 49);
        for (int o = 0; o < 64; ++o)
            for (int i = 0; i < cin * 49; ++i) hw[(size_t)o * cin * 49 + i] = (float)((double)w->data[(size_t)o * cin * 49 + i] * scale[o]);
        st.stem_cin = cin;
        st.stem_w = add_image(n, hw);
        const Buf &ob = n->bufs[st.out_buf];
        st.stem_scratch = add_image(n, nullptr, (size_t)n->max_batch * 64 * ob.H * ob.W * 4);
        return PN_OK;
    }
    auto wd = [&](int o, int t) -> double {      // the weight the stem folds, in double
        if (sum_cin <= 1) return (double)w->data[o * 49 + t];
        double s = 0;
        for (int c = 0; c < sum_cin; ++c) s += (double)w->data[((size_t)o * sum_cin + c) * 49 + t];
        return s;
    };
    std::vector<float> hw(49 * 64);
    for (int o = 0; o < 64; ++o)
        for (int t = 0; t < 49; ++t) hw[t * 64 + o] = (float)(wd(o, t) * scale[o]);
    st.stem_w = add_image(n, hw);
    // 8 A-fragments [cout tile t][k-step s][lane][8]: tile row 4q'+r' <-> cout 16q'+4t+r', k = ky*8 + kx+1 (the stem's own layout)
    std::vector<uint16_t> hf(16 * 64 * 8, 0);     // fragments 8..15: the lo halves of the split weights (bf16x3 mode)
    for (int t = 0; t < 4; ++t)
        for (int s2 = 0; s2 < 2; ++s2)
            for (int lane = 0; lane < 64; ++lane) {
                const int r16 = lane & 15, qa = lane >> 4;
                const int co = 16 * (r16 >> 2) + 4 * t + (r16 & 3);
                const int ky = 4 * s2 + qa;
                for (int j = 0; j < 8; ++j) {
                    float v = 0.f;
                    if (ky < 7 && j >= 1) v = hw[(ky * 7 + (j - 1)) * 64 + co];
                    hf[((t * 2 + s2) * 64 + lane) * 8 + j] = pn_f32_to_bf16(split_part(v, 0));
                    hf[((8 + t * 2 + s2) * 64 + lane) * 8 + j] = pn_f32_to_bf16(split_part(v, 1));
                }
            }
    st.stem_wfrag = add_image(n, hf);
    return PN_OK;
}

// bb64_kernel.h / bb64x3_kernel.h: bf16 [conv][18 k-steps = (half, tap)][4 cout tiles]; bf16x3 [conv][W_hi, W_lo][18 k-steps][4 cout tiles]
int pack_bblock(pn_net *n, Step &st) {
    const int nsel = n->x3 ? 2 : 1;
    std::vector<uint16_t> pk((size_t)36 * nsel * 4 * 64 * 8, 0);
    for (int cv = 0; cv < 2; ++cv) {
        const ConvSpec &cs = n->convs[st.conv_ids[cv]];
        const HostTensor *w = find_t(n, cs.w + ".weight");
        std::vector<double> scale;
        if (int rc = fold_bn(n, cs.w, cs.bn, 64, 64, scale, cv ? st.bb_bias2 : st.bb_bias1)) return rc;
        for (int sel = 0; sel < nsel; ++sel)
            for (int hh = 0; hh < 2; ++hh)
                for (int tap = 0; tap < 9; ++tap)
                    for (int t = 0; t < 4; ++t)
                        write_frag(&pk[((((size_t)cv * nsel + sel) * 18 + hh * 9 + tap) * 4 + t) * 512], false, t, 4, hh * 32, [&](int co, int ci) -> float {
                            const float v = (float)((double)w->data[((size_t)co * 64 + ci) * 9 + tap] * scale[co]);
                            return n->x3 ? split_part(v, sel) : v;
                        });
    }
    st.bb_wpack = add_image(n, pk);
    st.bb_tickets = add_image(n, nullptr, 256);
    return PN_OK;
}

// conv3_kernel.h, TAIL == 1: the fused 1x1 tail's weights [2 cout tiles][4 k-steps] and its bias (no BatchNorm: fuse_1x1_tails admits none)
int pack_tail(pn_net *n, ConvSpec &a) {
    const ConvSpec &b = n->convs[a.tail_conv];
    const HostTensor *w = find_t(n, b.w + ".weight");
    const int cout = (int)w->shape[0];
    std::vector<uint16_t> pk((size_t)2 * 4 * 64 * 8, 0);
    for (int t = 0; t < 2; ++t)
        for (int ks = 0; ks < 4; ++ks)
            write_frag(&pk[((size_t)t * 4 + ks) * 512], false, t, 2, ks * 32, [&](int co, int ci) { return co < cout ? w->data[(size_t)co * 128 + ci] : 0.f; });
    a.tail_wpack = add_image(n, pk);
    std::vector<double> unit;
    return fold_bn(n, b.w, "", cout, 32, unit, a.tail_bias);      // its bias alone
}
}  // namespace pnnet
