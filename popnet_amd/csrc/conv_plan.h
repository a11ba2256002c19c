// The convolution launch planner: ONE rule set for the inference nets (net.hip) and the planes training engine (trainx.hip), so a training-mode
// convolution runs exactly the kernel / tiling / launch the inference plan would pick for the same shape (and is covered by the same bit-identity tests).
//   pn_plan_level                              what a level of independent convolutions decides together (conv4 or not, shared 128-cout blocks)
//   pn_plan_conv_kernel / pn_plan_conv_tiles   which kernel runs one convolution, on what tiles
//   pn_conv_block_couts / pn_conv_cout_pad / pn_conv_pack_frags / pn_conv_pack_bytes     the cout block and the size of the weight pack that follow from it
//   pn_conv_same_launch                        may two planned convolutions share a kernel instantiation (one launch, blockIdx.y = problem)
//   pn_fill_conv_problem / pn_fill_conv_launch the geometry fields of the device descriptors
// What stays with the callers: where weights, biases and tensors live, the epilogue (act, residual, NCHW copy), and the nets' fused tails / pools / mixed launches.
#pragma once
#include <algorithm>
#include <vector>
#include "pn_internal.h"

struct ConvGeom {
    int ks = 3, stride = 1;                             // set by the caller; everything below is planned
    int dil = 1;                                        // set by the caller: tap distance (2: A2J's dilated layer4 blocks, generic kernel only)
    int acc = 0;                                        // set by the caller: 1 = fp32 blocked accumulation (the A2J net in fp32; generic kernel, which is all fp32 runs)
    int kern = 0, cfg = 0, pitch = 0, R = 0, Wt = 0;
    int wc = 0, wp = 0, nbuf = 0, pt = 7, rpg = 4;      // kern 3: conv3_kernel<ks, wc, wp, nbuf, pt, rpg>
};

inline int pn_pick_pitch(int cols) {
    const int classes[4] = {16, 32, 64, 120};
    for (int c : classes)
        if (cols <= c) return c;
    return -1;
}

inline int pn_pick_cfg(int cout) {
    if (cout % 128 == 0) return PN_CFG_C128;
    if (cout >= 64) return PN_CFG_C64;
    if (cout <= 16) return PN_CFG_C16;
    return PN_CFG_C32;
}

// One convolution of a level of independent convolutions (the three branches of a stage; a BasicBlock's 3x3 and its 1x1 shortcut).  In: the input map,
// rows = output channels (a data gradient: its output plane), ks / stride, cin_gt64 = more than one 64-channel chunk of input.  Out: what the level decided.
struct PnLevelConv {
    int H, W, rows, ks, stride;
    bool cin_gt64;
    int k4_level = 0, wc_min = 0, nbuf_min = 0;
};

// conv4: PnSwitches::conv4 (-1 by block count, 0 never, 1 whenever eligible).
inline void pn_plan_level(std::vector<PnLevelConv> &lv, int max_batch, bool x3, int conv4) {
    // conv4_kernel: the level has a stride-1 3x3 conv with >= 64 couts and Cin >= 128 (bf16x3: any Cin -- three plane pairs).  Its 128-cout x 224-pixel
    // blocks need >= 2 per CU to pay (profiles/README.md r02: level of 448 blocks 37.5 vs 40.4 us, level of 224 blocks 18.5 vs 12.5 us against
    // conv3_kernel): by block count = when the level's 3x3 convs make at least 448 such blocks at max_batch
    bool k4 = false;
    long blocks = 0;
    for (const PnLevelConv &c : lv) {
        if (c.ks != 3 || c.stride != 1 || c.rows < 64) continue;
        if (x3 || c.cin_gt64) k4 = true;
        const long strips = (long)max_batch * ((c.H + 3) / 4) * ((c.W + 29) / 30);
        blocks += ((strips + 1) / 2) * ((c.rows + 127) / 128);
    }
    if (conv4 < 0 ? blocks < 448 : conv4 == 0) k4 = false;
    for (PnLevelConv &c : lv) c.k4_level = k4 ? 1 : 0;
    // a 33..64-cout conv next to a wider sibling of the same kernel size takes the sibling's 128-cout block (its two surplus waves only help with the
    // halo DMA, conv3_kernel.h) and the double-buffered variant -- one launch instead of two
    for (int ks : {1, 3}) {
        bool wide = false, multi = false;
        for (const PnLevelConv &c : lv) {
            if (c.ks != ks || c.stride != 1) continue;
            if (c.rows > 64) wide = true;
            if (c.cin_gt64) multi = true;
        }
        if (!wide) continue;
        for (PnLevelConv &c : lv) {
            if (c.ks != ks || c.stride != 1 || c.rows <= 32) continue;
            c.wc_min = 4;
            if (multi) c.nbuf_min = 2;
        }
    }
}

// prec: PN_PREC_BF16 for the bf16 / bf16x3 nets, PN_PREC_F32 otherwise.  H, W: input map; the caller has set g.ks / g.stride (g.pt / g.rpg at their
// defaults 7 / 4).  wc_min / nbuf_min / k4_level: what pn_plan_level decided for the level this convolution belongs to (0 for a convolution planned
// alone).  sw: the switches of the net or trainer being compiled.
inline void pn_plan_conv_kernel(int prec, int max_batch, int num_cus, int H, int W, int cout, int cin_chunks, int wc_min, int nbuf_min, int k4_level,
                                const PnSwitches &sw, ConvGeom &g) {
    const int ks = g.ks, stride = g.stride;
    g.cfg = pn_pick_cfg(cout);
    {   // bf16 stride-1 layers run conv3_kernel (conv3_kernel.h) when the map splits into column strips (<= 30 wide: the
        // halo row is 32 pixels) whose 4-row tiles fill >= 75 % of a wave group's 112 pixel slots
        int segs = 0, wt = 0, rows = 0, rpg = 4;
        double best = 0;
        for (int sg = (W + 29) / 30; sg <= (W + 15) / 16; ++sg) {
            const int w = (W + sg - 1) / sg;
            for (int gg : {4, 8}) {                      // rows per wave group kept in LDS (8: narrow maps only, 3x3 / 128-cout blocks)
                if (gg == 8 && !(w <= 14 && ks == 3 && cout > 64 && sw.conv3_rpg8)) continue;   // measured slower than the generic kernel on 14x14 maps (profiles/README.md v15)
                const int r = std::min(std::min(H, gg), 112 / w);
                const double util = r * ((double)W / sg) / 112.0;
                if (util > best + 1e-9) { best = util; segs = sg; wt = w; rows = r; rpg = gg; }
            }
        }
        // (cout > 32: the <= 32-cout heads stay on the generic kernel -- on conv3_kernel<3, 1, 1, 1> the two head launches took 64 us per step against 25, round 6)
        if (prec == PN_PREC_BF16 && stride == 1 && (ks == 3 || ks == 1) && best >= 0.75 && cout > 32 && !sw.no_conv3 && g.dil == 1) {
            g.kern = 3;
            g.wc = std::max(cout > 64 ? 4 : (cout > 32 ? 2 : 1), wc_min);
            const long tiles112 = (long)max_batch * ((H + rows - 1) / rows) * segs;   // strip tiles of one wave group
            g.wp = (g.wc == 2 && rows == 4 && rpg == 4 && tiles112 * ((cout + 63) / 64) >= 1536) ? 2 : 1;   // big maps: 8-row tiles, 256 threads
            g.rpg = rpg;
            if (g.wp == 2 && ks == 3 && cin_chunks == 1 && sw.conv3_pt14 == 1) { g.wp = 1; g.pt = 14; g.rpg = 8; }   // 8 rows per WAVE: half the weight bytes
            // =2: 128-cout blocks of 224-pixel wave tiles on every 28-column 3x3 level as well
            if (sw.conv3_pt14 == 2 && ks == 3 && g.wc == 4 && g.wp == 1 && rpg == 4 && rows == 4 && H >= 8) { g.pt = 14; g.rpg = 8; }
            const int hr = rpg * g.wp + ks - 1, ngw = (8 * (hr / 2) + g.wc * g.wp - 1) / (g.wc * g.wp);
            // single halo image (4 waves / SIMD) beats the double-buffered variant (3 waves / SIMD) on every level
            // of both networks (profiles/README.md, r01 v8); POPNET_CONV3_NBUF2=1 selects the latter for experiments
            g.nbuf = ((cin_chunks > 1 || nbuf_min == 2) && ks == 3 && ngw <= 18 && sw.conv3_nbuf2) ? 2 : 1;
            g.Wt = wt;
            g.R = std::min(H, rows * g.wp * (g.pt / 7));          // rows * Wt <= 112 (224) pixel slots per wave group
            // conv4_kernel (both operands through LDS, 64-cout x 112-pixel wave tiles): the 3x3 layers with Cin >= 128 and
            // >= 64 couts on 4-row strip tiles; a Cin = 64 conv joins only as the sibling of such a layer (one launch per level)
            if (ks == 3 && g.wp == 1 && g.pt == 7 && g.rpg == 4 && cout >= 64 && k4_level)
                g.kern = 4;
        }
    }
    // Small maps on the generic kernel (YoloPoseNet's 14 x 14 levels: 2 tiles per frame): 128-cout blocks give fewer blocks than the chip
    // has CUs (128 at B = 32) -- 64-cout x 128-pixel blocks double them.  POPNET_GENERIC_C64=0 keeps the 128-cout blocks.
    if (g.kern == 0 && prec == PN_PREC_BF16 && g.cfg == PN_CFG_C128 && stride == 1) {
        const long blocks128 = (long)max_batch * ((H * W + 111) / 112) * (cout / 128);
        if (blocks128 < num_cus && !sw.generic_c64_off) g.cfg = PN_CFG_C64;
    }
}

// Tile geometry of the chosen kernel (kern 3 / 4: the strip tiles are already in g; the generic kernel: rows x segments of its pixel tile).
// Returns PN_OK, or a negative status with *why set (the caller formats the message).
inline int pn_plan_conv_tiles(int prec, int H, int W, ConvGeom &g, const char **why) {
    const int ks = g.ks, stride = g.stride;
    const int ksd = (ks - 1) * g.dil + 1;                        // rows / columns the taps span; padding dil * (ks / 2) keeps the stride-1 size
    const int Ho = (H + 2 * (ks / 2) - ks) / stride + 1, Wo = (W + 2 * (ks / 2) - ks) / stride + 1;
    if (g.kern == 3 || g.kern == 4) { g.pitch = 32; return PN_OK; }
    if (g.cfg == PN_CFG_C64 && ks == 3 && stride == 1 && g.dil == 1 && Wo >= 48 && (long)Ho * Wo >= 2048) g.cfg = PN_CFG_C64W;   // wide maps: 224-pixel tiles
    const int BP = pn_cfg_pixels(g.cfg);
    // a block owns R full rows when they fit its pixel tile, else one row cut into equal segments
    const int wt_cap = std::min(BP, (120 - ksd) / stride + 1);     // widest segment the largest pitch class holds
    const int segs = (Wo + wt_cap - 1) / wt_cap;
    g.Wt = (Wo + segs - 1) / segs;
    g.R = std::max(1, std::min(Ho, BP / g.Wt));
    // the narrowest LDS pitch class that holds the halo row AND has a built instance for (prec, ks, stride, cfg): the table (conv_inst_table.h) has
    // holes -- no 1x1 kernel at pitch 16, no stride-2 kernel below pitch 64 -- and a wider LDS row is always valid
    const int need = (g.Wt - 1) * stride + ksd;                  // the dilated halo is (ks - 1) * dil + 1 wide
    g.pitch = -1;
    for (int c : {16, 32, 64, 120})
        if (need <= c && (g.dil == 1 ? pn_conv_has_instance(prec, ks, stride, c, g.cfg) : g.dil == 2 && pn_conv_has_instance_d2(prec, ks, stride, c, g.cfg))) { g.pitch = c; break; }
    if (g.pitch < 0) { *why = pn_pick_pitch(need) < 0 ? "halo width has no pitch class" : "no generic kernel instance for this kernel size, stride and cout block at any pitch class"; return PN_ERR_UNSUPPORTED; }
    {   // the register-prefetched staging path holds at most this many halo pixels
        const int maxpx = pn_conv_stage_maxpx(prec, ks, stride, g.pitch, g.cfg);
        while (maxpx > 0 && g.R > 1 && ((g.R - 1) * stride + ksd) * need > maxpx) --g.R;
        if (maxpx > 0 && ((g.R - 1) * stride + ksd) * need > maxpx) { *why = "halo tile exceeds the staging capacity"; return PN_ERR_UNSUPPORTED; }
    }
    // one halo image must fit the LDS (conv_launch_one refuses the launch otherwise): tall tiles of a narrow strided map.  R = 1 always fits: at
    // most 3 rows x 120 pixels x 256 B = 90 KB
    while (g.R > 1 && pn_conv_lds_bytes(prec, ks, stride, g.pitch, g.R, g.dil) > PN_CONV_LDS_MAX) --g.R;
    return PN_OK;
}

// ---- what follows from the chosen kernel and tiles ----------------------------------------------------------------------------------------------------
// output channels per block, and `cout` padded to whole blocks (the rows of the weight pack and of the padded bias)
inline int pn_conv_block_couts(const ConvGeom &g) { return g.kern == 4 ? 128 : (g.kern == 3 ? g.wc * 32 : pn_cfg_couts(g.cfg)); }
inline int pn_conv_cout_pad(const ConvGeom &g, int cout) { const int BC = pn_conv_block_couts(g); return (cout + BC - 1) / BC * BC; }
// Weight pack: fragments [64 lanes][8 values] (1 KB bf16, 2 KB fp32) that hold weights.  conv4: [cout block][k-step (+3 spare)][8 tiles]; the others:
// [16-cout tile][k-step], and 5 spare fragments behind the last (the weight queue prefetches up to 5 k-steps ahead) -- counted in the bytes only.
inline size_t pn_conv_pack_frags(const ConvGeom &g, int cout_pad, int ksteps) {
    return g.kern == 4 ? (size_t)(cout_pad / 128) * (ksteps + 3) * 8 : (size_t)(cout_pad / 16) * ksteps;
}
inline size_t pn_conv_pack_bytes(int prec, const ConvGeom &g, int cout_pad, int ksteps) {
    return (pn_conv_pack_frags(g, cout_pad, ksteps) + (g.kern == 4 ? 0 : 5)) * (prec == PN_PREC_BF16 ? 1024 : 2048);
}

// two planned convolutions run the same kernel instantiation
inline bool pn_conv_same_launch(const ConvGeom &a, const ConvGeom &b) {
    return b.ks == a.ks && b.stride == a.stride && b.dil == a.dil && b.acc == a.acc && b.pitch == a.pitch && b.R == a.R && b.Wt == a.Wt && b.kern == a.kern &&
           (a.kern == 4 || (a.kern == 3 ? (b.wc == a.wc && b.wp == a.wp && b.nbuf == a.nbuf && b.pt == a.pt && b.rpg == a.rpg) : b.cfg == a.cfg));
}

// The input tensor of a convolution problem: NHWC with channel stride cs; plane = channels of one stored plane (bf16x3: two planes [hi | lo], cs = 2 * plane);
// bytes = size of the whole tensor at the batch it was allocated for, where its zero page starts (the padding source of the halo DMA).
struct PnConvInput { const void *p; int H, W, cs, plane; size_t bytes; };

// Fills the geometry of a zeroed ConvProblem.  The caller adds what is its own: weights / bias, in_coff, out / res / nchw, act, yolo_naf (and the nets'
// fused tail / pool overrides).
inline void pn_fill_conv_problem(ConvProblem &P, const PnConvInput &in, int B, int cin_chunks, int cout, const ConvGeom &g, int prec, bool x3) {
    P.in = in.p;
    P.B = B; P.H = in.H; P.W = in.W;
    P.Ho = (in.H + 2 * (g.ks / 2) - g.ks) / g.stride + 1;
    P.Wo = (in.W + 2 * (g.ks / 2) - g.ks) / g.stride + 1;
    P.cin_chunks = cin_chunks;
    P.in_cs = in.cs;
    P.in_wrap = x3 ? 2 * (in.plane / 64) : (1 << 20);      // (conv4_kernel doubles it: halves)
    P.cout = cout;
    P.R = g.R;
    P.Wt = g.Wt;
    P.tiles_x = (P.Wo + g.Wt - 1) / g.Wt;
    P.tiles_per_img = ((P.Ho + g.R - 1) / g.R) * P.tiles_x;
    const int BC = pn_conv_block_couts(g);
    P.cout_blocks = (cout + BC - 1) / BC;
    P.nblocks = B * P.tiles_per_img * P.cout_blocks;
    if (g.kern == 4) P.nblocks = ((B * P.tiles_per_img + 1) / 2) * P.cout_blocks;      // a block = two strips x 128 couts
    P.ksteps = cin_chunks * g.ks * g.ks * 2;
    P.ks = g.ks;
    P.lds_buf_bytes = (int)pn_conv_lds_bytes(prec, g.ks, g.stride, g.pitch, g.R, g.dil);
    P.lds_two = (cin_chunks > 1 && 2 * (size_t)P.lds_buf_bytes <= PN_CONV_LDS_MAX) ? 1 : 0;
    P.in_zero_off = (unsigned)in.bytes;
}

// Fills a launch of nprob problems that share the geometry g (pn_conv_same_launch); two_bufs: a problem has lds_two set.  probs_dev is the caller's.
inline void pn_fill_conv_launch(ConvLaunch &L, int prec, const ConvGeom &g, int nprob, int max_blocks, bool two_bufs) {
    L.prec = prec;
    L.ks = g.ks; L.stride = g.stride; L.pitch = g.pitch; L.cfg = g.cfg;
    L.dil = g.dil; L.acc = g.acc;
    L.kern = g.kern; L.wc = g.wc; L.wp = g.wp; L.nbuf = g.nbuf; L.pt = g.pt; L.rpg = g.rpg;
    L.tail = 0; L.mix = 0;
    L.nprob = nprob;
    L.max_blocks = max_blocks;
    L.lds_bytes = pn_conv_lds_bytes(prec, g.ks, g.stride, g.pitch, g.R, g.dil) * (two_bufs ? 2 : 1);
    if (g.kern == 3) L.lds_bytes = pn_conv3_lds_bytes(g.ks, g.wp, g.nbuf, g.rpg);
    if (g.kern == 4) L.lds_bytes = 0;                        // conv4_launch knows its own size
}
