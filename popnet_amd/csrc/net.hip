// Network objects: reference state_dict in, NHWC activation plan + step list out (host code only; net_internal.h has the two phases of finalize).
// Mirrors (structure only; kernels are in conv_mfma.hip / conv_misc.hip, packing in net_pack.hip, launches in net_run.hip):
//   rtpose_light3d.__init__/forward   tpm/lib/network/rtpose_light3d.py:249-356
//   ResPreprocessNet                  tpm/lib/network/rtpose_light3d.py:124-219
//   YoloPoseNet / ResNetBackBone      tpm/lib/network/yolo_posenet.py:26-56,87-158
// The stage-2 input "torch.cat([paf, heat, z, feat], 1)" (rtpose_light3d.py:339) is never copied:
// the stem and the three stage-1 heads write straight into one 192-channel NHWC buffer laid out
// [feat 0..127 | paf 128..155 | heat 156..171 | z 172..186 | 0-pad], and the stage-2 weights'
// input channels are permuted to that order when they are packed.
#include <algorithm>
#include <cstdio>
#include "net_internal.h"

namespace pnnet {
namespace {
int new_buf(pn_net *n, int H, int W, int C) {
    Buf b;
    b.H = H; b.W = W; b.plane = C; b.C = n->x3 ? 2 * C : C;       // bf16x3: planes [hi | lo] (the third plane pair of the K loop re-reads hi: ConvProblem::in_wrap)
    n->bufs.push_back(b);
    return (int)n->bufs.size() - 1;
}

int add_conv(pn_net *n, const std::string &w, const std::string &bn, int ks, int stride, int in_buf, int in_coff,
             int out_buf, int out_coff, int act, int res_buf = -1, int nchw_slot = -1,
             std::vector<int> cin_map = std::vector<int>(), int dil = 1) {
    ConvSpec cs;
    cs.w = w; cs.bn = bn; cs.ks = ks; cs.stride = stride; cs.dil = dil;
    cs.in_buf = in_buf; cs.in_coff = in_coff;
    cs.out_buf = out_buf; cs.out_coff = out_coff;
    cs.res_buf = res_buf; cs.act = act; cs.nchw_slot = nchw_slot;
    cs.cin_map = std::move(cin_map);
    n->convs.push_back(cs);
    return (int)n->convs.size() - 1;
}

// What a builder writes its graph into
struct Levels : std::vector<Level> {
    void convs(std::vector<int> ids) { push_back({Level::CONVS, std::move(ids)}); }
    void pool(int mode, int in_buf, int out_buf, int C, int out_coff) { push_back({Level::POOL, {}, mode, in_buf, out_buf, C, out_coff}); }
};

// What a level of independent convs decides together (conv_plan.h::pn_plan_level): here only the weight-shape lookup that feeds it.
void harmonize_level(pn_net *n, const std::vector<int> &ids) {
    std::vector<PnLevelConv> lv;
    std::vector<int> which;
    for (int id : ids) {
        const ConvSpec &c = n->convs[id];
        const HostTensor *w = find_t(n, c.w + ".weight");
        if (!w || w->shape.size() != 4) continue;          // prepare_conv reports it
        const Buf &ib = n->bufs[c.in_buf];
        PnLevelConv l;
        l.H = ib.H; l.W = ib.W; l.rows = (int)w->shape[0]; l.ks = c.ks; l.stride = c.stride;
        l.cin_gt64 = std::max<int64_t>(w->shape[1], (int64_t)c.cin_map.size()) > 64;      // (a cin_map is never shorter than the weight's Cin: build_rtpose)
        lv.push_back(l);
        which.push_back(id);
    }
    pn_plan_level(lv, n->max_batch, n->x3, n->sw.conv4);
    for (size_t i = 0; i < lv.size(); ++i) {
        ConvSpec &c = n->convs[which[i]];
        c.k4_level = lv[i].k4_level; c.wc_min = lv[i].wc_min; c.nbuf_min = lv[i].nbuf_min;
    }
}

void add_conv_level(pn_net *n, const std::vector<int> &ids) {
    // split a set of independent convs into launches that share one kernel instantiation
    std::vector<bool> used(ids.size(), false);
    for (size_t i = 0; i < ids.size(); ++i) {
        if (used[i]) continue;
        Step st;
        st.type = Step::CONV;
        const ConvSpec &a = n->convs[ids[i]];
        // conv3_mix_kernel: the 128-cout 3x3 blocks and the fused-tail 1x1 blocks of a level share one launch
        auto mixable = [](const ConvSpec &c) {
            return c.kern == 3 && c.stride == 1 && c.wc == 4 && c.wp == 1 && c.nbuf == 1 && c.pt == 7 && c.rpg == 4 && !c.pool_tail && (c.ks == 3 ? c.tail_conv < 0 : c.ks == 1);
        };
        for (size_t j = i; j < ids.size(); ++j) {
            const ConvSpec &b = n->convs[ids[j]];
            if (used[j]) continue;
            const bool same = (b.tail_conv >= 0) == (a.tail_conv >= 0) && b.pool_tail == a.pool_tail && pn_conv_same_launch(a, b);
            const bool mixed = !n->sw.no_mix && mixable(a) && mixable(b) && b.R == a.R && b.Wt == a.Wt && (a.ks == 3 || b.ks == 3 || (a.tail_conv >= 0) == (b.tail_conv >= 0));
            if (same || mixed) {
                st.conv_ids.push_back(ids[j]);
                used[j] = true;
            }
        }
        st.dev_probs = add_image(n, nullptr, st.conv_ids.size() * sizeof(ConvProblem));
        n->steps.push_back(st);
    }
}

// The 7x7 stride-2 stem with its folded BatchNorm (net_pack.hip::pack_stem has the three forms)
int add_stem(pn_net *n, int out_buf, const std::string &conv = "model0.conv1", const std::string &bn = "model0.bn1", int sum_cin = 1) {
    Step st;
    st.type = Step::STEM;
    st.out_buf = out_buf;
    if (int rc = pack_stem(n, st, conv, bn, sum_cin)) return rc;
    n->steps.push_back(st);
    n->flops_per_frame += 2.0 * n->bufs[out_buf].H * n->bufs[out_buf].W * 64.0 * 49.0 * st.stem_cin;
    return PN_OK;
}

int add_bblock(pn_net *n, int ia, int ib) {
    Step st;
    st.type = Step::BBLOCK;
    st.conv_ids = {ia, ib};
    const Buf &inb = n->bufs[n->convs[ia].in_buf];
    const int segs = (inb.W + 27) / 28;
    st.bb_wt = (inb.W + segs - 1) / segs;                    // <= 28 columns: the 32-pixel halo row holds Wt + 4
    if (int rc = pack_bblock(n, st)) return rc;
    n->steps.push_back(st);
    return PN_OK;
}

// Who touches a buffer after level `after`: the convolutions (or pools: conv = -1) that read it, in level order, up to and including the first level that
// writes it again -- from then on it holds another tensor.  A BasicBlock level counts with both its convolutions.
struct BufUse { size_t level; int conv; };
std::vector<BufUse> readers_after(const pn_net *n, const std::vector<Level> &levels, size_t after, int buf) {
    std::vector<BufUse> readers;
    bool rewritten = false;
    for (size_t lj = after + 1; lj < levels.size() && !rewritten; ++lj) {
        const Level &l = levels[lj];
        if (l.kind == Level::POOL) {
            if (l.in_buf == buf) readers.push_back({lj, -1});
            if (l.out_buf == buf) rewritten = true;
            continue;
        }
        for (int id : l.convs) {
            const ConvSpec &c = n->convs[id];
            if (c.in_buf == buf || c.res_buf == buf) readers.push_back({lj, id});
            if (c.out_buf == buf) rewritten = true;
        }
    }
    return readers;
}

// What fuse_1x1_tails and fuse_pool_tails ask of the convolution that takes a tail: 1x1, exactly 128 couts = one conv3 block of 4 waves, its whole output tile in LDS
bool can_take_tail(const ConvSpec &a) {
    return a.kern == 3 && a.ks == 1 && a.stride == 1 && a.cout == 128 && a.wc == 4 && a.wp == 1 && a.res_buf < 0 && a.nchw_slot < 0 && a.out_buf >= 0 && a.out_coff == 0 &&
           (a.act == PN_ACT_NONE || a.act == PN_ACT_RELU || a.act == PN_ACT_LEAKY);
}

// BasicBlock(64) pairs (conv a: 3x3 64->64 + ReLU into a scratch buffer; conv b: 3x3 64->64 on it + residual = a's input +
// ReLU) become ONE level of kind BBLOCK run by bb64_kernel (bf16) or bb64x3_kernel (bf16x3: two-plane LDS images, 6-row tiles).
void fuse_basic_blocks(pn_net *n, std::vector<Level> &levels) {
    if (n->prec != PN_PREC_BF16 || n->sw.no_bblock || n->sw.no_conv3) return;
    // bf16x3: the fused kernel is built, bit-identical and faster ALONE (2 x 227 us against 4 x 100 us of conv3_kernel<3, 2, 2, 1, 7, 4> per step
    // once tensors are stored as two planes), but a persistent 160-KB-of-LDS workgroup per CU shuts the other in-flight batches out of
    // every CU for its whole life: through the bench's pipelined region the two-launch plan wins (25.7 k against 24.0 k frames/s on the
    // same box, profiles/r04_bb64x3_ab.txt).  POPNET_BBLOCK_X3=1 selects the fused kernel (tests, one-stream latency runs).
    if (n->x3 && !n->sw.bblock_x3) return;
    for (size_t i = 0; i + 1 < levels.size(); ++i) {
        if (levels[i].kind != Level::CONVS || levels[i + 1].kind != Level::CONVS || levels[i].convs.size() != 1 || levels[i + 1].convs.size() != 1) continue;
        const int ia = levels[i].convs[0], ib = levels[i + 1].convs[0];
        const ConvSpec &a = n->convs[ia], &b = n->convs[ib];
        const HostTensor *wa = find_t(n, a.w + ".weight"), *wb = find_t(n, b.w + ".weight");
        if (!wa || !wb || wa->shape.size() != 4 || wb->shape.size() != 4) continue;
        auto is64 = [](const HostTensor *w) { return w->shape[0] == 64 && w->shape[1] == 64 && w->shape[2] == 3 && w->shape[3] == 3; };
        if (!is64(wa) || !is64(wb) || a.stride != 1 || b.stride != 1 || a.kern != 3 || b.kern != 3) continue;
        if (a.act != PN_ACT_RELU || b.act != PN_ACT_RELU || a.res_buf >= 0 || b.res_buf != a.in_buf || b.in_buf != a.out_buf) continue;
        if (a.in_coff || a.out_coff || b.in_coff || b.res_coff || a.nchw_slot >= 0 || b.nchw_slot >= 0 || b.out_buf < 0 || !a.cin_map.empty() || !b.cin_map.empty()) continue;
        const Buf &inb = n->bufs[a.in_buf];
        if (inb.W < 8 || inb.H < 8) continue;
        levels[i].kind = Level::BBLOCK;
        levels[i].convs = {ia, ib};
        levels.erase(levels.begin() + i + 1);
    }
}

// The PAF branch ends in `1x1 256 -> 128 + BN + LeakyReLU` followed by `1x1 128 -> 28 + bias` (rtpose_light3d.py:266-267): per pixel
// independent, so the second convolution can run on the first one's output tile before it ever leaves the CU.  A conv A
// (1x1, exactly 128 couts = one conv3 block of 4 waves) whose output buffer is read by exactly one conv B (1x1, 128 -> <= 32
// channels, next level) takes B as its tail: B disappears from its level, A's launch writes B's output.  bf16 only (the
// three-plane bf16x3 form keeps the two-launch path); POPNET_NO_TAILFUSE=1 keeps the two launches (bit-identity tests).
void fuse_1x1_tails(pn_net *n, std::vector<Level> &levels) {
    if (n->prec != PN_PREC_BF16 || n->x3 || n->sw.no_tailfuse || n->sw.no_conv3) return;
    for (size_t li = 0; li + 1 < levels.size(); ++li) {
        Level &next = levels[li + 1];
        if (levels[li].kind != Level::CONVS || next.kind != Level::CONVS || levels[li].convs.empty() || next.convs.empty()) continue;
        for (int ia : levels[li].convs) {
            ConvSpec &a = n->convs[ia];
            if (!can_take_tail(a)) continue;
            // the only reader of A's output before the buffer is written again must be ONE conv of the next level
            const std::vector<BufUse> readers = readers_after(n, levels, li, a.out_buf);
            if (readers.size() != 1 || readers[0].level != li + 1) continue;
            const int ib = readers[0].conv;
            ConvSpec &b = n->convs[ib];
            const HostTensor *wb = find_t(n, b.w + ".weight");
            if (!wb || wb->shape.size() != 4 || b.ks != 1 || b.stride != 1 || wb->shape[1] != 128 || wb->shape[0] > 32 || !b.bn.empty() || b.res_buf >= 0 || b.in_coff != 0 ||
                (b.act != PN_ACT_NONE && b.act != PN_ACT_SIG && b.act != PN_ACT_SIG_PM2) ||
                !b.cin_map.empty())
                continue;
            a.tail_conv = ib;
            a.flops += b.flops;
            next.convs.erase(std::find(next.convs.begin(), next.convs.end(), ib));
        }
    }
    levels.erase(std::remove_if(levels.begin(), levels.end(), [](const Level &l) { return l.kind != Level::POOL && l.convs.empty(); }), levels.end());
}

// `1x1 128 -> 128 + BN + ReLU` followed by AvgPool2d(3, 2, 1) (model0.conv2 / bn2 / relu -> avgpool, rtpose_light3d.py:154-158): the
// convolution is per pixel, so a block can compute exactly the 7 x 15 patch that 3 x 7 pooled pixels need and sum the windows
// from LDS (conv3_kernel.h, TAIL == 2).  The pool launch and the full-resolution map (25.7 MB written and read back at B = 32)
// disappear; blocks recompute one shared row and column (25 % more matrix work on a bandwidth-bound layer).  Same values, same
// summation order as the two launches: bit-identical (POPNET_NO_POOLFUSE=1 keeps them).  bf16 and (round 5) bf16x3: the parked tile as two planes.
void fuse_pool_tails(pn_net *n, std::vector<Level> &levels) {
    if (n->prec != PN_PREC_BF16 || n->sw.no_poolfuse || n->sw.no_conv3) return;       // (bf16x3 since round 5: two parked planes)
    for (size_t li = 0; li + 1 < levels.size(); ++li) {
        const Level &pl = levels[li + 1];
        if (levels[li].kind != Level::CONVS || levels[li].convs.size() != 1 || pl.kind != Level::POOL || pl.mode != 0) continue;      // mode 0 = average 3x3 s2
        ConvSpec &a = n->convs[levels[li].convs[0]];
        if (!can_take_tail(a) || a.tail_conv >= 0) continue;
        if (pl.in_buf != a.out_buf || pl.C != 128 || (pl.out_coff & 7)) continue;
        if (!readers_after(n, levels, li + 1, a.out_buf).empty()) continue;      // nothing else may read the full-resolution map
        a.pool_tail = true;
        a.pool_out_buf = pl.out_buf; a.pool_out_coff = pl.out_coff;
        a.rpg = 8; a.nbuf = 1;                                                 // 8-row image: the 7 patch rows
        levels.erase(levels.begin() + li + 1);
    }
}

// The common end of the three builders: plan and pack every convolution, fuse, and turn the levels into steps.  What each net runs here decides its launches.
// harmonize: the convolutions of a level plan together; bblocks: fuse_basic_blocks; tails: fuse_1x1_tails and fuse_pool_tails; blocked_acc_f32: ACC = 1 in fp32
struct BuildTail { bool harmonize, bblocks, tails, blocked_acc_f32; };
const BuildTail TAIL_RTPOSE = {true, true, true, false}, TAIL_YOLO = {false, true, false, false}, TAIL_A2J = {false, false, false, true};

int finish_build(pn_net *n, std::vector<Level> &levels, const BuildTail &t) {
    if (t.harmonize)
        for (auto &lv : levels)
            if (lv.kind == Level::CONVS) harmonize_level(n, lv.convs);
    if (t.blocked_acc_f32 && n->prec == PN_PREC_F32)
        for (auto &cs : n->convs) cs.acc = 1;
    for (auto &cs : n->convs)
        if (int rc = prepare_conv(n, cs)) return rc;
    for (auto &cs : n->convs) n->flops_per_frame += cs.flops;
    if (t.bblocks) fuse_basic_blocks(n, levels);
    if (t.tails) { fuse_1x1_tails(n, levels); fuse_pool_tails(n, levels); }
    for (auto &cs : n->convs)
        if (cs.tail_conv >= 0)
            if (int rc = pack_tail(n, cs)) return rc;
    for (auto &lv : levels) {
        if (lv.kind == Level::POOL) { n->steps.emplace_back(); n->steps.back().type = Step::POOL; n->steps.back().pool = lv; }
        else if (lv.kind == Level::BBLOCK) { if (int rc = add_bblock(n, lv.convs[0], lv.convs[1])) return rc; }
        else add_conv_level(n, lv.convs);
    }
    return PN_OK;
}

// ---- graph builders -------------------------------------------------------------------------
int build_rtpose(pn_net *n) {
    const int H = n->in_h, W = n->in_w;
    if (H % 8 || W % 8) return pn_set_error(n->ctx, PN_ERR_UNSUPPORTED, "input size must be a multiple of 8");
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8;
    const int J1 = n->num_parts + 1, L2 = 2 * n->a, LZ = n->a + 1;      // heat / paf / z channels
    // the stage-1 heads write channel slices of the concat buffer with vector stores: every slice starts on a multiple of 4 channels (the
    // reference's default topology, 18 parts / 19 limbs = 38 + 19 + 20 channels, leaves 2 + 1 pad channels between the slices; they are
    // never written, the buffer starts as zeros and the stage-2 weights of a pad channel are zero: rtpose_light3d.py:250,339)
    auto up4 = [](int v) { return (v + 3) / 4 * 4; };
    const int off_paf = 128, off_heat = up4(off_paf + L2), off_z = up4(off_heat + J1);
    const int cat_c = (off_z + LZ + 63) / 64 * 64;
    n->out_h = H8; n->out_w = W8;

    int A1 = new_buf(n, H2, W2, 64), A2 = new_buf(n, H2, W2, 64), T1 = new_buf(n, H2, W2, 64);
    int P1 = new_buf(n, H4, W4, 64), T2 = new_buf(n, H4, W4, 128), D2 = new_buf(n, H4, W4, 128);
    int A3 = new_buf(n, H4, W4, 128), A4 = new_buf(n, H4, W4, 128);
    int CAT = new_buf(n, H8, W8, cat_c);
    int BLa = new_buf(n, H8, W8, 256), BLb = new_buf(n, H8, W8, 256), BLc = new_buf(n, H8, W8, 128);
    int BSa = new_buf(n, H8, W8, 128), BSb = new_buf(n, H8, W8, 128);
    int BDa = new_buf(n, H8, W8, 128), BDb = new_buf(n, H8, W8, 64), BDc = new_buf(n, H8, W8, 64);
    n->named["feat"] = {CAT, 0, 128};
    n->named["paf1"] = {CAT, off_paf, L2};
    n->named["heat1"] = {CAT, off_heat, J1};
    n->named["z1"] = {CAT, off_z, LZ};

    if (int rc = add_stem(n, A1)) return rc;
    Levels levels;
    // layer1: two BasicBlocks(64) @ H/2
    levels.convs({add_conv(n, "model0.layer1.0.conv1", "model0.layer1.0.bn1", 3, 1, A1, 0, T1, 0, PN_ACT_RELU)});
    levels.convs({add_conv(n, "model0.layer1.0.conv2", "model0.layer1.0.bn2", 3, 1, T1, 0, A2, 0, PN_ACT_RELU, A1)});
    levels.convs({add_conv(n, "model0.layer1.1.conv1", "model0.layer1.1.bn1", 3, 1, A2, 0, T1, 0, PN_ACT_RELU)});
    levels.convs({add_conv(n, "model0.layer1.1.conv2", "model0.layer1.1.bn2", 3, 1, T1, 0, A1, 0, PN_ACT_RELU, A2)});
    levels.pool(0, A1, P1, 64, 0);    // avgpool1
    // layer2: BasicBlock(64->128) with 1x1 shortcut @ H/4
    levels.convs({add_conv(n, "model0.layer2.0.conv1", "model0.layer2.0.bn1", 3, 1, P1, 0, T2, 0, PN_ACT_RELU),
           add_conv(n, "model0.layer2.0.downsample.0", "model0.layer2.0.downsample.1", 1, 1, P1, 0, D2, 0, PN_ACT_NONE)});
    levels.convs({add_conv(n, "model0.layer2.0.conv2", "model0.layer2.0.bn2", 3, 1, T2, 0, A3, 0, PN_ACT_RELU, D2)});
    levels.convs({add_conv(n, "model0.conv2", "model0.bn2", 1, 1, A3, 0, A4, 0, PN_ACT_RELU)});
    levels.pool(0, A4, CAT, 128, 0);  // avgpool2 -> feat slice of the concat buffer

    // stage-2 input-channel map: my [feat | paf | heat | z | pad] -> reference [paf, heat, z, feat]
    std::vector<int> map2(cat_c, -1);
    for (int i = 0; i < 128; ++i) map2[i] = L2 + J1 + LZ + i;
    for (int i = 0; i < L2; ++i) map2[off_paf + i] = i;
    for (int i = 0; i < J1; ++i) map2[off_heat + i] = L2 + i;
    for (int i = 0; i < LZ; ++i) map2[off_z + i] = L2 + J1 + i;

    for (int stage = 1; stage <= 2; ++stage) {
        char p1[32], p2[32], p3[32];
        snprintf(p1, sizeof p1, "model%d_1", stage);
        snprintf(p2, sizeof p2, "model%d_2", stage);
        snprintf(p3, sizeof p3, "model%d_3", stage);
        auto nm = [](const char *p, int i) { return std::string(p) + "." + std::to_string(i); };
        std::vector<int> m = stage == 2 ? map2 : std::vector<int>();
        const bool last = stage == 2;
        levels.convs({add_conv(n, nm(p1, 0), nm(p1, 1), 3, 1, CAT, 0, BLa, 0, PN_ACT_LEAKY, -1, -1, m),
               add_conv(n, nm(p2, 0), nm(p2, 1), 3, 1, CAT, 0, BSa, 0, PN_ACT_LEAKY, -1, -1, m),
               add_conv(n, nm(p3, 0), nm(p3, 1), 3, 1, CAT, 0, BDa, 0, PN_ACT_LEAKY, -1, -1, m)});
        levels.convs({add_conv(n, nm(p1, 3), nm(p1, 4), 3, 1, BLa, 0, BLb, 0, PN_ACT_LEAKY),
               add_conv(n, nm(p2, 3), nm(p2, 4), 3, 1, BSa, 0, BSb, 0, PN_ACT_LEAKY),
               add_conv(n, nm(p3, 3), nm(p3, 4), 3, 1, BDa, 0, BDb, 0, PN_ACT_LEAKY)});
        levels.convs({add_conv(n, nm(p1, 6), nm(p1, 7), 3, 1, BLb, 0, BLa, 0, PN_ACT_LEAKY),
               add_conv(n, nm(p2, 6), nm(p2, 7), 3, 1, BSb, 0, BSa, 0, PN_ACT_LEAKY),
               add_conv(n, nm(p3, 6), nm(p3, 7), 3, 1, BDb, 0, BDc, 0, PN_ACT_LEAKY)});
        levels.convs({add_conv(n, nm(p1, 9), nm(p1, 10), 1, 1, BLa, 0, BLc, 0, PN_ACT_LEAKY),
               add_conv(n, nm(p2, 9), nm(p2, 10), 3, 1, BSa, 0, BSb, 0, PN_ACT_LEAKY),
               add_conv(n, nm(p3, 9), nm(p3, 10), 3, 1, BDc, 0, BDb, 0, PN_ACT_LEAKY)});
        levels.convs({add_conv(n, nm(p1, 12), "", 1, 1, BLc, 0, last ? -1 : CAT, off_paf, PN_ACT_SIG_PM2, -1, last ? 0 : -1),
               add_conv(n, nm(p2, 12), "", 3, 1, BSb, 0, last ? -1 : CAT, off_heat, PN_ACT_SIG, -1, last ? 1 : -1),
               add_conv(n, nm(p3, 12), "", 3, 1, BDb, 0, last ? -1 : CAT, off_z, PN_ACT_SIG_PM2, -1, last ? 2 : -1)});
    }

    return finish_build(n, levels, TAIL_RTPOSE);
}

int build_yolo(pn_net *n) {
    const int H = n->in_h, W = n->in_w;
    if (H % 16 || W % 16) return pn_set_error(n->ctx, PN_ERR_UNSUPPORTED, "input size must be a multiple of 16");
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8, H16 = H / 16, W16 = W / 16;
    n->out_h = H16; n->out_w = W16;
    int A1 = new_buf(n, H2, W2, 64);
    int X0 = new_buf(n, H4, W4, 64), X1 = new_buf(n, H4, W4, 64), XT = new_buf(n, H4, W4, 64);
    int Y0 = new_buf(n, H8, W8, 128), Y1 = new_buf(n, H8, W8, 128), YT = new_buf(n, H8, W8, 128), YD = new_buf(n, H8, W8, 128);
    int Na = new_buf(n, H8, W8, 256), Nb = new_buf(n, H8, W8, 256);
    int Ha = new_buf(n, H16, W16, 256), Hb = new_buf(n, H16, W16, 256), Hc = new_buf(n, H16, W16, 128);

    if (int rc = add_stem(n, A1)) return rc;
    Levels levels;
    // conv1 - bn1 - relu - maxpool (yolo_posenet.py:101-108): one launch in bf16 (conv_misc.hip::stem7x7_pool_kernel; the 112 x 112 x 64
    // map is never stored); POPNET_NO_STEMPOOL=1, fp32 and bf16x3 keep the stem and the pool as two launches
    if (n->prec == PN_PREC_BF16 && !n->x3 && n->input_dim == 1 && !n->sw.no_stempool) n->steps.back().stem_pool_buf = X0;
    else levels.pool(1, A1, X0, 64, 0);   // maxpool 3x3 s2
    int cur = X0, other = X1;
    for (int i = 0; i < 3; ++i) {
        std::string p = "model0.layer1." + std::to_string(i);
        levels.convs({add_conv(n, p + ".conv1", p + ".bn1", 3, 1, cur, 0, XT, 0, PN_ACT_RELU)});
        levels.convs({add_conv(n, p + ".conv2", p + ".bn2", 3, 1, XT, 0, other, 0, PN_ACT_RELU, cur)});
        std::swap(cur, other);
    }
    {   // layer2.0: the 3x3 stride-2 conv and its 1x1 stride-2 shortcut (resnet.py:59-77) read the same map at the same stride.  bf16 / bf16x3: the
        // shortcut runs as the centre tap of a 3x3 problem in the SAME launch (one launch and 12 us of pure latency less per step; every added
        // product is an exact zero, so the sums are the 1x1 convolution's bit for bit: POPNET_NO_EMBED3=1 keeps the two launches, tested)
        const bool embed = n->prec == PN_PREC_BF16 && !n->sw.no_embed3;
        const int c1 = add_conv(n, "model0.layer2.0.conv1", "model0.layer2.0.bn1", 3, 2, cur, 0, YT, 0, PN_ACT_RELU);
        const int cd = add_conv(n, "model0.layer2.0.downsample.0", "model0.layer2.0.downsample.1", embed ? 3 : 1, 2, cur, 0, YD, 0, PN_ACT_NONE);
        n->convs[cd].embed3 = embed;
        levels.convs({c1, cd});
    }
    levels.convs({add_conv(n, "model0.layer2.0.conv2", "model0.layer2.0.bn2", 3, 1, YT, 0, Y0, 0, PN_ACT_RELU, YD)});
    int yc = Y0, yo = Y1;
    for (int i = 1; i < 4; ++i) {
        std::string p = "model0.layer2." + std::to_string(i);
        levels.convs({add_conv(n, p + ".conv1", p + ".bn1", 3, 1, yc, 0, YT, 0, PN_ACT_RELU)});
        levels.convs({add_conv(n, p + ".conv2", p + ".bn2", 3, 1, YT, 0, yo, 0, PN_ACT_RELU, yc)});
        std::swap(yc, yo);
    }
    n->named["feat"] = {yc, 0, 128};
    levels.convs({add_conv(n, "model1.0", "model1.1", 3, 1, yc, 0, Na, 0, PN_ACT_LEAKY)});
    levels.convs({add_conv(n, "model1.3", "model1.4", 3, 1, Na, 0, Nb, 0, PN_ACT_LEAKY)});
    levels.convs({add_conv(n, "model1.6", "model1.7", 3, 1, Nb, 0, Na, 0, PN_ACT_LEAKY)});
    levels.convs({add_conv(n, "model1.9", "model1.10", 3, 1, Na, 0, Nb, 0, PN_ACT_LEAKY)});
    levels.convs({add_conv(n, "model1.12", "", 3, 1, Nb, 0, Na, 0, PN_ACT_NONE)});
    levels.convs({add_conv(n, "model2_1.0", "model2_1.1", 3, 1, Na, 0, Nb, 0, PN_ACT_LEAKY)});
    levels.pool(2, Nb, Ha, 256, 0);  // maxpool 2x2
    levels.convs({add_conv(n, "model2_2.0", "model2_2.1", 3, 1, Ha, 0, Hb, 0, PN_ACT_LEAKY)});
    levels.convs({add_conv(n, "model2_3.0", "model2_3.1", 3, 1, Hb, 0, Hc, 0, PN_ACT_LEAKY)});
    levels.convs({add_conv(n, "model2_4.0", "", 3, 1, Hc, 0, -1, 0, PN_ACT_YOLO, -1, 3)});

    return finish_build(n, levels, TAIL_YOLO);
}

// A2J_model (third_party_methods/A2J_experiments/model.py:145-186): ResNet-50 (resnet.py:61-164: Bottleneck layers [3, 4, 6, 3], the stride on conv2, a 1x1
// strided downsample; layer4 at stride 1 with conv2 of its blocks 1 and 2 at dilation 2 / padding 2, block 0 not dilated: resnet.py:112,142-145), output
// stride 16, and three heads of 4 x (3x3 conv + bias + BN + ReLU) + a 3x3 output conv with bias: classification on layer3's map, regression and depth on
// layer4's.  The head maps stay NHWC [B, h, w, 16 anchors x 15 joints (x 2)] in the buffers "cls" / "reg" / "dep": pn_a2j_vote reads them there.
// Backbone.model.fc.* is never executed (model.py:158-167) and is skipped at load.  bf16x3: every buffer a [hi | lo] plane pair like the other nets'; the
// head maps' planes (240 / 480 channels) are no multiple of 64, which is legal because nothing convolves them (pn_a2j_vote reads them as hi + lo).
int build_a2j(pn_net *n) {
    const int H = n->in_h, W = n->in_w;
    if (H % 16 || W % 16 || H < 16 || W < 16) return pn_set_error(n->ctx, PN_ERR_UNSUPPORTED, "input size must be a multiple of 16");
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H16 = H / 16, W16 = W / 16;
    n->out_h = H16; n->out_w = W16;
    const int A1 = new_buf(n, H2, W2, 64), X0 = new_buf(n, H4, W4, 64);
    if (int rc = add_stem(n, A1, "Backbone.model.conv1", "Backbone.model.bn1", 3)) return rc;
    Levels levels;
    // conv1 - bn1 - relu - maxpool as one launch, as build_yolo; bf16x3 keeps the two launches (the fused kernel stores one plane)
    if (n->prec == PN_PREC_BF16 && !n->x3 && !n->sw.no_stempool) n->steps.back().stem_pool_buf = X0;
    else levels.pool(1, A1, X0, 64, 0);
    int cur = X0, ch = H4, cw = W4;
    const int nblocks[4] = {3, 4, 6, 3}, planes[4] = {64, 128, 256, 512}, strides[4] = {1, 2, 2, 1}, dils[4] = {1, 1, 1, 2};
    int x3 = -1;
    for (int l = 0; l < 4; ++l) {
        const int p = planes[l], s = strides[l], oh = ch / s, ow = cw / s;
        const int t1 = new_buf(n, ch, cw, p), t1b = s == 1 ? t1 : new_buf(n, oh, ow, p), t2 = new_buf(n, oh, ow, p);
        const int d = new_buf(n, oh, ow, 4 * p);
        int a = new_buf(n, oh, ow, 4 * p), b = new_buf(n, oh, ow, 4 * p);
        const std::string L = "Backbone.model.layer" + std::to_string(l + 1) + ".";
        // block 0: conv1 and the (strided) downsample read the same map: one level
        levels.convs({add_conv(n, L + "0.conv1", L + "0.bn1", 1, 1, cur, 0, t1, 0, PN_ACT_RELU),
               add_conv(n, L + "0.downsample.0", L + "0.downsample.1", 1, s, cur, 0, d, 0, PN_ACT_NONE)});
        levels.convs({add_conv(n, L + "0.conv2", L + "0.bn2", 3, s, t1, 0, t2, 0, PN_ACT_RELU)});
        levels.convs({add_conv(n, L + "0.conv3", L + "0.bn3", 1, 1, t2, 0, a, 0, PN_ACT_RELU, d)});
        for (int i = 1; i < nblocks[l]; ++i) {
            const std::string P = L + std::to_string(i);
            levels.convs({add_conv(n, P + ".conv1", P + ".bn1", 1, 1, a, 0, t1b, 0, PN_ACT_RELU)});
            levels.convs({add_conv(n, P + ".conv2", P + ".bn2", 3, 1, t1b, 0, t2, 0, PN_ACT_RELU, -1, -1, std::vector<int>(), dils[l])});
            levels.convs({add_conv(n, P + ".conv3", P + ".bn3", 1, 1, t2, 0, b, 0, PN_ACT_RELU, a)});
            std::swap(a, b);
        }
        cur = a; ch = oh; cw = ow;
        if (l == 2) x3 = cur;
    }
    const int x4 = cur;
    n->named["x3"] = {x3, 0, 1024};
    n->named["x4"] = {x4, 0, 2048};
    const int na = 16 * n->num_parts;
    const char *hn[3] = {"classificationModel", "regressionModel", "DepthRegressionModel"}, *on[3] = {"cls", "reg", "dep"};
    int hin[3] = {x3, x4, x4}, ha[3], hb[3], ho[3];
    for (int k = 0; k < 3; ++k) {
        ha[k] = new_buf(n, H16, W16, 256); hb[k] = new_buf(n, H16, W16, 256);
        ho[k] = new_buf(n, H16, W16, k == 1 ? 2 * na : na);
        n->named[on[k]] = {ho[k], 0, k == 1 ? 2 * na : na};
    }
    for (int i = 1; i <= 4; ++i) {
        std::vector<int> ids;
        for (int k = 0; k < 3; ++k) {
            const std::string P = std::string(hn[k]) + ".";
            ids.push_back(add_conv(n, P + "conv" + std::to_string(i), P + "bn" + std::to_string(i), 3, 1, hin[k], 0, ha[k], 0, PN_ACT_RELU));
            hin[k] = ha[k];
            std::swap(ha[k], hb[k]);
        }
        levels.convs(ids);
    }
    levels.convs({add_conv(n, std::string(hn[0]) + ".output", "", 3, 1, hin[0], 0, ho[0], 0, PN_ACT_NONE),
           add_conv(n, std::string(hn[1]) + ".output", "", 3, 1, hin[1], 0, ho[1], 0, PN_ACT_NONE),
           add_conv(n, std::string(hn[2]) + ".output", "", 3, 1, hin[2], 0, ho[2], 0, PN_ACT_NONE)});
    // fp32: blocked accumulation (conv_mfma_kernel<..., ACC = 1>) -- this net's K loops run to 18 432 terms, and a serial fp32 chain of that length
    // leaves the heads about four times the reference's own fp32 error away from its fp64 run
    return finish_build(n, levels, TAIL_A2J);
}
}  // namespace

int compile_net(pn_net *n) {
    if (int rc = n->kind == PN_NET_RTPOSE_LIGHT3D ? build_rtpose(n) : n->kind == PN_NET_A2J ? build_a2j(n) : build_yolo(n)) return rc;
    for (auto &b : n->bufs) {
        b.bytes = (size_t)n->max_batch * b.H * b.W * b.C * n->esize();
        if (const size_t bytes = b.bytes + 2048; bytes >= ((size_t)1 << 32))     // + zero page; the kernels address a buffer with 32-bit byte offsets (zero page, epilogue stores)
            return pn_set_error(n->ctx, PN_ERR_UNSUPPORTED, "activation buffer %dx%dx%d%s x batch %d = %zu B exceeds the 4 GiB the kernels' 32-bit offsets address; lower max_batch", b.H, b.W, b.C,
                                n->x3 ? " (bf16x3: hi and lo planes)" : "", n->max_batch, bytes);
    }
    for (size_t i = 0; i < n->bufs.size(); ++i) {     // every buffer by number (pn_net_step_info's buffer indices), for per-layer checks
        const std::string nm = "buf" + std::to_string(i);
        n->named[nm] = {(int)i, 0, n->bufs[i].plane};
        for (int pl = 0; n->x3 && pl < 2; ++pl) n->named[nm + (pl ? ".lo" : ".hi")] = {(int)i, 0, n->bufs[i].plane, pl};
    }
    return PN_OK;
}
}  // namespace pnnet
