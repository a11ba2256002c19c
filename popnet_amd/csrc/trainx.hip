// The training step of rtpose_light3d on the INFERENCE convolution kernels (round 6).
//
// Replaces, for TrainEngine(precision = "bf16x3"), the NCHW fp32 primitives of train.hip (whose forward / data-gradient kernels spent
// 83 of 110 us per launch gathering an NCHW tensor into a channel-minor LDS image) with one C++ object that keeps every activation and
// gradient as NHWC [hi | lo] bf16 planes -- the layout of the bf16x3 inference net -- so that
//   * forward convolutions AND data gradients run conv3_kernel / conv4_kernel / conv_mfma_kernel unchanged (a data gradient is the same
//     convolution on the 180-degree-rotated, Cin <-> Cout-transposed weight pack: trainx_kernels.h::pack_kernel builds both packs of every
//     layer from the live fp32 parameters in ONE launch per step);
//   * train-mode BatchNorm, pooling, heads and loss are channel-minor 16-byte-vector passes (trainx_kernels.h);
//   * the weight gradient is a pixel-K MFMA GEMM over the same planes (trainx_wgrad.h), deterministic split-K.
// Reference being replaced (tpm/ = third_party_methods/):
//   tpm/train_rtpose_light3d_kdh3d_mpaug.py:153-212 (CR)   the per-batch body: model(img) -> loss -> backward
//   tpm/lib/network/rtpose_light3d.py:124-219,222-246,326-356   the module in train mode
//   tpm/lib/network/losses.py:65-106                        rtpose_light3d_loss_fgweight
// Parameters, gradients and BatchNorm running statistics stay in the caller's flat fp32 buffers (popnet_amd.train.TrainEngine): the
// optimiser, the data-parallel all-reduce and the checkpoint format are untouched.  The 7x7 single-channel stem keeps train.hip's NCHW
// kernels (Cin = 1: nothing for the matrix cores to contract over) behind two layout hand-overs.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>
#include "pn_internal.h"
#include "conv_plan.h"
#include "trainx_kernels.h"
#include "trainx_wgrad.h"

namespace {

using tx::bf;

struct TxTensor {                     // [B][H][W][2 * plane] bf16 planes [hi | lo], or (fp32 engine) [B][H][W][plane] float: 4 bytes per channel either way
    char *p = nullptr;
    int H = 0, W = 0, plane = 0;
    bool f32 = false;
    int cs() const { return f32 ? plane : 2 * plane; }      // channel stride in elements
    int split() const { return f32 ? 0 : plane; }           // plane distance in elements (0: one fp32 plane)
    char *at(int ch) const { return p + (size_t)ch * (f32 ? 4 : 2); }
};

struct TxBn {
    std::string name;
    int C = 0;
    const float *gamma = nullptr, *beta = nullptr;
    float *dgamma = nullptr, *dbeta = nullptr, *rm = nullptr, *rv = nullptr;
    float *mean = nullptr, *invstd = nullptr, *scale = nullptr, *shift = nullptr, *k1 = nullptr, *k2 = nullptr, *k3 = nullptr;
};

struct TxLayer {                      // one nn.Conv2d
    std::string name;
    int ks = 3, cin = 0, cout = 0;
    const float *w = nullptr, *b = nullptr;
    float *dw = nullptr, *db = nullptr;
    int x = -1;                       // input tensor
    bool cat = false;                 // reads the stage-2 input in this engine's channel order [feat | paf | heat | z | pad]
    bool bn_follows = false;          // its output goes straight into a train-mode BatchNorm: the batch mean cancels the bias, d loss / d bias == 0 exactly
    bf *pack_f = nullptr, *pack_d = nullptr;      // forward / data-gradient weight packs (built lazily by the group that needs them)
    float *bias_pad = nullptr;
};

struct OpDesc {                       // what ops[k] is, for pn_trainer_op_info: recorded beside the closure where it is pushed
    std::string kind, body;           // body: the JSON members after "kind" and "stream"
    bool side = false;
};

std::string jf(const char *fmt, ...) {
    char t[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t, sizeof t, fmt, ap);
    va_end(ap);
    return t;
}
std::string jref(int id, int coff, int c) { return id < 0 ? std::string("null") : jf("{\"t\": %d, \"coff\": %d, \"c\": %d}", id, coff, c); }

struct ConvUse {                      // one convolution launch problem
    int layer; bool dgrad;
    int in, out, out_coff, res;       // tensors (-1 = none)
    int act;
    float *out_nchw;
};

}  // namespace

struct pn_trainer {
    pn_ctx *ctx = nullptr;
    int B = 0, H = 0, W = 0;
    float *flat_p = nullptr, *flat_g = nullptr;
    std::map<std::string, std::pair<size_t, size_t>> params;      // name -> (offset, numel) in the flat buffers
    std::map<std::string, float *> stats;                        // running_mean / running_var device pointers
    bool finalized = false;
    PnSwitches sw;                   // read in pn_trainer_finalize
    bool legacy_wgrad = false;
    bool f32 = false;                // precision "fp32": one fp32 plane per tensor, the generic fp32 convolution kernel, K = 4 weight gradient
    std::vector<void *> allocs;
    std::vector<TxTensor> T;
    std::vector<TxBn> bns;
    std::vector<TxLayer> layers;
    std::vector<ConvLaunch> launches;
    std::vector<std::function<int(hipStream_t)>> ops;
    std::vector<OpDesc> op_desc;     // one per op (diagnostics: pn_trainer_op_info)
    std::vector<tx::PackDesc> packs;
    std::vector<tx::BiasDesc> biases;
    tx::PackDesc *packs_dev = nullptr;
    tx::BiasDesc *biases_dev = nullptr;
    unsigned pack_groups = 0, pack_units = 0;
    bool pack_gather = false;          // POPNET_TRAINX_PACK=gather: round 6's first pack kernel (one thread per 16-byte group; bit-identical)
    float *zero_bias = nullptr;
    int *cat_k_map = nullptr, *cat_ref_map = nullptr;           // [192] my channel -> reference channel ; [187] reference -> my channel
    double *partial = nullptr; size_t partial_doubles = 0;
    float *nchw_a = nullptr, *nchw_b = nullptr; size_t nchw_elems = 0;      // NCHW f32 scratch: the stem hand-over and the legacy weight gradient
    float *wg_partial = nullptr; size_t wg_partial_floats = 0;      // split-K scratch of the weight gradients
    // the weight gradients run on a second stream beside the BatchNorm / data-gradient chain (matrix-core-bound next to bandwidth-bound launches)
    hipStream_t side = nullptr;
    bool two_streams = true;
    std::vector<hipEvent_t> events;
    size_t side_tail = (size_t)-1;            // ops.size() right after the last side-stream op: nothing new on the step's stream since = no new fork needed
    float *head_out[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    // per-step arguments (read by the ops when they launch)
    const float *img = nullptr, *target[3] = {nullptr, nullptr, nullptr}, *fg = nullptr;
    float *loss = nullptr;
    float momentum = 0.1f, eps = 1e-5f;
    double flops_conv = 0;

    int prec() const { return f32 ? PN_PREC_F32 : PN_PREC_BF16; }       // as the convolution kernels see it (bf16x3 = bf16 kernels on [hi | lo] planes)
};

namespace {

const int HEAD_C[3] = {28, 16, 15};          // paf, heat, z            rtpose_light3d(15, 14, 2)
const int HEAD_KIND[3] = {1, 0, 1};          // (s - 0.5) * 4 | s | (s - 0.5) * 4      rtpose_light3d.py:335-337
const int HEAD_ACT[3] = {PN_ACT_SIG_PM2, PN_ACT_SIG, PN_ACT_SIG_PM2};
const int CAT_OFF[3] = {128, 156, 172};      // channel slices of the stage-2 input (net.hip::build_rtpose)
const int CAT_PLANE = 192;

int tx_alloc(pn_trainer *t, void **p, size_t bytes, bool zero) {
    PN_HIP_CHECK(t->ctx, hipMalloc(p, bytes));
    t->allocs.push_back(*p);
    if (zero) PN_HIP_CHECK(t->ctx, hipMemset(*p, 0, bytes));
    return PN_OK;
}

int new_tensor(pn_trainer *t, int H, int W, int plane, int *id) {
    TxTensor x;
    x.H = H; x.W = W; x.plane = plane; x.f32 = t->f32;
    const size_t bytes = (size_t)t->B * H * W * plane * 4 + 2048;          // (two bf16 planes or one fp32 plane) + zero page: the halo DMA's padding source
    if (bytes >= ((size_t)1 << 32)) return pn_set_error(t->ctx, PN_ERR_UNSUPPORTED, "pn_trainer: a %dx%dx%d tensor at batch %d exceeds the 4 GiB the kernels' 32-bit offsets address", H, W, plane, t->B);
    if (int rc = tx_alloc(t, (void **)&x.p, bytes, true)) return rc;
    t->T.push_back(x);
    *id = (int)t->T.size() - 1;
    return PN_OK;
}

int pad64(int c) { return (c + 63) / 64 * 64; }

// describes the op pushed last
void describe(pn_trainer *t, const char *kind, const std::string &body) {
    OpDesc d;
    d.kind = kind; d.body = body;
    t->op_desc.push_back(d);
}

int find_param(pn_trainer *t, const std::string &name, size_t numel, const float **p, float **g) {
    auto it = t->params.find(name);
    if (it == t->params.end()) return pn_set_error(t->ctx, PN_ERR_INVALID, "pn_trainer: parameter %s was not set", name.c_str());
    if (it->second.second != numel) return pn_set_error(t->ctx, PN_ERR_INVALID, "pn_trainer: parameter %s has %zu elements, %zu expected", name.c_str(), it->second.second, numel);
    *p = t->flat_p + it->second.first;
    *g = t->flat_g + it->second.first;
    return PN_OK;
}

int new_layer(pn_trainer *t, const std::string &name, int ks, int cin, int cout, bool bias, int x, bool cat, int *id) {
    TxLayer L;
    L.name = name; L.ks = ks; L.cin = cin; L.cout = cout; L.x = x; L.cat = cat;
    if (int rc = find_param(t, name + ".weight", (size_t)cout * cin * ks * ks, &L.w, &L.dw)) return rc;
    if (bias)
        if (int rc = find_param(t, name + ".bias", (size_t)cout, &L.b, &L.db)) return rc;
    t->layers.push_back(L);
    *id = (int)t->layers.size() - 1;
    return PN_OK;
}

int new_bn(pn_trainer *t, const std::string &name, int C, int *id) {
    TxBn b;
    b.name = name; b.C = C;
    if (int rc = find_param(t, name + ".weight", (size_t)C, &b.gamma, &b.dgamma)) return rc;
    const float *bp = nullptr;
    if (int rc = find_param(t, name + ".bias", (size_t)C, &bp, &b.dbeta)) return rc;
    b.beta = bp;
    auto rm = t->stats.find(name + ".running_mean"), rv = t->stats.find(name + ".running_var");
    if (rm == t->stats.end() || rv == t->stats.end()) return pn_set_error(t->ctx, PN_ERR_INVALID, "pn_trainer: running statistics of %s were not set", name.c_str());
    b.rm = rm->second; b.rv = rv->second;
    float *blk = nullptr;
    if (int rc = tx_alloc(t, (void **)&blk, (size_t)7 * C * 4, true)) return rc;
    b.mean = blk; b.invstd = blk + C; b.scale = blk + 2 * C; b.shift = blk + 3 * C; b.k1 = blk + 4 * C; b.k2 = blk + 5 * C; b.k3 = blk + 6 * C;
    t->bns.push_back(b);
    *id = (int)t->bns.size() - 1;
    return PN_OK;
}

unsigned grid_for(long items, int cus) {          // grid-stride elementwise launches: enough blocks to fill the chip, no more
    const long want = (items + 255) / 256;
    return (unsigned)std::max<long>(1, std::min<long>(want, (long)cus * 16));
}

// One 256-thread launch of kern, written once in terms of T: float in the fp32 engine, bf on [hi | lo] planes (TxTensor::split() is 0 / plane accordingly)
#define TX_LAUNCH_T(t, kern, grid, s, ...)                                                              \
    do {                                                                                               \
        if ((t)->f32) { using T = float; hipLaunchKernelGGL((kern), grid, dim3(256), 0, s, __VA_ARGS__); } \
        else { using T = bf; hipLaunchKernelGGL((kern), grid, dim3(256), 0, s, __VA_ARGS__); }          \
    } while (0)

// ---- convolution groups (one launch per kernel instantiation, blockIdx.y = problem) -------------------------------------------------
struct PlannedConv { ConvUse u; ConvGeom g; int rows, kplane, cin_chunks, cout_pad; };

int ensure_pack(pn_trainer *t, const PlannedConv &pc, bf **dst_out) {
    TxLayer &L = t->layers[pc.u.layer];
    bf *&slot = pc.u.dgrad ? L.pack_d : L.pack_f;
    if (slot) { *dst_out = slot; return PN_OK; }
    const int ksteps = pc.cin_chunks * pc.g.ks * pc.g.ks * 2;
    const bool k4 = pc.g.kern == 4;
    const size_t real_groups = pn_conv_pack_frags(pc.g, pc.cout_pad, ksteps) * 64;      // one lane's share of a fragment: 8 values
    if (int rc = tx_alloc(t, (void **)&slot, pn_conv_pack_bytes(t->prec(), pc.g, pc.cout_pad, ksteps), true)) return rc;
    tx::PackDesc d;
    memset(&d, 0, sizeof d);
    d.w = L.w; d.dst = slot; d.f32 = t->f32 ? 1 : 0; d.Cout = L.cout; d.Cin = L.cin; d.ks = pc.g.ks;
    d.transpose = pc.u.dgrad ? 1 : 0; d.conv4 = k4 ? 1 : 0;
    d.CT = pc.g.kern == 3 ? 2 : pn_cfg_ct(pc.g.cfg);
    d.rows_valid = pc.rows; d.kplane = pc.kplane; d.ksteps = ksteps;
    d.row_map = (pc.u.dgrad && L.cat) ? t->cat_k_map : nullptr;
    d.k_map = (!pc.u.dgrad && L.cat) ? t->cat_k_map : nullptr;
    d.first_group = t->pack_groups; d.ngroups = (unsigned)real_groups;
    t->pack_groups += (unsigned)real_groups;
    d.first_unit = t->pack_units; d.nunits = (unsigned)((size_t)pc.cout_pad * pc.kplane / 8);
    t->pack_units += d.nunits;
    t->packs.push_back(d);
    *dst_out = slot;
    return PN_OK;
}

int add_conv_group(pn_trainer *t, const std::vector<ConvUse> &uses) {
    pn_ctx *ctx = t->ctx;
    const int prec = t->prec();
    std::vector<PlannedConv> pcs;
    std::vector<PnLevelConv> lv;
    for (const ConvUse &u : uses) {
        const TxLayer &L = t->layers[u.layer];
        const TxTensor &in = t->T[u.in];
        PlannedConv pc;
        pc.u = u;
        pc.g = ConvGeom();
        pc.g.ks = L.ks;
        pc.rows = u.dgrad ? t->T[L.x].plane : L.cout;
        pc.kplane = in.plane;
        if (pc.kplane % 64) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "pn_trainer: %s: input plane %d is not a multiple of 64", L.name.c_str(), pc.kplane);
        pc.cin_chunks = (t->f32 ? 1 : 3) * pc.kplane / 64;
        pcs.push_back(pc);
        PnLevelConv l;
        l.H = in.H; l.W = in.W; l.rows = pc.rows; l.ks = L.ks; l.stride = 1; l.cin_gt64 = pc.kplane > 64;
        lv.push_back(l);
    }
    pn_plan_level(lv, t->B, !t->f32, -1);          // conv4 by block count: the trainer does not honour POPNET_CONV4
    for (size_t i = 0; i < pcs.size(); ++i) {
        PlannedConv &pc = pcs[i];
        const TxLayer &L = t->layers[pc.u.layer];
        const TxTensor &in = t->T[pc.u.in];
        pn_plan_conv_kernel(prec, t->B, ctx->num_cus, in.H, in.W, pc.rows, pc.cin_chunks, lv[i].wc_min, lv[i].nbuf_min, lv[i].k4_level, t->sw, pc.g);
        const char *why = "";
        if (int rc = pn_plan_conv_tiles(prec, in.H, in.W, pc.g, &why)) return pn_set_error(ctx, rc, "pn_trainer: %s: %s", L.name.c_str(), why);
        pc.cout_pad = pn_conv_cout_pad(pc.g, pc.rows);
    }
    std::vector<bool> used(pcs.size(), false);
    for (size_t i = 0; i < pcs.size(); ++i) {
        if (used[i]) continue;
        std::vector<size_t> members;
        const PlannedConv &a = pcs[i];
        for (size_t j = i; j < pcs.size(); ++j) {
            const PlannedConv &b = pcs[j];
            if (used[j]) continue;
            if (pn_conv_same_launch(a.g, b.g)) { members.push_back(j); used[j] = true; }
        }
        std::vector<ConvProblem> probs;
        int max_blocks = 0;
        bool two_bufs = false;
        for (size_t m : members) {
            const PlannedConv &pc = pcs[m];
            TxLayer &L = t->layers[pc.u.layer];
            const TxTensor &in = t->T[pc.u.in];
            ConvProblem P;
            memset(&P, 0, sizeof P);
            bf *pack = nullptr;
            if (int rc = ensure_pack(t, pc, &pack)) return rc;
            pn_fill_conv_problem(P, {in.p, in.H, in.W, in.cs(), in.plane, (size_t)t->B * in.H * in.W * in.plane * 4}, t->B, pc.cin_chunks, pc.rows, pc.g, prec, !t->f32);
            P.wpack = pack;
            if (!pc.u.dgrad && L.b) {
                if (!L.bias_pad) {
                    if (int rc = tx_alloc(t, (void **)&L.bias_pad, (size_t)pad64(std::max(pc.cout_pad, 128)) * 4, true)) return rc;
                    tx::BiasDesc bd;
                    bd.src = L.b; bd.dst = L.bias_pad; bd.n = L.cout; bd.npad = pad64(std::max(pc.cout_pad, 128));
                    t->biases.push_back(bd);
                }
                P.bias = L.bias_pad;
            } else P.bias = t->zero_bias;
            if (pc.u.out >= 0) { const TxTensor &o = t->T[pc.u.out]; P.out = o.p; P.out_cs = o.cs(); P.out_coff = pc.u.out_coff; P.split = o.split(); }
            if (pc.u.res >= 0) { const TxTensor &r = t->T[pc.u.res]; P.res = r.p; P.res_cs = r.cs(); P.res_coff = 0; P.res_split = r.split(); }
            P.out_nchw = pc.u.out_nchw;
            P.act = pc.u.act;
            P.yolo_naf = 50;
            if (P.lds_two) two_bufs = true;
            max_blocks = std::max(max_blocks, P.nblocks);
            probs.push_back(P);
            t->flops_conv += 2.0 * (t->f32 ? 1.0 : 3.0) * (double)t->B * in.H * in.W * pc.rows * pc.kplane * pc.g.ks * pc.g.ks;
        }
        ConvProblem *dev = nullptr;
        if (int rc = tx_alloc(t, (void **)&dev, probs.size() * sizeof(ConvProblem), false)) return rc;
        PN_HIP_CHECK(ctx, hipMemcpy(dev, probs.data(), probs.size() * sizeof(ConvProblem), hipMemcpyHostToDevice));
        ConvLaunch cl;
        pn_fill_conv_launch(cl, prec, a.g, (int)probs.size(), max_blocks, two_bufs);
        cl.probs_dev = dev;
        t->launches.push_back(cl);
        const size_t li = t->launches.size() - 1;
        t->ops.push_back([t, li](hipStream_t s) { return pn_launch_conv(t->ctx, t->launches[li], s); });
        std::string body = jf("\"kernels\": [\"%s\"], \"problems\": [", pn_conv_kernel_label(cl.prec, cl.kern, false, cl.ks, 1, cl.pitch, cl.cfg, cl.wc, cl.wp, cl.nbuf, cl.pt, cl.rpg).c_str());
        for (size_t m = 0; m < members.size(); ++m) {
            const PlannedConv &pc = pcs[members[m]];
            const TxLayer &L = t->layers[pc.u.layer];
            int hs = -1, hb = -1;
            for (int st = 0; st < 2; ++st)
                for (int b = 0; b < 3; ++b)
                    if (pc.u.out_nchw && pc.u.out_nchw == t->head_out[st][b]) { hs = st; hb = b; }
            body += jf("%s{\"layer\": \"%s\", \"dgrad\": %d, \"act\": %d, \"bias\": %d, \"ks\": %d, \"cin\": %d, \"cout\": %d, \"cat\": %d, \"rows\": %d, \"R\": %d, \"Wt\": %d, ",
                       m ? ", " : "", L.name.c_str(), pc.u.dgrad ? 1 : 0, pc.u.act, (!pc.u.dgrad && L.b) ? 1 : 0, pc.g.ks, L.cin, L.cout, L.cat ? 1 : 0, pc.rows, pc.g.R, pc.g.Wt);
            body += "\"in\": " + jref(pc.u.in, 0, t->T[pc.u.in].plane) + ", \"out\": " + jref(pc.u.out, pc.u.out_coff, pc.rows) + ", \"res\": " + jref(pc.u.res, 0, pc.rows);
            body += hs >= 0 ? jf(", \"nchw\": \"head_out.%d.%d\"}", hs, hb) : std::string(", \"nchw\": null}");
        }
        describe(t, "conv", body + "]");
    }
    return PN_OK;
}

// ---- BatchNorm / reductions ----------------------------------------------------------------------------------------------------------
int red_blocks(const pn_trainer *t, long npix, int C, int *ppb) {
    const int PL = 256 / (C / 8);
    long per = std::max<long>((npix + 4 * t->ctx->num_cus - 1) / (4 * t->ctx->num_cus), 8L * PL);     // >= 8 pixels per thread, ~4 blocks per CU
    per = (per + PL - 1) / PL * PL;
    *ppb = (int)per;
    return (int)((npix + per - 1) / per);
}

int need_partial(pn_trainer *t, size_t doubles) { t->partial_doubles = std::max(t->partial_doubles, doubles); return PN_OK; }

// split per-channel reductions over up to three tensors in one launch (blockIdx.y = tensor), their partial sums side by side in t->partial
struct RedPlan {
    struct Geo { long npix; int C, ppb, nblk; size_t poff; } g[3];
    size_t doubles = 0;
    int max_nblk = 0, max_c = 0;
    long max_items = 0;
    void add(pn_trainer *t, int i, int x, int C) {           // tensor x, its first C channels
        const TxTensor X = t->T[x];
        g[i].npix = (long)t->B * X.H * X.W; g[i].C = C;
        g[i].nblk = red_blocks(t, g[i].npix, C, &g[i].ppb);
        g[i].poff = doubles; doubles += (size_t)g[i].nblk * C * 2;
        max_nblk = std::max(max_nblk, g[i].nblk); max_c = std::max(max_c, C); max_items = std::max(max_items, g[i].npix * (C / 8));
        need_partial(t, doubles);
    }
};

struct BnUse { int bn, x, res, y, act; };                 // forward: y = act(bn(x) [+ res])
struct BnBwdUse { int bn, x, dy, y, dx, dres, act; bool has_res; };

// up to three independent BatchNorm layers (the branches of a stage level) per launch: blockIdx.y = layer
void op_bn_fwd(pn_trainer *t, std::vector<BnUse> uses) {
    const int n = (int)uses.size();
    RedPlan rp;
    for (int i = 0; i < n; ++i) rp.add(t, i, uses[i].x, t->bns[uses[i].bn].C);
    t->ops.push_back([=](hipStream_t s) {
        tx::Multi<tx::RedArgs> r;
        tx::Multi<tx::BnFinArgs> f;
        tx::Multi<tx::BnApplyArgs> a;
        memset(&r, 0, sizeof r); memset(&f, 0, sizeof f); memset(&a, 0, sizeof a);
        for (int i = 0; i < n; ++i) {
            const TxBn &b = t->bns[uses[i].bn];
            const TxTensor X = t->T[uses[i].x], Y = t->T[uses[i].y];
            tx::RedArgs &ri = r.a[i];
            ri.x = X.p; ri.x_cs = X.cs(); ri.x_split = X.split(); ri.C = rp.g[i].C; ri.npix = rp.g[i].npix; ri.ppb = rp.g[i].ppb; ri.nblk = rp.g[i].nblk; ri.partial = t->partial + rp.g[i].poff;
            tx::BnFinArgs &fi = f.a[i];
            fi.partial = t->partial + rp.g[i].poff; fi.nblk = rp.g[i].nblk; fi.C = rp.g[i].C; fi.n = (double)rp.g[i].npix; fi.gamma = b.gamma; fi.beta = b.beta;
            fi.mean = b.mean; fi.invstd = b.invstd; fi.scale = b.scale; fi.shift = b.shift; fi.running_mean = b.rm; fi.running_var = b.rv;
            fi.momentum = t->momentum; fi.eps = t->eps;
            tx::BnApplyArgs &ai = a.a[i];
            ai.x = X.p; ai.x_cs = X.cs(); ai.x_split = X.split();
            if (uses[i].res >= 0) { const TxTensor R = t->T[uses[i].res]; ai.res = R.p; ai.res_cs = R.cs(); ai.res_split = R.split(); }
            ai.y = Y.p; ai.y_cs = Y.cs(); ai.y_split = Y.split(); ai.scale = b.scale; ai.shift = b.shift; ai.act = uses[i].act; ai.C = rp.g[i].C; ai.npix = rp.g[i].npix;
        }
        TX_LAUNCH_T(t, (tx::reduce_kernel<0, T>), dim3(rp.max_nblk, n), s, r);
        hipLaunchKernelGGL(tx::bn_finish_kernel, dim3((rp.max_c + 3) / 4, n), dim3(256), 0, s, f);
        TX_LAUNCH_T(t, tx::bn_apply_kernel<T>, dim3(grid_for(rp.max_items, t->ctx->num_cus), n), s, a);
        PN_HIP_CHECK(t->ctx, hipGetLastError());
        return (int)PN_OK;
    });
    std::string body = jf("\"kernels\": [\"reduce_kernel<0>\", \"bn_finish_kernel\", \"bn_apply_kernel\"], \"problems\": [");
    for (int i = 0; i < n; ++i) {
        body += jf("%s{\"bn\": \"%s\", \"act\": %d, \"C\": %d, \"ppb\": %d, \"nblk\": %d, ", i ? ", " : "", t->bns[uses[i].bn].name.c_str(), uses[i].act, rp.g[i].C, rp.g[i].ppb, rp.g[i].nblk);
        body += "\"x\": " + jref(uses[i].x, 0, rp.g[i].C) + ", \"res\": " + jref(uses[i].res, 0, rp.g[i].C) + ", \"y\": " + jref(uses[i].y, 0, rp.g[i].C) + "}";
    }
    describe(t, "bn_fwd", body + "]");
}
void op_bn_fwd(pn_trainer *t, int bn, int x, int res, int y, int act) { op_bn_fwd(t, std::vector<BnUse>{{bn, x, res, y, act}}); }

void op_bn_bwd(pn_trainer *t, std::vector<BnBwdUse> uses) {
    const int n = (int)uses.size();
    RedPlan rp;
    for (int i = 0; i < n; ++i) rp.add(t, i, uses[i].x, t->bns[uses[i].bn].C);
    t->ops.push_back([=](hipStream_t s) {
        tx::Multi<tx::RedArgs> r;
        tx::Multi<tx::BnBwdFinArgs> f;
        tx::Multi<tx::BnBwdApplyArgs> a;
        memset(&r, 0, sizeof r); memset(&f, 0, sizeof f); memset(&a, 0, sizeof a);
        for (int i = 0; i < n; ++i) {
            const BnBwdUse &u = uses[i];
            const TxBn &b = t->bns[u.bn];
            const TxTensor X = t->T[u.x], DY = t->T[u.dy], Y = t->T[u.y], DX = u.dx >= 0 ? t->T[u.dx] : TxTensor();
            // the activation's sign: from the stored output when a residual went into it, else recomputed from x (one tensor less to read)
            const char *ysrc = (u.act && u.has_res) ? Y.p : nullptr;
            tx::RedArgs &ri = r.a[i];
            ri.x = X.p; ri.x_cs = X.cs(); ri.x_split = X.split(); ri.dy = DY.p; ri.dy_cs = DY.cs(); ri.dy_split = DY.split();
            ri.y = ysrc; ri.y_cs = Y.cs(); ri.mean = b.mean; ri.invstd = b.invstd; ri.scale = b.scale; ri.shift = b.shift; ri.act = u.act;
            ri.C = rp.g[i].C; ri.npix = rp.g[i].npix; ri.ppb = rp.g[i].ppb; ri.nblk = rp.g[i].nblk; ri.partial = t->partial + rp.g[i].poff;
            tx::BnBwdFinArgs &fi = f.a[i];
            fi.partial = t->partial + rp.g[i].poff; fi.nblk = rp.g[i].nblk; fi.C = rp.g[i].C; fi.n = (double)rp.g[i].npix; fi.gamma = b.gamma; fi.invstd = b.invstd;
            fi.dgamma = b.dgamma; fi.dbeta = b.dbeta; fi.k1 = b.k1; fi.k2 = b.k2; fi.k3 = b.k3;
            tx::BnBwdApplyArgs &ai = a.a[i];
            ai.x = X.p; ai.x_cs = X.cs(); ai.x_split = X.split(); ai.dy = DY.p; ai.dy_cs = DY.cs(); ai.dy_split = DY.split();
            ai.y = ysrc; ai.y_cs = Y.cs(); ai.mean = b.mean; ai.invstd = b.invstd; ai.k1 = b.k1; ai.k2 = b.k2; ai.k3 = b.k3; ai.scale = b.scale; ai.shift = b.shift;
            ai.dx = DX.p; ai.dx_cs = DX.cs(); ai.dx_split = DX.split();
            if (u.dres >= 0) { const TxTensor R = t->T[u.dres]; ai.dres = R.p; ai.dres_cs = R.cs(); ai.dres_split = R.split(); }
            ai.act = u.act; ai.C = rp.g[i].C; ai.npix = rp.g[i].npix;
        }
        TX_LAUNCH_T(t, (tx::reduce_kernel<1, T>), dim3(rp.max_nblk, n), s, r);
        hipLaunchKernelGGL(tx::bn_bwd_finish_kernel, dim3((rp.max_c + 3) / 4, n), dim3(256), 0, s, f);
        if (uses[0].dx < 0) {                     // sums and k1 / k2 / k3 only: the consumer applies them itself (the stem's weight gradient)
            PN_HIP_CHECK(t->ctx, hipGetLastError());
            return (int)PN_OK;
        }
        TX_LAUNCH_T(t, tx::bn_bwd_apply_kernel<T>, dim3(grid_for(rp.max_items, t->ctx->num_cus), n), s, a);
        PN_HIP_CHECK(t->ctx, hipGetLastError());
        return (int)PN_OK;
    });
    std::string body = uses[0].dx < 0 ? "\"kernels\": [\"reduce_kernel<1>\", \"bn_bwd_finish_kernel\"], \"problems\": ["
                                      : "\"kernels\": [\"reduce_kernel<1>\", \"bn_bwd_finish_kernel\", \"bn_bwd_apply_kernel\"], \"problems\": [";
    for (int i = 0; i < n; ++i) {
        const BnBwdUse &u = uses[i];
        body += jf("%s{\"bn\": \"%s\", \"act\": %d, \"has_res\": %d, \"C\": %d, \"ppb\": %d, \"nblk\": %d, ", i ? ", " : "", t->bns[u.bn].name.c_str(), u.act, u.has_res ? 1 : 0, rp.g[i].C, rp.g[i].ppb, rp.g[i].nblk);
        body += "\"x\": " + jref(u.x, 0, rp.g[i].C) + ", \"dy\": " + jref(u.dy, 0, rp.g[i].C) + ", \"y\": " + jref(u.y, 0, rp.g[i].C) + ", \"dx\": " + jref(u.dx, 0, rp.g[i].C) + ", \"dres\": " + jref(u.dres, 0, rp.g[i].C) + "}";
    }
    describe(t, "bn_bwd", body + "]");
}
void op_bn_bwd(pn_trainer *t, int bn, int x, int dy, int y, int dx, int dres, int act, bool has_res) {
    op_bn_bwd(t, std::vector<BnBwdUse>{{bn, x, dy, y, dx, dres, act, has_res}});
}

// bias gradient of layer `l` from its output gradient tensor dy (first cout channels)
void op_dbias(pn_trainer *t, int l, int dy) {
    const TxTensor DY = t->T[dy];
    RedPlan rp;
    rp.add(t, 0, dy, DY.plane);
    const long npix = rp.g[0].npix;
    const int C = DY.plane, ppb = rp.g[0].ppb, nblk = rp.g[0].nblk;
    t->ops.push_back([=](hipStream_t s) {
        const TxLayer &L = t->layers[l];
        tx::Multi<tx::RedArgs> r;
        memset(&r, 0, sizeof r);
        tx::RedArgs &ri = r.a[0];
        ri.x = DY.p; ri.x_cs = DY.cs(); ri.x_split = DY.split(); ri.C = C; ri.npix = npix; ri.ppb = ppb; ri.nblk = nblk; ri.partial = t->partial;
        TX_LAUNCH_T(t, (tx::reduce_kernel<2, T>), dim3(nblk, 1), s, r);
        hipLaunchKernelGGL(tx::sum_finish_kernel, dim3((L.cout + 3) / 4), dim3(256), 0, s, (const double *)t->partial, nblk, C, L.cout, L.db);
        PN_HIP_CHECK(t->ctx, hipGetLastError());
        return (int)PN_OK;
    });
    describe(t, "dbias", jf("\"kernels\": [\"reduce_kernel<2>\", \"sum_finish_kernel\"], \"layer\": \"%s\", \"cout\": %d, \"C\": %d, \"ppb\": %d, \"nblk\": %d, \"dy\": ",
                            t->layers[l].name.c_str(), t->layers[l].cout, C, ppb, nblk) + jref(dy, 0, C));
}

void op_add(pn_trainer *t, std::vector<std::array<int, 2>> ins /* (tensor, channel offset) */, int C, int out) {
    const TxTensor O = t->T[out];
    const long npix = (long)t->B * O.H * O.W;
    tx::AddArgs a;
    memset(&a, 0, sizeof a);
    a.n = (int)ins.size();
    for (int i = 0; i < a.n; ++i) { const TxTensor X = t->T[ins[i][0]]; a.in[i] = X.at(ins[i][1]); a.cs[i] = X.cs(); a.split[i] = X.split(); }
    a.out = O.p; a.out_cs = O.cs(); a.out_split = O.split(); a.C = C; a.npix = npix;
    t->ops.push_back([=](hipStream_t s) {
        TX_LAUNCH_T(t, tx::add_kernel<T>, dim3(grid_for(npix * (C / 8), t->ctx->num_cus)), s, a);
        PN_HIP_CHECK(t->ctx, hipGetLastError());
        return (int)PN_OK;
    });
    std::string body = "\"kernels\": [\"add_kernel\"], \"ins\": [";
    for (size_t i = 0; i < ins.size(); ++i) body += (i ? ", " : "") + jref(ins[i][0], ins[i][1], C);
    describe(t, "add", body + "], \"out\": " + jref(out, 0, C));
}

void op_pool_fwd(pn_trainer *t, int x, int y, int out_coff) {
    const TxTensor X = t->T[x], Y = t->T[y];
    t->ops.push_back([=](hipStream_t s) {
        return pn_launch_pool(t->ctx, t->prec(), 0, X.p, Y.p, t->B, X.H, X.W, X.plane, X.cs(), Y.cs(), out_coff, X.split(), Y.split(), s);
    });
    describe(t, "pool_fwd", jf("\"kernels\": [\"%s\"], \"x\": ", pn_pool_kernel_label(0, !t->f32).c_str()) + jref(x, 0, X.plane) + ", \"y\": " + jref(y, out_coff, X.plane));
}

void op_pool_bwd(pn_trainer *t, int dy, int dx) {
    const TxTensor DY = t->T[dy], DX = t->T[dx];
    t->ops.push_back([=](hipStream_t s) {
        const long items = (long)t->B * DX.H * DX.W * (DX.plane / 8);
        TX_LAUNCH_T(t, tx::avgpool_bwd_kernel<T>, dim3(grid_for(items, t->ctx->num_cus)), s, (const T *)DY.p, DY.cs(), DY.split(), (T *)DX.p, DX.cs(), DX.split(),
                    t->B, DX.H, DX.W, DY.H, DY.W, DX.plane);
        PN_HIP_CHECK(t->ctx, hipGetLastError());
        return (int)PN_OK;
    });
    describe(t, "pool_bwd", "\"kernels\": [\"avgpool_bwd_kernel\"], \"dy\": " + jref(dy, 0, DX.plane) + ", \"dx\": " + jref(dx, 0, DX.plane));
}

// loss terms and head gradients of a stage's three heads (one launch); dcat = the stage-2 input gradient whose slices reach the stage-1 heads (or -1)
void op_heads(pn_trainer *t, int stage, int dcat, const int dv[3]) {
    int nblk[3], HW = 0;
    long total[3];
    size_t poff[3], off = 0;
    int max_nblk = 0;
    TxTensor DV[3];
    for (int b = 0; b < 3; ++b) {
        DV[b] = t->T[dv[b]];
        HW = DV[b].H * DV[b].W;
        total[b] = (long)t->B * HEAD_C[b] * HW;
        nblk[b] = (int)((total[b] + 255) / 256);
        poff[b] = off; off += (size_t)nblk[b];
        max_nblk = std::max(max_nblk, nblk[b]);
    }
    need_partial(t, off);
    t->ops.push_back([=](hipStream_t s) {
        tx::Multi<tx::HeadArgs> h;
        tx::Multi<tx::LossFinArgs> f;
        memset(&h, 0, sizeof h); memset(&f, 0, sizeof f);
        for (int b = 0; b < 3; ++b) {
            tx::HeadArgs &a = h.a[b];
            a.out = t->head_out[stage][b]; a.target = t->target[b]; a.fg = b == 2 ? t->fg : nullptr;
            if (dcat >= 0) { const TxTensor D = t->T[dcat]; a.dextra = D.at(CAT_OFF[b]); a.de_cs = D.cs(); a.de_split = D.split(); }
            a.dv = DV[b].p; a.dv_cs = DV[b].cs(); a.dv_split = DV[b].split();
            a.kind = HEAD_KIND[b]; a.C = HEAD_C[b]; a.HW = HW; a.total = total[b]; a.inv_numel = (float)(1.0 / (double)total[b]); a.partial = t->partial + poff[b];
            f.a[b].partial = t->partial + poff[b]; f.a[b].nblocks = nblk[b]; f.a[b].numel = (double)total[b]; f.a[b].loss = t->loss + 3 * stage + b;
        }
        TX_LAUNCH_T(t, tx::head_kernel<T>, dim3(max_nblk, 3), s, h);
        hipLaunchKernelGGL(tx::loss_finish_kernel, dim3(3), dim3(256), 0, s, f);
        PN_HIP_CHECK(t->ctx, hipGetLastError());
        return (int)PN_OK;
    });
    std::string body = jf("\"kernels\": [\"head_kernel\", \"loss_finish_kernel\"], \"stage\": %d, \"heads\": [", stage);
    for (int b = 0; b < 3; ++b) {
        body += jf("%s{\"out\": \"head_out.%d.%d\", \"kind\": %d, \"C\": %d, \"fg\": %d, \"loss\": %d, ", b ? ", " : "", stage, b, HEAD_KIND[b], HEAD_C[b], b == 2 ? 1 : 0, 3 * stage + b);
        body += "\"dextra\": " + jref(dcat, dcat >= 0 ? CAT_OFF[b] : 0, HEAD_C[b]) + ", \"dv\": " + jref(dv[b], 0, DV[b].plane) + "}";
    }
    describe(t, "heads", body + "]");
}

// fork: the side stream may start once everything issued so far on the step's stream has finished; join: the other way round
int op_fork(pn_trainer *t) {
    if (!t->two_streams || t->ops.size() == t->side_tail) return PN_OK;
    hipEvent_t ev;
    PN_HIP_CHECK(t->ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    t->events.push_back(ev);
    t->ops.push_back([t, ev](hipStream_t s) {
        PN_HIP_CHECK(t->ctx, hipEventRecord(ev, s));
        PN_HIP_CHECK(t->ctx, hipStreamWaitEvent(t->side, ev, 0));
        return (int)PN_OK;
    });
    describe(t, "fork", "\"kernels\": []");
    return PN_OK;
}
int op_join(pn_trainer *t) {
    if (!t->two_streams) return PN_OK;
    hipEvent_t ev;
    PN_HIP_CHECK(t->ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    t->events.push_back(ev);
    t->ops.push_back([t, ev](hipStream_t s) {
        PN_HIP_CHECK(t->ctx, hipEventRecord(ev, t->side));
        PN_HIP_CHECK(t->ctx, hipStreamWaitEvent(s, ev, 0));
        return (int)PN_OK;
    });
    describe(t, "join", "\"kernels\": []");
    return PN_OK;
}
// every op appended since `from` runs on the side stream
void ops_to_side(pn_trainer *t, size_t from) {
    if (!t->two_streams) return;
    for (size_t i = from; i < t->ops.size(); ++i) {
        auto f = t->ops[i];
        t->ops[i] = [t, f](hipStream_t) { return f(t->side); };
        t->op_desc[i].side = true;
    }
    t->side_tail = t->ops.size();
}

// weight gradient of layer l: x = its input tensor, dy = gradient of its output
int op_wgrad(pn_trainer *t, int l, int dy) {
    const TxLayer &L = t->layers[l];
    const TxTensor X = t->T[L.x], DY = t->T[dy];
    if (t->legacy_wgrad) {
        // stepping stone / cross-check (POPNET_TRAINX_WGRAD=legacy): hand both operands to train.hip's NCHW f32 weight-gradient kernels
        const size_t need = (size_t)t->B * X.H * X.W * std::max(L.cin, L.cout);
        t->nchw_elems = std::max(t->nchw_elems, need);
        t->ops.push_back([=](hipStream_t s) {
            const TxLayer &LL = t->layers[l];
            const int HW = X.H * X.W;
            const int *cmap = LL.cat ? (const int *)t->cat_ref_map : (const int *)nullptr;
            TX_LAUNCH_T(t, tx::planes_to_nchw_kernel<T>, dim3((HW + 63) / 64, (LL.cin + 63) / 64, t->B), s, (const T *)X.p, X.cs(), X.split(), t->nchw_a, LL.cin, HW, cmap);
            TX_LAUNCH_T(t, tx::planes_to_nchw_kernel<T>, dim3((HW + 63) / 64, (LL.cout + 63) / 64, t->B), s, (const T *)DY.p, DY.cs(), DY.split(), t->nchw_b, LL.cout, HW, (const int *)nullptr);
            PN_HIP_CHECK(t->ctx, hipGetLastError());
            return pn_conv2d_wgrad(t->ctx, t->nchw_a, t->nchw_b, LL.dw, LL.db, t->B, LL.cin, X.H, X.W, LL.cout, LL.ks, 1, LL.ks / 2, (void *)s);
        });
        describe(t, "wgrad", jf("\"kernels\": [\"planes_to_nchw_kernel\", \"pn_conv2d_wgrad\"], \"layer\": \"%s\", \"ks\": %d, \"cin\": %d, \"cout\": %d, \"cat\": %d, \"bias\": %d, \"x\": ",
                                L.name.c_str(), L.ks, L.cin, L.cout, L.cat ? 1 : 0, L.db ? 1 : 0) + jref(L.x, 0, X.plane) + ", \"dy\": " + jref(dy, 0, DY.plane));
        return PN_OK;
    }
    if (L.b && !L.bn_follows) op_dbias(t, l, dy);      // (a bias in front of a BatchNorm: its gradient is identically zero and the flat gradient buffer already holds 0)
    if (int rc = op_fork(t)) return rc;
    const size_t from = t->ops.size();
    tx::WgPlan wp;
    auto plan = [&](auto *null) {              // typed by the null pointer: const float * or const bf *
        typedef decltype(null) P;
        return tx::plan_wgrad(t->ctx, t->B, X.H, X.W, (P)X.p, X.plane, (P)DY.p, DY.plane, L.cin, L.cout, L.ks, L.cat ? t->cat_k_map : nullptr, L.dw, &t->wg_partial, &t->wg_partial_floats, t->ops, &wp);
    };
    if (int rc = t->f32 ? plan((const float *)nullptr) : plan((const bf *)nullptr)) return rc;
    describe(t, "wgrad", jf("\"kernels\": [\"%s<%d, 2>\", \"wgrad_reduce_kernel\"], \"layer\": \"%s\", \"ks\": %d, \"cin\": %d, \"cout\": %d, \"cat\": %d, \"tiles_x\": %d, \"Wt\": %d, "
                            "\"rows_per_block\": %d, \"Sr\": %d, \"x\": ", t->f32 ? "wgrad_f32_kernel" : "wgrad_stream_kernel", L.ks, L.name.c_str(), L.ks, L.cin, L.cout, L.cat ? 1 : 0,
                            wp.tiles_x, wp.Wt, wp.rows_per_block, wp.Sr) + jref(L.x, 0, X.plane) + ", \"dy\": " + jref(dy, 0, DY.plane));
    ops_to_side(t, from);
    return PN_OK;
}

int build(pn_trainer *t) {
    pn_ctx *ctx = t->ctx;
    const int B = t->B, H = t->H, W = t->W;
    if (H % 8 || W % 8) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "pn_trainer: input size must be a multiple of 8");
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8;
    // one frame on a 1 x 1 stage map: the stage BatchNorms would see ONE value per channel -- batch variance 0, xhat == 0, and the gradient behind every one
    // of them identically zero: nothing trains (nn.BatchNorm2d raises for it, pn_bn_train_forward of the NCHW engine refuses it as well)
    if ((long)B * H8 * W8 < 2)
        return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "pn_trainer: model1_1.1: train-mode BatchNorm over one value per channel (batch %d on a %d x %d stage map): no batch statistics", B, H8, W8);
    int rc;
    if ((rc = tx_alloc(t, (void **)&t->zero_bias, 1024 * 4, true))) return rc;
    {   // channel maps of the stage-2 input: mine [feat 0..127 | paf 128.. | heat 156.. | z 172.. | pad] <-> reference [paf, heat, z, feat] (rtpose_light3d.py:339)
        std::vector<int> k(CAT_PLANE, -1), r(187, -1);
        for (int i = 0; i < 128; ++i) k[i] = 59 + i;
        for (int i = 0; i < 28; ++i) k[128 + i] = i;
        for (int i = 0; i < 16; ++i) k[156 + i] = 28 + i;
        for (int i = 0; i < 15; ++i) k[172 + i] = 44 + i;
        for (int i = 0; i < CAT_PLANE; ++i) if (k[i] >= 0) r[k[i]] = i;
        if ((rc = tx_alloc(t, (void **)&t->cat_k_map, k.size() * 4, false))) return rc;
        if ((rc = tx_alloc(t, (void **)&t->cat_ref_map, r.size() * 4, false))) return rc;
        PN_HIP_CHECK(ctx, hipMemcpy(t->cat_k_map, k.data(), k.size() * 4, hipMemcpyHostToDevice));
        PN_HIP_CHECK(ctx, hipMemcpy(t->cat_ref_map, r.data(), r.size() * 4, hipMemcpyHostToDevice));
    }
    auto TT = [&](int h, int w, int plane, int *id) { return new_tensor(t, h, w, plane, id); };
#define TX(expr) do { if ((rc = (expr))) return rc; } while (0)

    // ---------------- forward ----------------
    // step prologue: every weight pack and padded bias from the live parameters -- on the side stream, under the stem (which reads the raw parameters)
    TX(op_fork(t));
    const size_t pack_from = t->ops.size();
    t->ops.push_back([t](hipStream_t s) {
        if (t->pack_groups && t->pack_gather) hipLaunchKernelGGL(tx::pack_kernel, dim3((t->pack_groups + 255) / 256), dim3(256), 0, s, (const tx::PackDesc *)t->packs_dev, (int)t->packs.size(), t->pack_groups);
        else if (t->pack_units) hipLaunchKernelGGL(tx::pack_rows_kernel, dim3((t->pack_units + 255) / 256), dim3(256), 0, s, (const tx::PackDesc *)t->packs_dev, (int)t->packs.size(), t->pack_units);
        if (!t->biases.empty()) hipLaunchKernelGGL(tx::bias_kernel, dim3((unsigned)t->biases.size()), dim3(128), 0, s, (const tx::BiasDesc *)t->biases_dev, (int)t->biases.size());
        PN_HIP_CHECK(t->ctx, hipGetLastError());
        return (int)PN_OK;
    });
    describe(t, "pack", jf("\"kernels\": [\"%s\", \"bias_kernel\"]", t->pack_gather ? "pack_kernel" : "pack_rows_kernel"));
    ops_to_side(t, pack_from);
    // stem: model0.conv1 7x7 / 2 on the NCHW f32 image (train.hip), handed over as planes
    int C0, A0;
    TX(TT(H2, W2, 64, &C0)); TX(TT(H2, W2, 64, &A0));
    const float *w_stem = nullptr; float *dw_stem = nullptr;
    TX(find_param(t, "model0.conv1.weight", 64 * 49, &w_stem, &dw_stem));
    t->nchw_elems = std::max(t->nchw_elems, (size_t)B * 64 * H2 * W2);
    {
        const TxTensor c0 = t->T[C0];
        const bool handover = t->sw.trainx_stem_handover;                  // the NCHW f32 hand-over of the round's first builds (bit-identical; A/B)
        const int stem_gather = t->sw.trainx_stem_gather;                  // A/B: tconv_fwd_kernel<7, PL> instead of tstem_fwd_kernel (bit-identical)
        t->ops.push_back([=](hipStream_t s) {
            if (!handover) return pn_stem_forward_planes(t->ctx, t->img, w_stem, c0.p, c0.cs(), c0.split(), t->f32, B, 1, H, W, 64, 7, 2, 3, stem_gather, s);
            if (int r = pn_conv2d_forward(t->ctx, t->img, w_stem, nullptr, t->nchw_a, B, 1, H, W, 64, 7, 2, 3, 0, (void *)s)) return r;
            const int HW = H2 * W2;
            TX_LAUNCH_T(t, tx::nchw_to_planes_kernel<T>, dim3((HW + 63) / 64, 1, B), s, (const float *)t->nchw_a, (T *)c0.p, 64, HW, c0.cs(), c0.split());
            PN_HIP_CHECK(t->ctx, hipGetLastError());
            return (int)PN_OK;
        });
        describe(t, "stem_fwd", jf("\"kernels\": [%s], \"layer\": \"model0.conv1\", \"out\": ",
                                   handover ? "\"tconv_fwd_kernel\", \"nchw_to_planes_kernel\"" : (stem_gather ? "\"tconv_fwd_kernel<7>\"" : "\"tstem_fwd_kernel\"")) + jref(C0, 0, 64));
    }
    int bn_stem;
    TX(new_bn(t, "model0.bn1", 64, &bn_stem));
    op_bn_fwd(t, bn_stem, C0, -1, A0, 1);
    TX(op_join(t));                               // the packs are ready before the first planes convolution

    struct Block { int l1, l2, lds, bn1, bn2, bnds, C1, A1, C2, CD, D, in, out; };
    auto basic_block = [&](const std::string &p, int xin, int cin, int cout, int h, int w, bool down, Block *bk) -> int {
        int rc2;
        Block b;
        memset(&b, 0, sizeof b);
        b.in = xin; b.lds = b.bnds = b.CD = b.D = -1;
        if ((rc2 = TT(h, w, cout, &b.C1)) || (rc2 = TT(h, w, cout, &b.A1)) || (rc2 = TT(h, w, cout, &b.C2)) || (rc2 = TT(h, w, cout, &b.out))) return rc2;
        if ((rc2 = new_layer(t, p + ".conv1", 3, cin, cout, false, xin, false, &b.l1))) return rc2;
        if ((rc2 = new_bn(t, p + ".bn1", cout, &b.bn1))) return rc2;
        if ((rc2 = new_layer(t, p + ".conv2", 3, cout, cout, false, b.A1, false, &b.l2))) return rc2;
        if ((rc2 = new_bn(t, p + ".bn2", cout, &b.bn2))) return rc2;
        std::vector<ConvUse> lv = {{b.l1, false, xin, b.C1, 0, -1, PN_ACT_NONE, nullptr}};
        if (down) {
            if ((rc2 = TT(h, w, cout, &b.CD)) || (rc2 = TT(h, w, cout, &b.D))) return rc2;
            if ((rc2 = new_layer(t, p + ".downsample.0", 1, cin, cout, false, xin, false, &b.lds))) return rc2;
            if ((rc2 = new_bn(t, p + ".downsample.1", cout, &b.bnds))) return rc2;
            lv.push_back({b.lds, false, xin, b.CD, 0, -1, PN_ACT_NONE, nullptr});
        }
        if ((rc2 = add_conv_group(t, lv))) return rc2;
        op_bn_fwd(t, b.bn1, b.C1, -1, b.A1, 1);
        if (down) op_bn_fwd(t, b.bnds, b.CD, -1, b.D, 0);
        if ((rc2 = add_conv_group(t, {{b.l2, false, b.A1, b.C2, 0, -1, PN_ACT_NONE, nullptr}}))) return rc2;
        op_bn_fwd(t, b.bn2, b.C2, down ? b.D : xin, b.out, 1);
        *bk = b;
        return PN_OK;
    };
    Block b10, b11, b20;
    TX(basic_block("model0.layer1.0", A0, 64, 64, H2, W2, false, &b10));
    TX(basic_block("model0.layer1.1", b10.out, 64, 64, H2, W2, false, &b11));
    int P1;
    TX(TT(H4, W4, 64, &P1));
    op_pool_fwd(t, b11.out, P1, 0);
    TX(basic_block("model0.layer2.0", P1, 64, 128, H4, W4, true, &b20));
    int l_c2, bn_c2, C7, A7, FEAT, CAT;
    TX(TT(H4, W4, 128, &C7)); TX(TT(H4, W4, 128, &A7)); TX(TT(H8, W8, 128, &FEAT)); TX(TT(H8, W8, CAT_PLANE, &CAT));
    TX(new_layer(t, "model0.conv2", 1, 128, 128, false, b20.out, false, &l_c2));
    TX(new_bn(t, "model0.bn2", 128, &bn_c2));
    TX(add_conv_group(t, {{l_c2, false, b20.out, C7, 0, -1, PN_ACT_NONE, nullptr}}));
    op_bn_fwd(t, bn_c2, C7, -1, A7, 1);
    op_pool_fwd(t, A7, FEAT, 0);              // feat: the stage-1 input ...
    op_pool_fwd(t, A7, CAT, 0);               // ... and channels 0..127 of the stage-2 input (torch.cat is never executed)

    // stages (make_stages, rtpose_light3d.py:222-246, 263-309): conv BN LeakyReLU x 4, bare conv; three branches per level share a launch
    const int BR_C[3][4] = {{256, 256, 256, 128}, {128, 128, 128, 128}, {128, 64, 64, 64}};
    const int BR_KS[3][5] = {{3, 3, 3, 1, 1}, {3, 3, 3, 3, 3}, {3, 3, 3, 3, 3}};
    struct Branch { int l[5], bn[4], C[4], A[4]; };
    Branch br[2][3];
    for (int st = 0; st < 2; ++st) {
        const int xin = st == 0 ? FEAT : CAT;
        for (int b = 0; b < 3; ++b)
            for (int lv = 0; lv < 4; ++lv) { TX(TT(H8, W8, BR_C[b][lv], &br[st][b].C[lv])); TX(TT(H8, W8, BR_C[b][lv], &br[st][b].A[lv])); }
        for (int lv = 0; lv < 5; ++lv) {
            std::vector<ConvUse> uses;
            for (int b = 0; b < 3; ++b) {
                char nm[48];
                snprintf(nm, sizeof nm, "model%d_%d.%d", st + 1, b + 1, 3 * lv);
                const int in = lv == 0 ? xin : br[st][b].A[lv - 1];
                const int cin = lv == 0 ? (st == 0 ? 128 : 187) : BR_C[b][lv - 1];
                const int cout = lv < 4 ? BR_C[b][lv] : HEAD_C[b];
                TX(new_layer(t, nm, BR_KS[b][lv], cin, cout, true, in, lv == 0 && st == 1, &br[st][b].l[lv]));
                if (lv < 4) {
                    t->layers[br[st][b].l[lv]].bn_follows = true;
                    snprintf(nm, sizeof nm, "model%d_%d.%d", st + 1, b + 1, 3 * lv + 1);
                    TX(new_bn(t, nm, cout, &br[st][b].bn[lv]));
                    uses.push_back({br[st][b].l[lv], false, in, br[st][b].C[lv], 0, -1, PN_ACT_NONE, nullptr});
                } else {
                    TX(tx_alloc(t, (void **)&t->head_out[st][b], (size_t)B * cout * H8 * W8 * 4, true));
                    // the head's sigmoid range cast runs in the convolution epilogue; stage 1 also writes its slice of the stage-2 input
                    uses.push_back({br[st][b].l[lv], false, in, st == 0 ? CAT : -1, st == 0 ? CAT_OFF[b] : 0, -1, HEAD_ACT[b], t->head_out[st][b]});
                }
            }
            TX(add_conv_group(t, uses));
            if (lv < 4) {
                std::vector<BnUse> bu;
                for (int b = 0; b < 3; ++b) bu.push_back({br[st][b].bn[lv], br[st][b].C[lv], -1, br[st][b].A[lv], 2});
                op_bn_fwd(t, bu);
            }
        }
    }

    // ---------------- backward ----------------
    auto stage_bwd = [&](int st, int dcat_in /* -1 for stage 2 */, int dx_plane, int *dx_out /* three tensors */) -> int {
        int rc2;
        int dy[3];
        for (int b = 0; b < 3; ++b)
            if ((rc2 = TT(H8, W8, 64, &dy[b]))) return rc2;
        op_heads(t, st, dcat_in, dy);
        for (int lv = 4; lv >= 0; --lv) {
            int dc[3];
            std::vector<BnBwdUse> bu;
            for (int b = 0; b < 3; ++b) {
                if (lv < 4) {
                    if ((rc2 = TT(H8, W8, BR_C[b][lv], &dc[b]))) return rc2;
                    bu.push_back({br[st][b].bn[lv], br[st][b].C[lv], dy[b], br[st][b].A[lv], dc[b], -1, 2, false});
                } else dc[b] = dy[b];
            }
            if (!bu.empty()) op_bn_bwd(t, bu);
            for (int b = 0; b < 3; ++b)
                if ((rc2 = op_wgrad(t, br[st][b].l[lv], dc[b]))) return rc2;
            std::vector<ConvUse> uses;
            for (int b = 0; b < 3; ++b) {
                const int plane = lv == 0 ? dx_plane : BR_C[b][lv - 1];
                if ((rc2 = TT(H8, W8, plane, &dy[b]))) return rc2;
                uses.push_back({br[st][b].l[lv], true, dc[b], dy[b], 0, -1, PN_ACT_NONE, nullptr});
            }
            if ((rc2 = add_conv_group(t, uses))) return rc2;
        }
        for (int b = 0; b < 3; ++b) dx_out[b] = dy[b];
        return PN_OK;
    };
    int dcat_b[3], dfeat_b[3], DCAT, DFEAT;
    TX(stage_bwd(1, -1, CAT_PLANE, dcat_b));
    TX(TT(H8, W8, CAT_PLANE, &DCAT));
    op_add(t, {{dcat_b[0], 0}, {dcat_b[1], 0}, {dcat_b[2], 0}}, CAT_PLANE, DCAT);
    TX(stage_bwd(0, DCAT, 128, dfeat_b));
    TX(TT(H8, W8, 128, &DFEAT));
    op_add(t, {{DCAT, 0}, {dfeat_b[0], 0}, {dfeat_b[1], 0}, {dfeat_b[2], 0}}, 128, DFEAT);
    int dA7, dC7, dA6;
    TX(TT(H4, W4, 128, &dA7)); TX(TT(H4, W4, 128, &dC7)); TX(TT(H4, W4, 128, &dA6));
    op_pool_bwd(t, DFEAT, dA7);
    op_bn_bwd(t, bn_c2, C7, dA7, A7, dC7, -1, 1, false);
    TX(op_wgrad(t, l_c2, dC7));
    TX(add_conv_group(t, {{l_c2, true, dC7, dA6, 0, -1, PN_ACT_NONE, nullptr}}));

    auto block_bwd = [&](const Block &b, int dout, int *din, int scratch[6]) -> int {
        int rc2;
        // scratch: dC2, g (identity gradient / dD), dA1, dC1, dCD, tmp  (reused between the two 112x112 blocks)
        int dC2 = scratch[0], g = scratch[1], dA1 = scratch[2], dC1 = scratch[3];
        op_bn_bwd(t, b.bn2, b.C2, dout, b.out, dC2, g, 1, true);
        if ((rc2 = op_wgrad(t, b.l2, dC2))) return rc2;
        if ((rc2 = add_conv_group(t, {{b.l2, true, dC2, dA1, 0, -1, PN_ACT_NONE, nullptr}}))) return rc2;
        op_bn_bwd(t, b.bn1, b.C1, dA1, b.A1, dC1, -1, 1, false);
        if ((rc2 = op_wgrad(t, b.l1, dC1))) return rc2;
        if (b.lds >= 0) {
            int dCD = scratch[4], tmp = scratch[5];
            op_bn_bwd(t, b.bnds, b.CD, g, b.D, dCD, -1, 0, false);
            if ((rc2 = op_wgrad(t, b.lds, dCD))) return rc2;
            if ((rc2 = add_conv_group(t, {{b.lds, true, dCD, tmp, 0, -1, PN_ACT_NONE, nullptr}}))) return rc2;
            if ((rc2 = add_conv_group(t, {{b.l1, true, dC1, *din, 0, tmp, PN_ACT_NONE, nullptr}}))) return rc2;     // dx = dgrad(conv1) + dgrad(shortcut)
        } else {
            if ((rc2 = add_conv_group(t, {{b.l1, true, dC1, *din, 0, g, PN_ACT_NONE, nullptr}}))) return rc2;       // dx = dgrad(conv1) + identity gradient
        }
        return PN_OK;
    };
    int s56[6], dP1;
    for (int i = 0; i < 4; ++i) TX(TT(H4, W4, 128, &s56[i]));
    TX(TT(H4, W4, 128, &s56[4])); TX(TT(H4, W4, 64, &s56[5]));
    TX(TT(H4, W4, 64, &dP1));
    TX(block_bwd(b20, dA6, &dP1, s56));
    // (own scratch per block: a weight gradient still running on the side stream reads dC2 / dC1 of its block)
    // the stem's BatchNorm backward is applied inside its weight-gradient kernel (train.hip::tstem_wgrad_kernel): dC0 never exists
    const bool stem_handover = t->sw.trainx_stem_handover;                             // A/B: the NCHW f32 hand-over of the round's first builds (bit-identical)
    const bool stem_bn_separate = stem_handover || t->sw.trainx_stem_bn_separate;       // A/B: bn_bwd_apply_kernel writes dC0, the weight gradient reads it (bit-identical)
    const int stem_depth = t->sw.trainx_stem_depth;                                     // A/B: chunks of 32 pixels in flight per block (1, 2, 4; bit-identical): 102-163 / 83-91 / 105 us over six traces
    int s112[6], s112b[6], dA4, dA2, dA0, dC0 = -1;
    for (int i = 0; i < 4; ++i) { TX(TT(H2, W2, 64, &s112[i])); TX(TT(H2, W2, 64, &s112b[i])); }
    s112[4] = s112[5] = s112b[4] = s112b[5] = -1;
    TX(TT(H2, W2, 64, &dA4)); TX(TT(H2, W2, 64, &dA2));
    if (stem_bn_separate) TX(TT(H2, W2, 64, &dC0));
    op_pool_bwd(t, dP1, dA4);
    TX(block_bwd(b11, dA4, &dA2, s112));
    dA0 = dA4;                                   // free again: layer1.1's output gradient has been consumed (by launches of the step's own stream)
    TX(block_bwd(b10, dA2, &dA0, s112b));
    op_bn_bwd(t, bn_stem, C0, dA0, A0, stem_bn_separate ? dC0 : -1, -1, 1, false);
    {
        const TxTensor d0 = dC0 >= 0 ? t->T[dC0] : TxTensor(), a0 = t->T[dA0], c0 = t->T[C0];
        t->ops.push_back([=](hipStream_t s) {
            if (!stem_bn_separate) {
                const TxBn &b = t->bns[bn_stem];
                PnStemBn sb;
                sb.x = c0.p; sb.x_cs = c0.cs(); sb.x_split = c0.split();
                sb.mean = b.mean; sb.invstd = b.invstd; sb.k1 = b.k1; sb.k2 = b.k2; sb.k3 = b.k3; sb.scale = b.scale; sb.shift = b.shift; sb.act = 1;
                return pn_stem_wgrad_planes(t->ctx, t->img, a0.p, a0.cs(), a0.split(), t->f32, &sb, dw_stem, B, 1, H, W, 64, 7, 2, 3, stem_depth, s);
            }
            if (!stem_handover) return pn_stem_wgrad_planes(t->ctx, t->img, d0.p, d0.cs(), d0.split(), t->f32, nullptr, dw_stem, B, 1, H, W, 64, 7, 2, 3, stem_depth, s);
            const int HW = H2 * W2;
            TX_LAUNCH_T(t, tx::planes_to_nchw_kernel<T>, dim3((HW + 63) / 64, 1, B), s, (const T *)d0.p, d0.cs(), d0.split(), t->nchw_b, 64, HW, (const int *)nullptr);
            PN_HIP_CHECK(t->ctx, hipGetLastError());
            return pn_conv2d_wgrad(t->ctx, t->img, t->nchw_b, dw_stem, nullptr, B, 1, H, W, 64, 7, 2, 3, (void *)s);
        });
        describe(t, "stem_wgrad", jf("\"kernels\": [%s], \"layer\": \"model0.conv1\", \"bn\": %s, \"x\": ",
                                     stem_handover ? "\"planes_to_nchw_kernel\", \"pn_conv2d_wgrad\"" : "\"tstem_wgrad_kernel\"", stem_bn_separate ? "null" : "\"model0.bn1\"") +
                                      jref(C0, 0, 64) + ", \"dy\": " + jref(stem_bn_separate ? dC0 : dA0, 0, 64));
    }
    TX(op_join(t));                               // the step ends when the last weight gradient has landed
#undef TX
    // scratch and descriptor tables
    if ((rc = tx_alloc(t, (void **)&t->partial, std::max<size_t>(t->partial_doubles, 1) * 8, true))) return rc;
    if ((rc = tx_alloc(t, (void **)&t->nchw_a, std::max<size_t>(t->nchw_elems, 1) * 4, true))) return rc;
    if ((rc = tx_alloc(t, (void **)&t->nchw_b, std::max<size_t>(t->nchw_elems, 1) * 4, true))) return rc;
    if (t->wg_partial_floats)
        if ((rc = tx_alloc(t, (void **)&t->wg_partial, t->wg_partial_floats * 4, true))) return rc;
    if (!t->packs.empty()) {
        if ((rc = tx_alloc(t, (void **)&t->packs_dev, t->packs.size() * sizeof(tx::PackDesc), false))) return rc;
        PN_HIP_CHECK(ctx, hipMemcpy(t->packs_dev, t->packs.data(), t->packs.size() * sizeof(tx::PackDesc), hipMemcpyHostToDevice));
    }
    if (!t->biases.empty()) {
        if ((rc = tx_alloc(t, (void **)&t->biases_dev, t->biases.size() * sizeof(tx::BiasDesc), false))) return rc;
        PN_HIP_CHECK(ctx, hipMemcpy(t->biases_dev, t->biases.data(), t->biases.size() * sizeof(tx::BiasDesc), hipMemcpyHostToDevice));
    }
    PN_HIP_CHECK(ctx, hipDeviceSynchronize());
    if (t->op_desc.size() != t->ops.size()) return pn_set_error(ctx, PN_ERR_STATE, "pn_trainer: %zu ops, %zu descriptions", t->ops.size(), t->op_desc.size());
    return PN_OK;
}

}  // namespace

extern "C" {

pn_trainer *pn_trainer_create(pn_ctx *ctx) {
    if (!ctx) return nullptr;
    pn_trainer *t = new pn_trainer();
    t->ctx = ctx;
    return t;
}

void pn_trainer_destroy(pn_trainer *t) {
    if (!t) return;
    for (void *p : t->allocs) (void)hipFree(p);
    for (hipEvent_t ev : t->events) (void)hipEventDestroy(ev);
    if (t->side) (void)hipStreamDestroy(t->side);
    delete t;
}

int pn_trainer_set_param(pn_trainer *t, const char *name, size_t offset, size_t numel) {
    if (!t || !name) return PN_ERR_INVALID;
    if (t->finalized) return pn_set_error(t->ctx, PN_ERR_STATE, "pn_trainer: already finalized");
    t->params[name] = {offset, numel};
    return PN_OK;
}

int pn_trainer_set_stat(pn_trainer *t, const char *name, float *stat_dev) {
    if (!t || !name || !stat_dev) return PN_ERR_INVALID;
    if (t->finalized) return pn_set_error(t->ctx, PN_ERR_STATE, "pn_trainer: already finalized");
    t->stats[name] = stat_dev;
    return PN_OK;
}

int pn_trainer_set_precision(pn_trainer *t, int precision) {
    if (!t) return PN_ERR_INVALID;
    if (t->finalized) return pn_set_error(t->ctx, PN_ERR_STATE, "pn_trainer: already finalized");
    if (precision != PN_PREC_F32 && precision != PN_PREC_BF16X3) return pn_set_error(t->ctx, PN_ERR_INVALID, "pn_trainer_set_precision: PN_PREC_F32 or PN_PREC_BF16X3");
    t->f32 = precision == PN_PREC_F32;
    return PN_OK;
}

int pn_trainer_finalize(pn_trainer *t, float *flat_param_dev, float *flat_grad_dev, int B, int H, int W, float bn_momentum, float bn_eps) {
    if (!t) return PN_ERR_INVALID;
    pn_ctx *ctx = t->ctx;
    if (t->finalized) return pn_set_error(ctx, PN_ERR_STATE, "pn_trainer: already finalized");
    if (!flat_param_dev || !flat_grad_dev || B < 1 || H < 8 || W < 8) return pn_set_error(ctx, PN_ERR_INVALID, "pn_trainer_finalize: bad arguments");
    PN_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    t->flat_p = flat_param_dev; t->flat_g = flat_grad_dev; t->B = B; t->H = H; t->W = W; t->momentum = bn_momentum; t->eps = bn_eps;
    t->sw = pn_read_switches();
    t->legacy_wgrad = t->sw.trainx_legacy_wgrad;
    t->pack_gather = t->sw.trainx_pack_gather;
    t->two_streams = !t->sw.trainx_one_stream && !t->legacy_wgrad;
    if (t->two_streams) {
        // LOWEST priority: the weight gradients fill what the step's own stream (the dependency chain that bounds the step) leaves idle, never the other way round
        int lo = 0, hi = 0;
        PN_HIP_CHECK(ctx, hipDeviceGetStreamPriorityRange(&lo, &hi));
        PN_HIP_CHECK(ctx, hipStreamCreateWithPriority(&t->side, hipStreamNonBlocking, lo));
    }
    if (int rc = build(t)) return rc;
    t->finalized = true;
    return PN_OK;
}

// validates and stores the per-step arguments the ops read when they launch
static int tx_set_step_args(pn_trainer *t, const char *what, const float *img_dev, const float *heat_gt_dev, const float *paf_gt_dev, const float *z_gt_dev, const float *fg_mask_dev,
                            float *loss_terms_dev) {
    if (!t->finalized) return pn_set_error(t->ctx, PN_ERR_STATE, "%s: pn_trainer_finalize has not been called", what);
    if (!img_dev || !heat_gt_dev || !paf_gt_dev || !z_gt_dev || !fg_mask_dev || !loss_terms_dev) return pn_set_error(t->ctx, PN_ERR_INVALID, "%s: null device pointer", what);
    t->img = img_dev; t->target[0] = paf_gt_dev; t->target[1] = heat_gt_dev; t->target[2] = z_gt_dev; t->fg = fg_mask_dev; t->loss = loss_terms_dev;
    return PN_OK;
}

int pn_trainer_forward_backward(pn_trainer *t, const float *img_dev, const float *heat_gt_dev, const float *paf_gt_dev, const float *z_gt_dev, const float *fg_mask_dev,
                                float *loss_terms_dev, void *hip_stream) {
    if (!t) return PN_ERR_INVALID;
    if (int rc = tx_set_step_args(t, "pn_trainer_forward_backward", img_dev, heat_gt_dev, paf_gt_dev, z_gt_dev, fg_mask_dev, loss_terms_dev)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    for (auto &op : t->ops)
        if (int rc = op(s)) return rc;
    return PN_OK;
}

double pn_trainer_conv_flops(pn_trainer *t) { return t ? t->flops_conv : 0.0; }

// ---- diagnostics: the step as a list of described ops, runnable in ranges, with host access to every tensor (tests/test_gpu_train_layers.py) ----
int pn_trainer_num_ops(pn_trainer *t) {
    if (!t) return PN_ERR_INVALID;
    if (!t->finalized) return pn_set_error(t->ctx, PN_ERR_STATE, "pn_trainer_num_ops: trainer not finalized");
    return (int)t->ops.size();
}

int pn_trainer_op_info(pn_trainer *t, int k, char *out, size_t cap) {
    if (!t || !out || !cap) return PN_ERR_INVALID;
    pn_ctx *ctx = t->ctx;
    if (!t->finalized) return pn_set_error(ctx, PN_ERR_STATE, "pn_trainer_op_info: trainer not finalized");
    if (k < -1 || k >= (int)t->ops.size()) return pn_set_error(ctx, PN_ERR_INVALID, "pn_trainer_op_info: op %d outside [-1, %zu)", k, t->ops.size());
    std::string js;
    if (k == -1) {
        js = jf("{\"prec\": \"%s\", \"B\": %d, \"H\": %d, \"W\": %d, \"ops\": %zu, \"momentum\": %.9g, \"eps\": %.9g, \"tensors\": [", t->f32 ? "fp32" : "bf16x3", t->B, t->H, t->W, t->ops.size(),
                (double)t->momentum, (double)t->eps);
        for (size_t i = 0; i < t->T.size(); ++i) js += jf(i ? ", [%d, %d, %d]" : "[%d, %d, %d]", t->T[i].H, t->T[i].W, t->T[i].plane);
        js += "]}";
    } else {
        const OpDesc &d = t->op_desc[k];
        js = jf("{\"kind\": \"%s\", \"stream\": \"%s\", ", d.kind.c_str(), d.side ? "side" : "step") + d.body + "}";
    }
    if (js.size() + 1 > cap) return pn_set_error(ctx, PN_ERR_INVALID, "pn_trainer_op_info: %zu bytes needed", js.size() + 1);
    memcpy(out, js.c_str(), js.size() + 1);
    return PN_OK;
}

static int tx_sync(pn_trainer *t, hipStream_t s) {
    PN_HIP_CHECK(t->ctx, hipStreamSynchronize(s));
    if (t->side) PN_HIP_CHECK(t->ctx, hipStreamSynchronize(t->side));
    return PN_OK;
}

int pn_trainer_run_ops(pn_trainer *t, const float *img_dev, const float *heat_gt_dev, const float *paf_gt_dev, const float *z_gt_dev, const float *fg_mask_dev,
                       float *loss_terms_dev, int first, int last, void *hip_stream) {
    if (!t) return PN_ERR_INVALID;
    pn_ctx *ctx = t->ctx;
    if (int rc = tx_set_step_args(t, "pn_trainer_run_ops", img_dev, heat_gt_dev, paf_gt_dev, z_gt_dev, fg_mask_dev, loss_terms_dev)) return rc;
    if (first < 0 || last < first || last > (int)t->ops.size()) return pn_set_error(ctx, PN_ERR_INVALID, "pn_trainer_run_ops: [%d, %d) outside [0, %zu]", first, last, t->ops.size());
    hipStream_t s = (hipStream_t)hip_stream;
    for (int k = first; k < last; ++k)
        if (int rc = t->ops[k](s)) return rc;
    return tx_sync(t, s);          // both streams: a range may end between a fork and its join
}

static int tx_tensor_range(pn_trainer *t, const char *what, int id, int frame0, int nframes, size_t host_elems, size_t *frame_elems) {
    pn_ctx *ctx = t->ctx;
    if (!t->finalized) return pn_set_error(ctx, PN_ERR_STATE, "%s: trainer not finalized", what);
    if (id < 0 || id >= (int)t->T.size()) return pn_set_error(ctx, PN_ERR_INVALID, "%s: tensor %d outside [0, %zu)", what, id, t->T.size());
    if (frame0 < 0 || nframes < 1 || frame0 > t->B - nframes) return pn_set_error(ctx, PN_ERR_INVALID, "%s: frames [%d, %d + %d) outside [0, %d)", what, frame0, frame0, nframes, t->B);
    const TxTensor &X = t->T[id];
    *frame_elems = (size_t)X.H * X.W * X.plane;
    if (host_elems != *frame_elems * nframes) return pn_set_error(ctx, PN_ERR_INVALID, "%s: %zu host elements, %zu expected", what, host_elems, *frame_elems * nframes);
    return PN_OK;
}

int pn_trainer_read_tensor(pn_trainer *t, int id, int which, int frame0, int nframes, float *host_out, size_t host_elems, void *hip_stream) {
    if (!t || !host_out) return PN_ERR_INVALID;
    pn_ctx *ctx = t->ctx;
    size_t fe = 0;
    if (int rc = tx_tensor_range(t, "pn_trainer_read_tensor", id, frame0, nframes, host_elems, &fe)) return rc;
    if (which < 0 || which > 2 || (t->f32 && which)) return pn_set_error(ctx, PN_ERR_INVALID, "pn_trainer_read_tensor: plane selector %d (0 value, 1 hi, 2 lo; planes exist in a bf16x3 trainer only)", which);
    const TxTensor &X = t->T[id];
    if (int rc = tx_sync(t, (hipStream_t)hip_stream)) return rc;
    std::vector<uint32_t> raw(fe * nframes);              // 4 bytes per channel in both storage forms
    PN_HIP_CHECK(ctx, hipMemcpy(raw.data(), X.p + (size_t)frame0 * fe * 4, raw.size() * 4, hipMemcpyDeviceToHost));
    const size_t HW = (size_t)X.H * X.W;
    for (int f = 0; f < nframes; ++f)
        for (size_t p = 0; p < HW; ++p) {
            const char *px = (const char *)raw.data() + ((size_t)f * HW + p) * X.plane * 4;
            for (int c = 0; c < X.plane; ++c) {
                float v;
                if (t->f32) v = ((const float *)px)[c];
                else {
                    const uint16_t *h = (const uint16_t *)px;
                    const float hi = pn_bf16_to_f32(h[c]), lo = pn_bf16_to_f32(h[X.plane + c]);
                    v = which == 1 ? hi : which == 2 ? lo : hi + lo;
                }
                host_out[((size_t)f * X.plane + c) * HW + p] = v;
            }
        }
    return PN_OK;
}

int pn_trainer_write_tensor(pn_trainer *t, int id, int frame0, int nframes, const float *host_in, size_t host_elems, void *hip_stream) {
    if (!t || !host_in) return PN_ERR_INVALID;
    pn_ctx *ctx = t->ctx;
    size_t fe = 0;
    if (int rc = tx_tensor_range(t, "pn_trainer_write_tensor", id, frame0, nframes, host_elems, &fe)) return rc;
    const TxTensor &X = t->T[id];
    std::vector<uint32_t> raw(fe * nframes);
    const size_t HW = (size_t)X.H * X.W;
    for (int f = 0; f < nframes; ++f)
        for (size_t p = 0; p < HW; ++p) {
            char *px = (char *)raw.data() + ((size_t)f * HW + p) * X.plane * 4;
            for (int c = 0; c < X.plane; ++c) {
                const float v = host_in[((size_t)f * X.plane + c) * HW + p];
                if (t->f32) ((float *)px)[c] = v;
                else {                                   // Lay<bf>::st1: hi = bf(v), lo = bf(v - hi)
                    uint16_t *h = (uint16_t *)px;
                    h[c] = pn_f32_to_bf16(v);
                    h[X.plane + c] = pn_f32_to_bf16(v - pn_bf16_to_f32(h[c]));
                }
            }
        }
    if (int rc = tx_sync(t, (hipStream_t)hip_stream)) return rc;
    PN_HIP_CHECK(ctx, hipMemcpy(X.p + (size_t)frame0 * fe * 4, raw.data(), raw.size() * 4, hipMemcpyHostToDevice));
    return PN_OK;
}

int pn_trainer_read_vector(pn_trainer *t, const char *name, float *host_out, size_t host_elems, void *hip_stream) {
    if (!t || !name || !host_out) return PN_ERR_INVALID;
    pn_ctx *ctx = t->ctx;
    if (!t->finalized) return pn_set_error(ctx, PN_ERR_STATE, "pn_trainer_read_vector: trainer not finalized");
    const std::string nm = name;
    const float *src = nullptr;
    size_t n = 0;
    int st = -1, b = -1;
    if (sscanf(name, "head_out.%d.%d", &st, &b) == 2) {
        if (st < 0 || st > 1 || b < 0 || b > 2 || nm != jf("head_out.%d.%d", st, b)) return pn_set_error(ctx, PN_ERR_INVALID, "pn_trainer_read_vector: unknown '%s'", name);
        src = t->head_out[st][b]; n = (size_t)t->B * HEAD_C[b] * (t->H / 8) * (t->W / 8);
    } else {
        const size_t dot = nm.rfind('.');
        if (dot != std::string::npos) {
            const std::string bn = nm.substr(0, dot), what = nm.substr(dot + 1);
            static const char *names[7] = {"mean", "invstd", "scale", "shift", "k1", "k2", "k3"};
            for (const TxBn &x : t->bns)
                if (x.name == bn)
                    for (int i = 0; i < 7; ++i)
                        if (what == names[i]) { src = x.mean + (size_t)i * x.C; n = (size_t)x.C; }
        }
    }
    if (!src) return pn_set_error(ctx, PN_ERR_INVALID, "pn_trainer_read_vector: unknown '%s' (<BatchNorm>.mean|invstd|scale|shift|k1|k2|k3 or head_out.<stage>.<head>)", name);
    if (host_elems != n) return pn_set_error(ctx, PN_ERR_INVALID, "pn_trainer_read_vector: %zu host elements, %zu expected", host_elems, n);
    if (int rc = tx_sync(t, (hipStream_t)hip_stream)) return rc;
    PN_HIP_CHECK(ctx, hipMemcpy(host_out, src, n * 4, hipMemcpyDeviceToHost));
    return PN_OK;
}

}  // extern "C"
