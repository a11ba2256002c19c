// A compiled net on the device: the one upload of finalize, the per-batch launch descriptors, the step loop and per-launch profiling.
#include <algorithm>
#include <cstring>
#include "net_internal.h"

namespace pnnet {
// Second phase of pn_net_finalize: every allocation and copy the compiled net (net.hip::compile_net) asks for, then one synchronisation.
int upload_net(pn_net *n) {
    pn_ctx *ctx = n->ctx;
    PN_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    for (auto &b : n->bufs) {
        PN_HIP_CHECK(ctx, hipMalloc(&b.p, b.bytes + 2048));
        PN_HIP_CHECK(ctx, hipMemset(b.p, 0, b.bytes + 2048));      // zero: pad channels must read as 0
    }
    for (auto &im : n->images) {
        PN_HIP_CHECK(ctx, hipMalloc(&im.dev, im.bytes));
        if (im.host.empty()) PN_HIP_CHECK(ctx, hipMemset(im.dev, 0, im.bytes));
        else PN_HIP_CHECK(ctx, hipMemcpy(im.dev, im.host.data(), im.bytes, hipMemcpyHostToDevice));
    }
    PN_HIP_CHECK(ctx, hipDeviceSynchronize());      // the zero fills above ran on the null stream: a forward on a non-blocking stream must not overtake them
    return PN_OK;
}

void release_net(pn_net *n) {
    for (auto &b : n->bufs) if (b.p) (void)hipFree(b.p);
    for (auto &im : n->images) if (im.dev) (void)hipFree(im.dev);
    for (auto &r : n->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
}

// The convolutions of this launch run different bodies (3x3 beside 1x1, fused tail beside none): conv3_mix_kernel
bool level_is_mixed(const pn_net *n, const Step &st) {
    const ConvSpec &c0 = n->convs[st.conv_ids[0]];
    for (int id : st.conv_ids)
        if (c0.kern == 3 && (n->convs[id].ks != c0.ks || (n->convs[id].tail_conv >= 0) != (c0.tail_conv >= 0))) return true;
    return false;
}

// Kernel label of a step: the profiler's per-instantiation key (pn_net_profile_kernel) and pn_net_step_info's "kernel".
std::string step_label(const pn_net *n, const Step &st) {
    if (st.type == Step::STEM) {
        if (st.stem_pool_buf >= 0) return "stem7x7_pool_kernel";
        if (st.stem_cin > 1) return "conv2d_forward+nchw_relu_to_nhwc_kernel";
        if (n->prec == PN_PREC_F32) return "stem7x7_kernel";
        return n->x3 ? "stem7x7_mfma_kernel<x3>" : "stem7x7_mfma_kernel";
    }
    if (st.type == Step::POOL) return pn_pool_kernel_label(st.pool.mode, n->x3);
    if (st.type == Step::BBLOCK) return n->x3 ? "bb64x3_kernel" : "bb64_kernel";
    const ConvSpec &c0 = n->convs[st.conv_ids[0]];
    if (c0.dil != 1) return pn_conv_kernel_label_dil(n->prec, c0.ks, c0.stride, c0.pitch, c0.cfg, c0.dil);
    return pn_conv_kernel_label(n->prec, c0.kern, level_is_mixed(n, st), c0.ks, c0.stride, c0.pitch, c0.cfg, c0.wc, c0.wp, c0.nbuf, c0.pt, c0.rpg);
}

namespace {
int refresh_problems(pn_net *n, int B, hipStream_t stream) {
    for (auto &st : n->steps) {
        if (st.type != Step::CONV) continue;
        const ConvSpec &c0 = n->convs[st.conv_ids[0]];
        st.host_probs.clear();
        int max_blocks = 0;
        bool two_bufs = false, has_tail = false, pool_tail = false;
        for (int id : st.conv_ids) {
            const ConvSpec &cs = n->convs[id];
            const Buf &ib = n->bufs[cs.in_buf];
            if (n->x3 && ib.plane % 64)
                return pn_set_error(n->ctx, PN_ERR_UNSUPPORTED, "bf16x3: input plane of %d channels is not a multiple of 64 (the K loop wraps to the hi plane per 64-channel chunk)", ib.plane);
            ConvProblem P;
            memset(&P, 0, sizeof P);
            pn_fill_conv_problem(P, {ib.p, ib.H, ib.W, ib.C, ib.plane, ib.bytes}, B, cs.cin_chunks, cs.cout, cs, n->prec, n->x3);
            P.wpack = n->dev(cs.wpack);
            P.bias = (const float *)n->dev(cs.bias);
            P.in_coff = cs.in_coff;
            if (cs.out_buf >= 0) { P.out = n->bufs[cs.out_buf].p; P.out_cs = n->bufs[cs.out_buf].C; P.out_coff = cs.out_coff; P.split = n->x3 ? n->bufs[cs.out_buf].plane : 0; }
            if (cs.res_buf >= 0) { P.res = n->bufs[cs.res_buf].p; P.res_cs = n->bufs[cs.res_buf].C; P.res_coff = cs.res_coff; P.res_split = n->x3 ? n->bufs[cs.res_buf].plane : 0; }
            if (cs.nchw_slot >= 0) P.out_nchw = n->nchw_ptr[cs.nchw_slot];
            P.act = cs.act;
            P.yolo_naf = 5 + 3 * n->num_parts;
            if (cs.pool_tail) {                        // 3 x 7 pooled pixels per block, the pooled map as the only output
                const Buf &pb = n->bufs[cs.pool_out_buf];
                P.tiles_x = (pb.W + 6) / 7;
                P.tiles_per_img = ((pb.H + 2) / 3) * P.tiles_x;
                P.nblocks = B * P.tiles_per_img * P.cout_blocks;
                P.tail_out = pb.p; P.tail_out_cs = pb.C; P.tail_out_coff = cs.pool_out_coff;
                P.tail_split = n->x3 ? pb.plane : 0;
                P.out = nullptr;
                pool_tail = true;
            }
            if (cs.tail_conv >= 0) {
                const ConvSpec &tb = n->convs[cs.tail_conv];
                P.tail_w = n->dev(cs.tail_wpack); P.tail_bias = (const float *)n->dev(cs.tail_bias); P.tail_cout = tb.cout; P.tail_act = tb.act;
                if (tb.out_buf >= 0) { P.tail_out = n->bufs[tb.out_buf].p; P.tail_out_cs = n->bufs[tb.out_buf].C; P.tail_out_coff = tb.out_coff; }
                if (tb.nchw_slot >= 0) P.tail_nchw = n->nchw_ptr[tb.nchw_slot];
                P.out = nullptr;                       // the 128-channel tile never leaves the CU
                has_tail = true;
            }
            if (P.lds_two) two_bufs = true;
            max_blocks = std::max(max_blocks, P.nblocks);
            st.host_probs.push_back(P);
        }
        pn_fill_conv_launch(st.launch, n->prec, c0, (int)st.host_probs.size(), max_blocks, two_bufs);
        if (c0.kern == 3) {                        // on top of it: fused tails / pools, and launches that mix bodies
            st.launch.tail = has_tail ? 1 : pool_tail ? 2 : 0;
            if (level_is_mixed(n, st)) st.launch.mix = 1;
            for (int id : st.conv_ids) {
                const ConvSpec &cs = n->convs[id];
                st.launch.lds_bytes = std::max(st.launch.lds_bytes, pn_conv3_lds_bytes(cs.ks, cs.wp, cs.nbuf, cs.rpg));
            }
            if (st.launch.tail == 1) st.launch.lds_bytes = std::max<size_t>(st.launch.lds_bytes, 4 * 7 * 1024 + 1024);   // the tail's fragment image
            if (st.launch.tail == 2 && n->x3) st.launch.lds_bytes = std::max<size_t>(st.launch.lds_bytes, 2 * 4 * 7 * 1024);   // fused pool, bf16x3: hi and lo tiles parked
        }
        st.launch.probs_dev = (const ConvProblem *)n->dev(st.dev_probs);
        PN_HIP_CHECK(n->ctx, hipMemcpyAsync(n->dev(st.dev_probs), st.host_probs.data(), st.host_probs.size() * sizeof(ConvProblem),
                                            hipMemcpyHostToDevice, stream));
    }
    n->last_B = B;
    for (int i = 0; i < 4; ++i) n->last_nchw[i] = n->nchw_ptr[i];
    return PN_OK;
}

// The profiling record of the next launch (events are created on first use and kept), its start event recorded
int profile_step(pn_net *n, const Step &st, int B, hipStream_t stream, ProfRec **out) {
    pn_ctx *ctx = n->ctx;
    if (n->prof_used == n->prof.size()) {
        ProfRec r;
        PN_HIP_CHECK(ctx, hipEventCreate(&r.a));
        PN_HIP_CHECK(ctx, hipEventCreate(&r.b));
        n->prof.push_back(r);
    }
    ProfRec *pr = &n->prof[n->prof_used++];
    const bool conv = st.type == Step::CONV || st.type == Step::BBLOCK;      // a BasicBlock counts with the convolutions: both convs' algorithmic FLOPs
    pr->kind = conv ? (int)Step::CONV : (int)st.type;
    pr->flops = 0;
    for (int id : st.conv_ids) pr->flops += n->convs[id].flops * B;
    pr->label = conv ? step_label(n, st) : std::string();
    PN_HIP_CHECK(ctx, hipEventRecord(pr->a, stream));
    *out = pr;
    return PN_OK;
}
}  // namespace

// nsteps < 0: the whole step list; otherwise steps [0, nsteps) only (pn_net_forward_partial).  The callers have checked the device and `finalized` (net_api.hip).
int run_forward(pn_net *n, const float *x, int B, hipStream_t stream, int nsteps) {
    pn_ctx *ctx = n->ctx;
    if (B < 1 || B > n->max_batch) return pn_set_error(ctx, PN_ERR_INVALID, "batch %d outside [1, %d]", B, n->max_batch);
    bool dirty = B != n->last_B;
    for (int i = 0; i < 4; ++i) dirty |= n->nchw_ptr[i] != n->last_nchw[i];
    if (dirty) {
        if (n->locked)
            return pn_set_error(ctx, PN_ERR_STATE, "net is locked at batch %d (pn_net_lock): a forward with another batch size or other output buffers would rewrite descriptors a captured graph still reads", n->last_B);
        if (int rc = refresh_problems(n, B, stream)) return rc;
    }
    // bb64_kernel's tile tickets are persistent device state that only a COMPLETED launch returns to zero; one net must not run two forwards at once (one
    // stream per net: the engines keep it so), and after a forward that failed part-way the counters are re-zeroed here, in stream order, before anything
    // can read them (a non-zero ticket would make every later launch -- graph replays included -- skip tiles silently)
    if (n->tickets_suspect) {
        for (auto &st : n->steps)
            if (st.type == Step::BBLOCK && st.bb_tickets >= 0) PN_HIP_CHECK(ctx, hipMemsetAsync(n->dev(st.bb_tickets), 0, 256, stream));
        n->tickets_suspect = false;
    }
    for (size_t si = 0; si < n->steps.size(); ++si) {
        if ((int)si == nsteps) break;
        Step &st = n->steps[si];
        int rc = PN_OK;
        ProfRec *pr = nullptr;
        if (n->profiling)
            if (int prc = profile_step(n, st, B, stream, &pr)) return prc;
        if (st.type == Step::STEM) {
            const Buf &ob = n->bufs[st.out_buf];
            const PnFrameSrc *src = n->frame_src.frames ? &n->frame_src : nullptr;
            const float *w = (const float *)n->dev(st.stem_w), *bias = (const float *)n->dev(st.stem_b);
            float *scratch = (float *)n->dev(st.stem_scratch);
            if (st.stem_pool_buf >= 0) {
                const Buf &pb = n->bufs[st.stem_pool_buf];
                rc = pn_launch_stem_pool(ctx, x, n->dev(st.stem_wfrag), bias, pb.p, B, n->in_h, n->in_w, ob.H, ob.W, pb.C, stream, src);
            } else if (st.stem_cin > 1) {
                if (src) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "the frames-in forward takes single-channel depth frames (input_dim = 1)");
                rc = pn_conv2d_forward(ctx, x, w, bias, scratch, B, st.stem_cin, n->in_h, n->in_w, 64, 7, 2, 3, 0, (void *)stream);
                if (!rc) rc = pn_launch_nchw_relu_to_nhwc(ctx, n->prec, scratch, ob.p, B, ob.H, ob.W, 64, ob.C, n->x3 ? ob.plane : 0, stream);
            } else {
                rc = pn_launch_stem(ctx, n->x3 ? PN_PREC_BF16X3 : n->prec, x, w, n->dev(st.stem_wfrag), bias, ob.p, B, n->in_h, n->in_w, ob.H, ob.W, ob.C, n->x3 ? ob.plane : 0, stream, src);
            }
        } else if (st.type == Step::POOL) {
            const Buf &ib = n->bufs[st.pool.in_buf], &ob = n->bufs[st.pool.out_buf];
            rc = pn_launch_pool(ctx, n->prec, st.pool.mode, ib.p, ob.p, B, ib.H, ib.W, st.pool.C, ib.C, ob.C, st.pool.out_coff, n->x3 ? ib.plane : 0, n->x3 ? ob.plane : 0, stream);
        } else if (st.type == Step::BBLOCK) {
            const ConvSpec &ca = n->convs[st.conv_ids[0]], &cb = n->convs[st.conv_ids[1]];
            const Buf &ib = n->bufs[ca.in_buf], &ob = n->bufs[cb.out_buf];
            BBProblem P;
            memset(&P, 0, sizeof P);
            P.in = ib.p; P.out = ob.p; P.wpack = n->dev(st.bb_wpack); P.bias1 = (const float *)n->dev(st.bb_bias1); P.bias2 = (const float *)n->dev(st.bb_bias2);
            P.B = B; P.H = ib.H; P.W = ib.W;
            P.in_cs = ib.C; P.in_coff = ca.in_coff; P.out_cs = ob.C; P.out_coff = cb.out_coff;
            P.Wt = st.bb_wt; P.tiles_x = (ib.W + st.bb_wt - 1) / st.bb_wt;
            P.tiles_per_img = ((ib.H + (n->x3 ? 5 : 7)) / (n->x3 ? 6 : 8)) * P.tiles_x;      // bb64x3_kernel: 6-row tiles
            P.ntiles = B * P.tiles_per_img;
            P.in_zero_off = (unsigned)ib.bytes;
            P.in_split = n->x3 ? ib.plane : 0; P.out_split = n->x3 ? ob.plane : 0;
            P.tickets = (n->x3 || n->sw.bb64_static || P.ntiles < 4 * ctx->num_cus) ? nullptr : (int *)n->dev(st.bb_tickets);      // nullptr: blockIdx.x + k * gridDim.x
            P.halves = n->sw.bb64_halves;
            // The strip kernel (bb64s_kernel.h) walks column segments top-down and carries the intermediate's two overlap rows.  S segments per column: the
            // smallest count that gives every CU a segment, at most T / 2 (a segment has two tiles at least), lengths differing by at most one.  Default:
            // where a segment averages four row tiles -- the tile tickets' threshold; 56 x 56 maps, small batches and bf16x3 nets keep their kernels, and
            // so do POPNET_BB64_STATIC / POPNET_BB64_HALVES=2, which ask for a form of bb64_kernel.
            const int T = (ib.H + 7) / 8, ncols = B * P.tiles_x;
            int S = std::max(1, std::min((ctx->num_cus + ncols - 1) / ncols, T / 2));
            if (n->sw.bb64_strip == 2) S = std::max(1, std::min(2 * S, T / 2));
            const bool strip = !n->x3 && T >= 2 && (n->sw.bb64_strip >= 1 || (n->sw.bb64_strip < 0 && !n->sw.bb64_static && n->sw.bb64_halves != 2 && T >= 4 * S));
            if (strip) {
                P.strip_S = S; P.strip_T = T; P.nseg = ncols * S;
                P.tickets = (n->sw.bb64_static || P.nseg <= ctx->num_cus) ? nullptr : (int *)n->dev(st.bb_tickets);
            }
            rc = n->x3 ? pn_launch_bb64x3(ctx, P, stream) : strip ? pn_launch_bb64s(ctx, P, stream) : pn_launch_bb64(ctx, P, stream);
        } else {
            rc = pn_launch_conv(ctx, st.launch, stream);
        }
        if (rc) { n->tickets_suspect = true; return rc; }
        if (pr) PN_HIP_CHECK(ctx, hipEventRecord(pr->b, stream));
    }
    return PN_OK;
}
}  // namespace pnnet

using namespace pnnet;      // per-launch profiling (C ABI)

extern "C" {
int pn_net_profile_begin(pn_net *n) {
    if (!n) return PN_ERR_INVALID;
    n->prof_by_kernel.clear();
    n->profiling = true;
    n->prof_used = 0;
    return PN_OK;
}

int pn_net_profile_end(pn_net *n, double *conv_ms, int64_t *conv_launches, double *conv_flops, double *other_ms,
                       int64_t *other_launches) {
    if (!n) return PN_ERR_INVALID;
    pn_ctx *ctx = n->ctx;
    n->profiling = false;
    ProfRow conv, other;
    for (size_t i = 0; i < n->prof_used; ++i) {
        PN_HIP_CHECK(ctx, hipEventSynchronize(n->prof[i].b));
        float ms = 0.f;
        PN_HIP_CHECK(ctx, hipEventElapsedTime(&ms, n->prof[i].a, n->prof[i].b));
        auto add = [&](ProfRow &r) { r.ms += ms; r.launches += 1; r.flops += n->prof[i].flops; };
        if (n->prof[i].kind == (int)Step::CONV) { add(conv); add(n->prof_by_kernel[n->prof[i].label]); }
        else add(other);
    }
    n->prof_used = 0;
    if (conv_ms) *conv_ms = conv.ms;
    if (conv_launches) *conv_launches = conv.launches;
    if (conv_flops) *conv_flops = conv.flops;
    if (other_ms) *other_ms = other.ms;
    if (other_launches) *other_launches = other.launches;
    return PN_OK;
}

int pn_net_profile_kernel(pn_net *n, int rank, char *name, size_t name_cap, double *ms, int64_t *launches, double *flops) {
    if (!n || rank < 0) return PN_ERR_INVALID;
    std::vector<std::pair<double, std::string>> order;
    for (auto &kv : n->prof_by_kernel) order.push_back({-kv.second.ms, kv.first});
    std::sort(order.begin(), order.end());
    if ((size_t)rank >= order.size()) return PN_ERR_INVALID;
    const ProfRow &e = n->prof_by_kernel[order[rank].second];
    if (name && name_cap) { strncpy(name, order[rank].second.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (ms) *ms = e.ms;
    if (launches) *launches = e.launches;
    if (flops) *flops = e.flops;
    return PN_OK;
}
}  // extern "C"
