// The inference nets' C ABI (include/popnet_hip.h) and the JSON views of a compiled net and of the launch planner.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include "net_internal.h"

using namespace pnnet;

namespace {
// The planned geometry of one convolution as JSON fields (no braces): what pn_net_step_info reports per convolution and pn_conv_level_plan_info
// per planned convolution -- one writer, so the two views cannot differ in what they mean.  Tile and block counts are those of a launch at batch B.
std::string geom_json(int prec, bool x3, const ConvGeom &g, int H, int W, int cout, int cin_chunks, int B) {
    ConvProblem P;
    memset(&P, 0, sizeof P);
    pn_fill_conv_problem(P, {nullptr, H, W, 0, 64, 0}, B, cin_chunks, cout, g, prec, x3);
    char t[384];
    snprintf(t, sizeof t, "\"kernel\": \"%s\", \"kern\": %d, \"cfg\": %d, \"pitch\": %d, \"R\": %d, \"Wt\": %d, \"wc\": %d, \"wp\": %d, \"nbuf\": %d, \"pt\": %d, \"rpg\": %d, "
             "\"tiles_x\": %d, \"tiles_per_img\": %d, \"cout_blocks\": %d, \"nblocks\": %d, \"lds_two\": %d",
             (g.dil != 1 ? pn_conv_kernel_label_dil(prec, g.ks, g.stride, g.pitch, g.cfg, g.dil) : pn_conv_kernel_label(prec, g.kern, false, g.ks, g.stride, g.pitch, g.cfg, g.wc, g.wp, g.nbuf, g.pt, g.rpg)).c_str(), g.kern, g.cfg, g.pitch, g.R, g.Wt, g.wc,
             g.wp, g.nbuf, g.pt, g.rpg, P.tiles_x, P.tiles_per_img, P.cout_blocks, P.nblocks, P.lds_two);
    return t;
}

// What every forward entry point checks before it touches the device: the net's kind, the caller's pointers and (state) a device and a finalized net
int forward_entry(pn_net *n, int kind, bool pointers_ok, bool state = true) {
    if (!n) return PN_ERR_INVALID;
    pn_ctx *ctx = n->ctx;
    if (n->kind != kind)
        return pn_set_error(ctx, PN_ERR_INVALID, "not %s net", kind == PN_NET_RTPOSE_LIGHT3D ? "an rtpose_light3d" : kind == PN_NET_YOLO_POSENET ? "a YoloPoseNet" : "an A2J");
    if (!pointers_ok) return pn_set_error(ctx, PN_ERR_INVALID, "null device pointer");
    if (state && ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (state && !n->finalized) return pn_set_error(ctx, PN_ERR_STATE, "pn_net_finalize has not been called");
    return PN_OK;
}

// frames in: the 7x7 stem computes its input tile from the raw depth frames with pn_preprocess's arithmetic (preproc_pixel.h).
// nsteps < 0: the whole step list (pn_*_forward_frames); otherwise steps [0, nsteps) under pn_net_forward_partial's two rules
int forward_frames(pn_net *n, const void *depth_dev, int depth_dtype, int B, int H, int W, float depth_max, float depth_mean, float depth_std,
                   hipStream_t stream, int nsteps = -1, bool partial = false) {
    pn_ctx *ctx = n->ctx;
    if (!depth_dev || H < 2 || W < 2) return pn_set_error(ctx, PN_ERR_INVALID, "forward_frames: bad arguments");
    if (depth_dtype != PN_DEPTH_F16 && depth_dtype != PN_DEPTH_F32) return pn_set_error(ctx, PN_ERR_INVALID, "forward_frames: unknown depth dtype %d", depth_dtype);
    if (int rc = forward_entry(n, n->kind, true)) return rc;      // the state checks come after the argument checks here, as they always have
    if (n->prec != PN_PREC_BF16) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "the frames-in forward is built for the bf16 and bf16x3 nets (fp32: pn_preprocess + pn_*_forward)");
    if (n->in_h != n->in_w) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "the frames-in forward resizes to a square input (net finalized for %dx%d)", n->in_h, n->in_w);
    const int S = n->in_h;
    if (W == 2 * S && H == 2 * S)   // as pn_preprocess: cv::resize switches to INTER_AREA at exactly 2x decimation
        return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "forward_frames: %dx%d -> %d is an exact 2x decimation, where cv2.resize(INTER_LINEAR) runs INTER_AREA instead: not built", W, H, S);
    if (partial) {
        if (n->last_B < 0) return pn_set_error(ctx, PN_ERR_STATE, "pn_net_forward_frames_partial: run one full forward first");
        if (nsteps < 0 || nsteps > (int)n->steps.size()) return pn_set_error(ctx, PN_ERR_INVALID, "nsteps %d outside [0, %zu]", nsteps, n->steps.size());
    }
    PnFrameSrc fs;
    fs.frames = depth_dev; fs.dtype = depth_dtype; fs.H = H; fs.W = W;
    const double inv_x = (double)S / (double)W, inv_y = (double)S / (double)H;
    fs.scale_x = 1.0 / inv_x; fs.scale_y = 1.0 / inv_y;                    // as cv::resize computes them (pn_preprocess)
    fs.dmax = depth_max; fs.mean = depth_mean; fs.stdv = depth_std;
    n->frame_src = fs;
    const int rc = run_forward(n, nullptr, B, stream, nsteps);
    n->frame_src.frames = nullptr;
    return rc;
}
}  // namespace

extern "C" {
pn_net *pn_net_create(pn_ctx *ctx, int kind, int num_parts, int a, int input_dim) {
    if (!ctx) return nullptr;
    if (kind != PN_NET_RTPOSE_LIGHT3D && kind != PN_NET_YOLO_POSENET && kind != PN_NET_A2J) {
        pn_set_error(ctx, PN_ERR_INVALID, "unknown net kind %d", kind);
        return nullptr;
    }
    if (input_dim < 1 || input_dim > 16) {
        pn_set_error(ctx, PN_ERR_UNSUPPORTED, "input_dim %d outside [1, 16]", input_dim);
        return nullptr;
    }
    if (kind == PN_NET_A2J && input_dim != 1) {
        pn_set_error(ctx, PN_ERR_UNSUPPORTED, "the A2J net takes one-channel depth crops (input_dim = 1)");
        return nullptr;
    }
    pn_net *n = new pn_net();
    n->ctx = ctx; n->kind = kind; n->num_parts = num_parts; n->a = a; n->input_dim = input_dim;
    return n;
}

void pn_net_destroy(pn_net *n) {
    if (!n) return;
    release_net(n);
    delete n;
}

int pn_net_set_tensor(pn_net *n, const char *name, const float *host_data, const int64_t *shape, int ndim) {
    if (!n || !name || (!host_data && ndim > 0)) return PN_ERR_INVALID;
    if (n->finalized) return pn_set_error(n->ctx, PN_ERR_STATE, "net already finalized");
    std::string s(name);
    if (s.rfind("module.", 0) == 0) s = s.substr(7);
    if (n->kind == PN_NET_A2J && (s.rfind("Backbone.model.fc.", 0) == 0 || (s.size() > 19 && s.compare(s.size() - 19, 19, "num_batches_tracked") == 0)))
        return PN_OK;      // built by the reference, never executed (model.py:158-167)
    HostTensor t;
    size_t numel = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); numel *= (size_t)shape[i]; }
    t.data.assign(host_data, host_data + numel);
    n->tensors[s] = std::move(t);
    return PN_OK;
}

// Two phases (net_internal.h): compile on the host, then one upload.  A context without a device stops after the first: the plan views answer, the forwards refuse.
int pn_net_finalize(pn_net *n, int precision, int max_batch, int in_h, int in_w) {
    if (!n) return PN_ERR_INVALID;
    pn_ctx *ctx = n->ctx;
    if (n->finalized) return pn_set_error(ctx, PN_ERR_STATE, "net already finalized");
    if (precision != PN_PREC_F32 && precision != PN_PREC_BF16 && precision != PN_PREC_BF16X3) return pn_set_error(ctx, PN_ERR_INVALID, "bad precision %d", precision);
    if (max_batch < 1) return pn_set_error(ctx, PN_ERR_INVALID, "max_batch must be >= 1");
    n->x3 = precision == PN_PREC_BF16X3;                      // kernels and packing run as bf16; tensors carry three planes
    n->prec = n->x3 ? PN_PREC_BF16 : precision; n->max_batch = max_batch; n->in_h = in_h; n->in_w = in_w;
    n->sw = pn_read_switches();
    if (int rc = compile_net(n)) return rc;
    if (ctx->device >= 0)
        if (int rc = upload_net(n)) return rc;
    for (auto &im : n->images) std::vector<unsigned char>().swap(im.host);
    n->tensors.clear();
    n->finalized = true;
    return PN_OK;
}

int pn_rtpose_forward(pn_net *n, const float *x_dev, int B, float *paf_dev, float *heat_dev, float *z_dev, void *hip_stream) {
    if (int rc = forward_entry(n, PN_NET_RTPOSE_LIGHT3D, x_dev && paf_dev && heat_dev && z_dev)) return rc;
    n->nchw_ptr[0] = paf_dev; n->nchw_ptr[1] = heat_dev; n->nchw_ptr[2] = z_dev;
    return run_forward(n, x_dev, B, (hipStream_t)hip_stream);
}

int pn_yolo_forward(pn_net *n, const float *x_dev, int B, float *out_dev, void *hip_stream) {
    if (int rc = forward_entry(n, PN_NET_YOLO_POSENET, x_dev && out_dev)) return rc;
    n->nchw_ptr[3] = out_dev;
    return run_forward(n, x_dev, B, (hipStream_t)hip_stream);
}

// A2J_model.forward (third_party_methods/A2J_experiments/model.py:179-186): the heads stay on the device, NHWC
int pn_a2j_forward(pn_net *n, const float *crops_dev, int B, const void **cls_dev, const void **reg_dev, const void **dep_dev, void *hip_stream) {
    if (int rc = forward_entry(n, PN_NET_A2J, crops_dev != nullptr)) return rc;
    if (int rc = run_forward(n, crops_dev, B, (hipStream_t)hip_stream)) return rc;
    if (cls_dev) *cls_dev = n->bufs[n->named["cls"].buf].p;
    if (reg_dev) *reg_dev = n->bufs[n->named["reg"].buf].p;
    if (dep_dev) *dep_dev = n->bufs[n->named["dep"].buf].p;
    return PN_OK;
}

int pn_a2j_head_shape(pn_net *n, int *h, int *w, int *precision) {
    if (!n) return PN_ERR_INVALID;
    if (n->kind != PN_NET_A2J || !n->finalized) return pn_set_error(n->ctx, PN_ERR_STATE, "not a finalized A2J net");
    if (h) *h = n->out_h;
    if (w) *w = n->out_w;
    if (precision) *precision = n->x3 ? PN_PREC_BF16X3 : n->prec;      // bf16x3: the head rows are [hi | lo] pairs
    return PN_OK;
}

int pn_a2j_predict(pn_net *n, const void *frames_dev, int depth_dtype, int F, int H, int W, const float *rows_dev, int nrows, const pn_a2j_cfg *cfg,
                   const float *anchors_dev, float *crops_dev, int32_t *flags_dev, float *votes_dev, pn_a2j_record *records_dev, void *hip_stream) {
    if (!n) return PN_ERR_INVALID;
    pn_ctx *ctx = n->ctx;
    if (n->kind != PN_NET_A2J || !n->finalized) return pn_set_error(ctx, PN_ERR_STATE, "not a finalized A2J net");
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (!cfg || !crops_dev || !anchors_dev) return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_predict: null argument");
    if (cfg->crop_h != n->in_h || cfg->crop_w != n->in_w)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_predict: crops of %dx%d into a net finalized for %dx%d", cfg->crop_h, cfg->crop_w, n->in_h, n->in_w);
    if (nrows < 1 || nrows > n->max_batch) return pn_set_error(ctx, PN_ERR_INVALID, "pn_a2j_predict: %d rows outside [1, %d]", nrows, n->max_batch);
    if (int rc = pn_a2j_crop(ctx, frames_dev, depth_dtype, F, H, W, rows_dev, nrows, cfg, crops_dev, flags_dev, hip_stream)) return rc;
    const void *cls = nullptr, *reg = nullptr, *dep = nullptr;
    if (int rc = pn_a2j_forward(n, crops_dev, nrows, &cls, &reg, &dep, hip_stream)) return rc;
    return pn_a2j_vote(ctx, cls, reg, dep, n->x3 ? PN_PREC_BF16X3 : n->prec, nrows, n->out_h, n->out_w, 16, n->num_parts, anchors_dev, votes_dev, rows_dev, cfg, records_dev, hip_stream);
}

int pn_rtpose_forward_frames(pn_net *n, const void *depth_dev, int depth_dtype, int B, int H, int W, float depth_max, float depth_mean, float depth_std,
                             float *paf_dev, float *heat_dev, float *z_dev, void *hip_stream) {
    if (int rc = forward_entry(n, PN_NET_RTPOSE_LIGHT3D, paf_dev && heat_dev && z_dev, false)) return rc;
    n->nchw_ptr[0] = paf_dev; n->nchw_ptr[1] = heat_dev; n->nchw_ptr[2] = z_dev;
    return forward_frames(n, depth_dev, depth_dtype, B, H, W, depth_max, depth_mean, depth_std, (hipStream_t)hip_stream);
}

int pn_yolo_forward_frames(pn_net *n, const void *depth_dev, int depth_dtype, int B, int H, int W, float depth_max, float depth_mean, float depth_std,
                           float *out_dev, void *hip_stream) {
    if (int rc = forward_entry(n, PN_NET_YOLO_POSENET, out_dev != nullptr, false)) return rc;
    n->nchw_ptr[3] = out_dev;
    return forward_frames(n, depth_dev, depth_dtype, B, H, W, depth_max, depth_mean, depth_std, (hipStream_t)hip_stream);
}

int pn_net_copy_activation(pn_net *n, const char *name, int B, float *dev_out, void *hip_stream) {
    if (!n || !name || !dev_out) return PN_ERR_INVALID;
    pn_ctx *ctx = n->ctx;
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (!n->finalized) return pn_set_error(ctx, PN_ERR_STATE, "net not finalized");
    auto it = n->named.find(name);
    if (it == n->named.end()) return pn_set_error(ctx, PN_ERR_INVALID, "unknown activation '%s'", name);
    const NamedAct &a = it->second;
    const Buf &b = n->bufs[a.buf];
    const bool one = a.plane >= 0;        // one plane of a bf16x3 buffer, as stored; otherwise hi + lo
    return pn_launch_nhwc_to_nchw(ctx, n->prec, b.p, dev_out, B, b.H, b.W, a.C, b.C, a.coff + (one ? a.plane * b.plane : 0), n->x3 && !one ? b.plane : 0, (hipStream_t)hip_stream);
}

int pn_net_read_activation(pn_net *n, const char *name, int B, float *host_out, size_t host_elems, void *hip_stream) {
    if (!n || !name || !host_out) return PN_ERR_INVALID;
    pn_ctx *ctx = n->ctx;
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    auto it = n->named.find(name);
    if (it == n->named.end()) return pn_set_error(ctx, PN_ERR_INVALID, "unknown activation '%s'", name);
    const Buf &b = n->bufs[it->second.buf];
    const size_t elems = (size_t)B * it->second.C * b.H * b.W;
    if (host_elems < elems) return pn_set_error(ctx, PN_ERR_INVALID, "host buffer too small: %zu < %zu", host_elems, elems);
    float *tmp = nullptr;
    PN_HIP_CHECK(ctx, hipMalloc((void **)&tmp, elems * 4));
    hipStream_t s = (hipStream_t)hip_stream;
    int rc = pn_net_copy_activation(n, name, B, tmp, hip_stream);
    if (!rc) {
        hipError_t e = hipMemcpyAsync(host_out, tmp, elems * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = pn_set_error(ctx, PN_ERR_HIP, "read_activation copy: %s", hipGetErrorString(e));
    }
    (void)hipFree(tmp);
    return rc;
}

int pn_net_read_zero_page(pn_net *n, int buf, void *host_out, size_t cap) {
    if (!n || !host_out) return PN_ERR_INVALID;
    pn_ctx *ctx = n->ctx;
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (!n->finalized) return pn_set_error(ctx, PN_ERR_STATE, "net not finalized");
    if (buf < 0 || buf >= (int)n->bufs.size()) return pn_set_error(ctx, PN_ERR_INVALID, "buffer %d outside [0, %zu)", buf, n->bufs.size());
    if (cap < 2048) return pn_set_error(ctx, PN_ERR_INVALID, "host buffer too small: %zu < 2048", cap);
    const Buf &b = n->bufs[buf];
    PN_HIP_CHECK(ctx, hipMemcpy(host_out, (const char *)b.p + b.bytes, 2048, hipMemcpyDeviceToHost));      // the null stream: after every earlier launch of a blocking stream
    return PN_OK;
}

int pn_net_forward_partial(pn_net *n, const float *x_dev, int B, int nsteps, void *hip_stream) {
    if (!n) return PN_ERR_INVALID;
    if (!x_dev) return pn_set_error(n->ctx, PN_ERR_INVALID, "null device pointer");
    if (n->ctx->device < 0) return pn_set_error(n->ctx, PN_ERR_STATE, "context has no device");
    if (n->last_B < 0) return pn_set_error(n->ctx, PN_ERR_STATE, "pn_net_forward_partial: run one full forward first");
    if (nsteps < 0 || nsteps > (int)n->steps.size()) return pn_set_error(n->ctx, PN_ERR_INVALID, "nsteps %d outside [0, %zu]", nsteps, n->steps.size());
    return run_forward(n, x_dev, B, (hipStream_t)hip_stream, nsteps);
}

// steps [0, nsteps) of the frames-in forward: pn_*_forward_frames' checks in their order, then pn_net_forward_partial's; either net kind, and the
// output pointers of the last full forward stay as they are
int pn_net_forward_frames_partial(pn_net *n, const void *depth_dev, int depth_dtype, int B, int H, int W, float depth_max, float depth_mean,
                                  float depth_std, int nsteps, void *hip_stream) {
    if (!n) return PN_ERR_INVALID;
    if (n->kind != PN_NET_RTPOSE_LIGHT3D && n->kind != PN_NET_YOLO_POSENET) return pn_set_error(n->ctx, PN_ERR_INVALID, "not an rtpose_light3d or a YoloPoseNet net");
    return forward_frames(n, depth_dev, depth_dtype, B, H, W, depth_max, depth_mean, depth_std, (hipStream_t)hip_stream, nsteps, true);
}

int pn_net_num_steps(pn_net *n) {
    if (!n) return PN_ERR_INVALID;
    if (!n->finalized) return pn_set_error(n->ctx, PN_ERR_STATE, "net not finalized");
    return (int)n->steps.size();
}

int pn_net_step_info(pn_net *n, int k, char *out, size_t cap) {
    if (!n || !out || !cap) return PN_ERR_INVALID;
    pn_ctx *ctx = n->ctx;
    if (!n->finalized) return pn_set_error(ctx, PN_ERR_STATE, "net not finalized");
    if (k < -1 || k >= (int)n->steps.size()) return pn_set_error(ctx, PN_ERR_INVALID, "step %d outside [-1, %zu)", k, n->steps.size());
    std::string js;
    char t[256];
    auto add = [&](const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(t, sizeof t, fmt, ap);
        va_end(ap);
        js += t;
    };
    auto conv = [&](int id) {
        const ConvSpec &c = n->convs[id];
        add("{\"w\": \"%s\", \"bn\": \"%s\", \"ks\": %d, \"stride\": %d, \"act\": %d, \"cout\": %d, \"embed3\": %d, ",
            c.w.c_str(), c.bn.c_str(), c.embed3 ? 1 : c.ks, c.stride, c.act, c.cout, c.embed3 ? 1 : 0);
        add("\"in_buf\": %d, \"in_coff\": %d, \"res_buf\": %d, \"res_coff\": %d, \"out_buf\": %d, \"out_coff\": %d, \"nchw_slot\": %d, \"cin_map\": [",
            c.in_buf, c.in_coff, c.res_buf, c.res_coff, c.out_buf, c.out_coff, c.nchw_slot);
        for (size_t i = 0; i < c.cin_map.size(); ++i) add(i ? ", %d" : "%d", c.cin_map[i]);
        js += "], \"tail\": ";
        if (c.tail_conv >= 0) {
            const ConvSpec &b = n->convs[c.tail_conv];
            add("{\"w\": \"%s\", \"act\": %d, \"cout\": %d, \"out_buf\": %d, \"out_coff\": %d, \"nchw_slot\": %d}",
                b.w.c_str(), b.act, b.cout, b.out_buf, b.out_coff, b.nchw_slot);
        } else js += "null";
        js += ", \"pool\": ";
        if (c.pool_tail) add("{\"mode\": 0, \"out_buf\": %d, \"out_coff\": %d}", c.pool_out_buf, c.pool_out_coff);
        else js += "null";
        // the plan (conv_plan.h) as compiled; the counts at the batch of the last forward (max_batch before the first).  A fused pool (\"pool\") tiles
        // the POOLED map instead (net_run.hip::refresh_problems): tiles_x / tiles_per_img / nblocks are then not the launch's
        const Buf &ib = n->bufs[c.in_buf];
        js += ", " + geom_json(n->prec, n->x3, c, ib.H, ib.W, c.cout, c.cin_chunks, n->last_B > 0 ? n->last_B : n->max_batch);
        if (c.dil != 1) add(", \"dil\": %d", c.dil);      // the dilated convolutions only (A2J layer4 blocks 1 and 2)
        if (c.acc) add(", \"blocked_acc\": %d", c.acc);   // fp32 A2J only
        js += "}";
    };
    if (k == -1) {
        add("{\"prec\": \"%s\", \"in_h\": %d, \"in_w\": %d, \"input_dim\": %d, \"max_batch\": %d, \"steps\": %zu, \"bufs\": [",
            n->x3 ? "bf16x3" : n->prec == PN_PREC_BF16 ? "bf16" : "fp32", n->in_h, n->in_w, n->input_dim, n->max_batch, n->steps.size());
        for (size_t i = 0; i < n->bufs.size(); ++i) add(i ? ", [%d, %d, %d]" : "[%d, %d, %d]", n->bufs[i].H, n->bufs[i].W, n->bufs[i].plane);
        js += "]}";
    } else {
        const Step &st = n->steps[k];
        static const char *types[] = {"stem", "pool", "conv", "bblock"};
        add("{\"type\": \"%s\", \"kernel\": \"%s\"", types[(int)st.type], step_label(n, st).c_str());
        if (st.type == Step::STEM) add(", \"cin\": %d, \"out_buf\": %d, \"pool_buf\": %d", st.stem_cin, st.out_buf, st.stem_pool_buf);
        else if (st.type == Step::POOL) add(", \"mode\": %d, \"in_buf\": %d, \"out_buf\": %d, \"C\": %d, \"out_coff\": %d", st.pool.mode, st.pool.in_buf, st.pool.out_buf, st.pool.C, st.pool.out_coff);
        else {
            js += ", \"convs\": [";
            for (size_t i = 0; i < st.conv_ids.size(); ++i) {
                if (i) js += ", ";
                conv(st.conv_ids[i]);
            }
            js += "]";
        }
        js += "}";
    }
    if (js.size() + 1 > cap) return pn_set_error(ctx, PN_ERR_INVALID, "pn_net_step_info: %zu bytes needed", js.size() + 1);
    memcpy(out, js.c_str(), js.size() + 1);
    return PN_OK;
}

int pn_conv_level_plan_info(pn_ctx *ctx, int precision, int max_batch, int num_cus, int B, int H, int W, int together, int nconv, const int *cout,
                            const int *cin, const int *ks, const int *stride, char *out, size_t cap) {
    if (!ctx) return PN_ERR_INVALID;
    if (!out || !cout || !cin || !ks || !stride || nconv < 1 || nconv > 3 || max_batch < 1 || B < 1 || B > max_batch || num_cus < 1 || H < 1 || W < 1 ||
        (precision != PN_PREC_F32 && precision != PN_PREC_BF16 && precision != PN_PREC_BF16X3))
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv_level_plan_info: bad arguments");
    for (int i = 0; i < nconv; ++i)
        if (cout[i] < 1 || cin[i] < 1 || (ks[i] != 1 && ks[i] != 3) || (stride[i] != 1 && stride[i] != 2))
            return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv_level_plan_info: convolution %d: bad arguments", i);
    const bool x3 = precision == PN_PREC_BF16X3;
    const int prec = x3 ? PN_PREC_BF16 : precision;
    const PnSwitches sw = pn_read_switches();
    std::vector<PnLevelConv> lv(nconv);
    for (int i = 0; i < nconv; ++i) {
        lv[i].H = H; lv[i].W = W; lv[i].rows = cout[i]; lv[i].ks = ks[i]; lv[i].stride = stride[i];
        lv[i].cin_gt64 = cin[i] > 64;
    }
    if (together) pn_plan_level(lv, max_batch, x3, sw.conv4);      // build_rtpose; build_yolo plans every convolution alone
    std::string js = "{\"convs\": [";
    for (int i = 0; i < nconv; ++i) {
        const int cin_chunks = ((x3 ? 3 : 1) * cin[i] + 63) / 64;      // bf16x3: the K loop runs over three planes of the input buffer (net_pack.hip::prepare_conv)
        ConvGeom g;
        g.ks = ks[i]; g.stride = stride[i];
        pn_plan_conv_kernel(prec, max_batch, num_cus, H, W, cout[i], cin_chunks, lv[i].wc_min, lv[i].nbuf_min, lv[i].k4_level, sw, g);
        const char *why = "";
        if (int rc = pn_plan_conv_tiles(prec, H, W, g, &why)) return pn_set_error(ctx, rc, "conv %d: %s", i, why);
        js += (i ? ", {" : "{") + geom_json(prec, x3, g, H, W, cout[i], cin_chunks, B) + "}";
    }
    js += "]}";
    if (js.size() + 1 > cap) return pn_set_error(ctx, PN_ERR_INVALID, "pn_conv_level_plan_info: %zu bytes needed", js.size() + 1);
    memcpy(out, js.c_str(), js.size() + 1);
    return PN_OK;
}

double pn_net_flops_per_frame(pn_net *n) { return n ? n->flops_per_frame : 0.0; }

int pn_net_lock(pn_net *n, int locked) {
    if (!n) return PN_ERR_INVALID;
    if (n->ctx->device < 0) return pn_set_error(n->ctx, PN_ERR_STATE, "context has no device");
    if (locked && n->last_B < 0) return pn_set_error(n->ctx, PN_ERR_STATE, "pn_net_lock: run one forward first");
    n->locked = locked != 0;
    return PN_OK;
}
}  // extern "C"
