// The inference nets' host structures, shared by net.hip (graph builders, fusion passes), net_pack.hip (BatchNorm fold, weight packing), net_run.hip (upload,
// launch descriptors, step loop, profiling) and net_api.hip (C ABI, JSON views).  pn_net_finalize has two phases: compile_net (net.hip) builds buffers, levels,
// plans, fusions, steps and every packed image in host memory with no HIP call, so a context without a device compiles the same net; upload_net (net_run.hip)
// allocates and copies once.  Device memory a step or a convolution refers to is an index into pn_net::images.
#pragma once
#include <map>
#include <string>
#include <vector>
#include "pn_internal.h"
#include "conv_plan.h"
#include "preproc_pixel.h"

namespace pnnet {
struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    size_t numel() const { return data.size(); }
};

struct Buf {
    void *p = nullptr;
    int H = 0, W = 0, C = 0;   // C = channel stride
    int plane = 0;             // bf16x3: channels of one of the two stored planes [hi | lo] (C = 2 * plane); otherwise = C
    size_t bytes = 0;          // max_batch maps (compile_net); the allocation is 2 KiB longer: the zero page the kernels' halo padding reads
};

// One device allocation besides the activation buffers: packed on the host by the compile pass, copied (or, without a host image, zero-filled) by upload_net
struct Image {
    std::vector<unsigned char> host;
    size_t bytes = 0;
    void *dev = nullptr;
};

struct ConvSpec : ConvGeom {    // ks / stride as given; kernel and tiles as planned (conv_plan.h)
    std::string w;            // "<prefix>" of "<prefix>.weight" (and ".bias" when present)
    std::string bn;           // BN prefix or ""
    int in_buf = -1, in_coff = 0;
    std::vector<int> cin_map; // my input channel -> reference input channel (-1 = zero); empty = identity
    int out_buf = -1, out_coff = 0;
    int res_buf = -1, res_coff = 0;
    int act = PN_ACT_NONE;
    int nchw_slot = -1;       // index into pn_net::nchw_ptr or -1
    int cout = 0;
    // derived
    int cin_chunks = 0;
    int wc_min = 0, nbuf_min = 0;             // set by harmonize_level: share the launch of a wider sibling conv
    int k4_level = 0;                         // set by harmonize_level: a 3x3 conv of this level has Cin >= 128 and >= 64 couts (conv4_kernel)
    int wpack = -1, bias = -1;                // images
    double flops = 0;
    int tail_conv = -1;       // fuse_1x1_tails: index of the 1x1 conv (<= 32 couts) that runs inside this conv's launch on its output tile
    int tail_wpack = -1, tail_bias = -1;      // images (pack_tail)
    bool embed3 = false;      // a 1x1 convolution run as the centre tap of a 3x3 one (zero weights elsewhere: the same sums, exact zeros added), so that it shares
                              // the launch of a 3x3 sibling of the same stride: YoloPoseNet's layer2.0 stride-2 shortcut (resnet.py:59-77, build_yolo)
    bool pool_tail = false;   // fuse_pool_tails: the AvgPool2d(3, 2, 1) that follows runs inside this conv's launch (conv3_kernel<1, 4, 1, 1, 7, 8, 2>)
    int pool_out_buf = -1, pool_out_coff = 0;
};

// What the builders emit and the fusion passes rewrite: a set of independent convolutions, a pool, or (fuse_basic_blocks) a BasicBlock(64) pair
struct Level {
    enum Kind { CONVS, POOL, BBLOCK } kind = CONVS;
    std::vector<int> convs;                                          // CONVS: indices into pn_net::convs; BBLOCK: {a, b}
    int mode = 0, in_buf = -1, out_buf = -1, C = 0, out_coff = 0;    // POOL
};

struct Step {
    enum Type { STEM, POOL, CONV, BBLOCK } type;
    // BBLOCK: fused BasicBlock(64) = convs[conv_ids[0]] (3x3 + ReLU) -> convs[conv_ids[1]] (3x3 + residual + ReLU), bb64_kernel.h
    int bb_wt = 0;
    int bb_wpack = -1, bb_bias1 = -1, bb_bias2 = -1;   // images
    int bb_tickets = -1;             // image of zeroed ints: bb64_kernel's tile tickets (BBProblem::tickets)
    // STEM
    int out_buf = -1;
    int stem_pool_buf = -1;          // >= 0: the MaxPool2d(3, 2, 1) that follows runs inside the stem launch and writes this buffer (build_yolo)
    int stem_w = -1, stem_b = -1;    // images
    int stem_wfrag = -1;             // image: bf16 MFMA fragments of the same weights
    int stem_cin = 1;                // > 1: multi-channel input (input_dim != 1): stem_w = folded [64][Cin][7][7] f32 for pn_conv2d_forward, stem_scratch = its NCHW f32 map
    int stem_scratch = -1;           // image
    Level pool;                      // POOL: the level as built
    // CONV: indices into pn_net::convs, all sharing one kernel instantiation; BBLOCK: the pair
    std::vector<int> conv_ids;
    ConvLaunch launch;
    std::vector<ConvProblem> host_probs;
    int dev_probs = -1;              // image
};

struct NamedAct { int buf = -1, coff = 0, C = 0, plane = -1; };      // plane >= 0: bf16x3 "buf<i>.hi" / "buf<i>.lo": that one stored plane (0 / 1) instead of hi + lo
struct ProfRec { hipEvent_t a, b; int kind; double flops; std::string label; };
struct ProfRow { double ms = 0; int64_t launches = 0; double flops = 0; };
}  // namespace pnnet

struct pn_net {
    pn_ctx *ctx = nullptr;
    int kind = 0, num_parts = 15, a = 14, input_dim = 1;
    std::map<std::string, pnnet::HostTensor> tensors;
    bool finalized = false;
    int prec = PN_PREC_F32, max_batch = 0, in_h = 0, in_w = 0;
    PnSwitches sw;                   // read when the net is compiled (pn_net_finalize)
    std::vector<pnnet::Buf> bufs;
    std::vector<pnnet::ConvSpec> convs;
    std::vector<pnnet::Step> steps;
    std::vector<pnnet::Image> images;
    float *nchw_ptr[4] = {nullptr, nullptr, nullptr, nullptr};
    int last_B = -1;
    bool x3 = false;                 // PN_PREC_BF16X3: tensors stored as [hi | lo] bf16 planes, read as [hi | lo | hi] against weights [W_hi | W_hi | W_lo]
    bool locked = false;             // pn_net_lock: descriptors frozen (a captured hipGraph reads them at replay time)
    bool tickets_suspect = false;    // a forward of this net failed part-way: bb64_kernel's tile tickets may be non-zero -- re-zeroed before the next launch
    float *last_nchw[4] = {nullptr, nullptr, nullptr, nullptr};
    std::map<std::string, pnnet::NamedAct> named;
    double flops_per_frame = 0;
    int out_h = 0, out_w = 0;
    // optional per-launch HIP-event timing (bench.py's live roofline measurement)
    bool profiling = false;
    std::map<std::string, pnnet::ProfRow> prof_by_kernel;   // kernel label -> its launches, filled by pn_net_profile_end
    std::vector<pnnet::ProfRec> prof;
    size_t prof_used = 0;
    // pn_*_forward_frames: the stem reads the raw depth frames (frame_src.frames != nullptr during that call)
    PnFrameSrc frame_src = {};

    size_t esize() const { return prec == PN_PREC_BF16 ? 2 : 4; }
    void *dev(int image) const { return image < 0 ? nullptr : images[image].dev; }
};

namespace pnnet {
inline const HostTensor *find_t(const pn_net *n, const std::string &name) {
    auto it = n->tensors.find(name);
    return it == n->tensors.end() ? nullptr : &it->second;
}
// A device allocation to be: a copy of `data`, or `bytes` of zeros when data == nullptr.  Returns its index in pn_net::images.
inline int add_image(pn_net *n, const void *data, size_t bytes) {
    n->images.emplace_back();
    n->images.back().bytes = bytes;
    if (data) n->images.back().host.assign((const unsigned char *)data, (const unsigned char *)data + bytes);
    return (int)n->images.size() - 1;
}
template <class T> int add_image(pn_net *n, const std::vector<T> &v) { return add_image(n, v.data(), v.size() * sizeof(T)); }

int compile_net(pn_net *n);      // net.hip; host only: everything pn_net_step_info reports and every host image
int prepare_conv(pn_net *n, ConvSpec &cs);      // net_pack.hip
int pack_stem(pn_net *n, Step &st, const std::string &conv, const std::string &bn, int sum_cin);
int pack_bblock(pn_net *n, Step &st);
int pack_tail(pn_net *n, ConvSpec &a);
int upload_net(pn_net *n);      // net_run.hip
void release_net(pn_net *n);
bool level_is_mixed(const pn_net *n, const Step &st);
std::string step_label(const pn_net *n, const Step &st);
int run_forward(pn_net *n, const float *x, int B, hipStream_t stream, int nsteps = -1);
}  // namespace pnnet
