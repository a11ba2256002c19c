/*
 * popnet_hip.h -- C ABI of libpopnet_hip.so, the MI355X (gfx950) implementation of the
 * PoP-Net / MP-3DHP inference hot path:
 *
 *     depth frame -> resize/clamp/normalise -> CNN forward -> pose parsing -> 2D/3D joints
 *
 * Plain C types only (pointers, sizes, a HIP stream passed as void*): no torch, no C++ types.
 * Device pointers are raw HIP allocations owned by the CALLER; the library owns only the
 * workspace inside a pn_ctx / pn_net.  Every call returns 0 on success or a negative
 * pn_status; the message is retrievable with pn_last_error().  Nothing aborts, nothing is
 * global except the seven legacy `pafprocess` symbols at the end of this file.
 *
 * Each entry point cites the reference interface (file:line under /root/reference) it
 * replaces.  "tpm/" = third_party_methods/.
 */
#ifndef POPNET_HIP_H
#define POPNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PN_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------------------------ */
enum pn_status {
    PN_OK = 0,
    PN_ERR_INVALID = -1,     /* bad argument / unknown tensor name / shape mismatch */
    PN_ERR_HIP = -2,         /* a HIP runtime call failed (message has the hipError string) */
    PN_ERR_STATE = -3,       /* call order violated (e.g. forward before finalize) */
    PN_ERR_UNSUPPORTED = -4  /* shape outside what the kernels are built for */
};

/* ---- compute / storage precision of the conv stack ---------------------------------------- */
enum pn_precision {
    PN_PREC_F32 = 0,   /* fp32 storage, fp32-input MFMA (v_mfma_f32_16x16x4_f32): parity mode */
    PN_PREC_BF16 = 1,  /* bf16 storage, bf16 MFMA (v_mfma_f32_16x16x32_bf16), fp32 accumulate: throughput mode */
    PN_PREC_BF16X3 = 2 /* split-bf16 ("3 x bf16"): every tensor and weight is kept as hi + lo bf16
                          parts (16 significant bits), a product is x_hi w_hi + x_lo w_hi + x_hi w_lo on the bf16 matrix
                          cores with fp32 accumulation; fp32-class results (north_star's 1e-3 m) at ~1/3 of the bf16 rate */
};

enum pn_net_kind {
    PN_NET_RTPOSE_LIGHT3D = 0,  /* "Open-Pose+"  tpm/lib/network/rtpose_light3d.py:249-356 */
    PN_NET_YOLO_POSENET = 1,    /* "Yolo-Pose+"  tpm/lib/network/yolo_posenet.py:87-158   */
    PN_NET_A2J = 2              /* "Yolo-A2J" second stage: A2J_model  third_party_methods/A2J_experiments/model.py:145-186, resnet.py:61-164 */
};

enum pn_depth_dtype {
    PN_DEPTH_F16 = 0,
    PN_DEPTH_F32 = 1,
    PN_DEPTH_NET = 2   /* the ablation entries only: the buffer is the network input [B,1,S,S] f32, clamped and normalised */
};

typedef struct pn_ctx pn_ctx;
typedef struct pn_net pn_net;

/* ---- context -------------------------------------------------------------------------------
 * One context per GPU / stream owner.  Not thread-safe per context; independent contexts are. */
int pn_abi_version(void);
/* Always 0: the library has no lab-build variant and honours no result-changing environment variable.  Kept for ABI
 * compatibility (earlier lab builds returned 1; bench.py refuses to time a library that does). */
int pn_build_experiments(void);
/* Measurement aid (bench.py `roofline.peak_sustained_tflops`; no reference counterpart -- the reference has no device code): runs a loop of
 * nothing but v_mfma_f32_16x16x32_bf16 on random bf16 operands (`waves_per_simd` waves on every SIMD of every CU, no memory traffic)
 * back to back for `seconds` and reports what the LAST batch of launches sustained, i.e. the matrix-core ceiling of THIS box at the
 * clock its power limit allows, next to the 2.5 PFLOP/s spec figure; *in_kernel_ghz (may be NULL) = median shader clock inside the
 * kernel (s_memtime / s_memrealtime).  Synchronises the stream. */
int pn_mfma_sustained(pn_ctx *ctx, double seconds, int waves_per_simd, double *tflops, double *in_kernel_ghz, void *hip_stream);
pn_ctx *pn_create(int device_id);
void pn_destroy(pn_ctx *ctx);
/* Copies the last error message of this context into buf (NUL-terminated). Returns its length. */
int pn_last_error(pn_ctx *ctx, char *buf, size_t buf_len);

/* ---- pre-processing -------------------------------------------------------------------------
 * Replaces test-mode KDH3D_Keypoints.__getitem__ image path:
 *   tpm/lib/datasets/datasets_kdh3d_rtpose_mpreal.py:225-246 (CR line endings)
 *   tpm/lib/datasets/data_augmentation_2d3d.py:76-89 (Cvt2ndarray), :507-522 (Resize, cv2 INTER_LINEAR)
 * depth_dev: [B, H, W] f16 or f32 metres (device).  out_dev: [B, 1, S, S] f32 (device),
 * = (clip(bilinear(depth), 0, depth_max) - depth_mean) / depth_std.                            */
int pn_preprocess(pn_ctx *ctx, const void *depth_dev, int depth_dtype, int B, int H, int W,
                  float *out_dev, int S, float depth_max, float depth_mean, float depth_std,
                  void *hip_stream);

/* ---- networks -------------------------------------------------------------------------------
 * pn_net_create + pn_net_set_tensor + pn_net_finalize replace
 *   model = rtpose_light3d(num_parts, num_limbs, num_stages, input_dim); model.load_state_dict(sd)
 *   (tpm/evaluate/evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py:135-144)
 * and the YoloPoseNet twin (tpm/evaluate/evaluation_yolo_posenet_kdh3d_mpreal.py:119-128).
 * Tensor names are the reference state_dict keys, without "module.".
 * `a` = num_limbs for rtpose_light3d, number of anchors for YoloPoseNet.  input_dim = channels of the input batch [B, input_dim, H, W]
 * (1 = depth, the path north_star names: fused matrix-core stem, frames-in forward; 2..16, e.g. the reference constructors' default 3
 * (rtpose_light3d.py:250, yolo_posenet.py:88): the 7x7 stem on the generic fp32 convolution, pn_*_forward only).                          */
pn_net *pn_net_create(pn_ctx *ctx, int kind, int num_parts, int a, int input_dim);
void pn_net_destroy(pn_net *net);
/* Host fp32 data, copied.  Unknown names are rejected, except keys the reference builds but
 * never executes (YoloPoseNet model0.layer3.*, *.num_batches_tracked), which are accepted and
 * ignored. */
int pn_net_set_tensor(pn_net *net, const char *name, const float *host_data,
                      const int64_t *shape, int ndim);
/* Folds BatchNorm (eval mode, eps 1e-5) into the convolutions, packs weights into MFMA
 * fragment order, uploads, allocates NHWC activation workspace for `max_batch` frames of
 * in_h x in_w.  Must be called once after all tensors are set. */
int pn_net_finalize(pn_net *net, int precision, int max_batch, int in_h, int in_w);

/* rtpose_light3d.forward (tpm/lib/network/rtpose_light3d.py:326-356), stage-2 outputs:
 *   x_dev [B,1,in_h,in_w] f32 NCHW -> paf [B,2L,h,w], heat [B,J+1,h,w], z [B,L+1,h,w]
 *   f32 NCHW device buffers (h = in_h/8).  Sigmoid range casts applied.                        */
int pn_rtpose_forward(pn_net *net, const float *x_dev, int B, float *paf_dev, float *heat_dev,
                      float *z_dev, void *hip_stream);
/* YoloPoseNet.forward (tpm/lib/network/yolo_posenet.py:131-158):
 *   x_dev [B,1,in_h,in_w] -> out [B, A*(5+3J), in_h/16, in_w/16] f32 NCHW, slice casts applied. */
int pn_yolo_forward(pn_net *net, const float *x_dev, int B, float *out_dev, void *hip_stream);
/* Frames in (round 3): pn_preprocess + pn_rtpose_forward / pn_yolo_forward as ONE call on the raw depth frames -- the image half of
 * test-mode KDH3D_Keypoints.__getitem__ (tpm/lib/datasets/datasets_kdh3d_rtpose_mpreal.py:225-246 (CR), data_augmentation_2d3d.py:
 * 76-89,507-522) followed by model(img) (tpm/evaluate/evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py:171-178 /
 * evaluation_yolo_posenet_kdh3d_mpreal.py:160-166).  The 7x7 stem computes its input tile with pn_preprocess's arithmetic, so the
 * maps are bit-identical to the two-call form; the pre-processed [B,1,S,S] tensor is never written.  depth_dev [B,H,W] f16 / f32
 * metres (device), resized to the square S = in_h = in_w the net was finalized for.  bf16 and bf16x3 nets (the fp32 parity mode
 * keeps the two calls: PN_ERR_UNSUPPORTED).                                                                                       */
int pn_rtpose_forward_frames(pn_net *net, const void *depth_dev, int depth_dtype, int B, int H, int W, float depth_max,
                             float depth_mean, float depth_std, float *paf_dev, float *heat_dev, float *z_dev,
                             void *hip_stream);
int pn_yolo_forward_frames(pn_net *net, const void *depth_dev, int depth_dtype, int B, int H, int W, float depth_max,
                           float depth_mean, float depth_std, float *out_dev, void *hip_stream);
/* Test/diagnostic: copies a named internal activation of the last forward to the host as
 * f32 NCHW.  Names: "feat" (stem output), "paf1" "heat1" "z1" (stage-1 outputs) for
 * rtpose_light3d; "feat" (layer2 output) for YoloPoseNet.  Synchronises the stream.           */
int pn_net_read_activation(pn_net *net, const char *name, int B, float *host_out,
                           size_t host_elems, void *hip_stream);
/* Same, device to device: writes f32 NCHW into dev_out on the stream, no synchronisation.  This is
 * how the Python module materialises forward()'s `saved_for_loss` stage-1 entries
 * (tpm/lib/network/rtpose_light3d.py:340-342).                                                   */
int pn_net_copy_activation(pn_net *net, const char *name, int B, float *dev_out, void *hip_stream);
/* Test/diagnostic, read-only: copies the 2048 bytes that follow activation buffer `buf` (the zero page the kernels' halo padding
 * reads; zero-filled once by pn_net_finalize and never written) to host_out.  Synchronises on the null stream.  PN_ERR_INVALID for a
 * buffer index outside the net's buffers or cap < 2048.                                                                            */
int pn_net_read_zero_page(pn_net *net, int buf, void *host_out, size_t cap);
/* Test/diagnostic (per-layer checks). Every activation buffer is also readable by number through
 * pn_net_read_activation / pn_net_copy_activation as "buf<i>" (all channels, f32 NCHW; a bf16x3 buffer
 * reads as hi + lo) and, in a bf16x3 net, "buf<i>.hi" / "buf<i>.lo" (one stored plane).
 * pn_net_forward_partial runs steps [0, nsteps) of the compiled step list and stops: the same forward,
 * descriptors, lock and batch rules as pn_*_forward.  It needs one full pn_*_forward first, at the same
 * batch size, whose output buffers stay valid (a head step writes them).
 * pn_net_num_steps: the number of steps.  pn_net_step_info writes a JSON description of step k into out
 * (type stem / pool / conv / bblock, the kernel label, and per convolution its weight / BN prefixes, ks,
 * stride, act, buffers with channel offsets, input-channel map, fused tail or pool); k = -1 describes the
 * net (precision, input size, buffers as [H, W, C]).  PN_ERR_INVALID when cap is too small.
 * pn_net_forward_frames_partial: the same for the frames-in forward -- steps [0, nsteps) of pn_rtpose_forward_frames /
 * pn_yolo_forward_frames (either net kind), with their argument and state checks and refusals in their order, then the two above
 * (one full forward first, nsteps in range).  No output pointer is touched.  nsteps = 1 runs the stem that reads the raw frames.      */
int pn_net_forward_partial(pn_net *net, const float *x_dev, int B, int nsteps, void *hip_stream);
int pn_net_forward_frames_partial(pn_net *net, const void *depth_dev, int depth_dtype, int B, int H, int W, float depth_max,
                                  float depth_mean, float depth_std, int nsteps, void *hip_stream);
int pn_net_num_steps(pn_net *net);
int pn_net_step_info(pn_net *net, int k, char *out, size_t cap);
/* The plan of one LEVEL of up to three independent convolutions that read the same H x W map, as pn_net_finalize would plan it, without a
 * net and without a device (a context from pn_create(-1) will do; nothing is launched).  precision: pn_precision, PN_PREC_BF16X3 included;
 * num_cus: the compute units the plan is made for; cin[i]: the input channels the K loop covers (the input BUFFER's channels where the
 * buffer is wider than the weight's Cin: bf16x3 reads whole buffers); together != 0: the convolutions decide as one level (conv4 or not, shared
 * 128-cout blocks: rtpose_light3d's levels), 0: each is planned alone (YoloPoseNet's).  Kernel switches are read from the environment at the call, as
 * pn_net_finalize reads them.  out: {"convs": [{"kernel", "kern", "cfg", "pitch", "R", "Wt", "wc", "wp", "nbuf", "pt", "rpg", "tiles_x",
 * "tiles_per_img", "cout_blocks", "nblocks", "lds_two"}, ...]}, the block counts at batch B <= max_batch -- the fields pn_net_step_info
 * reports for every convolution of a compiled net.  PN_ERR_UNSUPPORTED (message: "conv <i>: <reason>") where pn_net_finalize refuses the
 * shape.  pn_conv_has_instance: 1 when the generic MFMA convolution is built for (prec = PN_PREC_BF16 / PN_PREC_F32, kernel size, stride,
 * LDS pitch class, tile configuration "cfg"): the table the launch dispatch and the planner both read. */
int pn_conv_level_plan_info(pn_ctx *ctx, int precision, int max_batch, int num_cus, int B, int H, int W, int together, int nconv,
                            const int *cout, const int *cin, const int *ks, const int *stride, char *out, size_t cap);
int pn_conv_has_instance(int prec, int ks, int stride, int pitch, int cfg);
/* Algorithmic FLOPs (2*MAC, convolutions only) of one frame through the finalized net. */
double pn_net_flops_per_frame(pn_net *net);
/* Freezes the launch descriptors at the batch size / output pointers of the last forward: afterwards a forward with
 * another batch size or other output buffers returns PN_ERR_STATE instead of rewriting descriptors that a captured
 * hipGraph reads at replay time.  pn_net_lock(net, 0) lifts the freeze.                                               */
int pn_net_lock(pn_net *net, int locked);
/* Measurement hooks: between begin and end every kernel launch of pn_*_forward is bracketed by
 * HIP events recorded on the caller's stream.  end() waits for them and returns the summed
 * durations: conv_* = the MFMA convolution launches (with the algorithmic FLOPs they covered),
 * other_* = stem + pooling launches.  Event pairs are recycled; nothing is allocated per call once
 * the first profiled forward has run. */
int pn_net_profile_begin(pn_net *net);
int pn_net_profile_end(pn_net *net, double *conv_ms, int64_t *conv_launches, double *conv_flops,
                       double *other_ms, int64_t *other_launches);
/* After pn_net_profile_end: the convolution kernel instantiation with the rank-th largest summed
 * duration (rank 0 = the dominant kernel), its launches and the algorithmic FLOPs they covered.
 * PN_ERR_INVALID when rank is past the last instantiation. */
int pn_net_profile_kernel(pn_net *net, int rank, char *name, size_t name_cap, double *ms,
                          int64_t *launches, double *flops);

/* ---- Open-Pose+ parsing ---------------------------------------------------------------------
 * Replaces, per frame, paf_to_pose + paf_to_human_list + the depth read-out / rescale /
 * back-projection glue:
 *   tpm/lib/utils/paf_to_pose.py:33-377, tpm/lib/utils/common.py:5-32,272-293,
 *   tpm/evaluate/evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py:179-262.
 * Limits are compile-time; exceeding one sets PN_FRAME_OVERFLOW in the frame's status and
 * truncates deterministically (first-come in reference order).                                  */
#define PN_NUM_JOINTS 15
#define PN_NUM_LIMBS 14
#define PN_MAX_PEAKS_PER_JOINT 32
#define PN_MAX_PEAKS (PN_NUM_JOINTS * PN_MAX_PEAKS_PER_JOINT)
#define PN_MAX_CONN_PER_LIMB PN_MAX_PEAKS_PER_JOINT
#define PN_MAX_PERSONS 32

#define PN_FRAME_OVERFLOW_PEAKS 1u
#define PN_FRAME_OVERFLOW_PERSONS 2u

/* The joint depth read-out of the two evaluation scripts:
 *   HEAT_WEIGHTED  retrieve_depth_heat_weighted(radius=1) around cell (int(x / downsample), int(y / downsample)) of joint j's heat and z maps
 *                  (evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py)
 *   CELL           the one cell z[z_chn[j]][int(y / downsample)][int(x / downsample)] * depth_std + depth_mean in float32
 *                  (evaluation_rtpose_light3d_itop.py:176-191).  The script indexes without a check and raises IndexError for a refined peak
 *                  whose cell index lies past the last row or column; here the index is clamped to the last cell, nothing else is read. */
#define PN_Z_READOUT_HEAT_WEIGHTED 0
#define PN_Z_READOUT_CELL 1

typedef struct pn_parse_cfg {
    float thresh_heatmap;      /* cfg.TEST.THRESH_HEATMAP  = 0.1   tpm/lib/config/default.py:126 */
    float thresh_paf;          /* cfg.TEST.THRESH_PAF      = 0.05  :127 */
    int   num_intermed_pts;    /* 2 .. 32 (default 10)  cfg.TEST.NUM_INTERMED_PTS_BETWEEN_KEYPOINTS :128 */
    int   downsample;          /* 1, 2, 4, 8 or 16 (default 8)  cfg.MODEL.DOWNSAMPLE :41 */
    int   input_size;          /* 224: network input side, divisor of the rescale */
    int   w_org, h_org;        /* original frame size for the rescale (480, 640) */
    double fx, fy, cx, cy;     /* pinhole intrinsics  util/util_functions.py:4 */
    float depth_mean, depth_std; /* 3, 2   util/util_functions.py:11-12 */
    int   z_readout;           /* PN_Z_READOUT_*: how a joint's depth is read from the pose-depth map (default HEAT_WEIGHTED) */
    int   z_chn[PN_NUM_JOINTS]; /* PN_Z_READOUT_CELL only: the pose-depth channel of joint j (joint2chn), each in 0 .. PN_NUM_LIMBS;
                                  the heat-weighted rule reads channel j, as its script does (joint2chn = range(num_parts)) */
} pn_parse_cfg;

/* One frame of results.  Doubles where the reference keeps float64 (everything after NMS). */
typedef struct pn_pose_frame {
    int32_t  n_persons;
    int32_t  n_peaks;                                   /* rows of joint_list */
    uint32_t status;                                    /* PN_FRAME_OVERFLOW_* bits */
    int32_t  reserved;
    /* joint_list (paf_to_pose return value 0): x, y, score, id, type */
    float    peak_x[PN_MAX_PEAKS];                      /* integer-valued pixel coords, 224 frame */
    float    peak_y[PN_MAX_PEAKS];
    float    peak_score[PN_MAX_PEAKS];
    int32_t  peak_type[PN_MAX_PEAKS];
    /* person_to_joint_assoc (return value 1): J joint ids (-1 = missing), score, count */
    int32_t  person_joint[PN_MAX_PERSONS][PN_NUM_JOINTS];
    double   person_score[PN_MAX_PERSONS];
    int32_t  person_count[PN_MAX_PERSONS];
    /* glue outputs, already rescaled to the original frame / back-projected */
    double   joints_2d[PN_MAX_PERSONS][PN_NUM_JOINTS][2];   /* human_pred_set_2d entry   */
    double   joints_3d[PN_MAX_PERSONS][PN_NUM_JOINTS][3];   /* human_pred_set_3d entry   */
    double   part_conf[PN_MAX_PERSONS][PN_NUM_JOINTS];      /* human_pred_set_part_conf  */
} pn_pose_frame;

void pn_parse_cfg_default(pn_parse_cfg *cfg);
size_t pn_sizeof_parse_cfg(void);
/* heat [B,J+1,h,w], paf [B,2L,h,w], z [B,L+1,h,w]: f32 NCHW device buffers (z normalised, as
 * the network emits it).  frames_dev: device array of B pn_pose_frame.  cfg->downsample = 8 with
 * cfg->num_intermed_pts = 10 runs the kernels built for the workload; every other supported pair
 * (see pn_parse_cfg) runs generic ones with the same results contract, and anything else is
 * PN_ERR_UNSUPPORTED before any launch -- here, in pn_parse_paf_wire and in pn_parse_paf_unbounded. */
int pn_parse_paf(pn_ctx *ctx, const float *heat_dev, const float *paf_dev, const float *z_dev,
                 int B, int h, int w, const pn_parse_cfg *cfg, pn_pose_frame *frames_dev,
                 void *hip_stream);
/* Sizes the context's parse scratch for batches of up to max_batch frames, once, so that pn_parse_paf never
 * allocates on the launch path (a captured hipGraph keeps the scratch pointer: growing it later would free memory
 * the graph still uses).  pn_parse_paf returns PN_ERR_STATE instead of growing the scratch while its stream is being
 * captured, and after pn_parse_reserve has fixed the size.                                                          */
int pn_parse_reserve(pn_ctx *ctx, int max_batch);

/* The same parse WITHOUT the record capacities (the reference has none): one frame (heat [J+1,h,w], paf [2L,h,w], z [L+1,h,w]
 * device maps), every list in a workspace sized from the frame's own counts (up to h*w peaks per joint map).  The second pass
 * for a frame whose fixed-size record carries PN_FRAME_OVERFLOW_*: same arithmetic, same order, variable-length result.
 * Synchronises the stream; *n_peaks / *n_persons size the arrays pn_parse_paf_unbounded_fetch copies out (any of them may be
 * NULL): peaks_xys [n_peaks][3] (x, y, score; id = row, as paf_to_pose's joint_list), peak_type [n_peaks], person_joint
 * [n_persons][J], person_score / person_count [n_persons], joints_2d [n][J][2], joints_3d [n][J][3], part_conf [n][J].
 * The result lives in the context until the next pn_parse_paf_unbounded call (not re-entrant per context). */
int pn_parse_paf_unbounded(pn_ctx *ctx, const float *heat_dev, const float *paf_dev, const float *z_dev, int h, int w,
                           const pn_parse_cfg *cfg, int *n_peaks, int *n_persons, void *hip_stream);
int pn_parse_paf_unbounded_fetch(pn_ctx *ctx, float *peaks_xys, int *peak_type, int *person_joint, double *person_score,
                                 int *person_count, double *joints_2d, double *joints_3d, double *part_conf);

/* Read-only views of the connection lists (find_connected_joints, tpm/lib/utils/paf_to_pose.py:156-264) a parse left in the context:
 * per limb the count and, in matching order, the indices (i into the source joint type's peaks, j into the destination's) and the
 * float64 limb score.  Host arrays; both calls block until the device is idle and touch nothing on the launch path.
 * pn_parse_debug_connections: frame `frame` of the last pn_parse_paf / pn_parse_paf_wire batch; count [L], conn_i / conn_j / conn_s
 * [L][PN_MAX_CONN_PER_LIMB].  PN_ERR_STATE when no parse has run on the context or frame is outside that batch.
 * pn_parse_paf_unbounded_connections: the last pn_parse_paf_unbounded; arrays [L][cap], cap >= every limb's count (the n_peaks that
 * call returned always suffices), else PN_ERR_INVALID.                                                                              */
int pn_parse_debug_connections(pn_ctx *ctx, int frame, int *count, int *conn_i, int *conn_j, double *conn_s);
int pn_parse_paf_unbounded_connections(pn_ctx *ctx, int cap, int *count, int *conn_i, int *conn_j, double *conn_s);

/* NMS(heatmaps, upsampFactor, bool_refine_center=True, config) (tpm/lib/utils/paf_to_pose.py:75-153) alone, on n_maps maps
 * [n_maps, h, w] f32 of one frame (any topology: `paf_to_pose_cpp`, paf_to_pose.py:381-385, runs it on the 18 COCO parts before
 * `process_paf`).  No capacity: count_dev [n_maps] int32 receives every map's peak count, peak_x / peak_y / peak_score_dev
 * [n_maps][h*w] f32 the peaks of map m at [m][0 .. count[m]) in the reference's order (row-major cells): refined x, y in
 * up-sampled pixels and the bicubic score.  upsample: 1, 2, 4, 8 or 16, else PN_ERR_UNSUPPORTED.  Asynchronous on hip_stream, no
 * allocation.                                                                                                                 */
int pn_nms_peaks(pn_ctx *ctx, const float *heat_dev, int n_maps, int h, int w, float thresh, int upsample, int *count_dev,
                 float *peak_x_dev, float *peak_y_dev, float *peak_score_dev, void *hip_stream);
/* The same with the reference's other two arguments.  refine_center = 0 (bool_refine_center=False): x = (px + 0.5) * upsample - 0.5, y
 * alike, score = the map's own value at the peak; no patch is up-sampled and gaussian_filt is ignored, as in the reference (:143-146).
 * gaussian_filt != 0 (bool_gaussian_filt=True): scipy.ndimage.gaussian_filter(patch_up, sigma=3) on the float32 up-sampled patch in
 * front of the arg-max, bit for bit (radius 12, float64 accumulation per axis, 'reflect' border).  pn_nms_opt_default sets
 * {8, 1, 0}: with those pn_nms_peaks_opt is pn_nms_peaks(..., 8, ...), the same launch.  Outputs as pn_nms_peaks.                  */
typedef struct pn_nms_opt { int upsample; int refine_center; int gaussian_filt; } pn_nms_opt;
void pn_nms_opt_default(pn_nms_opt *opt);
int pn_nms_peaks_opt(pn_ctx *ctx, const float *heat_dev, int n_maps, int h, int w, float thresh, const pn_nms_opt *opt, int *count_dev,
                     float *peak_x_dev, float *peak_y_dev, float *peak_score_dev, void *hip_stream);

/* retrieve_depth_heat_weighted(center, depthmap, heatmap, radius) (tpm/lib/utils/common.py:272-293)
 * for n centres (x, y int32 pairs) on one [h, w] f32 map pair; like the reference it first clamps
 * negative heat values in place.  out_dev: n float32 (the reference's np.sum/np.sum is float32).   */
int pn_retrieve_depth(pn_ctx *ctx, const float *depthmap_dev, float *heatmap_dev, int h, int w,
                      const int *centers_xy_dev, int n, int radius, float *out_dev, void *hip_stream);
size_t pn_sizeof_pose_frame(void);

/* Compact wire form of pn_pose_frame for the multi-GPU gather ("[frames, P_max, 15, 6] float32 +
 * count"): what crosses xGMI / PCIe when only the per-person results are needed (6.2 KB instead of 33 KB per
 * frame).  vals = (x, y) in the original frame, (X, Y, Z) metres, part confidence, rounded to float32 from the
 * float64 record; person_joint = the peak ids of person_to_joint_assoc (-1 = missing), so assignments stay exact.
 * Frames with more than PN_WIRE_MAX_PERSONS persons set PN_FRAME_OVERFLOW_PERSONS in status and keep the first
 * PN_WIRE_MAX_PERSONS rows (n_persons still holds the true count). */
#define PN_WIRE_MAX_PERSONS 16
typedef struct pn_pose_wire {
    int32_t  n_persons;
    uint32_t status;
    int16_t  person_joint[PN_WIRE_MAX_PERSONS][PN_NUM_JOINTS];
    float    vals[PN_WIRE_MAX_PERSONS][PN_NUM_JOINTS][6];
} pn_pose_wire;
int pn_pack_pose_frames(pn_ctx *ctx, const pn_pose_frame *frames_dev, int B, pn_pose_wire *wire_dev, void *hip_stream);
/* pn_parse_paf that also writes the compact records (wire_dev: B pn_pose_wire, may be NULL) in the same pass of the
 * read-out kernel -- identical bytes to pn_parse_paf followed by pn_pack_pose_frames, one launch fewer.               */
int pn_parse_paf_wire(pn_ctx *ctx, const float *heat_dev, const float *paf_dev, const float *z_dev,
                      int B, int h, int w, const pn_parse_cfg *cfg, pn_pose_frame *frames_dev,
                      pn_pose_wire *wire_dev, void *hip_stream);
size_t pn_sizeof_pose_wire(void);

/* ---- depth-ablation arms of the MP-3DHP evaluation (csrc/ablation.hip) ------------------------------------------------------------
 * The four read-outs tpm/evaluate/evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py compares (2D location from the prediction or
 * from the ground truth x depth from the pose-depth map or from the "raw depth" frame); pn_parse_paf writes the first
 * (human_pred_set_3d), these write the other three.  "Raw depth" is the script's un-normalised network input (:183-185, `img *= std;
 * img += mean` on float32): raw[y, x] = fl32(fl32(norm * depth_std) + depth_mean), norm = the pixel pn_preprocess writes -- re-derived
 * here from the raw frames with the same arithmetic, so the pre-processed tensor need not exist (pn_rtpose_forward_frames never
 * writes it).  depth_dev [B, H, W] f16 / f32 metres, resized to the square S = cfg->input_size; an exactly 2S x 2S frame is
 * PN_ERR_UNSUPPORTED as in pn_preprocess.  One launch per call, no allocation; the two pn_ablation_* calls do not synchronise.
 *   pn_ablation_pred_raw     human_pred_set_3d_read_raw_depth (:198-218, :245-274): frames_dev = the B records pn_parse_paf wrote; person i,
 *                            joint j with peak (x, y) = peak_x / peak_y[person_joint[i][j]] reads raw[int(y), int(x)] and gives
 *                            ((x2 - cx) raw / fx, (y2 - cy) raw / fy, raw) in float64, (x2, y2) = joints_2d[i][j]; a missing joint has raw = -1
 *                            and (x2, y2) = (-1, -1) through the same expression.  out_dev double [B][PN_MAX_PERSONS][PN_NUM_JOINTS][3], rows at
 *                            or beyond n_persons zero; the persons of a record with an overflow status are computed all the same.
 *   pn_ablation_perfect_2d   human_pred_set_3d_perfect_2d and _perfect_2d_read_raw_depth (:220-242, :279-299): gt_2d_dev double [B][Gmax][J][2]
 *                            (original-frame pixels, straight from the labels), gt_count_dev int32 [B] persons per frame; z_dev [B, L+1, h, w]
 *                            the pose-depth map as the network emits it, h = w = input_size / downsample.  Joint (gx, gy) reads
 *                            d = fl32(fl32(z[j][cy][cx] * depth_std) + depth_mean) at cx = clamp(int(gx / w_org * input_size / downsample), 0, w - 1)
 *                            (float64 left to right, int() truncating toward zero; cy alike with h_org) and raw[py, px] at
 *                            px = clamp(int(gx / w_org * input_size), 0, input_size - 1); out_map_dev / out_raw_dev double [B][Gmax][J][3] =
 *                            ((gx - cx) d / fx, (gy - cy) d / fy, d) with d resp. raw, rows at or beyond the frame's count zero.
 *                            Gmax = 0 or B = 0: nothing to do, PN_OK.
 *   pn_depth_probe           raw[y, x] of frame b for n points pts_dev int32 [n][3] = (frame, y, x) -> out_dev float [n].  The second-pass
 *                            entry (frames whose record overflowed are re-parsed without capacities and read their raw depth here) and a
 *                            test handle for the pixel arithmetic.  A point outside the batch or the S x S frame is PN_ERR_INVALID, never
 *                            clamped: the points are checked on the host first, so this call waits for the stream.
 * depth_dtype = PN_DEPTH_NET (all three): depth_dev is the network input itself, [B,1,S,S] f32 already clamped and normalised, as the
 * scripts that compose or augment their frames hold it (evaluation_rtpose_light3d_kdh3d_mpaug_ablation.py:206-207; there is no raw frame
 * to re-derive it from): raw[y, x] = fl32(fl32(depth_dev[b][y][x] * depth_std) + depth_mean).  H == W == S is required, else
 * PN_ERR_INVALID before any launch; depth_max is ignored and the 2x refusal does not apply (nothing is resized).                   */
int pn_ablation_pred_raw(pn_ctx *ctx, const void *depth_dev, int depth_dtype, int B, int H, int W, float depth_max,
                         const pn_parse_cfg *cfg, const pn_pose_frame *frames_dev, double *out_dev, void *hip_stream);
int pn_ablation_perfect_2d(pn_ctx *ctx, const void *depth_dev, int depth_dtype, int B, int H, int W, float depth_max,
                           const float *z_dev, int h, int w, const pn_parse_cfg *cfg, const double *gt_2d_dev,
                           const int *gt_count_dev, int Gmax, double *out_map_dev, double *out_raw_dev, void *hip_stream);
int pn_depth_probe(pn_ctx *ctx, const void *depth_dev, int depth_dtype, int B, int H, int W, int S, float depth_max,
                   float depth_mean, float depth_std, const int *pts_dev, int n, float *out_dev, void *hip_stream);

/* ---- training targets ----------------------------------------------------------
 * The CPU data-loader work of the reference's training dataset, as device kernels:
 *   pn_compose_depth      the z-buffer multi-person compositor of KDH3D_Keypoints.__getitem__
 *                         (tpm/lib/datasets/datasets_kdh3d_rtpose_mpaug.py:231-266, CR line endings): per output frame up to S
 *                         source frames fg_depth [B,S,H,W] (f16 / f32 metres) with foreground masks fg_mask [B,S,H,W]
 *                         (uint8 0 / 1), the first n_src[b] of them used, pasted over bg [B,H,W]; out [B,H,W] f32.
 *   pn_rasterize_targets  get_ground_truth (:318-401) = putGaussianMaps (heatmap.py:20-36) + putVecMaps (paf.py:18-69) +
 *                         putJointZ (posemap.py:83-106): kp2d [B,Pmax,15,2] f32 joint positions in network-input pixels
 *                         (as Resize leaves them), kp_z [B,Pmax,15] f64 joint depths (metres), n_persons [B],
 *                         depth_resize [B,h,w] f32 (the clamped input at stride resolution) ->
 *                         heat [B,16,h,w], paf [B,28,h,w], z [B,15,h,w] (normalised), fg [B,15,h,w]  f32 NCHW, h = input / stride. */
typedef struct pn_target_cfg {
    int input_x, input_y;      /* network input size (224) */
    int stride;                /* 8 */
    int z_radius;              /* 2   train_rtpose_light3d_kdh3d_mpaug.py default */
    double sigma;              /* 7.0 pixels  datasets_kdh3d_rtpose_mpaug.py:357 */
    double depth_max, depth_mean, depth_std;   /* 6, 3, 2 */
} pn_target_cfg;
void pn_target_cfg_default(pn_target_cfg *cfg);
int pn_compose_depth(pn_ctx *ctx, const void *fg_depth_dev, const unsigned char *fg_mask_dev, const int *n_src_dev,
                     const void *bg_dev, int depth_dtype, int B, int S, int H, int W, float depth_max, float *out_dev,
                     void *hip_stream);
int pn_rasterize_targets(pn_ctx *ctx, const float *kp2d_dev, const double *kp_z_dev, const int *n_persons_dev, int B, int Pmax,
                         const float *depth_resize_dev, const pn_target_cfg *cfg, float *heat_dev, float *paf_dev,
                         float *z_dev, float *fg_dev, void *hip_stream);
/* The background swap of the single-person loader (tpm/lib/datasets/datasets_kdh3d_rtpose.py:227-234, bg_aug):
 * out = fg_mask > 0 ? fg_depth : bg per pixel -- no z-buffer and no 2 * depth_max cap, so a foreground pixel beyond the cap survives
 * (pn_compose_depth with one source would cut it).  fg_depth, bg [B,H,W] f16 / f32 metres (depth_dtype), fg_mask [B,H,W] uint8, out
 * [B,H,W] f32; B <= 65535; asynchronous on hip_stream, one launch, like pn_compose_depth.                                          */
int pn_compose_bg(pn_ctx *ctx, const void *fg_depth_dev, const unsigned char *fg_mask_dev, const void *bg_dev, int depth_dtype,
                  int B, int H, int W, float *out_dev, void *hip_stream);

/* ---- random training augmentation ---------------------------------------------------------------------
 * The image half of the reference's training transform Compose([Cvt2ndarray, Rotate(cx, cy), RenderDepth(cx, cy, max_ratio), Crop,
 * Resize(S)]) (tpm/lib/datasets/data_augmentation_2d3d.py:411-448, 283-350, 94-128, 497-522) plus the clamp and normalisation of
 * pn_preprocess, as ONE launch for the batch: composed [B,H,W] f32 (what pn_compose_depth writes) -> out [B,1,S,S] f32
 *   out = (clamp(Resize(Crop(RenderDepth(Rotate(frame)))), 0, depth_max) - depth_mean) / depth_std
 * bit for bit what OpenCV 4.2's scalar float32 paths of warpAffine(INTER_LINEAR, constant border 0) and resize(INTER_LINEAR) give.
 * An item with hflip set is the ITOP trainers' chain, Hflip (:452-493) between RenderDepth and Crop: np.flip(axis=1) of the render image, as an
 * index reflection inside the same launch; items with hflip clear are computed exactly as before.
 * Each item has its own record.  The host decides every integer of the geometry (the int() truncations of RenderDepth and Crop,
 * numpy's clamping of slice ends) and inverts the rotation matrix in double, in warpAffine's own operation order.
 * items_host holds the B records; the call checks them, enqueues their upload into items_dev (room for B records, the caller's
 * buffer: nothing is allocated) on the stream and launches the kernel behind it, so the kernel reads exactly what was checked.  It
 * does not synchronise; items_host must stay untouched until the stream has passed the call (with pageable host memory the runtime
 * stages the bytes before the call returns).  An item whose source is exactly 2S x 2S is PN_ERR_UNSUPPORTED like pn_preprocess
 * (cv::resize runs INTER_AREA there); inconsistent geometry is PN_ERR_INVALID; nothing is copied or launched in either case.       */
typedef struct pn_augment_item {
    double m[6];                  /* Rotate: the INVERTED 2x3 matrix (destination pixel -> source), row major, as warpAffine holds it */
    float scale;                  /* RenderDepth: float32(a), a recomputed from the truncated corner                                  */
    int render_x, render_y;       /* where pixel (0,0) of the render image lies in the rotated frame: the slice start when a <= 1,
                                     (-dx, -dy) of the paste into the zero image otherwise                                            */
    int render_w, render_h;       /* size of the render image                                                                        */
    int crop_x0, crop_y0, crop_x1, crop_y1;   /* Crop's slice of the render image, ends exclusive and already clamped to its size    */
    int src_w, src_h;             /* the size Resize sees: crop_x1 - crop_x0, crop_y1 - crop_y0                                      */
    int hflip;                    /* Hflip (data_augmentation_2d3d.py:452-493), between RenderDepth and Crop: 1 = column x of the render
                                     image reads column render_w - 1 - x, 0 = no flip                                                */
} pn_augment_item;
size_t pn_sizeof_augment_item(void);
int pn_augment_resize(pn_ctx *ctx, const float *composed_dev, const pn_augment_item *items_host, pn_augment_item *items_dev,
                      int B, int H, int W, float *out_dev, int S, float depth_max, float depth_mean, float depth_std, void *hip_stream);

/* ---- training step primitives (BASELINE configs[4]) ------------------------------
 * fp32, NCHW, contiguous -- the layout of the reference's own tensors, so every intermediate can be laid next to the
 * reference module's.  One entry per differentiable primitive of rtpose_light3d in train mode; popnet_amd/train.py
 * strings them together (forward, rtpose_light3d_loss_fgweight, backward, Nesterov SGD).  All asynchronous on the stream.
 * They share ONE scratch buffer inside the pn_ctx (rotated weights, split-reduction partials), reused in stream order: drive a
 * pn_ctx's training primitives from one stream at a time (TrainEngine owns a private pn_ctx for that reason).
 *   pn_conv2d_forward   nn.Conv2d (tpm/lib/network/rtpose_light3d.py:31-40,144,232-246): kernel 1 / 3 / 7, any stride and
 *                       padding; accumulate != 0 adds into y.  w [Cout, Cin, k, k], bias [Cout] or NULL.
 *   pn_conv2d_dgrad     its input gradient (stride 1): dx [N,Cin,H,W] (+)= conv_transpose(dy [N,Cout,Ho,Wo], w)
 *   pn_conv2d_wgrad     its weight (and bias, if dbias != NULL) gradient
 *   pn_bn_train_forward nn.BatchNorm2d in train mode: batch statistics (biased variance, eps), running statistics updated
 *                       with `momentum` (unbiased variance) when given, y = act(bn(x) + res); act = 0 none, 1 ReLU,
 *                       2 LeakyReLU(0.1); res (BasicBlock identity, rtpose_light3d.py:66-67) or NULL
 *   pn_bn_train_backward  gradient of the above: dy is the gradient w.r.t. y, out = y (for the activation mask) -- or NULL when the
 *                       forward had no residual input: the mask is then recomputed from x with the forward's own expression
 *                       (same float operations, same result; one tensor less to read, beta required);
 *                       dres (or NULL) receives / accumulates the gradient of the residual input
 *   pn_avgpool3s2_*     nn.AvgPool2d(3, 2, 1) (rtpose_light3d.py:152,158), planes = N * C
 *   pn_head_forward     s = sigmoid(v); out = kind ? (s - 0.5) * 4 : s (rtpose_light3d.py:335-337) written with an image
 *                       stride of out_ld channels (a slice of the stage-2 input, :339); *loss = mean(w (out - target)^2),
 *                       w = 0.1 + 0.9 fg when fg != NULL (rtpose_light3d_loss_fgweight, losses.py:65-90)
 *   pn_head_backward    dv = (d loss / d out + dextra) * d out / d v; dextra [N, dextra_ld, HW] slice or NULL
 *   pn_slice_copy       torch.cat / its gradient: copy (or add) a [N, C, HW] tensor between channel slices
 *   pn_sgd_nesterov     torch.optim.SGD(momentum, nesterov=True) on a flat buffer (train_rtpose_light3d_kdh3d_mpaug.py:313-316);
 *                       grad_scale multiplies the gradient first (1 / world size after the all-reduce)
 *   pn_train_set_precision  PN_PREC_F32 (default: every product on v_mfma_f32_16x16x4_f32, exact fp32 FMA chains) or
 *                       PN_PREC_BF16X3: the 3x3 forward / data-gradient convolutions split every operand into two bf16
 *                       (16 mantissa bits) and run three v_mfma_f32_16x16x32_bf16 per product block -- fp32 tensors in and
 *                       out, results within ~1e-5 relative of the fp32 kernels, 5.3x less matrix-pipe time */
int pn_train_set_precision(pn_ctx *ctx, int precision);
/* keep != 0: a hipGraph captured from the training primitives points into the context's scratch; from now on a call that
 * needs a larger scratch retires the old block (freed by pn_destroy) instead of freeing it, so the graph stays replayable. */
int pn_train_ws_keep(pn_ctx *ctx, int keep);
/* Weight-pack cache of the 3x3 training convolutions (round 4).  Off (default): pn_conv2d_forward / _dgrad re-pack their weights
 * (transpose / rotate / split) into the context's scratch on every call.  On: the packs live in persistent buffers keyed by (weight
 * pointer, shape, rotation, precision); pn_train_pack_refresh re-packs ALL of them in one launch (call it once per step, before the
 * first convolution: popnet_amd.train.TrainEngine does), pn_sgd_nesterov marks them stale, a stale or unknown pack is rebuilt by the
 * call that needs it.  Weights changed by anything but pn_sgd_nesterov need a refresh before the next convolution.  Replaces the
 * 62 pack launches per step of train_rtpose_light3d_kdh3d_mpaug.py:160-180's forward / backward (tpm/lib/network/rtpose_light3d.py). */
int pn_train_pack_cache(pn_ctx *ctx, int enable);
int pn_train_pack_refresh(pn_ctx *ctx, void *hip_stream);
int pn_conv2d_forward(pn_ctx *ctx, const float *x_dev, const float *w_dev, const float *bias_dev, float *y_dev, int N, int Cin,
                      int H, int W, int Cout, int ks, int stride, int pad, int accumulate, void *hip_stream);
int pn_conv2d_dgrad(pn_ctx *ctx, const float *dy_dev, const float *w_dev, float *dx_dev, int N, int Cin, int H, int W, int Cout,
                    int ks, int pad, int accumulate, void *hip_stream);
int pn_conv2d_wgrad(pn_ctx *ctx, const float *x_dev, const float *dy_dev, float *dw_dev, float *dbias_dev, int N, int Cin, int H,
                    int W, int Cout, int ks, int stride, int pad, void *hip_stream);
int pn_bn_train_forward(pn_ctx *ctx, const float *x_dev, const float *gamma_dev, const float *beta_dev, const float *res_dev,
                        float *y_dev, float *save_mean_dev, float *save_invstd_dev, float *running_mean_dev,
                        float *running_var_dev, float momentum, float eps, int act, int N, int C, int HW, void *hip_stream);
int pn_bn_train_backward(pn_ctx *ctx, const float *x_dev, const float *dy_dev, const float *out_dev, const float *gamma_dev,
                         const float *beta_dev, const float *save_mean_dev, const float *save_invstd_dev, int act, int N, int C, int HW, float *dx_dev,
                         float *dgamma_dev, float *dbeta_dev, float *dres_dev, int dres_accumulate, void *hip_stream);
int pn_avgpool3s2_forward(pn_ctx *ctx, const float *x_dev, float *y_dev, int planes, int H, int W, void *hip_stream);
int pn_avgpool3s2_backward(pn_ctx *ctx, const float *dy_dev, float *dx_dev, int planes, int H, int W, void *hip_stream);
int pn_head_forward(pn_ctx *ctx, const float *v_dev, const float *target_dev, const float *fg_dev, int kind, int N, int C, int HW,
                    float *s_dev, float *out_dev, int out_ld, float *loss_dev, void *hip_stream);
int pn_head_backward(pn_ctx *ctx, const float *s_dev, const float *target_dev, const float *fg_dev, const float *dextra_dev,
                     int dextra_ld, int kind, int N, int C, int HW, float *dv_dev, void *hip_stream);
int pn_slice_copy(pn_ctx *ctx, const float *src_dev, int src_ld, float *dst_dev, int dst_ld, int N, int C, int HW, int accumulate,
                  void *hip_stream);
int pn_sgd_nesterov(pn_ctx *ctx, float *param_dev, const float *grad_dev, float *momentum_buf_dev, size_t n, float lr,
                    float momentum, float weight_decay, int first_step, float grad_scale, void *hip_stream);
/* Diagnostics (tests): which kernel a convolution primitive would launch for a shape under the context's current precision
 * (pn_train_set_precision) and kernel switches, as JSON: "kernel" (the label, e.g. tconv3_tile_x3w_kernel, tconv_wgrad_kernel<1>), "pack"
 * (the weight pack kernel the call runs or reads from the cache), the tile geometry "TW", "R", "tiles_x", "tiles_y" (0 for the generic
 * kernels), "grid"; for PN_PLAN_WGRAD also "slices", "per_slice" tiles or pixels ("per_slice_unit") and "t_slices", the slices of the
 * bias-gradient reduction.  It calls the very functions the launches decide with and launches nothing: a context without a device will
 * do (so does pn_train_set_precision).  PN_PLAN_DGRAD ignores stride.  PN_ERR_INVALID for arguments the entry itself refuses or when cap
 * is too small.  pn_train_reduce_slices: the slices of pn_bn_train_forward / _backward's per-channel reductions (negative: bad arguments). */
enum { PN_PLAN_FORWARD = 0, PN_PLAN_DGRAD = 1, PN_PLAN_DGRAD_STRIDED = 2, PN_PLAN_WGRAD = 3 };
int pn_train_conv_plan_info(pn_ctx *ctx, int which, int N, int Cin, int H, int W, int Cout, int ks, int stride, int pad, char *out,
                            size_t cap);
int pn_train_reduce_slices(pn_ctx *ctx, int N, int C, int HW);

/* ---- YoloPoseNet training primitives (csrc/train_yolo.hip) ------------------------------------------------------------------
 * What YoloPoseNet's train-mode forward / loss / backward needs beyond the rtpose primitives above; fp32 NCHW, asynchronous on the
 * stream, fixed summation orders (a repeated call gives the same bits), no float atomics.
 *   pn_conv2d_dgrad_strided  input gradient of nn.Conv2d at any stride (ks 1 or 3; layer2.0.conv1 / layer2.0.downsample.0 of
 *                       tpm/lib/network/resnet.py run at stride 2): dx [N,Cin,H,W] (+)= the gather over the taps that hit each input
 *                       pixel of dy [N,Cout,Ho,Wo] * w [Cout,Cin,ks,ks] -- one fmaf chain per pixel, output channel outer, taps row-major
 *   pn_maxpool_forward  nn.MaxPool2d(k, stride, pad) (tpm/lib/network/yolo_posenet.py:36,114), planes = N * C; idx = int32 flat index
 *                       of the maximum inside its plane; ties and NaN as PyTorch's CPU max_pool2d_with_indices (first maximum of the
 *                       row-major window, the last NaN of a window)
 *   pn_maxpool_backward dx [planes,H,W] = per pixel, the sum in output row-major order of the dy whose idx is that pixel
 *   pn_yolo_loss        the per-slice casts of YoloPoseNet.forward (yolo_posenet.py:146-156) applied to the last convolution's raw
 *                       output v [N, A(5+3J), h, w] (channel a(5+3J) + k) -> out (the module's output), terms [4] = loss_prior,
 *                       loss_bbox, loss_obj, loss_selfpose of yolo_loss_fgweight_poseweight (weight_map [N,A,h,w] given) or
 *                       yolo_loss_fgweight (weight_map NULL) (tpm/lib/network/losses.py:397-466), and dv = d loss_prior / d v;
 *                       prior_map as out, mask_conf / mask_coord [N,A,h,w]
 *   pn_build_prior_targets  build_prior_targets + bbox_ious (tpm/lib/datasets/datasets_kdh3d_mpaug.py:353-417,505-533, CR) for a
 *                       batch: boxes [B,Pmax,4] f64 (x0, y0, x1, y1 network-input pixels, as Resize leaves ann['bbox']), kp2d
 *                       [B,Pmax,J,2] f32, kp_z [B,Pmax,J] f64 metres, pose_weight [B,Pmax] f64, n_persons [B] -> prior_map
 *                       [B,A(5+3J),h,w], mask_conf / mask_coord / weight_map [B,A,h,w] f32, h = int(input_y / stride_prior).
 *                       float64 arithmetic in the reference's order, stored as float32; where persons share a cell the last one
 *                       in list order writes it.  boxes / kp2d / kp_z / pose_weight may be NULL when Pmax = 0. */
#define PN_YOLO_MAX_ANCHORS 8
typedef struct pn_yolo_target_cfg {
    int input_x, input_y;      /* network input size (224) */
    int stride_prior;          /* 16  datasets_kdh3d_mpaug.py:229-230 */
    int num_joints;            /* 15 */
    int num_anchors;           /* 2 */
    double anchors[PN_YOLO_MAX_ANCHORS][2];   /* (w, h) in prior cells: (6, 3), (12, 6)  train_yolo_posenet_kdh3d_mpaug.py:45 */
    double noobject_scale, object_scale;      /* 0.1, 1.0 */
    double depth_mean, depth_std;             /* 3, 2 */
} pn_yolo_target_cfg;
void pn_yolo_target_cfg_default(pn_yolo_target_cfg *cfg);
int pn_conv2d_dgrad_strided(pn_ctx *ctx, const float *dy_dev, const float *w_dev, float *dx_dev, int N, int Cin, int H, int W, int Cout,
                            int ks, int stride, int pad, int accumulate, void *hip_stream);
int pn_maxpool_forward(pn_ctx *ctx, const float *x_dev, float *y_dev, int *idx_dev, int planes, int H, int W, int k, int stride, int pad,
                       void *hip_stream);
int pn_maxpool_backward(pn_ctx *ctx, const float *dy_dev, const int *idx_dev, float *dx_dev, int planes, int H, int W, int k, int stride,
                        int pad, void *hip_stream);
int pn_yolo_loss(pn_ctx *ctx, const float *v_dev, const float *prior_map_dev, const float *mask_conf_dev, const float *mask_coord_dev,
                 const float *weight_map_dev, int N, int A, int J, int h, int w, float *out_dev, float *terms_dev, float *dv_dev,
                 void *hip_stream);
int pn_build_prior_targets(pn_ctx *ctx, const double *boxes_dev, const float *kp2d_dev, const double *kp_z_dev, const double *pose_weight_dev,
                           const int *n_persons_dev, int B, int Pmax, const pn_yolo_target_cfg *cfg, float *prior_map_dev,
                           float *mask_conf_dev, float *mask_coord_dev, float *weight_map_dev, void *hip_stream);

/* ---- A2J training primitives (csrc/train_a2j.hip; the dilated convolutions in csrc/train.hip) ---------------------------------
 * What A2J_model's train-mode forward / loss / backward / optimizer step (third_party_methods/A2J_experiments/train_a2j_mpaug_new.py)
 * needs beyond the primitives above; fp32, asynchronous on the stream, fixed summation orders (a repeated call gives the same bits),
 * no float atomics.
 *   pn_conv2d_forward_dil / _dgrad_dil / _wgrad_dil   pn_conv2d_forward / _dgrad / _wgrad with the taps `dil` pixels apart
 *                       (layer4.1 / layer4.2 conv2, resnet.py:112,145: kernel 3, padding = dilation = 2).  Accepted: ks == 3, stride 1,
 *                       dil >= 1, 0 <= pad <= 2 dil, Ho = H + 2 pad - 2 dil >= 1; anything else is PN_ERR_INVALID before any launch.
 *                       dil == 1 IS the undilated entry (same bits).  dil > 1: the matrix-core implicit GEMM of the generic path
 *                       (v_mfma_f32_16x16x4_f32, k = (ci, ky, kx) in order) gathering at iy0 + ky dil; the data gradient is that forward
 *                       on the rotated, transposed weights with padding 2 dil - pad; the weight gradient sums pixel slices in slice order.
 *   pn_a2j_loss         A2J_loss.forward (anchor.py:84-154) and its gradient on the three raw head maps where the last convolutions left
 *                       them: cls / dep [B, A P, h, w], reg [B, A P 2, h, w] NCHW, channel a P + p (reg: (a P + p) 2 + c), anchor
 *                       k = (x h + y) A + a of anchors_dev [K, 2] (the array pn_a2j_vote takes).  h == 0: the reference's own layout
 *                       [B, K, P] / [B, K, P, 2] with K = w and A = 1.  labels_dev [B, P, 3]: two columns in the anchors' coordinate order, then z.
 *                       Per crop and joint: w_k = softmax_k(cls) (max-subtracted); Cls = mean over (P, 2) of smooth-L1 (beta 1) of
 *                       |gt - sum_k w_k anchor_k|; Reg = spatial_factor x the same with anchor_k + reg_k, plus mean_P |gt_z - sum_k w_k dep_k|
 *                       (the PLAIN L1: anchor.py:151 adds regression_diff_depth.mean(), not its smooth form).  Both are means over the batch.
 *                       terms_dev [2] = (Cls, Reg).  dcls / dreg / ddep (all three or all NULL; the inputs' layout) receive
 *                       d (s_cls Cls + s_reg Reg) / d input with (s_cls, s_reg) read from scale_dev [2] ON THE DEVICE (an autograd backward
 *                       passes its incoming gradients without a host synchronisation); d|x|/dx = 0 at 0, as torch.abs.  One workgroup per
 *                       (crop, joint), lanes along x; the per-(crop, joint) partials are summed by a second launch in a fixed order.
 *   pn_adam             torch.optim.Adam(betas, eps, weight_decay) on a flat buffer, step t >= 1 counted by the caller:
 *                       g = grad_scale g + wd p; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g;
 *                       p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps), the hyperparameters as the doubles torch holds them, the element
                       arithmetic in double, p / m / v rounded to float once each.  Any n; 16-byte accesses only when all four buffers are
 *                       16-byte aligned, and then only on the first n - n % 4 elements.  Marks the context's cached weight packs stale, as
 *                       pn_sgd_nesterov does. */
int pn_conv2d_forward_dil(pn_ctx *ctx, const float *x_dev, const float *w_dev, const float *bias_dev, float *y_dev, int N, int Cin,
                          int H, int W, int Cout, int ks, int stride, int pad, int dil, int accumulate, void *hip_stream);
int pn_conv2d_dgrad_dil(pn_ctx *ctx, const float *dy_dev, const float *w_dev, float *dx_dev, int N, int Cin, int H, int W, int Cout,
                        int ks, int pad, int dil, int accumulate, void *hip_stream);
int pn_conv2d_wgrad_dil(pn_ctx *ctx, const float *x_dev, const float *dy_dev, float *dw_dev, float *dbias_dev, int N, int Cin, int H,
                        int W, int Cout, int ks, int stride, int pad, int dil, void *hip_stream);
int pn_a2j_loss(pn_ctx *ctx, const float *cls_dev, const float *reg_dev, const float *dep_dev, int B, int h, int w, int A, int P,
                const float *anchors_dev, const float *labels_dev, float spatial_factor, const float *scale_dev, float *terms_dev,
                float *dcls_dev, float *dreg_dev, float *ddep_dev, void *hip_stream);
int pn_adam(pn_ctx *ctx, float *param_dev, const float *grad_dev, float *exp_avg_dev, float *exp_avg_sq_dev, size_t n, double lr,
            double beta1, double beta2, double eps, double weight_decay, int t, double grad_scale, void *hip_stream);

/* ---- 1x1 training convolutions in split bf16 (csrc/conv1x1_x3.hip, conv1x1_x3_kernels.h) -----------------------------------------
 * The 1x1, stride-1, pad-0 convolutions of a ResNet bottleneck (conv1, conv3, the stride-1 downsample) on the bf16 matrix cores, for
 * A2JTrainEngine(precision="bf16x3").  Entries of their own: pn_conv2d_forward / _dgrad / _wgrad keep running every 1x1 call on the fp32
 * kernels whatever pn_train_set_precision says, and these do not read that switch.  Tensors are fp32 NCHW with HW = H W pixels per map:
 *   pn_conv1x1_x3_forward   y[n, co, p] (+)= bias[co] + sum_ci x[n, ci, p] w[co, ci]            (bias_dev may be NULL)
 *   pn_conv1x1_x3_dgrad     dx[n, ci, p] (+)= sum_co dy[n, co, p] w[co, ci]                     (the forward kernel on the transposed pack)
 *   pn_conv1x1_x3_wgrad     dw[co, ci] = sum_{n, p} dy[n, co, p] x[n, ci, p]; dbias[co] = sum dy (dbias_dev may be NULL; pn_conv2d_wgrad's
 *                           double-precision channel reduction)
 * Arithmetic: BOTH operands are split, hi = RNE_bf16(v), lo = RNE_bf16(fp32(v - hi)), and every block of 32 k is three
 * v_mfma_f32_16x16x32_bf16 into one fp32 accumulator: a_hi b_hi + a_hi b_lo + a_lo b_hi, no lo * lo term.  The bias is added once to the
 * accumulator; with accumulate != 0 the previous output is added after it.  k runs in order (chunks of 32 channels; for the weight gradient
 * chunks of 32 pixels that never straddle two images, in slices whose partial sums a second launch adds in slice order): the summation
 * order depends on the shape alone, a repeated call gives the same bits, no float atomics.  Any N, Cin, HW, Cout >= 1 (k tails, ragged
 * channel blocks and pixel tiles are masked in the kernels; the weight gradient uses 16-byte loads only when HW % 4 == 0 and both
 * tensors are 16-byte aligned, element loads otherwise and at the ragged end of an image); N, Cin, HW, Cout < 1 or a NULL tensor is
 * PN_ERR_INVALID before any launch.  The [hi | lo] weight pack and its transpose live in the pack cache (pn_train_pack_cache;
 * pn_train_pack_refresh rebuilds them, pn_adam / pn_sgd_nesterov mark them stale); with the cache off they are packed on every call.
 *   pn_conv1x1_x3_plan_info  the launch code's own plan of one call as JSON, launching nothing; works on pn_create(-1).  which =
 *                           PN_PLAN_FORWARD / PN_PLAN_DGRAD / PN_PLAN_WGRAD.  Fields: kernel (label; "split": true -- no shape is kept on
 *                           the fp32 kernels), BM / BN / BK (block tile: A rows, B rows, k), grid, lds; forward / dgrad: M, K (output and
 *                           reduced channels), P = N HW, chunks; wgrad: slices, per_slice (pixels, a multiple of 32: chunk padding counted),
 *                           per_slice_chunks, chunks, chunks_per_image, aligned (the label says <vec> / <scalar>; for 16-byte aligned
 *                           tensors), csl (the bias gradient's slices). */
int pn_conv1x1_x3_forward(pn_ctx *ctx, const float *x_dev, const float *w_dev, const float *bias_dev, float *y_dev, int N, int Cin, int HW,
                          int Cout, int accumulate, void *hip_stream);
int pn_conv1x1_x3_dgrad(pn_ctx *ctx, const float *dy_dev, const float *w_dev, float *dx_dev, int N, int Cin, int HW, int Cout,
                        int accumulate, void *hip_stream);
int pn_conv1x1_x3_wgrad(pn_ctx *ctx, const float *x_dev, const float *dy_dev, float *dw_dev, float *dbias_dev, int N, int Cin, int HW,
                        int Cout, void *hip_stream);
int pn_conv1x1_x3_plan_info(pn_ctx *ctx, int which, int N, int Cin, int HW, int Cout, char *out, size_t cap);

/* ---- training step on NHWC [hi | lo] bf16 planes (round 6; csrc/trainx.hip) -------------------------------------------------
 * One object runs forward + loss + backward of rtpose_light3d(15, 14, 2, input_dim = 1) in train mode for ONE batch shape:
 * the per-batch body of tpm/train_rtpose_light3d_kdh3d_mpaug.py:160-180 (CR) up to (not including) optimizer.step(), i.e.
 * model(img) (tpm/lib/network/rtpose_light3d.py:326-356, BatchNorm on batch statistics, running statistics updated),
 * rtpose_light3d_loss_fgweight (tpm/lib/network/losses.py:65-106) and loss.backward().  Split-bf16 arithmetic (PN_PREC_BF16X3:
 * 16 significant bits per operand, fp32 accumulate); forward and data-gradient convolutions run the inference kernels
 * (conv3_kernel / conv4_kernel / conv_mfma_kernel), the weight gradient a pixel-K MFMA GEMM (trainx_wgrad.h).
 * Parameters and gradients live in the CALLER's flat fp32 buffers (one float per parameter element, any tensor order):
 *   pn_trainer_set_param   where tensor `name` ("model0.layer1.0.conv1.weight", ...; the reference's state_dict keys) starts in
 *                          both flat buffers (offset in floats; 16-byte aligned offsets recommended) and how many elements it has
 *   pn_trainer_set_stat    device pointer of a BatchNorm running_mean / running_var tensor (updated in place every step)
 *   pn_trainer_finalize    plans the step for batch B of H x W inputs (multiples of 8), allocates every activation / gradient
 *                          tensor and descriptor; nothing is allocated afterwards (the step can be captured in a hipGraph)
 *   pn_trainer_forward_backward   img [B,1,H,W], heat_gt [B,16,H/8,W/8], paf_gt [B,28,..], z_gt [B,15,..], fg_mask [B,15,..] f32 NCHW;
 *                          writes the six loss terms (l1_paf, l1_heat, l1_z, l2_paf, l2_heat, l2_z) and every gradient
 *                          (asynchronous on hip_stream); apply them with pn_sgd_nesterov. */
typedef struct pn_trainer pn_trainer;
pn_trainer *pn_trainer_create(pn_ctx *ctx);
void pn_trainer_destroy(pn_trainer *t);
/* PN_PREC_BF16X3 (default): tensors as [hi | lo] bf16 planes, split-bf16 MFMA.  PN_PREC_F32: one fp32 plane per tensor, every product an exact fp32 FMA
 * chain on v_mfma_f32_16x16x4_f32 (the generic fp32 inference kernel for forward / data gradient, a K = 4 pixel weight gradient): the parity mode.
 * Call before pn_trainer_finalize. */
int pn_trainer_set_precision(pn_trainer *t, int precision);
int pn_trainer_set_param(pn_trainer *t, const char *name, size_t offset, size_t numel);
int pn_trainer_set_stat(pn_trainer *t, const char *name, float *stat_dev);
int pn_trainer_finalize(pn_trainer *t, float *flat_param_dev, float *flat_grad_dev, int B, int H, int W, float bn_momentum, float bn_eps);
int pn_trainer_forward_backward(pn_trainer *t, const float *img_dev, const float *heat_gt_dev, const float *paf_gt_dev, const float *z_gt_dev,
                                const float *fg_mask_dev, float *loss_terms_dev, void *hip_stream);
/* split-bf16 MFMA FLOPs (3 x 2 MAC) of the convolutions one step runs on the matrix cores (forward + data gradient; the weight gradient has the forward's count) */
double pn_trainer_conv_flops(pn_trainer *t);
/* Diagnostics of a finalized trainer (per-op checks; nothing here runs unless called).
 * pn_trainer_num_ops: entries of the step's op list.  pn_trainer_op_info writes a JSON description of op k: "kind" (pack, stem_fwd, bn_fwd,
 * conv, pool_fwd, heads, bn_bwd, dbias, wgrad, add, pool_bwd, stem_wgrad, fork, join), "stream" (step / side), "kernels" (labels; convolutions as
 * pn_net_step_info labels them), and per problem the layer / BatchNorm name and every tensor read or written as {"t": id, "coff", "c"}; a
 * weight gradient also has tiles_x, Wt, rows_per_block and the slice count Sr.  k = -1 describes the trainer: precision, B, H, W and the
 * tensor table [H, W, plane] by id.  PN_ERR_INVALID when cap is too small.
 * pn_trainer_run_ops runs ops [first, last) with the per-step pointers of pn_trainer_forward_backward, then waits for hip_stream AND the side
 * stream (a range may end between a fork and its join).
 * pn_trainer_read_tensor / pn_trainer_write_tensor move frames [frame0, frame0 + nframes) of tensor `id` as f32 NCHW [nframes][plane][H][W]
 * (host memory; host_elems must be exactly that count).  which: 0 the value (hi + lo), 1 / 2 the stored hi / lo plane (bf16x3 trainers).
 * Writing splits as the kernels' stores do: hi = bf16(v), lo = bf16(v - hi).  Both wait for the two streams first.
 * pn_trainer_read_vector: "<BatchNorm name>.mean | invstd | scale | shift | k1 | k2 | k3" ([C]) or "head_out.<stage 0|1>.<0 paf|1 heat|2 z>"
 * (f32 NCHW).  A bad id, range, name or element count is PN_ERR_INVALID. */
int pn_trainer_num_ops(pn_trainer *t);
int pn_trainer_op_info(pn_trainer *t, int k, char *out, size_t cap);
int pn_trainer_run_ops(pn_trainer *t, const float *img_dev, const float *heat_gt_dev, const float *paf_gt_dev, const float *z_gt_dev,
                       const float *fg_mask_dev, float *loss_terms_dev, int first, int last, void *hip_stream);
int pn_trainer_read_tensor(pn_trainer *t, int id, int which, int frame0, int nframes, float *host_out, size_t host_elems, void *hip_stream);
int pn_trainer_write_tensor(pn_trainer *t, int id, int frame0, int nframes, const float *host_in, size_t host_elems, void *hip_stream);
int pn_trainer_read_vector(pn_trainer *t, const char *name, float *host_out, size_t host_elems, void *hip_stream);

/* ---- Yolo-Pose+ decode ----------------------------------------------------------------------
 * Replaces parse_prior_pose (tpm/lib/utils/prior_pose_align.py:10-168, pred_vis=False), quirks
 * included (candidate order anchor-major; suppression loop over rows 1..n-2; inclusive
 * visibility test).  Unlike the reference it does NOT modify posemaps in place.               */
#define PN_YOLO_MAX_DET 64
typedef struct pn_yolo_frame {
    int32_t n_det;                 /* surviving boxes (<= PN_YOLO_MAX_DET) */
    int32_t n_candidates;          /* conf > threshold before NMS */
    uint32_t status;               /* bit0: more than PN_YOLO_MAX_DET survivors (truncated) */
    int32_t reserved;
    float   bbox[PN_YOLO_MAX_DET][5];                 /* x1, y1, x2, y2, conf (pixels) */
    float   human[PN_YOLO_MAX_DET][PN_NUM_JOINTS][3]; /* x, y (pixels), Z (metres) */
    int32_t visibility[PN_YOLO_MAX_DET][PN_NUM_JOINTS];
    /* per-frame glue of tpm/evaluate/evaluation_yolo_posenet_kdh3d_mpreal.py:182-217 (float32, as the
     * script computes it): joints rescaled to the original frame and back-projected; part confidence =
     * bbox[4] for every joint.  Filled when pn_parse_yolo is given a glue configuration. */
    float   joints_2d[PN_YOLO_MAX_DET][PN_NUM_JOINTS][2];
    float   joints_3d[PN_YOLO_MAX_DET][PN_NUM_JOINTS][3];
    float   bbox_org[PN_YOLO_MAX_DET][4];             /* box corners rescaled to the original frame (:197-200) */
} pn_yolo_frame;

int pn_parse_yolo(pn_ctx *ctx, const float *posemaps_dev, int B, int h, int w,
                  const float *anchors_wh, int num_anchors, int num_joints, int w_out, int h_out,
                  float depth_mean, float depth_std, float conf_threshold, float nms_threshold,
                  int vis_margin, const pn_parse_cfg *glue /* may be NULL: input_size, w_org, h_org, intrinsics */,
                  pn_yolo_frame *frames_dev, void *hip_stream);

/* pred_vis=True (prior_pose_align.py:62,120,153-157): the maps carry 5 + 4 J channels per anchor, the last J being predicted
 * visibilities; vis_pred_dev [B][PN_YOLO_MAX_DET][J] float32 receives (in-bounds test) * (that channel), the value the
 * reference returns as `visibility` in this mode.  Everything else as pn_parse_yolo. */
int pn_parse_yolo_predvis(pn_ctx *ctx, const float *posemaps_dev, int B, int h, int w,
                          const float *anchors_wh, int num_anchors, int num_joints, int w_out, int h_out,
                          float depth_mean, float depth_std, float conf_threshold, float nms_threshold,
                          int vis_margin, const pn_parse_cfg *glue, pn_yolo_frame *frames_dev, float *vis_pred_dev,
                          void *hip_stream);

size_t pn_sizeof_yolo_frame(void);

/* Host-only diagnostic: the four float32 bicubic taps (OpenCV interpolateCubic, A = -0.75) the
 * parse kernels use for fractional offset x.  Lets CPU tests pin the table against the oracle.   */
void pn_debug_cubic_coeffs(float x, float *out4);

/* ---- Yolo-A2J: per-box crops, A2J_model, anchor vote -------------------------------------------
 * The third baseline of the reference's results table (third_party_methods/A2J_experiments/): YoloPoseNet finds the boxes
 * (evaluation_yolo_posenet_kdh3d_mpreal_a2j_preprocess.py:153-228: rows [x0, y0, x1, y1, conf] in original-frame pixels, one row
 * [-1, -1, -1, -1, 0] for a frame without a detection), A2J regresses 15 joints per box crop.
 * A net of kind PN_NET_A2J (pn_net_create(ctx, PN_NET_A2J, 15, 16, 1)) takes the reference's A2J_model state dict ("Backbone.model.*",
 * "regressionModel.*", "classificationModel.*", "DepthRegressionModel.*"; Backbone.model.fc.* and *.num_batches_tracked are accepted and
 * ignored) and any input size that is a multiple of 16, in any of the three precisions (PN_PREC_BF16X3: every map, the heads included, is a [hi | lo] plane pair).  The three
 * identical input channels of ResNetBackBone.forward (model.py:155-156) are one channel with the 7x7 weights summed over Cin in double.
 * layer4's blocks 1 and 2 run conv2 at dilation 2 (resnet.py:112,145): pn_net_step_info reports "dil": 2 for those steps only.
 * In PN_PREC_F32 the convolutions of this net accumulate in blocks (the 32 products of a k-step are summed from zero, then added to the running
 * sum; "blocked_acc": 1 in pn_net_step_info): its K loops run to 18 432 terms, where one serial fp32 chain is several times the reference's own
 * fp32 error away from an fp64 run.  The other nets keep the serial chain they are tested bit for bit with.                                 */
typedef struct pn_a2j_cfg {
    int img_w, img_h;          /* the module constants imgWidth / imgHeight of a2j_test_pred_box_new.py:30-31 (480, 512): a box that leaves
                                  [0, img_w] x [0, img_h] is pasted into a zero image -- independent of the frame's real shape */
    int crop_w, crop_h;        /* cropWidth / cropHeight (:32-33), 288 x 288 */
    float mean, std;           /* MEAN / STD (:61-62), 3 and 2 */
    float conf_min;            /* a row with conf <= conf_min is an all-zero crop (:273), 0.01 */
    double fx, fy, cx, cy;     /* intrinsics (:35) */
} pn_a2j_cfg;
void pn_a2j_cfg_default(pn_a2j_cfg *cfg);
/* One fixed-size record per crop (a2j_test_pred_box_new.py:373-421): per joint x, y (original-frame pixels), X, Y, Z (metres), then the
 * box confidence (the part confidence of every joint, :385) and the frame index of the row. */
typedef struct pn_a2j_record {
    float joint[PN_NUM_JOINTS][5];
    float conf;
    int32_t frame;
} pn_a2j_record;
size_t pn_sizeof_a2j_record(void);
/* dataPreprocess (a2j_test_pred_box_new.py:268-313), one launch for all rows, bit for bit, quirks included.  frames_dev [F, H, W] f16 / f32
 * (device); rows_dev [n][6] f32 (device): frame index, x0, y0, x1, y1, conf.  out_dev [n, 1, crop_h, crop_w] f32: what the net's stem reads.
 *   conf <= conf_min: zeros.  Otherwise the box is clipped to the frame (max(., 0), min(., W - 1 / H - 1)), depth[int(ymin):int(ymax),
 *   int(xmin):int(xmax)] is taken (last row and column excluded); if the RAW box leaves [0, img_w] x [0, img_h] the crop is pasted into a zero
 *   image of int(y1 - y0) x int(x1 - x0) whose paste loop tests start < i < end strictly (the first pasted row and column stay zero); then
 *   cv2.resize(INTER_NEAREST) (source index min(floor(d * (1 / (dsize / ssize))), ssize - 1) in double) and (v - mean) / std in fp32, no clamp.
 *   Where the reference raises -- the image handed to cv2.resize is empty: a clipped region without rows or columns that is not pasted, or a
 *   paste image without rows or columns -- the crop is zeros and flags_dev[row] (may be NULL) is 1, else 0.  A clipped END that is negative
 *   counts from the far edge, as Python's slice does (depth[2:-3]), which is also what popnet_amd.a2j_crops.box_items uploads.
 *   The rows are device data: nothing in them is trusted.  A row above conf_min whose x0, y0, x1, y1, x1 - x0 or y1 - y0 is NaN, infinite or
 *   past what an int holds (|v| > 2^31 - 128) is such a raise as well (int(nan), int(inf), a zero image of an absurd size): zeros, flag 1; at
 *   or below conf_min (a NaN confidence included) the coordinates are never read: zeros, flag 0.  A frame index outside [0, F), NaN included,
 *   names no frame the reference could load, which it does before it looks at the confidence: zeros, flag 1, whatever the confidence.
 *   pn_a2j_vote's record of such a row carries the frame index as it is, or -1 where it is NaN or past an int. */
int pn_a2j_crop(pn_ctx *ctx, const void *frames_dev, int depth_dtype, int F, int H, int W, const float *rows_dev, int n,
                const pn_a2j_cfg *cfg, float *out_dev, int32_t *flags_dev, void *hip_stream);
/* A2J_model.forward (model.py:179-186) on crops_dev [B, 1, in_h, in_w] f32.  The head maps stay on the device as the last convolutions
 * left them: NHWC [B, h, w, 16 x 15] (classification, depth) and [B, h, w, 16 x 15 x 2] (regression), h = in_h / 16, bf16 or f32 by the
 * net's precision (pn_a2j_head_shape; PN_PREC_BF16X3: a pixel's row is the bf16 planes [hi | lo], the value hi + lo).  The pointers stay valid until the net is destroyed; the next forward overwrites the maps. */
int pn_a2j_forward(pn_net *net, const float *crops_dev, int B, const void **cls_dev, const void **reg_dev, const void **dep_dev,
                   void *hip_stream);
int pn_a2j_head_shape(pn_net *net, int *h, int *w, int *precision);
/* post_process.forward (anchor.py:57-82): per crop and joint w = softmax(cls over all K anchors), P_yx = sum w (anchor + reg),
 * P_z = sum w dep -- max-subtracted softmax and sums in fp32, one block per (crop, joint), one launch.  anchors_dev [K][2] f32 (y, x) is
 * shift([h, w], stride, generate_anchors()) (anchor.py:7-42) computed by the caller in the reference's own arithmetic: anchor k belongs to
 * cell k / A, column (k / A) / h, row (k / A) % h (W-major, as the reference's permute(0, 3, 2, 1)).
 * h > 0: the heads are the NHWC maps of pn_a2j_forward (precision = the net's), read in place.  PN_PREC_BF16X3: a value is hi + lo added in
 * fp32 (exact); one block per crop reads the plane pairs in 16-byte pieces (A x P a multiple of 8).  h == 0 (f32 only): the heads are f32 tensors in the
 * reference's layout [B, K, P] / [B, K, P, 2] (K = w: pass the anchor count as w).  A = anchors per cell, P = joints.
 * votes_dev [B, P, 3] f32 (y, x, z), may be NULL when records are wanted only.
 * rows_dev / cfg / records_dev (all or none): the map back to the frame (a2j_test_pred_box_new.py:373-421) in the same launch, in the
 * script's float32 arithmetic -- x = x_crop (x1 - x0) / crop_w + x0, X = (x - cx) Z / fx. */
int pn_a2j_vote(pn_ctx *ctx, const void *cls_dev, const void *reg_dev, const void *dep_dev, int precision, int B, int h, int w, int A, int P,
                const float *anchors_dev, float *votes_dev, const float *rows_dev, const pn_a2j_cfg *cfg, pn_a2j_record *records_dev,
                void *hip_stream);
/* frames + box rows -> records: pn_a2j_crop, pn_a2j_forward and pn_a2j_vote for n <= the net's max_batch rows.  crops_dev: scratch
 * [n, 1, crop_h, crop_w] f32; the net must be finalized for crop_h x crop_w; anchors_dev as in pn_a2j_vote for stride 16. */
int pn_a2j_predict(pn_net *net, const void *frames_dev, int depth_dtype, int F, int H, int W, const float *rows_dev, int n,
                   const pn_a2j_cfg *cfg, const float *anchors_dev, float *crops_dev, int32_t *flags_dev, float *votes_dev,
                   pn_a2j_record *records_dev, void *hip_stream);

/* ---- A2J training crops: the crop-level augmentation of the A2J trainers (csrc/a2j_traincrop.hip) ------------------------------
 * dataPreprocess + transform of third_party_methods/A2J_experiments/itop_train_64.py:208-295, train_a2j_base.py:236-317 and
 * train_a2j_bgaug_new.py:251-338 as ONE launch for n crops: the box region of a frame, (pasted into the zero image of the raw box,)
 * cv2.resize(INTER_NEAREST) to crop_w x crop_h, float32, (the ITOP depth window,) (v - mean) / std and, when `warp` is set,
 * cv2.warpAffine(INTER_LINEAR, constant border 0) of that NORMALISED crop onto crop_w x crop_h with the item's rotation and scale about
 * the crop centre -- bit for bit what numpy and OpenCV 4.2's scalar float32 paths give (agreement with a live cv2 build is unverified, as
 * for pn_augment_resize).  The shape of pn_augment_resize: one record per crop, every integer of the geometry and every scalar decided on
 * the host (popnet_amd/a2j_crops.py), the records checked here and uploaded in stream order; the kernel never re-derives a truncation.
 *   warp == 0   one source pixel per output pixel (augment=False: the reference does not call transform at all)
 *   warp == 1   the four warpAffine taps; each tap is one pixel of the normalised crop, a tap outside the crop reads 0 (NOT normalised
 *               zero depth); m is the INVERTED matrix as warpAffine holds it, the convention of pn_augment_item.m
 *   one tap     INTER_NEAREST index min(floor(d * (1 / (dsize / ssize))), ssize - 1) in double; padded: the paste loop's strict
 *               start < i < end test and its int(i - start) index, in float32; the frame's pixel as float32; window: v >= hi -> fill,
 *               then v <= lo -> fill, then (v - sub) * scale (a NaN fails both comparisons and stays NaN); (v - mean) / std
 * sh < 1 or sw < 1 is the empty image on which cv2.resize raises: the crop is zeros and flags_dev[row] (may be NULL) is 1, else 0.
 * mean / std / crop_w / crop_h come from cfg; its other fields are not read.  frames_dev [F, H, W] f16 / f32.  items_host holds the n
 * records; items_dev has room for n (the caller's buffer, nothing is allocated); out_dev [n, 1, crop_h, crop_w] f32.  No synchronisation;
 * items_host stays untouched until the stream has passed the call.  Refusals (PN_ERR_INVALID, the text names the item; nothing is copied
 * or launched): inconsistent geometry, a non-finite matrix or scalar, a matrix outside |m0|, |m1|, |m3|, |m4| <= 64 and |m2|, |m5| <= 2^19 (the
 * fixed-point products then fit an int for every crop size; a crop-centre rotation at scales from 1/64 up lies far inside), n > 65535, a crop side
 * over 4096, std == 0.  n == 0 is PN_OK.  */
typedef struct pn_a2j_crop_item {
    double m[6];                       /* warp: the inverted 2x3 matrix (destination pixel -> pixel of the normalised crop), row major   */
    int frame;                         /* index into frames_dev                                                                           */
    int cy0, cx0, ih, iw;              /* the clipped region depth[cy0 : cy0 + ih, cx0 : cx0 + iw] (Python's slice rules applied): inside
                                          the frame                                                                                       */
    int sh, sw;                        /* the image cv2.resize reads: ih x iw, or the padded image int(y1 - y0) x int(x1 - x0)            */
    int padded;                        /* 1: the region is pasted into the zero image sh x sw                                             */
    float start1, start2, end1, end2;  /* the paste loop's bounds (rows: 1, columns: 2), read when padded                                 */
    int window;                        /* 1: the ITOP depth window                                                                        */
    float hi, lo, fill, sub, scale;    /* centre depth +- depth_thres, the centre depth (twice), float32(RandomScale); read when window   */
    int warp;                          /* 1: transform() follows (augment=True)                                                           */
} pn_a2j_crop_item;
size_t pn_sizeof_a2j_crop_item(void);
int pn_a2j_train_crop(pn_ctx *ctx, const void *frames_dev, int depth_dtype, int F, int H, int W, const pn_a2j_crop_item *items_host,
                      pn_a2j_crop_item *items_dev, int n, const pn_a2j_cfg *cfg, float *out_dev, int32_t *flags_dev, void *hip_stream);

/* ---- legacy plug-in ABI: the SWIG module `pafprocess` -----------------------------------------
 * Same seven symbols, same argument meaning and the same (non re-entrant, global-state)
 * semantics as tpm/lib/pafprocess/pafprocess.h:53-59, COCO-18 topology (pafprocess.h:6-24).
 * Inputs are HOST float32 C-contiguous arrays, borrowed for the duration of the call:
 *   peaks [p1][p2][p3>=5] (x, y, score, -, part), heatmap [h1][h2][h3] (unused, as in the
 *   reference), pafmap [f1][f2][f3=38].
 * Differences: returns a negative pn_status instead of 0 when the GPU path fails; peaks that
 * would index outside the PAF map are rejected instead of read out of bounds
 * (pafprocess.cpp:232-233 has no bounds check).                                                 */
int process_paf(int p1, int p2, int p3, float *peaks, int h1, int h2, int h3, float *heatmap,
                int f1, int f2, int f3, float *pafmap);
int get_num_humans(void);
int get_part_cid(int human_id, int part_id);
float get_score(int human_id);
int get_part_x(int cid);
int get_part_y(int cid);
float get_part_score(int cid);

#ifdef __cplusplus
}
#endif
#endif /* POPNET_HIP_H */
