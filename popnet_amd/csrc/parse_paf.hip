// Open-Pose+ pose parsing on the GPU: heat-map NMS with bicubic sub-cell refinement, part-affinity
// limb scoring, greedy one-to-one matching, person assembly, depth read-out and back-projection.
//
// Replaces the reference's per-frame NumPy/SciPy/cv2 post-processing (Python loops on the host):
//   find_peaks / NMS              tpm/lib/utils/paf_to_pose.py:33-153
//   find_connected_joints         tpm/lib/utils/paf_to_pose.py:156-264
//   group_limbs_of_same_person    tpm/lib/utils/paf_to_pose.py:267-351
//   paf_to_human_list             tpm/lib/utils/common.py:5-32
//   retrieve_depth_heat_weighted  tpm/lib/utils/common.py:272-293
//   read-out / rescale / pinhole  tpm/evaluate/evaluation_rtpose_light3d_kdh3d_mpreal_ablation.py:179-262
//
// Three launches per batch, all HBM/L2-latency bound (185 KB of maps in, <30 KB of records out per
// frame); none materialises the reference's 224x224x28 up-sampled PAF tensor (5.6 MB/frame): the
// x8 bicubic value is evaluated at the ten sample points of each candidate limb only.
//   k1  one workgroup per (frame, joint map): peak flags -> ordered ballot compaction -> one wave
//       per peak up-samples its <=5x5 patch x8 (<=40x40) and wave-reduces the first arg-max
//       (parse_peaks.hip).
//   k2  one workgroup per (frame, limb): lanes = (candidate pair, sample point); stable rank sort;
//       greedy matching.
//   k3  one wave per frame: sequential person assembly with wave-parallel row search, pruning,
//       heat-weighted depth read-out, rescale and back-projection into fixed-size records.
//
// This file: the bounded batch path (fixed-size records, every list in LDS) and its entry points.  Every launch serves every supported
// (downsample, num_intermed_pts); the workload's own (8, 10) gets the literal instantiations.  The arithmetic contract and the steps shared
// with the unbounded second pass (parse_unbounded.hip) are parse_device.h.
#pragma clang fp contract(off)
#include "parse_device.h"

extern "C" void pn_debug_cubic_coeffs(float x, float *out4) { host_cubic_coeffs(x, out4); }

// ---------------------------------------------------------------------------------------------
// k2: limb scoring + greedy matching.  grid = (L, B), block = 256.  <3, 10>: 25 pairs x 10 sample points = 250 lanes busy per pass.
// ---------------------------------------------------------------------------------------------
template <int LF, int N>
__global__ __launch_bounds__(256) void limb_match_kernel(const float *__restrict__ paf, int h, int w, int paf_c, float thresh_paf, int up_h,
                                                          int lf_arg, int n_arg, CubicTab tab, ParseWs *__restrict__ ws) {
    __shared__ LimbLds<LF, N> S;
    __shared__ int s_ncand;
    __shared__ double s_cand_s[MAXP * MAXP];
    __shared__ unsigned char s_cand_i[MAXP * MAXP], s_cand_j[MAXP * MAXP];
    __shared__ unsigned short s_order[MAXP * MAXP];
    const int limb = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x;
    ParseWs &W = ws[b];
    const int jsrc = pn_limb_src(limb), jdst = pn_limb_dst(limb);
    const int ns = min(W.peak_count[jsrc], MAXP), nd = min(W.peak_count[jdst], MAXP);
    if (ns == 0 || nd == 0) {
        if (tid == 0) W.conn_count[limb] = 0;
        return;
    }
    const int nc = limb_score_pass(S, s_ncand, paf + ((size_t)b * paf_c + 2 * limb) * h * w, h, w, W.peak_x[jsrc], W.peak_y[jsrc], W.peak_x[jdst],
                                   W.peak_y[jdst], ns, nd, thresh_paf, up_h, lf_arg, n_arg, tab, [&](int pos, double score, int i, int j) {
                                       s_cand_s[pos] = score;
                                       s_cand_i[pos] = (unsigned char)i;
                                       s_cand_j[pos] = (unsigned char)j;
                                   });

    // stable descending sort by score (Python sorted(..., reverse=True) keeps insertion order on ties)
    for (int k = tid; k < nc; k += 256) {
        const double sk = s_cand_s[k];
        int rank = 0;
        for (int m = 0; m < nc; ++m) {
            const double sm = s_cand_s[m];
            rank += (sm > sk || (sm == sk && m < k)) ? 1 : 0;
        }
        s_order[rank] = (unsigned short)k;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long used_i = 0, used_j = 0;
        const int maxc = min(ns, nd);
        int n = 0;
        for (int r = 0; r < nc && n < maxc; ++r) {
            const int k = s_order[r];
            const int i = s_cand_i[k], j = s_cand_j[k];
            if (!((used_i >> i) & 1ull) && !((used_j >> j) & 1ull)) {
                used_i |= 1ull << i;
                used_j |= 1ull << j;
                W.conn_i[limb][n] = i;
                W.conn_j[limb][n] = j;
                W.conn_s[limb][n] = s_cand_s[k];
                ++n;
            }
        }
        W.conn_count[limb] = n;
    }
}

// ---------------------------------------------------------------------------------------------
// k3: person assembly + read-out.  grid = B, block = 64 (one wave).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void group_readout_kernel(const float *__restrict__ heat, const float *__restrict__ z,
                                                            int h, int w, int heat_c, int z_c, pn_parse_cfg cfg,
                                                            const ParseWs *__restrict__ ws, pn_pose_frame *__restrict__ frames,
                                                            pn_pose_wire *__restrict__ wire) {
    __shared__ double rows[PN_MAX_PERSONS][J_ + 2];
    __shared__ int s_base[J_ + 1];
    __shared__ __attribute__((aligned(16))) unsigned s_ws[(sizeof(ParseWs) + 7) / 8 * 2];
    __shared__ unsigned long long s_kbal;
    __shared__ int s_nkeep;
    // 256 threads: the scratch staging, the joint list and the read-out use all four waves; the serial person assembly
    // in between runs on wave 0 alone (the other waves wait at the block barrier behind it)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // The assembly below is a serial walk over connections: served from global memory every step was a
    // dependent ~1 us load (measured 25 us per launch).  Stage this frame's 13 KB of scratch in LDS once.
    {
        static_assert(sizeof(ParseWs) % 8 == 0, "staged in 8-byte pieces");
        // (round 5: every piece of the thread in flight at once -- the plain loop compiled to one load, one s_waitcnt vmcnt(0) per iteration: seven
        // dependent round trips in front of everything else the block does)
        const uint2 *src = reinterpret_cast<const uint2 *>(&ws[b]);
        constexpr int NW8 = (int)(sizeof(ParseWs) / 8), NIT = (NW8 + 255) / 256;
        uint2 stg[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) stg[it] = src[min(tid + 256 * it, NW8 - 1)];
#pragma unroll
        for (int it = 0; it < NIT; ++it)
            if (tid + 256 * it < NW8) reinterpret_cast<uint2 *>(s_ws)[tid + 256 * it] = stg[it];
        // rows beyond n_peaks / n_persons are never written below: the record starts as zeros, so that it is a pure function of its frame
        // (bit-identical wherever in a batch, and in whatever buffer, the frame was processed).  Round 4: zeroed HERE, by the block that owns
        // the record (the barrier below drains these stores -- vmcnt(0) -- before any thread writes a result), instead of by a 1 MB memset
        // launch in front of the three parse kernels.
        static_assert(sizeof(pn_pose_frame) % 16 == 0, "zeroed in 16-byte pieces");
        uint4 *fz = reinterpret_cast<uint4 *>(&frames[b]);
        for (int i = tid; i < (int)(sizeof(pn_pose_frame) / 16); i += 256) fz[i] = uint4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    const ParseWs &W = *reinterpret_cast<const ParseWs *>(s_ws);
    pn_pose_frame &F = frames[b];
    unsigned status = 0;

    if (tid == 0) {
        int acc = 0;
        for (int j = 0; j < J_; ++j) {
            s_base[j] = acc;
            acc += min(W.peak_count[j], MAXP);
        }
        s_base[J_] = acc;
    }
    for (int j = 0; j < J_; ++j)
        if (W.peak_count[j] > MAXP) status |= PN_FRAME_OVERFLOW_PEAKS;      // every thread: uniform
    __syncthreads();
    const int npeaks = s_base[J_];
    // joint_list rows (id == row index)
    for (int j = 0; j < J_; ++j) {
        const int n = min(W.peak_count[j], MAXP);
        for (int k = tid; k < n; k += 256) {
            const int id = s_base[j] + k;
            F.peak_x[id] = W.peak_x[j][k];
            F.peak_y[id] = W.peak_y[j][k];
            F.peak_score[id] = W.peak_s[j][k];
            F.peak_type[id] = j;
        }
    }

    // ---- group_limbs_of_same_person (paf_to_pose.py:280-335), wave-uniform control flow, wave 0 only ----
    int np = 0;
    if (wave == 0) {
    for (int limb = 0; limb < L_; ++limb) {
        const int st = pn_limb_src(limb), dt = pn_limb_dst(limb);
        const int nconn = W.conn_count[limb];
        for (int cidx = 0; cidx < nconn; ++cidx) {
            const int ci = W.conn_i[limb][cidx], cj = W.conn_j[limb][cidx];
            const double src_id = (double)(s_base[st] + ci), dst_id = (double)(s_base[dt] + cj);
            const double lscore = W.conn_s[limb][cidx];
            const double s_src = (double)W.peak_s[st][ci], s_dst = (double)W.peak_s[dt][cj];
            bool hit = false;
            if (lane < np) hit = (rows[lane][st] == src_id) || (rows[lane][dt] == dst_id);
            const unsigned long long bal = __ballot(hit);
            const int nh = __popcll(bal);
            if (nh == 1) {
                const int p = __ffsll((long long)bal) - 1;
                if (lane == 0 && rows[p][dt] != dst_id) {
                    rows[p][dt] = dst_id;
                    rows[p][J_ + 1] += 1.0;
                    rows[p][J_] += s_dst + lscore;
                }
            } else if (nh == 2) {
                const int p1 = __ffsll((long long)bal) - 1;
                const int p2 = __ffsll((long long)(bal & (bal - 1))) - 1;
                bool both = false;
                if (lane < J_) both = (rows[p1][lane] >= 0.0) && (rows[p2][lane] >= 0.0);
                const bool overlap = __ballot(both) != 0ull;
                if (!overlap) {
                    if (lane < J_) rows[p1][lane] += rows[p2][lane] + 1.0;
                    if (lane == 0) {
                        rows[p1][J_] += rows[p2][J_];
                        rows[p1][J_ + 1] += rows[p2][J_ + 1];
                        rows[p1][J_] += lscore;
                    }
                    WAVE_LDS_SYNC();
                    // person_to_joint_assoc.pop(p2): shift the later rows down by one
                    double tmp[J_ + 2];
                    const bool mv = lane >= p2 && lane < np - 1;
                    if (mv)
                        for (int k = 0; k < J_ + 2; ++k) tmp[k] = rows[lane + 1][k];
                    WAVE_LDS_SYNC();
                    if (mv)
                        for (int k = 0; k < J_ + 2; ++k) rows[lane][k] = tmp[k];
                    --np;
                } else if (lane == 0) {
                    rows[p1][dt] = dst_id;
                    rows[p1][J_ + 1] += 1.0;
                    rows[p1][J_] += s_dst + lscore;
                }
            } else {
                if (np < PN_MAX_PERSONS) {
                    if (lane < J_) rows[np][lane] = (lane == st) ? src_id : ((lane == dt) ? dst_id : -1.0);
                    if (lane == 0) {
                        rows[np][J_ + 1] = 2.0;
                        rows[np][J_] = (s_src + s_dst) + lscore;      // sum([a, b]) + c
                    }
                    ++np;
                } else {
                    status |= PN_FRAME_OVERFLOW_PERSONS;
                }
            }
            WAVE_LDS_SYNC();
        }
    }

    // ---- prune (paf_to_pose.py:338-346) + read-out ----
    bool keep = false;
    if (lane < np) {
        const double cnt = rows[lane][J_ + 1], sc = rows[lane][J_];
        keep = !(cnt < 3.0 || sc / cnt < 0.2);
    }
    const unsigned long long kbal0 = __ballot(keep);
    if (keep) {
        const unsigned long long kbal = kbal0;
        const int o = __popcll(kbal & ((1ull << lane) - 1ull));
        for (int j = 0; j < J_; ++j) F.person_joint[o][j] = (int)rows[lane][j];
        F.person_score[o] = rows[lane][J_];
        F.person_count[o] = (int)rows[lane][J_ + 1];
    }
    if (lane == 0) {
        F.n_persons = __popcll(kbal0);
        F.n_peaks = npeaks;
        F.status = status;
        F.reserved = 0;
        s_kbal = kbal0;
        s_nkeep = __popcll(kbal0);
    }
    }   // wave 0
    __syncthreads();
    const unsigned long long kbal = s_kbal;
    const int nkeep = s_nkeep;

    const int hw = h * w;
    const float *heat_b = heat + (size_t)b * heat_c * hw;
    const float *z_b = z + (size_t)b * z_c * hw;
    for (int t = tid; t < nkeep * J_; t += 256) {
        const int o = t / J_, j = t - o * J_;
        // o-th kept row -> source row index
        unsigned long long m = kbal;
        for (int k = 0; k < o; ++k) m &= m - 1;
        const int r = __ffsll((long long)m) - 1;
        const int id = (int)rows[r][j];
        const int k = id - s_base[j];
        const JointOut q = joint_readout(id >= 0, W.peak_x[j][max(k, 0)], W.peak_y[j][max(k, 0)], W.peak_s[j][max(k, 0)], heat_b, z_b, j, h, w, cfg);
        const double x2 = q.x2, y2 = q.y2, depth = q.depth, X3 = q.X3, Y3 = q.Y3, conf = q.conf;
        F.joints_2d[o][j][0] = x2;
        F.joints_2d[o][j][1] = y2;
        F.joints_3d[o][j][0] = X3;
        F.joints_3d[o][j][1] = Y3;
        F.joints_3d[o][j][2] = depth;
        F.part_conf[o][j] = conf;
        if (wire && o < PN_WIRE_MAX_PERSONS) {            // the compact record, in the same pass (what pn_pack_pose_frames derives from F)
            pn_pose_wire &Wr = wire[b];
            Wr.person_joint[o][j] = (int16_t)id;
            Wr.vals[o][j][0] = (float)x2; Wr.vals[o][j][1] = (float)y2;
            Wr.vals[o][j][2] = (float)X3; Wr.vals[o][j][3] = (float)Y3; Wr.vals[o][j][4] = (float)depth;
            Wr.vals[o][j][5] = (float)conf;
        }
    }
    if (wire) {
        pn_pose_wire &Wr = wire[b];
        if (tid == 0) {
            Wr.n_persons = nkeep;
            Wr.status = status | (nkeep > PN_WIRE_MAX_PERSONS ? PN_FRAME_OVERFLOW_PERSONS : 0u);
        }
        for (int t = tid; t < PN_WIRE_MAX_PERSONS * J_; t += 256) {      // rows beyond the last person: the same filler pack_pose_kernel writes
            const int o = t / J_, j = t - o * J_;
            if (o < nkeep) continue;
            Wr.person_joint[o][j] = (int16_t)-1;
#pragma unroll
            for (int k = 0; k < 6; ++k) Wr.vals[o][j][k] = 0.f;
        }
    }
}

// k2's launch: the literal instantiation for the workload's own (x8, ten points), the run-time one for anything else
static void launch_limbs(hipStream_t s, const float *paf_dev, int B, int h, int w, float thresh_paf, int f, int npts, ParseWs *ws) {
    auto *kern = (f == 8 && npts == 10) ? limb_match_kernel<3, 10> : limb_match_kernel<LF_ARG, N_ARG>;
    hipLaunchKernelGGL(kern, dim3(L_, B), dim3(256), 0, s, paf_dev, h, w, 2 * L_, thresh_paf, h * f, pn_parse_factor_log2(f), npts, pn_cubic_tab(f), ws);
}

extern "C" int pn_parse_paf(pn_ctx *ctx, const float *heat_dev, const float *paf_dev, const float *z_dev, int B, int h,
                            int w, const pn_parse_cfg *cfg, pn_pose_frame *frames_dev, void *hip_stream) {
    return pn_parse_paf_wire(ctx, heat_dev, paf_dev, z_dev, B, h, w, cfg, frames_dev, nullptr, hip_stream);
}

extern "C" int pn_parse_paf_wire(pn_ctx *ctx, const float *heat_dev, const float *paf_dev, const float *z_dev, int B, int h,
                                 int w, const pn_parse_cfg *cfg, pn_pose_frame *frames_dev, pn_pose_wire *wire_dev, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (!heat_dev || !paf_dev || !z_dev || !cfg || !frames_dev || B < 1)
        return pn_set_error(ctx, PN_ERR_INVALID, "pn_parse_paf: bad arguments");
    if (int rc = pn_parse_check_map(ctx, "pn_parse_paf", h, w)) return rc;
    if (int rc = pn_parse_check_cfg(ctx, "pn_parse_paf", cfg)) return rc;
    const size_t need = (size_t)B * sizeof(ParseWs);
    if (ctx->parse_ws_bytes < need) {
        // never move the scratch under a graph: not while this stream is capturing, not once its size was fixed
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hip_stream && hipStreamIsCapturing((hipStream_t)hip_stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
            return pn_set_error(ctx, PN_ERR_STATE, "pn_parse_paf: batch %d needs a larger parse scratch while the stream is being captured (call pn_parse_reserve first)", B);
        if (ctx->parse_ws_fixed)
            return pn_set_error(ctx, PN_ERR_STATE, "pn_parse_paf: batch %d exceeds the batch size given to pn_parse_reserve", B);
        if (ctx->parse_ws) (void)hipFree(ctx->parse_ws);
        ctx->parse_ws = nullptr;
        ctx->parse_ws_bytes = 0;
        PN_HIP_CHECK(ctx, hipMalloc(&ctx->parse_ws, need));
        ctx->parse_ws_bytes = need;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    ParseWs *ws = (ParseWs *)ctx->parse_ws;
    const PnPeakOut po = {ws->peak_count, &ws->peak_x[0][0], &ws->peak_y[0][0], &ws->peak_s[0][0], MAXP, sizeof(ParseWs)};
    if (int rc = pn_launch_peaks(ctx, s, heat_dev, J_, B, h, w, J_ + 1, cfg->thresh_heatmap, cfg->downsample, 1, 0, po)) return rc;
    launch_limbs(s, paf_dev, B, h, w, cfg->thresh_paf, cfg->downsample, cfg->num_intermed_pts, ws);
    // (rows beyond n_peaks / n_persons read as zero: group_readout_kernel zeroes its own record first)
    hipLaunchKernelGGL(group_readout_kernel, dim3(B), dim3(256), 0, s, heat_dev, z_dev, h, w, J_ + 1, L_ + 1, *cfg,
                       (const ParseWs *)ws, frames_dev, wire_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    ctx->parse_last_b = B;
    return PN_OK;
}

// Read-only view of the connection lists the last pn_parse_paf / pn_parse_paf_wire left in the context's scratch (tests compare them with
// find_connected_joints).  Host side, blocking; nothing on the launch path knows about it.
extern "C" int pn_parse_debug_connections(pn_ctx *ctx, int frame, int *count, int *conn_i, int *conn_j, double *conn_s) {
    if (!ctx) return PN_ERR_INVALID;
    if (!count || !conn_i || !conn_j || !conn_s) return pn_set_error(ctx, PN_ERR_INVALID, "pn_parse_debug_connections: bad arguments");
    if (!ctx->parse_ws || ctx->parse_last_b < 1) return pn_set_error(ctx, PN_ERR_STATE, "pn_parse_debug_connections: no parse has run on this context");
    if (frame < 0 || frame >= ctx->parse_last_b)
        return pn_set_error(ctx, PN_ERR_STATE, "pn_parse_debug_connections: frame %d outside the last batch of %d", frame, ctx->parse_last_b);
    PN_HIP_CHECK(ctx, hipDeviceSynchronize());
    const ParseWs *W = (const ParseWs *)ctx->parse_ws + frame;
    PN_HIP_CHECK(ctx, hipMemcpy(count, W->conn_count, sizeof W->conn_count, hipMemcpyDeviceToHost));
    PN_HIP_CHECK(ctx, hipMemcpy(conn_i, W->conn_i, sizeof W->conn_i, hipMemcpyDeviceToHost));
    PN_HIP_CHECK(ctx, hipMemcpy(conn_j, W->conn_j, sizeof W->conn_j, hipMemcpyDeviceToHost));
    PN_HIP_CHECK(ctx, hipMemcpy(conn_s, W->conn_s, sizeof W->conn_s, hipMemcpyDeviceToHost));
    return PN_OK;
}

extern "C" int pn_parse_reserve(pn_ctx *ctx, int max_batch) {
    if (!ctx) return PN_ERR_INVALID;
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (max_batch < 1) return pn_set_error(ctx, PN_ERR_INVALID, "pn_parse_reserve: max_batch must be >= 1");
    const size_t need = (size_t)max_batch * sizeof(ParseWs);
    if (ctx->parse_ws_bytes < need) {
        // an explicit reserve may grow the scratch (engines of different batch sizes share the per-device context); it is
        // the caller's contract that no hipGraph captured on THIS context is still alive then -- graph-captured engines
        // own private contexts (pipeline.StreamingEngine)
        if (ctx->parse_ws) (void)hipFree(ctx->parse_ws);
        ctx->parse_ws = nullptr;
        ctx->parse_ws_bytes = 0;
        PN_HIP_CHECK(ctx, hipMalloc(&ctx->parse_ws, need));
        ctx->parse_ws_bytes = need;
    }
    ctx->parse_ws_fixed = true;
    return PN_OK;
}

