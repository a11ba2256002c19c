// Unbounded path: the same algorithm WITHOUT the record capacities (the reference has none: paf_to_pose.py:33-153,267-351).
// One frame per call, every list in a global-memory workspace sized from the frame's own counts (up to h*w peaks per joint
// map, min(ns, nd) connections per limb, one person per connection), results fetched as variable-length arrays.  It is the
// second pass for a frame the fixed-size records flag as overflowing (PN_FRAME_OVERFLOW_*): slower (lists in L2 instead of
// LDS, the greedy matching as repeated arg-max instead of a rank sort) but the same arithmetic in the same order, so a frame
// that fits the records gives the same values through either path (tests/test_gpu_parity.py): the scoring pass, the read-out and the
// NMS kernels are the bounded path's own (parse_device.h, parse_peaks.hip).  Also here: pn_nms_peaks*, the same NMS stand-alone.
#pragma clang fp contract(off)
#include <algorithm>
#include "parse_device.h"

// limb scoring + greedy matching without capacities.  grid = L, block = 256.
template <int LF, int N>
__global__ __launch_bounds__(256) void limb_unbounded_kernel(const float *__restrict__ paf, int h, int w, float thresh_paf, int up_h, int lf_arg,
                                                              int n_arg, CubicTab tab, BigWs W) {
    __shared__ LimbLds<LF, N> S;
    __shared__ int s_ncand;
    __shared__ unsigned s_used_i[MAX_MAP / 32], s_used_j[MAX_MAP / 32];
    __shared__ double s_best_s[256];
    __shared__ int s_best_k[256];
    const int limb = blockIdx.x, tid = threadIdx.x;
    const int jsrc = pn_limb_src(limb), jdst = pn_limb_dst(limb);
    const int ns = W.peak_count[jsrc], nd = W.peak_count[jdst];
    if (ns == 0 || nd == 0) {
        if (tid == 0) W.conn_count[limb] = 0;
        return;
    }
    const int hw = h * w;
    double *cs = W.cand_s + W.cand_off[limb];
    unsigned short *ci = W.cand_i + W.cand_off[limb], *cj = W.cand_j + W.cand_off[limb];
    for (int i = tid; i < MAX_MAP / 32; i += 256) { s_used_i[i] = 0u; s_used_j[i] = 0u; }
    const int nc = limb_score_pass(S, s_ncand, paf + (size_t)(2 * limb) * hw, h, w, W.px + (size_t)jsrc * hw, W.py + (size_t)jsrc * hw, W.px + (size_t)jdst * hw,
                                   W.py + (size_t)jdst * hw, ns, nd, thresh_paf, up_h, lf_arg, n_arg, tab, [&](int pos, double score, int i, int j) {
                                       cs[pos] = score;
                                       ci[pos] = (unsigned short)i;
                                       cj[pos] = (unsigned short)j;
                                   });
    __threadfence_block();
    // greedy matching = walk the candidates in stable descending score order and take every pair whose two peaks are both
    // free (paf_to_pose.py:246-262): equivalently, repeatedly take the best (score desc, insertion order asc) candidate
    // among those whose peaks are both still free
    const int maxc = min(ns, nd);
    int n = 0;
    while (n < maxc) {
        double bs = -INFINITY;
        int bk = 0x7fffffff;
        for (int k = tid; k < nc; k += 256) {
            const int i = ci[k], j = cj[k];
            if (((s_used_i[i >> 5] >> (i & 31)) & 1u) || ((s_used_j[j >> 5] >> (j & 31)) & 1u)) continue;
            const double sk = cs[k];
            if (sk > bs || (sk == bs && k < bk) || bk == 0x7fffffff) { bs = sk; bk = k; }
        }
        s_best_s[tid] = bs;
        s_best_k[tid] = bk;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (tid < off) {
                const double os = s_best_s[tid + off];
                const int ok_ = s_best_k[tid + off];
                const double ms = s_best_s[tid];
                const int mk = s_best_k[tid];
                if (ok_ != 0x7fffffff && (mk == 0x7fffffff || os > ms || (os == ms && ok_ < mk))) { s_best_s[tid] = os; s_best_k[tid] = ok_; }
            }
            __syncthreads();
        }
        const int k = s_best_k[0];
        if (k == 0x7fffffff) break;                       // no free candidate left (block-uniform)
        if (tid == 0) {
            const int i = ci[k], j = cj[k];
            s_used_i[i >> 5] |= 1u << (i & 31);
            s_used_j[j >> 5] |= 1u << (j & 31);
            W.conn_i[(size_t)limb * hw + n] = i;
            W.conn_j[(size_t)limb * hw + n] = j;
            W.conn_s[(size_t)limb * hw + n] = s_best_s[0];
        }
        ++n;
        __syncthreads();
    }
    if (tid == 0) W.conn_count[limb] = n;
}

// person assembly + read-out without capacities: rows in global memory, row search by block atomics.  grid = 1, block = 256.
__global__ __launch_bounds__(256) void big_group_kernel(const float *__restrict__ heat, const float *__restrict__ z, int h, int w, pn_parse_cfg cfg, BigWs W) {
    __shared__ int s_base[J_ + 1];
    __shared__ int s_nh, s_h1, s_h2, s_overlap, s_np, s_nkeep;
    const int tid = threadIdx.x;
    const int hw = h * w;
    constexpr int RW = J_ + 2;
    if (tid == 0) {
        int acc = 0;
        for (int j = 0; j < J_; ++j) { s_base[j] = acc; acc += W.peak_count[j]; }
        s_base[J_] = acc;
        s_np = 0;
    }
    __syncthreads();
    const int npeaks = s_base[J_];
    for (int j = 0; j < J_; ++j) {
        const int n = W.peak_count[j];
        for (int k = tid; k < n; k += 256) {
            const int id = s_base[j] + k;
            W.o_peak[3 * (size_t)id + 0] = W.px[(size_t)j * hw + k];
            W.o_peak[3 * (size_t)id + 1] = W.py[(size_t)j * hw + k];
            W.o_peak[3 * (size_t)id + 2] = W.ps[(size_t)j * hw + k];
            W.o_peak_type[id] = j;
        }
    }
    double *rows = W.rows;
    // ---- group_limbs_of_same_person (paf_to_pose.py:280-335): serial over connections, row search across the block ----
    for (int limb = 0; limb < L_; ++limb) {
        const int st = pn_limb_src(limb), dt = pn_limb_dst(limb);
        const int nconn = W.conn_count[limb];
        for (int cidx = 0; cidx < nconn; ++cidx) {
            const int ci = W.conn_i[(size_t)limb * hw + cidx], cj = W.conn_j[(size_t)limb * hw + cidx];
            const double src_id = (double)(s_base[st] + ci), dst_id = (double)(s_base[dt] + cj);
            const double lscore = W.conn_s[(size_t)limb * hw + cidx];
            const double s_src = (double)W.ps[(size_t)st * hw + ci], s_dst = (double)W.ps[(size_t)dt * hw + cj];
            const int np = s_np;
            if (tid == 0) { s_nh = 0; s_h1 = 0x7fffffff; s_h2 = 0x7fffffff; s_overlap = 0; }
            __syncthreads();
            for (int r = tid; r < np; r += 256)
                if (rows[(size_t)r * RW + st] == src_id || rows[(size_t)r * RW + dt] == dst_id) { atomicAdd(&s_nh, 1); atomicMin(&s_h1, r); }
            __syncthreads();
            const int nh = s_nh, p1 = s_h1;
            if (nh == 2) {
                for (int r = tid; r < np; r += 256)
                    if (r != p1 && (rows[(size_t)r * RW + st] == src_id || rows[(size_t)r * RW + dt] == dst_id)) atomicMin(&s_h2, r);
                __syncthreads();
                const int p2 = s_h2;
                if (tid < J_ && rows[(size_t)p1 * RW + tid] >= 0.0 && rows[(size_t)p2 * RW + tid] >= 0.0) atomicOr(&s_overlap, 1);
                __syncthreads();
                if (!s_overlap) {
                    if (tid < J_) rows[(size_t)p1 * RW + tid] += rows[(size_t)p2 * RW + tid] + 1.0;
                    if (tid == 0) {
                        rows[(size_t)p1 * RW + J_] += rows[(size_t)p2 * RW + J_];
                        rows[(size_t)p1 * RW + J_ + 1] += rows[(size_t)p2 * RW + J_ + 1];
                        rows[(size_t)p1 * RW + J_] += lscore;
                    }
                    __syncthreads();
                    // person_to_joint_assoc.pop(p2): the later rows move down by one (through the second buffer)
                    for (long long e = (long long)p2 * RW + tid; e < (long long)(np - 1) * RW; e += 256) W.rows2[e] = rows[e + RW];
                    __threadfence_block();
                    __syncthreads();
                    for (long long e = (long long)p2 * RW + tid; e < (long long)(np - 1) * RW; e += 256) rows[e] = W.rows2[e];
                    if (tid == 0) s_np = np - 1;
                } else if (tid == 0) {
                    rows[(size_t)p1 * RW + dt] = dst_id;
                    rows[(size_t)p1 * RW + J_ + 1] += 1.0;
                    rows[(size_t)p1 * RW + J_] += s_dst + lscore;
                }
            } else if (nh == 1) {
                if (tid == 0 && rows[(size_t)p1 * RW + dt] != dst_id) {
                    rows[(size_t)p1 * RW + dt] = dst_id;
                    rows[(size_t)p1 * RW + J_ + 1] += 1.0;
                    rows[(size_t)p1 * RW + J_] += s_dst + lscore;
                }
            } else {
                if (tid < J_) rows[(size_t)np * RW + tid] = (tid == st) ? src_id : ((tid == dt) ? dst_id : -1.0);
                if (tid == 0) {
                    rows[(size_t)np * RW + J_ + 1] = 2.0;
                    rows[(size_t)np * RW + J_] = (s_src + s_dst) + lscore;
                    s_np = np + 1;
                }
            }
            __threadfence_block();
            __syncthreads();
        }
    }
    // ---- prune (paf_to_pose.py:338-346), order kept ----
    if (tid == 0) {
        int nk = 0;
        for (int r = 0; r < s_np; ++r) {
            const double cnt = rows[(size_t)r * RW + J_ + 1], sc = rows[(size_t)r * RW + J_];
            if (!(cnt < 3.0 || sc / cnt < 0.2)) W.keep_idx[nk++] = r;
        }
        s_nkeep = nk;
        W.counts[0] = npeaks;
        W.counts[1] = nk;
    }
    __threadfence_block();
    __syncthreads();
    const int nkeep = s_nkeep;
    for (int t = tid; t < nkeep * J_; t += 256) {
        const int o = t / J_, j = t - o * J_;
        const int r = W.keep_idx[o];
        const int id = (int)rows[(size_t)r * RW + j];
        W.o_person_joint[(size_t)o * J_ + j] = id;
        if (j == 0) {
            W.o_person_score[o] = rows[(size_t)r * RW + J_];
            W.o_person_count[o] = (int)rows[(size_t)r * RW + J_ + 1];
        }
        const size_t k = (size_t)j * hw + max(id - s_base[j], 0);
        const JointOut q = joint_readout(id >= 0, W.px[k], W.py[k], W.ps[k], heat, z, j, h, w, cfg);
        const double x2 = q.x2, y2 = q.y2, depth = q.depth, X3 = q.X3, Y3 = q.Y3, conf = q.conf;
        W.o_j2d[2 * (size_t)t + 0] = x2;
        W.o_j2d[2 * (size_t)t + 1] = y2;
        W.o_j3d[3 * (size_t)t + 0] = X3;
        W.o_j3d[3 * (size_t)t + 1] = Y3;
        W.o_j3d[3 * (size_t)t + 2] = depth;
        W.o_conf[t] = conf;
    }
}

namespace {
struct BigHost { BigWs w; size_t bytes_a = 0, bytes_b = 0; void *blk_a = nullptr, *blk_b = nullptr; int hw = 0, npeaks = 0, npersons = 0; };
char *bump(char *&p, size_t bytes) { char *r = p; p += (bytes + 255) & ~(size_t)255; return r; }
}  // namespace

extern "C" int pn_parse_paf_unbounded(pn_ctx *ctx, const float *heat_dev, const float *paf_dev, const float *z_dev, int h, int w,
                                      const pn_parse_cfg *cfg, int *n_peaks, int *n_persons, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (!heat_dev || !paf_dev || !z_dev || !cfg || !n_peaks || !n_persons) return pn_set_error(ctx, PN_ERR_INVALID, "pn_parse_paf_unbounded: bad arguments");
    if (int rc = pn_parse_check_map(ctx, "pn_parse_paf_unbounded", h, w)) return rc;
    if (int rc = pn_parse_check_cfg(ctx, "pn_parse_paf_unbounded", cfg)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    BigHost *B = (BigHost *)ctx->parse_big;
    if (!B) { B = new BigHost(); ctx->parse_big = B; }
    const int hw = h * w;
    // block A: everything whose size depends on the map only
    {
        const size_t need = 256 * 8 + (size_t)J_ * hw * 12 + (size_t)L_ * hw * 16 + 4096;
        if (B->bytes_a < need) {
            if (B->blk_a) { PN_HIP_CHECK(ctx, hipDeviceSynchronize()); (void)hipFree(B->blk_a); B->blk_a = nullptr; B->bytes_a = 0; }
            PN_HIP_CHECK(ctx, hipMalloc(&B->blk_a, need));
            B->bytes_a = need;
        }
        char *p = (char *)B->blk_a;
        B->w.peak_count = (int *)bump(p, J_ * 4);
        B->w.conn_count = (int *)bump(p, L_ * 4);
        B->w.counts = (int *)bump(p, 2 * 4);
        B->w.px = (float *)bump(p, (size_t)J_ * hw * 4);
        B->w.py = (float *)bump(p, (size_t)J_ * hw * 4);
        B->w.ps = (float *)bump(p, (size_t)J_ * hw * 4);
        B->w.conn_i = (int *)bump(p, (size_t)L_ * hw * 4);
        B->w.conn_j = (int *)bump(p, (size_t)L_ * hw * 4);
        B->w.conn_s = (double *)bump(p, (size_t)L_ * hw * 8);
    }
    B->hw = hw;
    const PnPeakOut po = {B->w.peak_count, B->w.px, B->w.py, B->w.ps, hw, 0};
    if (int rc = pn_launch_peaks(ctx, s, heat_dev, J_, 1, h, w, J_, cfg->thresh_heatmap, cfg->downsample, 1, 0, po)) return rc;
    int pc[J_];
    PN_HIP_CHECK(ctx, hipMemcpyAsync(pc, B->w.peak_count, sizeof pc, hipMemcpyDeviceToHost, s));
    PN_HIP_CHECK(ctx, hipStreamSynchronize(s));
    // block B: sized from this frame's peak counts
    long long ncand = 0, maxp = 1, npk = 0;
    for (int j = 0; j < J_; ++j) npk += pc[j];
    for (int l = 0; l < L_; ++l) {
        B->w.cand_off[l] = ncand;
        ncand += (long long)pc[pn_limb_src(l)] * pc[pn_limb_dst(l)];
        maxp += std::min(pc[pn_limb_src(l)], pc[pn_limb_dst(l)]);
    }
    B->w.cand_off[L_] = ncand;
    B->w.maxp = (int)maxp;
    {
        const size_t need = (size_t)ncand * 12 + (size_t)maxp * ((J_ + 2) * 16 + 4 + J_ * 4 + 8 + 4 + J_ * (16 + 24 + 8)) + (size_t)npk * 16 + 16 * 256;
        if (B->bytes_b < need) {
            if (B->blk_b) { PN_HIP_CHECK(ctx, hipDeviceSynchronize()); (void)hipFree(B->blk_b); B->blk_b = nullptr; B->bytes_b = 0; }
            PN_HIP_CHECK(ctx, hipMalloc(&B->blk_b, need + need / 4));
            B->bytes_b = need + need / 4;
        }
        char *p = (char *)B->blk_b;
        B->w.cand_s = (double *)bump(p, (size_t)ncand * 8);
        B->w.cand_i = (unsigned short *)bump(p, (size_t)ncand * 2);
        B->w.cand_j = (unsigned short *)bump(p, (size_t)ncand * 2);
        B->w.rows = (double *)bump(p, (size_t)maxp * (J_ + 2) * 8);
        B->w.rows2 = (double *)bump(p, (size_t)maxp * (J_ + 2) * 8);
        B->w.keep_idx = (int *)bump(p, (size_t)maxp * 4);
        B->w.o_peak = (float *)bump(p, (size_t)npk * 12);
        B->w.o_peak_type = (int *)bump(p, (size_t)npk * 4);
        B->w.o_person_joint = (int *)bump(p, (size_t)maxp * J_ * 4);
        B->w.o_person_score = (double *)bump(p, (size_t)maxp * 8);
        B->w.o_person_count = (int *)bump(p, (size_t)maxp * 4);
        B->w.o_j2d = (double *)bump(p, (size_t)maxp * J_ * 16);
        B->w.o_j3d = (double *)bump(p, (size_t)maxp * J_ * 24);
        B->w.o_conf = (double *)bump(p, (size_t)maxp * J_ * 8);
    }
    {   // the literal instantiation for the workload's own (x8, ten points), the run-time one for anything else
        const int f = cfg->downsample, npts = cfg->num_intermed_pts;
        auto *kern = (f == 8 && npts == 10) ? limb_unbounded_kernel<3, 10> : limb_unbounded_kernel<LF_ARG, N_ARG>;
        hipLaunchKernelGGL(kern, dim3(L_), dim3(256), 0, s, paf_dev, h, w, cfg->thresh_paf, h * f, pn_parse_factor_log2(f), npts, pn_cubic_tab(f), B->w);
    }
    hipLaunchKernelGGL(big_group_kernel, dim3(1), dim3(256), 0, s, heat_dev, z_dev, h, w, *cfg, B->w);
    int cnt[2] = {0, 0};
    PN_HIP_CHECK(ctx, hipMemcpyAsync(cnt, B->w.counts, sizeof cnt, hipMemcpyDeviceToHost, s));
    PN_HIP_CHECK(ctx, hipStreamSynchronize(s));
    PN_HIP_CHECK(ctx, hipGetLastError());
    B->npeaks = cnt[0];
    B->npersons = cnt[1];
    *n_peaks = cnt[0];
    *n_persons = cnt[1];
    return PN_OK;
}

extern "C" int pn_parse_paf_unbounded_fetch(pn_ctx *ctx, float *peaks_xys, int *peak_type, int *person_joint, double *person_score,
                                            int *person_count, double *joints_2d, double *joints_3d, double *part_conf) {
    if (!ctx) return PN_ERR_INVALID;
    BigHost *B = (BigHost *)ctx->parse_big;
    if (!B || !B->blk_b) return pn_set_error(ctx, PN_ERR_STATE, "pn_parse_paf_unbounded_fetch: no result (call pn_parse_paf_unbounded first)");
    const size_t np = (size_t)B->npeaks, P = (size_t)B->npersons;
    if (np && peaks_xys) PN_HIP_CHECK(ctx, hipMemcpy(peaks_xys, B->w.o_peak, np * 12, hipMemcpyDeviceToHost));
    if (np && peak_type) PN_HIP_CHECK(ctx, hipMemcpy(peak_type, B->w.o_peak_type, np * 4, hipMemcpyDeviceToHost));
    if (P && person_joint) PN_HIP_CHECK(ctx, hipMemcpy(person_joint, B->w.o_person_joint, P * J_ * 4, hipMemcpyDeviceToHost));
    if (P && person_score) PN_HIP_CHECK(ctx, hipMemcpy(person_score, B->w.o_person_score, P * 8, hipMemcpyDeviceToHost));
    if (P && person_count) PN_HIP_CHECK(ctx, hipMemcpy(person_count, B->w.o_person_count, P * 4, hipMemcpyDeviceToHost));
    if (P && joints_2d) PN_HIP_CHECK(ctx, hipMemcpy(joints_2d, B->w.o_j2d, P * J_ * 16, hipMemcpyDeviceToHost));
    if (P && joints_3d) PN_HIP_CHECK(ctx, hipMemcpy(joints_3d, B->w.o_j3d, P * J_ * 24, hipMemcpyDeviceToHost));
    if (P && part_conf) PN_HIP_CHECK(ctx, hipMemcpy(part_conf, B->w.o_conf, P * J_ * 8, hipMemcpyDeviceToHost));
    return PN_OK;
}

// Read-only view of the connection lists of the last pn_parse_paf_unbounded on this context: limb l's count[l] connections at [l][0 .. count[l]) of
// arrays [L][cap].  A limb connects distinct peaks of two joint types, so cap = the n_peaks that call returned always suffices.
extern "C" int pn_parse_paf_unbounded_connections(pn_ctx *ctx, int cap, int *count, int *conn_i, int *conn_j, double *conn_s) {
    if (!ctx) return PN_ERR_INVALID;
    if (!count || !conn_i || !conn_j || !conn_s || cap < 0) return pn_set_error(ctx, PN_ERR_INVALID, "pn_parse_paf_unbounded_connections: bad arguments");
    BigHost *B = (BigHost *)ctx->parse_big;
    if (!B || !B->blk_b) return pn_set_error(ctx, PN_ERR_STATE, "pn_parse_paf_unbounded_connections: no result (call pn_parse_paf_unbounded first)");
    PN_HIP_CHECK(ctx, hipDeviceSynchronize());
    PN_HIP_CHECK(ctx, hipMemcpy(count, B->w.conn_count, L_ * sizeof(int), hipMemcpyDeviceToHost));
    for (int l = 0; l < L_; ++l) {
        const size_t n = (size_t)count[l];
        if (n > (size_t)cap || n > (size_t)B->hw) return pn_set_error(ctx, PN_ERR_INVALID, "pn_parse_paf_unbounded_connections: limb %d has %d connections, cap is %d", l, count[l], cap);
        if (!n) continue;
        PN_HIP_CHECK(ctx, hipMemcpy(conn_i + (size_t)l * cap, B->w.conn_i + (size_t)l * B->hw, n * sizeof(int), hipMemcpyDeviceToHost));
        PN_HIP_CHECK(ctx, hipMemcpy(conn_j + (size_t)l * cap, B->w.conn_j + (size_t)l * B->hw, n * sizeof(int), hipMemcpyDeviceToHost));
        PN_HIP_CHECK(ctx, hipMemcpy(conn_s + (size_t)l * cap, B->w.conn_s + (size_t)l * B->hw, n * sizeof(double), hipMemcpyDeviceToHost));
    }
    return PN_OK;
}

// Stand-alone NMS (tpm/lib/utils/paf_to_pose.py:75-153 with bool_refine_center=True, no Gaussian filter) on ANY number of maps of one
// frame: what `paf_to_pose_cpp` (paf_to_pose.py:381-385) runs before it hands the peaks to `process_paf` -- there with the 18 COCO parts, a
// topology the three fixed-size parse kernels (15 joints / 14 limbs) do not serve.  Same kernel as the unbounded second pass: no capacity, peaks
// of map m at [m][0 .. count[m]) in row-major cell order (= the reference's ids), refined x / y in up-sampled pixels and the bicubic score.
extern "C" void pn_nms_opt_default(pn_nms_opt *opt) {
    if (!opt) return;
    opt->upsample = 8;
    opt->refine_center = 1;
    opt->gaussian_filt = 0;
}

// pn_nms_peaks with the reference's other arguments (paf_to_pose.py:75): any supported up-sampling factor, bool_refine_center off (the cell centre
// and the map's own value), bool_gaussian_filt on (scipy's gaussian_filter(sigma=3) of the up-sampled patch in front of the arg-max).  Which
// kernel serves which options is pn_launch_peaks' choice (parse_peaks.hip).
extern "C" int pn_nms_peaks_opt(pn_ctx *ctx, const float *heat_dev, int n_maps, int h, int w, float thresh, const pn_nms_opt *opt, int *count_dev,
                                float *peak_x_dev, float *peak_y_dev, float *peak_score_dev, void *hip_stream) {
    if (!ctx) return PN_ERR_INVALID;
    if (ctx->device < 0) return pn_set_error(ctx, PN_ERR_STATE, "context has no device");
    if (!heat_dev || !opt || !count_dev || !peak_x_dev || !peak_y_dev || !peak_score_dev || n_maps < 1) return pn_set_error(ctx, PN_ERR_INVALID, "pn_nms_peaks: bad arguments");
    if (int rc = pn_parse_check_map(ctx, "pn_nms_peaks", h, w)) return rc;
    if (pn_parse_factor_log2(opt->upsample) < 0)
        return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "pn_nms_peaks: upsampFactor %d: supported are " PN_PARSE_FACTORS_TEXT, opt->upsample);
    const PnPeakOut po = {count_dev, peak_x_dev, peak_y_dev, peak_score_dev, h * w, 0};
    if (int rc = pn_launch_peaks(ctx, (hipStream_t)hip_stream, heat_dev, n_maps, 1, h, w, n_maps, thresh, opt->upsample, opt->refine_center, opt->gaussian_filt, po)) return rc;
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

extern "C" int pn_nms_peaks(pn_ctx *ctx, const float *heat_dev, int n_maps, int h, int w, float thresh, int upsample, int *count_dev,
                            float *peak_x_dev, float *peak_y_dev, float *peak_score_dev, void *hip_stream) {
    pn_nms_opt opt;
    pn_nms_opt_default(&opt);
    opt.upsample = upsample;
    return pn_nms_peaks_opt(ctx, heat_dev, n_maps, h, w, thresh, &opt, count_dev, peak_x_dev, peak_y_dev, peak_score_dev, hip_stream);
}

void pn_parse_big_free(pn_ctx *ctx) {
    BigHost *B = (BigHost *)ctx->parse_big;
    if (!B) return;
    if (B->blk_a) (void)hipFree(B->blk_a);
    if (B->blk_b) (void)hipFree(B->blk_b);
    delete B;
    ctx->parse_big = nullptr;
}

