// The arithmetic of the pose parse, every step defined once for the three kernel families: the bounded batch path (parse_paf.hip), the unbounded
// second pass (parse_unbounded.hip) and the kernels for any supported up-sampling factor / sample count / NMS option (the <-1, 0> instantiations
// and parse_peaks.hip::gen_peaks_kernel).
//
// Arithmetic contract (bit-exact against oracle/parse_paf.py and, for the non-default arguments, the reference's own NMS / paf_to_pose under the
// cv2.resize restatement): float32 for everything the reference computes from float32 maps (bicubic taps in OpenCV's order: horizontal pass then
// vertical pass, products summed left to right), float64 for what NumPy promotes to float64 (sample coordinates, dot products, means, person scores,
// rescale, back-projection), NumPy's pairwise summation order for np.mean / np.sum, round-half-even for np.round, and no fused multiply-add anywhere
// in a file that includes this one.
//
//   up-sampling by f   destination d has t = 2d + 1 - f: first tap floor(t / 2f) - 1, fraction (t mod 2f) / 2f -- phase p = (t mod 2f) >> 1
//                      has fraction (2p + 1) / 2f for even f; f = 1 has the one fraction 0 (taps 0, 1, 0, 0).  Exact in float32 for powers
//                      of two, which is why other factors are refused.
//
// Template arguments LF (log2 f) and N (sample points per limb): a value >= 0 / > 0 is a literal, LF_ARG / N_ARG means "taken from the kernel
// arguments".  The default path instantiates <3, 10>; at those literals every helper folds to the expression the x8 / ten-point kernels spelled out.
#pragma once
#pragma clang fp contract(off)
#include <cmath>
#include "parse_ws.h"

constexpr int LF_ARG = -1, N_ARG = 0;

// ---- cubic coefficients ----
struct CubicTab { float c[16][4]; };   // phase p of an up-sampling by f: fraction (2p + 1) / 2f; f = 1: phase 0, fraction 0

// interpolateCubic(x, coeffs), A = -0.75, float32 -- same expression order as oracle/cv2_resize.py
inline void host_cubic_coeffs(float x, float *c) {
    const float A = -0.75f;
    c[0] = ((A * (x + 1.f) - 5.f * A) * (x + 1.f) + 8.f * A) * (x + 1.f) - 4.f * A;
    c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
    const float xm = 1.f - x;
    c[2] = ((A + 2.f) * xm - (A + 3.f)) * xm * xm + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

inline CubicTab pn_cubic_tab(int f) {
    CubicTab t = {};
    if (f == 1) host_cubic_coeffs(0.f, t.c[0]);
    else for (int p = 0; p < f; ++p) host_cubic_coeffs((float)(2 * p + 1) / (float)(2 * f), t.c[p]);
    return t;
}

// the table into LDS (NPH phases of 4): per-lane phases index it -- from the kernel argument that index is a vector-memory load per use (in the
// refinement loops 25 dependent ones per peak, round 5)
template <int NPH>
__device__ __forceinline__ void stage_tab(float (*s_tab)[4], const CubicTab &tab) {
    const int tid = threadIdx.x;
    if (tid < 4 * NPH) s_tab[tid >> 2][tid & 3] = tab.c[tid >> 2][tid & 3];
}

// destination index d of an up-sampling by f = 1 << lf -> first tap (sx - 1) and coefficient phase
template <int LF>
__device__ __forceinline__ void up_src(int d, int lf_arg, int &s0, int &phase) {
    const int lf = LF >= 0 ? LF : lf_arg, f = 1 << lf;
    const int t = 2 * d + 1 - f;                  // (d + 0.5) / f - 0.5 = t / 2f
    s0 = (t >> (lf + 1)) - 1;                     // floor(t / 2f) - 1 (arithmetic shift)
    phase = (t & (2 * f - 1)) >> 1;
}

// value of cv2.resize(src, fx=f, fy=f, INTER_CUBIC)[uy, ux] for a [sh, sw] float32 image with row stride `ld` (replicate border): horizontal
// pass on the four source rows, then vertical pass.
template <int LF>
__device__ __forceinline__ float bicubic(const float *src, int ld, int sh, int sw, int uy, int ux, int lf_arg, const float (*tab)[4]) {
    int sx0, px, sy0, py;
    up_src<LF>(ux, lf_arg, sx0, px);
    up_src<LF>(uy, lf_arg, sy0, py);
    int cx[4], cy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cx[k] = min(max(sx0 + k, 0), sw - 1);
        cy[k] = min(max(sy0 + k, 0), sh - 1);
    }
    float v = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float *row = src + cy[r] * ld;
        float hv = row[cx[0]] * tab[px][0];
        hv = hv + row[cx[1]] * tab[px][1];
        hv = hv + row[cx[2]] * tab[px][2];
        hv = hv + row[cx[3]] * tab[px][3];
        const float t = hv * tab[py][r];
        v = (r == 0) ? t : v + t;
    }
    return v;
}

// np.sum of n < 128 elements at(0) .. at(n - 1) of type T in NumPy's pairwise order: sequential from -0.0 below 8 elements, otherwise eight
// accumulators over the whole blocks of 8, their tree, then the tail
template <typename T, typename F>
__device__ __forceinline__ T np_pairwise_sum(int n, F at) {
    if (n < 8) {
        T res = (T)-0.0;
        for (int k = 0; k < n; ++k) res = res + at(k);
        return res;
    }
    T r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = at(j);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + at(i + j);
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + at(i);
    return res;
}

// ---- peak scan ----
// per-wave ordered peak lists (cell index) of one map; CAP = entries kept per wave (positions past it are counted only)
template <int CAP>
struct PeakLists { int cnt[4]; unsigned short cell[4][CAP]; };
struct PeakCounts { int c0, c1, c2, total; };

// Stages one [h, w] map in LDS and lists its peaks: peak <=> v == max over the 4-connected cross (scipy 'reflect': an out-of-image neighbour is
// the pixel itself) and v > thresh.  Row-major order (= the reference's ids) is kept by an ordered compaction: each wave scans one contiguous
// quarter of the map and compacts with ballots only (no block barrier inside the scan); the four lists are concatenated by prefix counts
// (peak_cell).  block = 256; ends with a block barrier, which also covers whatever the caller wrote to LDS before the call.
template <int CAP>
__device__ __forceinline__ PeakCounts peak_scan(const float *__restrict__ src, int h, int w, float thresh, float *map, PeakLists<CAP> &pk) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hw = h * w;
    for (int i = tid; i < hw; i += 256) map[i] = src[i];
    __syncthreads();
    const int Q = (hw + 3) / 4;
    const int lo = wave * Q, hi = min(hw, lo + Q);
    int wcnt = 0;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        bool is_pk = false;
        if (i < hi) {
            const int y = i / w, x = i - y * w;
            const float v = map[i];
            float m = v;
            if (y > 0) m = fmaxf(m, map[i - w]);
            if (y < h - 1) m = fmaxf(m, map[i + w]);
            if (x > 0) m = fmaxf(m, map[i - 1]);
            if (x < w - 1) m = fmaxf(m, map[i + 1]);
            is_pk = (m == v) && (v > thresh);
        }
        const unsigned long long bal = __ballot(is_pk);
        const int pos = wcnt + __popcll(bal & ((1ull << lane) - 1ull));
        if (is_pk && pos < CAP) pk.cell[wave][pos] = (unsigned short)i;
        wcnt += __popcll(bal);
    }
    if (lane == 0) pk.cnt[wave] = wcnt;
    __syncthreads();
    const int c0 = pk.cnt[0], c1 = pk.cnt[1], c2 = pk.cnt[2];
    return {c0, c1, c2, c0 + c1 + c2 + pk.cnt[3]};
}

// cell of peak p in global order = wave 0's list, then wave 1's, ...  (p < total, and p < CAP where a list may have dropped entries)
template <int CAP>
__device__ __forceinline__ int peak_cell(const PeakLists<CAP> &pk, const PeakCounts &n, int p) {
    if (p < n.c0) return pk.cell[0][p];
    if (p < n.c0 + n.c1) return pk.cell[1][p - n.c0];
    if (p < n.c0 + n.c1 + n.c2) return pk.cell[2][p - n.c0 - n.c1];
    return pk.cell[3][p - n.c0 - n.c1 - n.c2];
}

// the rows of map m of frame b in a PnPeakOut
struct PeakRow { int *count; float *x, *y, *s; };
__device__ __forceinline__ PeakRow peak_row(const PnPeakOut &O, int m, int b) {
    const size_t fo = (size_t)b * O.frame_stride, mo = (size_t)m * O.cap;
    return {(int *)((char *)O.count + fo) + m, (float *)((char *)O.x + fo) + mo, (float *)((char *)O.y + fo) + mo, (float *)((char *)O.s + fo) + mo};
}

// ---- x8 refinement of one peak by one wave ----
// x8 bicubic of the clipped 5x5 patch around `cell` of the staged map, first arg-max in row-major order -> (x, y) in up-sampled pixels and the
// bicubic score, valid in every lane.  The up-sampling is evaluated separably, exactly as cv2 does it (and as bicubic() does per point): the
// horizontal pass of each of the <= 5 source rows once (<= 5 x 40 values, kept in the wave's LDS buffer hb[5 * 40]), then the vertical pass per
// output pixel -- the same float32 operations in the same order as the point-wise form, 4 instead of 16 taps per output pixel.  s_tab: the 8
// phases in LDS, 16-byte aligned.  f = 8 ONLY: the row split (int)((i + 0.5f) * inv_uw) is exact for uw <= 40 and has not been shown for more.
__device__ __forceinline__ void refine_peak_x8(const float *map, int h, int w, int cell, float *hb, const float (*s_tab)[4], int lane, float &out_x,
                                               float &out_y, float &out_s) {
    const int px = cell % w, py = cell / w;
    const int x_min = max(0, px - 2), y_min = max(0, py - 2);
    const int x_max = min(w - 1, px + 2), y_max = min(h - 1, py + 2);
    const int pw = x_max - x_min + 1, ph = y_max - y_min + 1;
    const int uw = pw * 8, un = uw * ph * 8;
    const float inv_uw = 1.0f / (float)uw;
    const float *patch = map + y_min * w + x_min;
    // (fixed trip counts -- <= 5 x 40 and <= 40 x 40 values -- so that the LDS reads of several iterations are in flight; same values in the
    // same ascending order per lane)
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int i = lane + 64 * it;
        if (i < ph * uw) {
            const int r = (int)(((float)i + 0.5f) * inv_uw), ux = i - r * uw;
            int sx0, phx;
            up_src<3>(ux, 3, sx0, phx);
            const float *row = patch + r * w;
            const float4 cf = *reinterpret_cast<const float4 *>(s_tab[phx]);
            float hv = row[min(max(sx0, 0), pw - 1)] * cf.x;
            hv = hv + row[min(max(sx0 + 1, 0), pw - 1)] * cf.y;
            hv = hv + row[min(max(sx0 + 2, 0), pw - 1)] * cf.z;
            hv = hv + row[min(max(sx0 + 3, 0), pw - 1)] * cf.w;
            hb[r * 40 + ux] = hv;
        }
    }
    WAVE_LDS_SYNC();
    float best = -INFINITY;
    int best_i = 0x7fffffff;
#pragma unroll 5
    for (int it = 0; it < 25; ++it) {
        const int i = lane + 64 * it;
        if (i < un) {
            const int uy = (int)(((float)i + 0.5f) * inv_uw), ux = i - uy * uw;
            int sy0, phy;
            up_src<3>(uy, 3, sy0, phy);
            const float4 cf = *reinterpret_cast<const float4 *>(s_tab[phy]);
            float v = hb[min(max(sy0, 0), ph - 1) * 40 + ux] * cf.x;
            v = v + hb[min(max(sy0 + 1, 0), ph - 1) * 40 + ux] * cf.y;
            v = v + hb[min(max(sy0 + 2, 0), ph - 1) * 40 + ux] * cf.z;
            v = v + hb[min(max(sy0 + 3, 0), ph - 1) * 40 + ux] * cf.w;
            if (v > best || best_i == 0x7fffffff) { best = v; best_i = i; }   // i ascending: first max kept
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off);
        const int oi = __shfl_xor(best_i, off);
        if (ov > best || (ov == best && oi < best_i)) { best = ov; best_i = oi; }
    }
    const int my = (int)(((float)best_i + 0.5f) * inv_uw), mx = best_i - my * uw;
    out_x = (float)(8 * x_min + mx);
    out_y = (float)(8 * y_min + my);
    out_s = best;
    WAVE_LDS_SYNC();                                 // the next peak of this wave reuses hb
}

// ---- limb scoring ----
// round-half-even of i*step + start (np.round(np.linspace(...))) as int
__device__ __forceinline__ int linspace_round(double start, double stop, double step, int i, int num) {
    const double v = (i == num - 1) ? stop : ((double)i * step + start);
    return (int)rint(v);
}

// score of sample point pt of n on the segment (sx, sy) -> (ex, ey): the up-sampled PAF vector at the rounded point, dotted with the unit direction
template <int LF>
__device__ __forceinline__ double sample_score(const float *pm0, const float *pm1, int h, int w, double sx, double sy, double ex, double ey, int pt,
                                               int n, int lf_arg, const float (*tab)[4]) {
    const double ddx = ex - sx, ddy = ey - sy;
    const double dist = sqrt(ddx * ddx + ddy * ddy) + 1e-8;
    const double dxn = ddx / dist, dyn_ = ddy / dist;
    // np.linspace(start, stop, n): step = (stop - start) / (n - 1); y_i = i * step + start; y_{n-1} = stop
    const double div = (double)(n - 1);
    const double stepx = (ex - sx) / div, stepy = (ey - sy) / div;
    const int qx = linspace_round(sx, ex, stepx, pt, n);
    const int qy = linspace_round(sy, ey, stepy, pt, n);
    const float vx = bicubic<LF>(pm0, w, h, w, qy, qx, lf_arg, tab);
    const float vy = bicubic<LF>(pm1, w, h, w, qy, qx, lf_arg, tab);
    return (double)vx * dxn + (double)vy * dyn_;      // intermed_paf.dot(limb_dir): both products rounded, as the oracle
}

// one candidate pair from its n point scores: np.mean (NumPy's pairwise sum), criterion 1 (count > 0.8 n in float64; n = 10: cnt > 8, 0.8 * 10.0
// is exactly 8.0), the length penalty min(0.5 * H / dist - 1, 0)
__device__ __forceinline__ bool finish_pair(const double *s, int n, float thresh_paf, double ax, double ay, double bx, double by, int up_h,
                                            double &score) {
    const double mean = np_pairwise_sum<double>(n, [&](int k) { return s[k]; }) / (double)n;
    int cnt = 0;
    for (int k = 0; k < n; ++k) cnt += (s[k] > (double)thresh_paf) ? 1 : 0;
    const double ddx = bx - ax, ddy = by - ay;
    const double dd = sqrt(ddx * ddx + ddy * ddy) + 1e-8;
    const double pen = fmin(0.5 * (double)up_h / dd - 1.0, 0.0);
    score = mean + pen;
    return ((double)cnt > 0.8 * (double)n) && (score > 0.0);
}

// LDS of the scoring pass, shared by the bounded and the unbounded limb kernel (a multiple of 16 bytes at <3, 10>: no padding behind it)
template <int LF, int N>
struct LimbLds {
    static constexpr int PPP = N > 0 ? (256 / N < 64 ? 256 / N : 64) : 64;   // pairs per pass (N_ARG: its largest value)
    static constexpr int NPH = LF >= 0 ? (1 << LF) : 16;                     // coefficient phases
    float pmap[2][MAX_MAP];
    double pts[N > 0 ? PPP * N : 256];
    float tab[NPH][4];
};

// The scoring pass of one limb: stages its two PAF maps, scores every (source peak i, destination peak j) pair, i-major, and hands the pairs that
// pass both criteria to sink(pos, score, i, j) with pos = 0, 1, .. in pair order.  Returns their number (after a block barrier); s_ncand: an int in LDS.  block = 256:
// min(64, 256 / n) pairs per pass, thread = (pair, sample point); then lane k of wave 0 finishes pair k, and an ordered ballot compaction keeps the
// src-major order.  sx / sy / dx / dy: the refined coordinates of the ns source and nd destination peaks (ns, nd >= 1).
template <int LF, int N, typename Sink>
__device__ __forceinline__ int limb_score_pass(LimbLds<LF, N> &S, int &s_ncand, const float *__restrict__ paf_xy, int h, int w, const float *sx, const float *sy,
                                               const float *dx, const float *dy, int ns, int nd, float thresh_paf, int up_h, int lf_arg, int n_arg,
                                               const CubicTab &tab, Sink sink) {
    const int tid = threadIdx.x, hw = h * w;
    const int n = N > 0 ? N : n_arg;
    for (int i = tid; i < hw; i += 256) {
        S.pmap[0][i] = paf_xy[i];
        S.pmap[1][i] = paf_xy[hw + i];
    }
    if (tid == 0) s_ncand = 0;
    stage_tab<LimbLds<LF, N>::NPH>(S.tab, tab);
    __syncthreads();
    const int ppp = min(64, 256 / n);
    const int npairs = ns * nd;                      // <= MAX_MAP^2 = 2^24
    for (int pbase = 0; pbase < npairs; pbase += ppp) {
        const int lp = tid / n, pt = tid - lp * n;
        const int pair = pbase + lp;
        if (lp < ppp && pair < npairs) {
            const int i = pair / nd, j = pair - i * nd;
            S.pts[lp * n + pt] = sample_score<LF>(S.pmap[0], S.pmap[1], h, w, (double)sx[i], (double)sy[i], (double)dx[j], (double)dy[j], pt, n, lf_arg, S.tab);
        }
        __syncthreads();
        if (tid < 64) {
            bool ok = false;
            double score = 0;
            const int pr = pbase + tid;
            const int i = pr / nd, j = pr - i * nd;
            if (tid < ppp && pr < npairs)
                ok = finish_pair(S.pts + tid * n, n, thresh_paf, (double)sx[i], (double)sy[i], (double)dx[j], (double)dy[j], up_h, score);
            const unsigned long long bal = __ballot(ok);
            const int basec = s_ncand;
            if (ok) sink(basec + __popcll(bal & ((1ull << tid) - 1ull)), score, i, j);
            if (tid == 0) s_ncand = basec + __popcll(bal);
        }
        __syncthreads();
    }
    return s_ncand;
}

// ---- per-joint read-out ----
struct JointOut { double x2, y2, depth, X3, Y3, conf; };

// Joint j of one person: its depth by the rule of cfg.z_readout, the rescale to the original frame and the pinhole back-projection.
//   PN_Z_READOUT_HEAT_WEIGHTED  retrieve_depth_heat_weighted([int(x/f), int(y/f)], z*std+mean, heat, radius=1) on the joint's own [h, w] heat and z maps
//   PN_Z_READOUT_CELL           z[z_chn[j]][int(y/f)][int(x/f)] * std + mean in float32 (evaluation_rtpose_light3d_itop.py:176-191); an index past the
//                               last row / column (where the script raises IndexError) is clamped to the last cell: no other cell is read
// heat_f / z_f: the frame's heat and pose-depth maps, channel-major [., h, w].  have == false (the person lacks the joint): (-1, -1, -1) and conf 0,
// back-projected like any other value.  A negative fy (ITOP: Y = -(y - cy) z / f) needs no branch: IEEE division is sign-symmetric.
__device__ __forceinline__ JointOut joint_readout(bool have, float peak_x, float peak_y, float peak_s, const float *__restrict__ heat_f,
                                                  const float *__restrict__ z_f, int j, int h, int w, const pn_parse_cfg &cfg) {
    JointOut o = {-1.0, -1.0, -1.0, 0.0, 0.0, 0.0};
    if (have && cfg.z_readout == PN_Z_READOUT_CELL) {
        const double x = (double)peak_x, y = (double)peak_y, dsz = (double)cfg.downsample;
        o.conf = (double)peak_s;
        const int cx0 = min(max((int)(x / dsz), 0), w - 1), cy0 = min(max((int)(y / dsz), 0), h - 1);
        const int zc = min(max(cfg.z_chn[j], 0), L_);      // checked on the host (pn_parse_check_cfg); the clamp keeps the load inside the map regardless
        float dv = z_f[(size_t)zc * h * w + cy0 * w + cx0] * cfg.depth_std;      // posedepth *= depth_std; posedepth += depth_mean (float32)
        dv = dv + cfg.depth_mean;
        o.depth = (double)dv;
        o.x2 = x / (double)cfg.input_size * (double)cfg.w_org;
        o.y2 = y / (double)cfg.input_size * (double)cfg.h_org;
    } else if (have) {
        const float *__restrict__ hm = heat_f + (size_t)j * h * w, *__restrict__ zm = z_f + (size_t)j * h * w;
        const double x = (double)peak_x, y = (double)peak_y, dsz = (double)cfg.downsample;
        o.conf = (double)peak_s;
        const int cx0 = (int)(x / dsz), cy0 = (int)(y / dsz);
        const int min_x = min(max(cx0 - 1, 0), w - 1), max_x = max(min(cx0 + 1, w - 1), 0);
        const int min_y = min(max(cy0 - 1, 0), h - 1), max_y = max(min(cy0 + 1, h - 1), 0);
        float pw_[9], ww_[9];
        int n = 0;
        // (round 5: the <= 3 x 3 window's eighteen loads are issued before the first is used -- nested loops with run-time bounds waited for
        // every cell in turn; same cells, same row-major order, same arithmetic)
        float hraw[9], zraw[9];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int c = min(min_y + dy, max_y) * w + min(min_x + dx, max_x);
                hraw[dy * 3 + dx] = hm[c];
                zraw[dy * 3 + dx] = zm[c];
            }
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                if (min_y + dy > max_y || min_x + dx > max_x) continue;
                float hv = hraw[dy * 3 + dx];
                if (hv < 0.f) hv = 0.f;
                const float wv = hv + 0.000000001f;
                float dv = zraw[dy * 3 + dx] * cfg.depth_std;
                dv = dv + cfg.depth_mean;
                pw_[n] = dv * wv;
                ww_[n] = wv;
                ++n;
            }
        const float sp = np_pairwise_sum<float>(n, [&](int k) { return pw_[k]; }), sw = np_pairwise_sum<float>(n, [&](int k) { return ww_[k]; });
        o.depth = (double)(sp / sw);
        o.x2 = x / (double)cfg.input_size * (double)cfg.w_org;
        o.y2 = y / (double)cfg.input_size * (double)cfg.h_org;
    }
    o.X3 = (o.x2 - cfg.cx) * o.depth / cfg.fx;
    o.Y3 = (o.y2 - cfg.cy) * o.depth / cfg.fy;
    return o;
}
