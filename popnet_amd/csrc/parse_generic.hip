// The pose parse for every argument the reference accepts (tpm/lib/utils/paf_to_pose.py:75 NMS(heatmaps, upsampFactor, bool_refine_center,
// bool_gaussian_filt); MODEL.DOWNSAMPLE and TEST.NUM_INTERMED_PTS_BETWEEN_KEYPOINTS in find_connected_joints :156-264).
//
// parse_paf.hip's kernels are specialised for the workload's own arguments (x8 up-sampling, ten sample points, refined centres, no filter)
// and stay the only ones that path launches.  The kernels here take the up-sampling factor f in {1, 2, 4, 8, 16}, the number of sample
// points n in [2, 32] and the two NMS flags as data; the launchers in parse_paf.hip start them only when an argument differs from the
// default.  Correctness first: one workgroup per joint map walks its peaks one after the other, no tuning.
//
// Same arithmetic contract as parse_paf.hip (bit-exact against the reference under the cv2.resize restatement): float32 bicubic taps in
// OpenCV's order, float64 where NumPy promotes, NumPy's pairwise summation for np.mean, no fused multiply-add.
//
//   up-sampling by f   destination d has t = 2d + 1 - f: first tap floor(t / 2f) - 1, fraction (t mod 2f) / 2f -- phase p = (t mod 2f) >> 1
//                      has fraction (2p + 1) / 2f for even f; f = 1 has the one fraction 0 (taps 0, 1, 0, 0).  Exact in float32 for powers
//                      of two, which is why other factors are refused.
//   Gaussian filter    scipy.ndimage.gaussian_filter(patch, sigma=3) on float32: radius int(4 * 3 + 0.5) = 12, weights exp(-x^2 / 18)
//                      normalised in float64 (frozen below), axis 0 then axis 1, each output a float64 accumulation
//                      x[l] w[12] + sum_{k=-12..-1} (x[l+k] + x[l-k]) w[k+12] rounded to float32, boundary mode 'reflect'.
#pragma clang fp contract(off)
#include <cmath>
#include "parse_ws.h"

namespace {

__constant__ int g_limb_src[L_] = {8, 9, 11, 8, 10, 12, 8, 1, 2, 4, 1, 3, 5, 1};
__constant__ int g_limb_dst[L_] = {9, 11, 13, 10, 12, 14, 1, 2, 4, 6, 3, 5, 7, 0};

// scipy.ndimage._filters._gaussian_kernel1d(3.0, 0, 12)[0..12] (the kernel is symmetric, [12] is the centre), float64, written as hex
// literals so that no decimal conversion stands between scipy's values and these (tests/golden/make_golden_parse_options.py stores them)
#define GAUSS_R 12
__constant__ double g_gauss[GAUSS_R + 1] = {
    0x1.763a210dfb306p-15, 0x1.4fbe39149e277p-13, 0x1.0d8a5ad43c165p-11, 0x1.8345966f69518p-10, 0x1.f1e9915139406p-9,
    0x1.1e6bccad344bap-7,  0x1.26defcaeb0202p-6,  0x1.0fa58939b528fp-5,  0x1.bfde9c12bec92p-5,  0x1.4a614d1afd337p-4,
    0x1.b42a57d56c0bep-4,  0x1.01a25f86eb137p-3,  0x1.105a329f98197p-3};

struct CubicTabF { float c[16][4]; };   // phase p of an up-sampling by f: fraction (2p + 1) / 2f; f = 1: phase 0, fraction 0

// interpolateCubic, A = -0.75, float32 (parse_paf.hip::host_cubic_coeffs through its exported handle)
CubicTabF make_tab(int f) {
    CubicTabF t = {};
    if (f == 1) pn_debug_cubic_coeffs(0.f, t.c[0]);
    else for (int p = 0; p < f; ++p) pn_debug_cubic_coeffs((float)(2 * p + 1) / (float)(2 * f), t.c[p]);
    return t;
}

// destination index d of an up-sampling by f = 1 << lf -> first tap (sx - 1) and coefficient phase
__device__ __forceinline__ void upf_src(int d, int lf, int &s0, int &phase) {
    const int f = 1 << lf;
    const int t = 2 * d + 1 - f;                  // (d + 0.5) / f - 0.5 = t / 2f
    s0 = (t >> (lf + 1)) - 1;                     // floor(t / 2f) - 1 (arithmetic shift)
    phase = (t & (2 * f - 1)) >> 1;
}

// scipy 'reflect' (d c b a | a b c d | d c b a) of index i into [0, n)
__device__ __forceinline__ int reflect_idx(int i, int n) {
    const int n2 = 2 * n;
    int m = i % n2;
    if (m < 0) m += n2;
    return m >= n ? n2 - 1 - m : m;
}

// value of cv2.resize(src, fx=f, fy=f, INTER_CUBIC)[uy, ux] for a [sh, sw] float32 image with row stride ld (replicate border)
__device__ __forceinline__ float bicubic_f(const float *src, int ld, int sh, int sw, int uy, int ux, int lf, const float (*tab)[4]) {
    int sx0, px, sy0, py;
    upf_src(ux, lf, sx0, px);
    upf_src(uy, lf, sy0, py);
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

// ---------------------------------------------------------------------------------------------
// peaks + refinement.  grid = (maps, B), block = 256.  Peak detection and ordering are peaks_refine_kernel's; then the whole block works on
// one peak at a time.  Dynamic LDS: hb [<= 5][5f] (horizontal pass) and, with the filter, up [5f][5f] and tmp [5f][5f].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gen_peaks_kernel(const float *__restrict__ heat, int h, int w, int heat_c, float thresh, int lf, int refine,
                                                         int gauss, CubicTabF tab, PnPeakOut O) {
    extern __shared__ float dyn[];
    __shared__ float map[MAX_MAP];
    __shared__ int s_wave_cnt[4];
    __shared__ unsigned short s_wlist[4][MAX_MAP / 4 + 1];
    __shared__ float s_tab[16][4];
    __shared__ float s_red_v[4];
    __shared__ int s_red_i[4];
    const int m = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hw = h * w, f = 1 << lf;
    const float *src = heat + ((size_t)b * heat_c + m) * hw;
    for (int i = tid; i < hw; i += 256) map[i] = src[i];
    if (tid < 64) s_tab[tid >> 2][tid & 3] = tab.c[tid >> 2][tid & 3];
    __syncthreads();
    {
        const int Q = (hw + 3) / 4;
        const int lo = wave * Q, hi = min(hw, lo + Q);
        int wcnt = 0;
        for (int base = lo; base < hi; base += 64) {
            const int i = base + lane;
            bool pk = false;
            if (i < hi) {
                const int y = i / w, x = i - y * w;
                const float v = map[i];
                float mx = v;
                if (y > 0) mx = fmaxf(mx, map[i - w]);
                if (y < h - 1) mx = fmaxf(mx, map[i + w]);
                if (x > 0) mx = fmaxf(mx, map[i - 1]);
                if (x < w - 1) mx = fmaxf(mx, map[i + 1]);
                pk = (mx == v) && (v > thresh);
            }
            const unsigned long long bal = __ballot(pk);
            const int pos = wcnt + __popcll(bal & ((1ull << lane) - 1ull));
            if (pk) s_wlist[wave][pos] = (unsigned short)i;
            wcnt += __popcll(bal);
        }
        if (lane == 0) s_wave_cnt[wave] = wcnt;
    }
    __syncthreads();
    const int c0 = s_wave_cnt[0], c1 = s_wave_cnt[1], c2 = s_wave_cnt[2];
    const int total = c0 + c1 + c2 + s_wave_cnt[3];
    const size_t fo = (size_t)b * O.frame_stride;
    int *o_cnt = (int *)((char *)O.count + fo);
    float *opx = (float *)((char *)O.x + fo) + (size_t)m * O.cap;
    float *opy = (float *)((char *)O.y + fo) + (size_t)m * O.cap;
    float *ops = (float *)((char *)O.s + fo) + (size_t)m * O.cap;
    if (tid == 0) o_cnt[m] = total;
    const int n = min(total, O.cap);
    float *hb = dyn, *up = dyn + 5 * 5 * f, *tmp = up + 25 * f * f;

    for (int p = 0; p < n; ++p) {                   // block-uniform
        int cell;
        if (p < c0) cell = s_wlist[0][p];
        else if (p < c0 + c1) cell = s_wlist[1][p - c0];
        else if (p < c0 + c1 + c2) cell = s_wlist[2][p - c0 - c1];
        else cell = s_wlist[3][p - c0 - c1 - c2];
        const int px = cell % w, py = cell / w;
        if (!refine) {                              // (peak + 0.5) * f - 0.5, the map's own value; the filter flag is ignored (paf_to_pose.py:143-146)
            if (tid == 0) {
                opx[p] = (float)(((double)px + 0.5) * (double)f - 0.5);
                opy[p] = (float)(((double)py + 0.5) * (double)f - 0.5);
                ops[p] = map[cell];
            }
            continue;
        }
        const int x_min = max(0, px - 2), y_min = max(0, py - 2);
        const int x_max = min(w - 1, px + 2), y_max = min(h - 1, py + 2);
        const int pw = x_max - x_min + 1, ph = y_max - y_min + 1;
        const int uw = pw * f, uh = ph * f, un = uw * uh;
        const float *patch = map + y_min * w + x_min;
        for (int i = tid; i < ph * uw; i += 256) {
            const int r = i / uw, ux = i - r * uw;
            int sx0, phx;
            upf_src(ux, lf, sx0, phx);
            const float *row = patch + r * w;
            float hv = row[min(max(sx0, 0), pw - 1)] * s_tab[phx][0];
            hv = hv + row[min(max(sx0 + 1, 0), pw - 1)] * s_tab[phx][1];
            hv = hv + row[min(max(sx0 + 2, 0), pw - 1)] * s_tab[phx][2];
            hv = hv + row[min(max(sx0 + 3, 0), pw - 1)] * s_tab[phx][3];
            hb[i] = hv;
        }
        __syncthreads();
        float best = -INFINITY;
        int best_i = 0x7fffffff;
        for (int i = tid; i < un; i += 256) {
            const int uy = i / uw, ux = i - uy * uw;
            int sy0, phy;
            upf_src(uy, lf, sy0, phy);
            float v = hb[min(max(sy0, 0), ph - 1) * uw + ux] * s_tab[phy][0];
            v = v + hb[min(max(sy0 + 1, 0), ph - 1) * uw + ux] * s_tab[phy][1];
            v = v + hb[min(max(sy0 + 2, 0), ph - 1) * uw + ux] * s_tab[phy][2];
            v = v + hb[min(max(sy0 + 3, 0), ph - 1) * uw + ux] * s_tab[phy][3];
            if (gauss) up[i] = v;
            else if (v > best || best_i == 0x7fffffff) { best = v; best_i = i; }      // i ascending: first max kept
        }
        if (gauss) {
            __syncthreads();
            for (int i = tid; i < un; i += 256) {             // axis 0: along y, over the whole patch, rounded to float32
                const int uy = i / uw, ux = i - uy * uw;
                double t = (double)up[i] * g_gauss[GAUSS_R];
                for (int k = -GAUSS_R; k < 0; ++k)
                    t = t + ((double)up[reflect_idx(uy + k, uh) * uw + ux] + (double)up[reflect_idx(uy - k, uh) * uw + ux]) * g_gauss[k + GAUSS_R];
                tmp[i] = (float)t;
            }
            __syncthreads();
            for (int i = tid; i < un; i += 256) {             // axis 1: along x
                const int uy = i / uw, ux = i - uy * uw;
                const float *row = tmp + uy * uw;
                double t = (double)row[ux] * g_gauss[GAUSS_R];
                for (int k = -GAUSS_R; k < 0; ++k)
                    t = t + ((double)row[reflect_idx(ux + k, uw)] + (double)row[reflect_idx(ux - k, uw)]) * g_gauss[k + GAUSS_R];
                const float v = (float)t;
                if (v > best || best_i == 0x7fffffff) { best = v; best_i = i; }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(best, off);
            const int oi = __shfl_xor(best_i, off);
            if (oi != 0x7fffffff && (best_i == 0x7fffffff || ov > best || (ov == best && oi < best_i))) { best = ov; best_i = oi; }
        }
        if (lane == 0) { s_red_v[wave] = best; s_red_i[wave] = best_i; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < 4; ++k) {
                const float ov = s_red_v[k];
                const int oi = s_red_i[k];
                if (oi != 0x7fffffff && (best_i == 0x7fffffff || ov > best || (ov == best && oi < best_i))) { best = ov; best_i = oi; }
            }
            const int my = best_i / uw, mx = best_i - my * uw;
            opx[p] = (float)(f * x_min + mx);
            opy[p] = (float)(f * y_min + my);
            ops[p] = best;
        }
        __syncthreads();                            // the next peak reuses hb / up / tmp / s_red
    }
}

// round-half-even of i*step + start (np.round(np.linspace(...))) as int
__device__ __forceinline__ int linspace_round(double start, double stop, double step, int i, int num) {
    const double v = (i == num - 1) ? stop : ((double)i * step + start);
    return (int)rint(v);
}

// score of sample point pt of n on the segment (sx, sy) -> (ex, ey): the up-sampled PAF vector at the rounded point, dotted with the unit direction
__device__ __forceinline__ double sample_score(const float *pm0, const float *pm1, int h, int w, double sx, double sy, double ex, double ey, int pt,
                                               int n, int lf, const float (*tab)[4]) {
    const double ddx = ex - sx, ddy = ey - sy;
    const double dist = sqrt(ddx * ddx + ddy * ddy) + 1e-8;
    const double dxn = ddx / dist, dyn_ = ddy / dist;
    // np.linspace(start, stop, n): step = (stop - start) / (n - 1); y_i = i * step + start; y_{n-1} = stop
    const double div = (double)(n - 1);
    const double stepx = (ex - sx) / div, stepy = (ey - sy) / div;
    const int qx = linspace_round(sx, ex, stepx, pt, n);
    const int qy = linspace_round(sy, ey, stepy, pt, n);
    const float vx = bicubic_f(pm0, w, h, w, qy, qx, lf, tab);
    const float vy = bicubic_f(pm1, w, h, w, qy, qx, lf, tab);
    return (double)vx * dxn + (double)vy * dyn_;      // intermed_paf.dot(limb_dir): both products rounded, as limb_match_kernel and the oracle
}

// one candidate pair from its n point scores: np.mean (NumPy's pairwise sum), criterion 1 (count > 0.8 n in float64), the length penalty
__device__ __forceinline__ bool finish_pair(const double *s, int n, float thresh_paf, double ax, double ay, double bx, double by, int up_h,
                                            double &score) {
    double res;
    if (n < 8) {
        res = 0.0;
        for (int k = 0; k < n; ++k) res = res + s[k];
    } else {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = s[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = r[j] + s[i + j];
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res = res + s[i];
    }
    const double mean = res / (double)n;
    int cnt = 0;
    for (int k = 0; k < n; ++k) cnt += (s[k] > (double)thresh_paf) ? 1 : 0;
    const double ddx = bx - ax, ddy = by - ay;
    const double dd = sqrt(ddx * ddx + ddy * ddy) + 1e-8;
    const double pen = fmin(0.5 * (double)up_h / dd - 1.0, 0.0);
    score = mean + pen;
    return ((double)cnt > 0.8 * (double)n) && (score > 0.0);
}

// ---------------------------------------------------------------------------------------------
// limb scoring + greedy matching: limb_match_kernel with n sample points and the xf bicubic.  grid = (L, B), block = 256;
// min(64, 256 / n) pairs per pass, thread = (pair, sample point).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gen_limb_kernel(const float *__restrict__ paf, int h, int w, int paf_c, float thresh_paf, int up_h, int lf,
                                                        int npts, CubicTabF tab, ParseWs *__restrict__ ws) {
    __shared__ float pmap[2][MAX_MAP];
    __shared__ double s_pts[256];
    __shared__ double s_cand_s[MAXP * MAXP];
    __shared__ unsigned char s_cand_i[MAXP * MAXP], s_cand_j[MAXP * MAXP];
    __shared__ unsigned short s_order[MAXP * MAXP];
    __shared__ int s_ncand;
    __shared__ float s_tab[16][4];
    const int limb = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x;
    ParseWs &W = ws[b];
    const int jsrc = g_limb_src[limb], jdst = g_limb_dst[limb];
    const int ns = min(W.peak_count[jsrc], MAXP), nd = min(W.peak_count[jdst], MAXP);
    if (ns == 0 || nd == 0) {
        if (tid == 0) W.conn_count[limb] = 0;
        return;
    }
    const int hw = h * w;
    const float *px_map = paf + ((size_t)b * paf_c + 2 * limb) * hw;
    for (int i = tid; i < hw; i += 256) {
        pmap[0][i] = px_map[i];
        pmap[1][i] = px_map[hw + i];
    }
    if (tid == 0) s_ncand = 0;
    if (tid < 64) s_tab[tid >> 2][tid & 3] = tab.c[tid >> 2][tid & 3];
    __syncthreads();

    const int ppp = min(64, 256 / npts);
    const int npairs = ns * nd;
    for (int pbase = 0; pbase < npairs; pbase += ppp) {
        const int lp = tid / npts, pt = tid - lp * npts;
        const int pair = pbase + lp;
        if (lp < ppp && pair < npairs) {
            const int i = pair / nd, j = pair - i * nd;
            s_pts[lp * npts + pt] = sample_score(pmap[0], pmap[1], h, w, (double)W.peak_x[jsrc][i], (double)W.peak_y[jsrc][i],
                                                 (double)W.peak_x[jdst][j], (double)W.peak_y[jdst][j], pt, npts, lf, s_tab);
        }
        __syncthreads();
        if (tid < 64) {                              // one pair per lane of wave 0; ordered compaction keeps src-major order
            bool ok = false;
            double score = 0;
            const int pr = pbase + tid;
            if (tid < ppp && pr < npairs) {
                const int i = pr / nd, j = pr - i * nd;
                ok = finish_pair(s_pts + tid * npts, npts, thresh_paf, (double)W.peak_x[jsrc][i], (double)W.peak_y[jsrc][i],
                                 (double)W.peak_x[jdst][j], (double)W.peak_y[jdst][j], up_h, score);
            }
            const unsigned long long bal = __ballot(ok);
            const int basec = s_ncand;
            if (ok) {
                const int pos = basec + __popcll(bal & ((1ull << tid) - 1ull));
                s_cand_s[pos] = score;
                s_cand_i[pos] = (unsigned char)(pr / nd);
                s_cand_j[pos] = (unsigned char)(pr % nd);
            }
            if (tid == 0) s_ncand = basec + __popcll(bal);
        }
        __syncthreads();
    }

    // stable descending sort by score (Python sorted(..., reverse=True) keeps insertion order on ties)
    const int nc = s_ncand;
    for (int k = tid; k < nc; k += 256) {
        const double sk = s_cand_s[k];
        int rank = 0;
        for (int q = 0; q < nc; ++q) {
            const double sq = s_cand_s[q];
            rank += (sq > sk || (sq == sk && q < k)) ? 1 : 0;
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

// the same for the unbounded second pass: big_limb_kernel with n sample points and the xf bicubic.  grid = L, block = 256.
__global__ __launch_bounds__(256) void gen_big_limb_kernel(const float *__restrict__ paf, int h, int w, float thresh_paf, int up_h, int lf, int npts,
                                                            CubicTabF tab, BigWs W) {
    __shared__ float pmap[2][MAX_MAP];
    __shared__ double s_pts[256];
    __shared__ unsigned s_used_i[MAX_MAP / 32], s_used_j[MAX_MAP / 32];
    __shared__ double s_best_s[256];
    __shared__ int s_best_k[256];
    __shared__ int s_ncand;
    __shared__ float s_tab[16][4];
    const int limb = blockIdx.x, tid = threadIdx.x;
    const int jsrc = g_limb_src[limb], jdst = g_limb_dst[limb];
    const int ns = W.peak_count[jsrc], nd = W.peak_count[jdst];
    if (ns == 0 || nd == 0) {
        if (tid == 0) W.conn_count[limb] = 0;
        return;
    }
    const int hw = h * w;
    const float *sx_ = W.px + (size_t)jsrc * hw, *sy_ = W.py + (size_t)jsrc * hw;
    const float *dx_ = W.px + (size_t)jdst * hw, *dy_ = W.py + (size_t)jdst * hw;
    double *cs = W.cand_s + W.cand_off[limb];
    unsigned short *ci = W.cand_i + W.cand_off[limb], *cj = W.cand_j + W.cand_off[limb];
    const float *px_map = paf + (size_t)(2 * limb) * hw;
    for (int i = tid; i < hw; i += 256) {
        pmap[0][i] = px_map[i];
        pmap[1][i] = px_map[hw + i];
    }
    for (int i = tid; i < MAX_MAP / 32; i += 256) { s_used_i[i] = 0u; s_used_j[i] = 0u; }
    if (tid == 0) s_ncand = 0;
    if (tid < 64) s_tab[tid >> 2][tid & 3] = tab.c[tid >> 2][tid & 3];
    __syncthreads();
    const int ppp = min(64, 256 / npts);
    const long long npairs = (long long)ns * nd;
    for (long long pbase = 0; pbase < npairs; pbase += ppp) {
        const int lp = tid / npts, pt = tid - lp * npts;
        const long long pair = pbase + lp;
        if (lp < ppp && pair < npairs) {
            const int i = (int)(pair / nd), j = (int)(pair - (long long)i * nd);
            s_pts[lp * npts + pt] = sample_score(pmap[0], pmap[1], h, w, (double)sx_[i], (double)sy_[i], (double)dx_[j], (double)dy_[j], pt, npts, lf, s_tab);
        }
        __syncthreads();
        if (tid < 64) {
            bool ok = false;
            double score = 0;
            const long long pr = pbase + tid;
            if (tid < ppp && pr < npairs) {
                const int i = (int)(pr / nd), j = (int)(pr - (long long)i * nd);
                ok = finish_pair(s_pts + tid * npts, npts, thresh_paf, (double)sx_[i], (double)sy_[i], (double)dx_[j], (double)dy_[j], up_h, score);
            }
            const unsigned long long bal = __ballot(ok);
            const int basec = s_ncand;
            if (ok) {
                const int pos = basec + __popcll(bal & ((1ull << tid) - 1ull));
                cs[pos] = score;
                ci[pos] = (unsigned short)(pr / nd);
                cj[pos] = (unsigned short)(pr % nd);
            }
            if (tid == 0) s_ncand = basec + __popcll(bal);
        }
        __syncthreads();
    }
    __threadfence_block();
    // greedy matching as in big_limb_kernel: repeatedly the best (score desc, insertion order asc) candidate whose two peaks are both free
    const int nc = s_ncand, maxc = min(ns, nd);
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

}  // namespace

int pn_gen_launch_peaks(pn_ctx *ctx, hipStream_t s, const float *heat_dev, int n_maps, int B, int h, int w, int heat_c, float thresh, int f, int refine,
                        int gauss, const PnPeakOut &out) {
    const int lf = pn_parse_factor_log2(f);
    if (lf < 0) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "up-sampling factor %d: supported are " PN_PARSE_FACTORS_TEXT, f);
    gauss = (refine && gauss) ? 1 : 0;
    // hb always; up + tmp only under the filter: 52.8 KB at f = 16, on top of 25 KB of static LDS (map + peak lists) -- above the 64 KB a
    // kernel gets without opting in
    const size_t lds = ((size_t)5 * 5 * f + (gauss ? (size_t)2 * 25 * f * f : 0)) * sizeof(float);
    static PnLdsAttr attr;
    const int rc = pn_lds_attr(ctx, attr, (const void *)gen_peaks_kernel, ((size_t)5 * 5 * 16 + (size_t)2 * 25 * 16 * 16) * sizeof(float));
    if (rc != PN_OK) return rc;
    hipLaunchKernelGGL(gen_peaks_kernel, dim3(n_maps, B), dim3(256), lds, s, heat_dev, h, w, heat_c, thresh, lf, refine ? 1 : 0, gauss, make_tab(f), out);
    return PN_OK;
}

int pn_gen_launch_limbs(pn_ctx *ctx, hipStream_t s, const float *paf_dev, int B, int h, int w, float thresh_paf, int f, int npts, ParseWs *ws) {
    const int lf = pn_parse_factor_log2(f);
    if (lf < 0 || !pn_parse_pts_ok(npts)) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "limb scoring: factor %d / %d sample points unsupported", f, npts);
    hipLaunchKernelGGL(gen_limb_kernel, dim3(L_, B), dim3(256), 0, s, paf_dev, h, w, 2 * L_, thresh_paf, h * f, lf, npts, make_tab(f), ws);
    return PN_OK;
}

int pn_gen_launch_big_limbs(pn_ctx *ctx, hipStream_t s, const float *paf_dev, int h, int w, float thresh_paf, int f, int npts, const BigWs &W) {
    const int lf = pn_parse_factor_log2(f);
    if (lf < 0 || !pn_parse_pts_ok(npts)) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "limb scoring: factor %d / %d sample points unsupported", f, npts);
    hipLaunchKernelGGL(gen_big_limb_kernel, dim3(L_), dim3(256), 0, s, paf_dev, h, w, thresh_paf, h * f, lf, npts, make_tab(f), W);
    return PN_OK;
}
