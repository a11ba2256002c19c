// NMS of the pose parse (tpm/lib/utils/paf_to_pose.py:75 NMS(heatmaps, upsampFactor, bool_refine_center, bool_gaussian_filt)), for every path:
// the bounded batch (parse_paf.hip), the unbounded second pass and pn_nms_peaks (parse_unbounded.hip).  Two kernels share the peak scan of
// parse_device.h: peaks_refine_kernel for the workload's own arguments (x8 up-sampling, refined centres, no filter), one wave per peak, and
// gen_peaks_kernel, which takes the factor f in {1, 2, 4, 8, 16} and the two flags as data.  pn_launch_peaks picks.
//
//   Gaussian filter    scipy.ndimage.gaussian_filter(patch, sigma=3) on float32: radius int(4 * 3 + 0.5) = 12, weights exp(-x^2 / 18)
//                      normalised in float64 (frozen below), axis 0 then axis 1, each output a float64 accumulation
//                      x[l] w[12] + sum_{k=-12..-1} (x[l+k] + x[l-k]) w[k+12] rounded to float32, boundary mode 'reflect'.
#pragma clang fp contract(off)
#include "parse_device.h"

namespace {

// scipy.ndimage._filters._gaussian_kernel1d(3.0, 0, 12)[0..12] (the kernel is symmetric, [12] is the centre), float64, written as hex
// literals so that no decimal conversion stands between scipy's values and these (tests/golden/make_golden_parse_options.py stores them)
#define GAUSS_R 12
__constant__ double g_gauss[GAUSS_R + 1] = {
    0x1.763a210dfb306p-15, 0x1.4fbe39149e277p-13, 0x1.0d8a5ad43c165p-11, 0x1.8345966f69518p-10, 0x1.f1e9915139406p-9,
    0x1.1e6bccad344bap-7,  0x1.26defcaeb0202p-6,  0x1.0fa58939b528fp-5,  0x1.bfde9c12bec92p-5,  0x1.4a614d1afd337p-4,
    0x1.b42a57d56c0bep-4,  0x1.01a25f86eb137p-3,  0x1.105a329f98197p-3};

// scipy 'reflect' (d c b a | a b c d | d c b a) of index i into [0, n)
__device__ __forceinline__ int reflect_idx(int i, int n) {
    const int n2 = 2 * n;
    int m = i % n2;
    if (m < 0) m += n2;
    return m >= n ? n2 - 1 - m : m;
}

// ---------------------------------------------------------------------------------------------
// k1 of the default arguments: peaks + x8 refinement.  grid = (maps, B), block = 256: peak flags -> ordered ballot compaction -> one wave per
// peak up-samples its <= 5x5 patch x8 (<= 40x40) and wave-reduces the first arg-max.  CAP: entries of the per-wave lists -- MAXP where the
// output keeps at most MAXP peaks per map (the bounded records), MAX_MAP / 4 + 1 (a wave's whole quarter) where it keeps them all.
// ---------------------------------------------------------------------------------------------
template <int CAP>
__global__ __launch_bounds__(256) void peaks_refine_kernel(const float *__restrict__ heat, int h, int w, int heat_c, float thresh, CubicTab tab,
                                                            PnPeakOut O) {
    __shared__ float map[MAX_MAP];
    __shared__ PeakLists<CAP> s_pk;
    __shared__ float s_h[4][5 * 40];                 // per wave: horizontal pass of the patch being refined
    __shared__ __attribute__((aligned(16))) float s_tab[8][4];
    const int m = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    stage_tab<8>(s_tab, tab);
    const PeakCounts pc = peak_scan(heat + ((size_t)b * heat_c + m) * h * w, h, w, thresh, map, s_pk);
    const PeakRow R = peak_row(O, m, b);
    if (tid == 0) *R.count = pc.total;
    const int n = min(pc.total, O.cap);
    for (int p = wave; p < n; p += 4) {
        float x, y, sc;
        refine_peak_x8(map, h, w, peak_cell(s_pk, pc, p), s_h[wave], s_tab, lane, x, y, sc);
        if (lane == 0) { R.x[p] = x; R.y[p] = y; R.s[p] = sc; }
    }
}

// ---------------------------------------------------------------------------------------------
// peaks + refinement for any factor / flags.  grid = (maps, B), block = 256.  Peak detection and ordering are peaks_refine_kernel's; then the whole
// block works on one peak at a time (correctness first, no tuning).  Dynamic LDS: hb [<= 5][5f] (horizontal pass) and, with the filter,
// up [5f][5f] and tmp [5f][5f].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gen_peaks_kernel(const float *__restrict__ heat, int h, int w, int heat_c, float thresh, int lf, int refine,
                                                         int gauss, CubicTab tab, PnPeakOut O) {
    extern __shared__ float dyn[];
    __shared__ float map[MAX_MAP];
    __shared__ PeakLists<MAX_MAP / 4 + 1> s_pk;
    __shared__ float s_tab[16][4];
    __shared__ float s_red_v[4];
    __shared__ int s_red_i[4];
    const int m = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hw = h * w, f = 1 << lf;
    stage_tab<16>(s_tab, tab);
    const PeakCounts pc = peak_scan(heat + ((size_t)b * heat_c + m) * hw, h, w, thresh, map, s_pk);
    const PeakRow R = peak_row(O, m, b);
    float *opx = R.x, *opy = R.y, *ops = R.s;
    if (tid == 0) *R.count = pc.total;
    const int n = min(pc.total, O.cap);
    float *hb = dyn, *up = dyn + 5 * 5 * f, *tmp = up + 25 * f * f;

    for (int p = 0; p < n; ++p) {                   // block-uniform
        const int cell = peak_cell(s_pk, pc, p);
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
            up_src<LF_ARG>(ux, lf, sx0, phx);
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
            up_src<LF_ARG>(uy, lf, sy0, phy);
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

}  // namespace

int pn_launch_peaks(pn_ctx *ctx, hipStream_t s, const float *heat_dev, int n_maps, int B, int h, int w, int heat_c, float thresh, int f, int refine,
                    int gauss, const PnPeakOut &out) {
    const dim3 grid(n_maps, B);
    gauss = (refine && gauss) ? 1 : 0;
    if (f == 8 && refine && !gauss) {
        // a record that keeps <= MAXP peaks per map needs only the first MAXP of each wave's list
        if (out.cap <= MAXP) hipLaunchKernelGGL(peaks_refine_kernel<MAXP>, grid, dim3(256), 0, s, heat_dev, h, w, heat_c, thresh, pn_cubic_tab(8), out);
        else hipLaunchKernelGGL(peaks_refine_kernel<MAX_MAP / 4 + 1>, grid, dim3(256), 0, s, heat_dev, h, w, heat_c, thresh, pn_cubic_tab(8), out);
        return PN_OK;
    }
    // hb always; up + tmp only under the filter: 52.8 KB at f = 16, on top of 25 KB of static LDS (map + peak lists) -- above the 64 KB a
    // kernel gets without opting in
    const size_t lds = ((size_t)5 * 5 * f + (gauss ? (size_t)2 * 25 * f * f : 0)) * sizeof(float);
    static PnLdsAttr attr;
    const int rc = pn_lds_attr(ctx, attr, (const void *)gen_peaks_kernel, ((size_t)5 * 5 * 16 + (size_t)2 * 25 * 16 * 16) * sizeof(float));
    if (rc != PN_OK) return rc;
    hipLaunchKernelGGL(gen_peaks_kernel, grid, dim3(256), lds, s, heat_dev, h, w, heat_c, thresh, pn_parse_factor_log2(f), refine ? 1 : 0, gauss,
                       pn_cubic_tab(f), out);
    return PN_OK;
}
