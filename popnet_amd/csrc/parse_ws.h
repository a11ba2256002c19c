// Scratch layouts, capacities, argument checks and the one cross-file launcher of the pose-parse translation units: parse_paf.hip (the
// bounded batch path), parse_unbounded.hip (the second pass and pn_nms_peaks), parse_peaks.hip (the NMS kernels of both), parse_utils.hip.
// The arithmetic they share is parse_device.h.
#pragma once
#include "pn_internal.h"

#define J_ PN_NUM_JOINTS
#define L_ PN_NUM_LIMBS
#define MAXP PN_MAX_PEAKS_PER_JOINT
#define MAXC PN_MAX_CONN_PER_LIMB
#define MAX_MAP 4096      // largest h*w the parse kernels stage in LDS (64 KB static-LDS budget)

// LDS hand-over between lanes of ONE wave (a wave's LDS instructions execute in order; the waits and the compiler fence
// make the earlier writes visible to the later reads of other lanes).  Used where the waves of a block run loops of
// different trip counts, so a block barrier is not available.
#define WAVE_LDS_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

struct ParseWs {                       // per-frame scratch between the three kernels
    int peak_count[J_];                // uncapped count (overflow detection)
    float peak_x[J_][MAXP], peak_y[J_][MAXP], peak_s[J_][MAXP];
    int conn_count[L_];
    int conn_i[L_][MAXC], conn_j[L_][MAXC];
    double conn_s[L_][MAXC];
};

struct BigWs {                       // the unbounded second pass: every list in global memory, sized from the frame's own counts
    int *peak_count;                 // [J]
    float *px, *py, *ps;             // [J][hw]
    int *conn_count;                 // [L]
    int *conn_i, *conn_j;            // [L][hw]
    double *conn_s;                  // [L][hw]
    double *cand_s;                  // candidates of all limbs, limb l at cand_off[l]
    unsigned short *cand_i, *cand_j;
    long long cand_off[L_ + 1];
    double *rows, *rows2;            // [maxp][J + 2]
    int maxp;
    int *keep_idx;                   // [maxp]
    int *counts;                     // [0] peaks, [1] persons
    // results
    float *o_peak;                   // [npeaks][3]: x, y, score
    int *o_peak_type;                // [npeaks]
    int *o_person_joint;             // [P][J]
    double *o_person_score;          // [P]
    int *o_person_count;             // [P]
    double *o_j2d, *o_j3d, *o_conf;  // [P][J][2], [P][J][3], [P][J]
};

// ---- the arguments every path accepts: up-sampling factor f in {1, 2, 4, 8, 16} (powers of two: the bicubic phases are exact in float32), 2..32
// sample points per limb.  The workload's own (x8, ten points, refined centres, no filter) get the specialised kernel instantiations.
#define PN_PARSE_FACTORS_TEXT "1, 2, 4, 8, 16"
#define PN_PARSE_MIN_PTS 2
#define PN_PARSE_MAX_PTS 32
// log2 of a supported up-sampling factor, -1 otherwise
inline int pn_parse_factor_log2(int f) { return f == 1 ? 0 : f == 2 ? 1 : f == 4 ? 2 : f == 8 ? 3 : f == 16 ? 4 : -1; }
inline bool pn_parse_pts_ok(int n) { return n >= PN_PARSE_MIN_PTS && n <= PN_PARSE_MAX_PTS; }

// the checks of pn_parse_paf(_wire) and pn_parse_paf_unbounded (`who`), PN_OK or the error set on ctx
inline int pn_parse_check_map(pn_ctx *ctx, const char *who, int h, int w) {
    if (h * w > MAX_MAP || h < 1 || w < 1) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "%s: map %dx%d exceeds %d cells", who, h, w, MAX_MAP);
    return PN_OK;
}
inline int pn_parse_check_cfg(pn_ctx *ctx, const char *who, const pn_parse_cfg *cfg) {
    if (pn_parse_factor_log2(cfg->downsample) < 0 || !pn_parse_pts_ok(cfg->num_intermed_pts))
        return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "%s: downsample %d / num_intermed_pts %d: supported are downsample in {" PN_PARSE_FACTORS_TEXT "} and %d..%d intermediate points",
                            who, cfg->downsample, cfg->num_intermed_pts, PN_PARSE_MIN_PTS, PN_PARSE_MAX_PTS);
    if (cfg->z_readout != PN_Z_READOUT_HEAT_WEIGHTED && cfg->z_readout != PN_Z_READOUT_CELL)
        return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "%s: z_readout %d is neither PN_Z_READOUT_HEAT_WEIGHTED nor PN_Z_READOUT_CELL", who, cfg->z_readout);
    if (cfg->z_readout == PN_Z_READOUT_CELL)
        for (int j = 0; j < J_; ++j)
            if (cfg->z_chn[j] < 0 || cfg->z_chn[j] > L_)      // the pose-depth map has L + 1 channels
                return pn_set_error(ctx, PN_ERR_INVALID, "%s: z_chn[%d] = %d is not a channel of the pose-depth map (0..%d)", who, j, cfg->z_chn[j], L_);
    return PN_OK;
}

// where the peaks of map m of frame b go: count[m], x / y / s [m][cap], frame b `frame_stride` bytes further on; peaks past cap are counted only
struct PnPeakOut { int *count; float *x, *y, *s; int cap; size_t frame_stride; };
// parse_peaks.hip: the NMS launch of every path -- peaks_refine_kernel for (x8, refined centres, no filter), gen_peaks_kernel for anything else.
// Neither allocates nor synchronises.
int pn_launch_peaks(pn_ctx *ctx, hipStream_t s, const float *heat_dev, int n_maps, int B, int h, int w, int heat_c, float thresh, int f, int refine,
                    int gauss, const PnPeakOut &out);
