// Convolution kernels of the NCHW training engine (train.hip): forward and, with flipped weights, the stride-1 data gradient.
//   tconv_fwd_kernel<KS>           any kernel size / stride: implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains), gathered operand
//   tconv3_tile_kernel             3x3 stride 1 on halo tiles, fp32 MFMA
//   tconv3_tile_x3 / _x3w_kernel   the same tiles on split-bf16 MFMA ("bf16x3"): 128 / 256 pixel slots per block
//   tstem_fwd_kernel               the planes engine's 7x7 / 2 single-channel stem (trainx.hip)
//   wpack3 / wpack3_x3 / wpack_all / wflip   weight packs of the kernels above (the pack formats themselves: train_conv_common.h)
// What the kernels share is written once: t_tile_epilogue (all four NCHW epilogues), t_tile_block / t_tile_slot / t_halo_off (the tile kernels'
// decodes), TXRows80 / TXRowsSwz + t_x3_load_w / t_x3_store_w / t_x3_next_w / t_x3_stage_halo (the two split-bf16 tile kernels, which differ in
// their LDS address function and their pixel-tile count).  The launches, the geometry functions and the planners are in train.hip.
#pragma once
#include "train_conv_common.h"

struct TConv {
    const float *x;      // [N, Cin, H, W]
    const float *w;      // [Cout, Cin * KS * KS]
    const float *bias;   // [Cout] or nullptr
    float *y;            // [N, Cout, Ho, Wo]
    int N, Cin, H, W, Cout, Ho, Wo, stride, pad, accumulate;
    int Kdim;            // Cin * KS * KS
    int P;               // N * Ho * Wo
    // round 6 (the planes training engine's stem, trainx.hip): y / dY as a channel-minor planes tensor [pixel][pl_cs] instead of NCHW f32 --
    // PL = 1: two bf16 planes [hi | lo] `pl_split` elements apart (value = hi + lo), PL = 2: one f32 plane.  Same values, same MFMA order as the
    // NCHW form followed / preceded by trainx_kernels.h's layout pass: bit-identical, one 103 MB round trip less each way.
    void *pl = nullptr;
    int pl_cs = 0, pl_split = 0;
    int dil = 1;         // tap spacing; read by the DIL instantiations of tconv_fwd_kernel / tconv_wgrad_kernel only (pn_conv2d_*_dil)
};

// ---------------------------------------------------------------------------------------------------------------------
// Forward (and, with flipped weights, the stride-1 data gradient): D[cout][pixel] = sum_k W[cout][k] * X[k][pixel],
// k = (ci, ky, kx).  Block = 64 couts x 128 pixels, 4 waves (each 64 couts x 32 pixels = 4 x 2 MFMA tiles), K chunks of 16
// staged through LDS (weights k-major, the gathered input k-major; lanes run along the pixels, so every global gather is a
// run of consecutive addresses), next chunk's global loads in flight during the MFMAs of the current one.
// ---------------------------------------------------------------------------------------------------------------------
#define TC_KC 16
#define TC_AP 80      // LDS pitches: 4 k rows x 16 lanes of an MFMA operand read fall on 64 different banks
#define TC_BP 144

// The bias of this lane's sixteen couts co0 + 16 m + 4 q + i (element i of MFMA tile m), gathered once (round 5: `v += c.bias[co]` inside the store loop
// compiled to load, s_waitcnt vmcnt(0), add -- sixteen dependent round trips per pixel tile, as did the accumulate form's old values, which the compiler
// had sunk to their uses)
__device__ __forceinline__ void t_bias16(const TConv &c, int co0, int q, float (&bv)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int co = co0 + 16 * (k >> 2) + 4 * q + (k & 3);
        bv[k] = c.bias ? c.bias[co < c.Cout ? co : 0] : 0.f;
    }
    T_PIN16(bv);
}
// NCHW epilogue of the forward kernels: acc[m][n][i] is cout co0 + 16 m + 4 q + i of the lane's pixel slot n; slot(n, pok) returns the address of that pixel
// in cout plane 0 of y (any valid address when the slot is unused: pok = 0).  y (+)= bias + acc; the accumulate form first gathers all sixteen old values of
// a slot (independent loads in flight), then adds and stores.
template <int NT, class Slot>
__device__ __forceinline__ void t_tile_epilogue(const TConv &c, int HoWo, int co0, int q, const t_f32x4 (&acc)[4][NT], Slot slot) {
    float bv[16];
    t_bias16(c, co0, q, bv);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        int pok;
        float *yb = slot(n, pok);
        float old[16];
        if (c.accumulate) {
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int co = co0 + 16 * m + 4 * q + i;
                    old[4 * m + i] = yb[(co * HoWo) & -(int)(co < c.Cout)];
                }
            T_PIN16(old);                               // all sixteen loads issued, THEN used (see T_PIN16)
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = co0 + 16 * m + 4 * q + i;
                float v = acc[m][n][i];
                v += bv[4 * m + i];
                if (c.accumulate) v += old[4 * m + i];
                if (pok && co < c.Cout) yb[(size_t)co * HoWo] = v;
            }
    }
}

// DIL: the taps are c.dil pixels apart (A2J's layer4.1 / layer4.2 conv2, third_party_methods/A2J_experiments/resnet.py:112,145) -- the gather address
// changes, the k order and the MFMA order do not.  DIL = false is the kernel as it always was.
template <int KS, int PL = 0, bool DIL = false>
__global__ __launch_bounds__(256) void tconv_fwd_kernel(TConv c) {
    __shared__ float As[TC_KC][TC_AP];
    __shared__ float Bs[TC_KC][TC_BP];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    T_DECODE_TILE_CB(pblk, cblk);
    const int p0 = pblk * 128, co0 = cblk * 64;
    const int HoWo = c.Ho * c.Wo;
    // staging roles
    const int b_pn = t & 127, b_k0 = t >> 7;            // B: pixel column, k rows b_k0 + 2j
    const int a_co = t & 63, a_k0 = (t >> 6) * 4;       // A: cout row, k rows a_k0 + j
    const int bp = p0 + b_pn;
    const bool bp_ok = bp < c.P;
    int bn = 0, iy0 = 0, ix0 = 0;
    if (bp_ok) {
        bn = bp / HoWo;
        const int rem = bp - bn * HoWo, oy = rem / c.Wo, ox = rem - oy * c.Wo;
        iy0 = oy * c.stride - c.pad;
        ix0 = ox * c.stride - c.pad;
    }
    // every load is unconditional (an out-of-range element reads index 0; it is zeroed when the value goes to LDS, one chunk
    // later -- a select right after the load would put an s_waitcnt vmcnt(0) in front of the MFMAs the load is meant to
    // overlap with, and a conditional load becomes a branch of its own: 73 of them in the first version of this loop)
    const float *xb = c.x + (size_t)bn * c.Cin * c.H * c.W;
    const bool a_ok = co0 + a_co < c.Cout;
    const float *wa = c.w + (a_ok ? (size_t)(co0 + a_co) * c.Kdim : 0);

    float ra[4], rb[8];
    unsigned okm = 0;          // bit j: rb[j] valid, bit 8 + j: ra[j] valid
    auto load = [&](int k0) {
        okm = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + a_k0 + j;
            const int ok = (int)(a_ok & (k < c.Kdim));
            ra[j] = wa[k & -ok];
            okm |= (unsigned)ok << (8 + j);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + b_k0 + 2 * j;
            const int ci = k / (KS * KS), rr = k - ci * (KS * KS), ky = rr / KS, kx = rr - ky * KS;
            const int iy = DIL ? iy0 + ky * c.dil : iy0 + ky, ix = DIL ? ix0 + kx * c.dil : ix0 + kx;
            const int ok = (int)(bp_ok & (k < c.Kdim) & (iy >= 0) & (iy < c.H) & (ix >= 0) & (ix < c.W));
            rb[j] = xb[((ci * c.H + iy) * c.W + ix) & -ok];
            okm |= (unsigned)ok << j;
        }
    };
    t_f32x4 acc[4][2];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = t_f32x4{0.f, 0.f, 0.f, 0.f};

    load(0);
    for (int k0 = 0; k0 < c.Kdim; k0 += TC_KC) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) As[a_k0 + j][a_co] = (okm >> (8 + j)) & 1u ? ra[j] : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) Bs[b_k0 + 2 * j][b_pn] = (okm >> j) & 1u ? rb[j] : 0.f;
        __syncthreads();
        if (k0 + TC_KC < c.Kdim) load(k0 + TC_KC);
#pragma unroll
        for (int ks = 0; ks < TC_KC / 4; ++ks) {
            float a[4], b[2];
#pragma unroll
            for (int m = 0; m < 4; ++m) a[m] = As[4 * ks + q][16 * m + r];
#pragma unroll
            for (int n = 0; n < 2; ++n) b[n] = Bs[4 * ks + q][32 * wave + 16 * n + r];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[n], acc[m][n], 0, 0, 0);
        }
    }
    // epilogue: lane holds couts 16m + 4q + i of pixel 32 wave + 16 n + r
    if (!PL) {
        t_tile_epilogue<2>(c, HoWo, co0, q, acc, [&](int n, int &pok) {
            const int p = p0 + 32 * wave + 16 * n + r;
            pok = (int)(p < c.P);
            const int pc = p & -pok, img = pc / HoWo, rem = pc - img * HoWo;
            return c.y + (size_t)img * c.Cout * HoWo + rem;
        });
        return;
    }
    // planes: this lane's four consecutive couts of a 16-cout tile are one 8-byte (bf16 hi, lo) / 16-byte (f32) store
    float bv[16];
    t_bias16(c, co0, q, bv);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int p = p0 + 32 * wave + 16 * n + r;
        const int pok = (int)(p < c.P);
        const int pc = p & -pok;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int co = co0 + 16 * m + 4 * q;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = acc[m][n][i] + bv[4 * m + i];
            if (!pok || co >= c.Cout) continue;
            if (PL == 2) {
                *reinterpret_cast<t_f32x4 *>((float *)c.pl + (size_t)pc * c.pl_cs + co) = t_f32x4{v[0], v[1], v[2], v[3]};
            } else {
                t_bf4 h, l;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const __bf16 hi = (__bf16)v[i];
                    h[i] = hi;
                    l[i] = (__bf16)(v[i] - (float)hi);
                }
                __bf16 *o = (__bf16 *)c.pl + (size_t)pc * c.pl_cs + co;
                *reinterpret_cast<t_bf4 *>(o) = h;
                *reinterpret_cast<t_bf4 *>(o + c.pl_split) = l;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 3x3 stride-1 convolutions (95 % of the step's FLOPs), second generation.  PMC on the gather kernel above: the texture
// addresser is as busy per CU as the matrix pipe per SIMD (TA/MFMA 1.01, MfmaUtil 28 %) -- every input element is fetched
// nine times, once per tap, four bytes per lane.  Here a block stages the HALO TILE of 16 input channels once (rows of the
// image, coalesced) plus the 9 x 16 x 64 weight slice (pre-transposed to [tap][ci][cout] by wpack_kernel, coalesced along
// cout) and runs 288 MFMAs per wave between two barriers; the nine taps are LDS address offsets.  Output tile = R rows x TW
// columns of one image, R * TW <= 128 (28-wide maps: 4 x 28, 56: 2 x 56, 112: 1 x 112).  Two blocks per CU overlap one
// block's staging with the other's MFMAs.
// ---------------------------------------------------------------------------------------------------------------------
struct TTile {
    int TW, R, tiles_x, tiles_y;   // output tile, tiles per image
    int HC, HR;                    // halo columns / rows = TW + 2, R + 2
    int CHP;                       // LDS floats per halo channel (HR * HC rounded up to = 16 mod 64: forward, = 4 mod 64: wgrad)
    int NI;                        // ceil(HR * HC / 256)
};
#define TT_AP 80
#define TT_MAXNI 2

// The block's tile (b = tile index of the grid, image-major): image, top-left output pixel, first cout
struct TBlock { int img, y0, x0, co0; };
__device__ __forceinline__ TBlock t_tile_block(const TTile &g, int b, int cblk) {
    const int tx = b % g.tiles_x, ty = (b / g.tiles_x) % g.tiles_y;
    return TBlock{b / (g.tiles_x * g.tiles_y), ty * g.R, tx * g.TW, cblk * 64};
}
// Pixel slot sl of the tile (an MFMA column; row-major, TW slots per row): hpix = the halo pixel of its top-left tap, opix = its pixel in the output plane;
// a slot beyond the tile or the map reads halo pixel 0 and has opix = -1
__device__ __forceinline__ void t_tile_slot(const TConv &c, const TTile &g, const TBlock &k, int sl, int &hpix, int &opix) {
    const int ry = sl / g.TW, rx = sl - ry * g.TW;
    const bool ok = ry < g.R && k.y0 + ry < c.Ho && k.x0 + rx < c.Wo;
    hpix = ok ? ry * g.HC + rx : 0;
    opix = ok ? (k.y0 + ry) * c.Wo + k.x0 + rx : -1;
}
// Halo element e (row-major, HC per row): its offset inside an input plane, or -1 = zero padding / beyond the halo tile
__device__ __forceinline__ int t_halo_off(const TConv &c, const TTile &g, const TBlock &k, int e) {
    const int hy = e / g.HC, hx = e - hy * g.HC;
    const int iy = k.y0 - c.pad + hy, ix = k.x0 - c.pad + hx;
    return (e < g.HR * g.HC && iy >= 0 && iy < c.H && ix >= 0 && ix < c.W) ? iy * c.W + ix : -1;
}
// the tile kernels' epilogue: slot n is pixel opix[n] of image k.img (opix < 0: unused)
template <int NT>
__device__ __forceinline__ void t_tile_epilogue(const TConv &c, const TBlock &k, int q, const t_f32x4 (&acc)[4][NT], const int (&opix)[NT]) {
    const int HoWo = c.Ho * c.Wo;
    t_tile_epilogue<NT>(c, HoWo, k.co0, q, acc, [&](int n, int &pok) {
        pok = (int)(opix[n] >= 0);
        return c.y + (size_t)k.img * c.Cout * HoWo + (opix[n] & -pok);
    });
}

// PN_PACK_TILE3 (flip: the data gradient's transposed, rotated weights), per call
__global__ void wpack3_kernel(const float *__restrict__ w, float *__restrict__ wp, int Cout, int Cin, int flip) {
    t_pack_element<PN_PACK_TILE3>(w, wp, Cout, Cin, flip, (size_t)blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256, 2) void tconv3_tile_kernel(TConv c, TTile g, const float *__restrict__ wp) {
    extern __shared__ float t_smem[];
    float *As = t_smem;                       // [9 * 16][TT_AP]   weights  (tap, channel) x cout
    float *Hs = t_smem + 144 * TT_AP;         // [16][CHP]         halo tile of 16 input channels
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    T_DECODE_TILE_CB(b, cblk);
    const TBlock k = t_tile_block(g, b, cblk);
    const int co0 = k.co0, HW = c.H * c.W;
    // this lane's two pixel slots (MFMA columns)
    int hb[2], opix[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) t_tile_slot(c, g, k, 32 * wave + 16 * n + r, hb[n], opix[n]);
    // halo elements this thread stages for every channel: offset inside the image plane (or -1 = zero padding)
    int hoff[TT_MAXNI], hdst[TT_MAXNI];
#pragma unroll
    for (int i = 0; i < TT_MAXNI; ++i) {
        const int e = t + 256 * i;
        hdst[i] = e < g.HR * g.HC ? e : -1;
        hoff[i] = t_halo_off(c, g, k, e);
    }
    const float *xb = c.x + (size_t)k.img * c.Cin * HW;
    const int a_co = t & 63, a_r0 = t >> 6;
    const bool a_ok = co0 + a_co < c.Cout;
    const float *wa = wp + (a_ok ? co0 + a_co : 0);

    t_f32x4 acc[4][2];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = t_f32x4{0.f, 0.f, 0.f, 0.f};

    // software pipeline: the global loads of chunk c0 + 16 stay in flight (in registers) under the 288 MFMAs of chunk c0, so a
    // block does not depend on its CU neighbour being in the opposite phase (co-resident blocks start together and stay in
    // lockstep: both stage, then both compute at half rate each)
    float rh[16 * TT_MAXNI];
    float rw[36];
    auto load = [&](int c0) {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const int cok = (int)(c0 + kk < c.Cin);
#pragma unroll
            for (int i = 0; i < TT_MAXNI; ++i) {
                const int ok = cok & (int)(hoff[i] >= 0);
                rh[kk * TT_MAXNI + i] = xb[((c0 + kk) * HW + hoff[i]) & -ok];
            }
        }
#pragma unroll
        for (int j = 0; j < 36; ++j) {            // row = tap * 16 + kk
            const int row = a_r0 + 4 * j, tap = row >> 4, kk = row & 15;
            const int ok = (int)(c0 + kk < c.Cin);
            rw[j] = wa[((tap * c.Cin + c0 + kk) * c.Cout) & -ok];
        }
    };
    load(0);
    for (int c0 = 0; c0 < c.Cin; c0 += 16) {
        __syncthreads();                          // the previous chunk's MFMAs have read their fragments
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
            for (int i = 0; i < TT_MAXNI; ++i)
                if (hdst[i] >= 0) Hs[kk * g.CHP + hdst[i]] = (c0 + kk < c.Cin && hoff[i] >= 0) ? rh[kk * TT_MAXNI + i] : 0.f;
#pragma unroll
        for (int j = 0; j < 36; ++j) {
            const int row = a_r0 + 4 * j;
            As[row * TT_AP + a_co] = (a_ok && c0 + (row & 15) < c.Cin) ? rw[j] : 0.f;
        }
        __syncthreads();
        if (c0 + 16 < c.Cin) load(c0 + 16);
        // 9 taps x 4 k-quads; the operands of the next step are read from LDS before the 8 MFMAs of the current one issue (the
        // compiler's own schedule was read -> s_waitcnt lgkmcnt(0) -> 4 MFMAs, every LDS latency exposed).  The tap loop is
        // NOT unrolled: fully unrolled the hoisted LDS addresses of 36 steps push the kernel past 256 VGPRs.
        float a[2][4], bb[2][2];
        auto frag = [&](int tap, int ks, float (&fa)[4], float (&fb)[2]) {
            const int ty3 = tap / 3;
            const int toff = ty3 * g.HC + (tap - 3 * ty3);
#pragma unroll
            for (int m = 0; m < 4; ++m) fa[m] = As[(tap * 16 + 4 * ks + q) * TT_AP + 16 * m + r];
#pragma unroll
            for (int n = 0; n < 2; ++n) fb[n] = Hs[(4 * ks + q) * g.CHP + hb[n] + toff];
        };
        frag(0, 0, a[0], bb[0]);
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                if (ks < 3) frag(tap, ks + 1, a[(ks + 1) & 1], bb[(ks + 1) & 1]);
                else frag(tap < 8 ? tap + 1 : 8, 0, a[0], bb[0]);           // (the last one re-reads tap 8: harmless)
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks & 1][m], bb[ks & 1][n], acc[m][n], 0, 0, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);      // next step's 6 LDS reads ...
                __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);      // ... then this step's 8 MFMAs
            }
        }
    }
    t_tile_epilogue<2>(c, k, q, acc, opix);
}

// ---------------------------------------------------------------------------------------------------------------------
// The same 3x3 tile convolution on the bf16 matrix instruction with SPLIT operands ("bf16x3", opt-in through
// pn_train_set_precision): every fp32 value v is staged as hi = bf16(v), lo = bf16(v - hi) (16 mantissa bits together) and
// a product sum is hi*hi + hi*lo + lo*hi in fp32 accumulators (the dropped lo*lo term is 2^-16 relative) -- three
// v_mfma_f32_16x16x32_bf16 (16 cycles each, K = 32) do the work of eight v_mfma_f32_16x16x4_f32 (32 cycles each): 5.3x less
// matrix-pipe time for fp32-class results.  Chunks of 32 input channels; LDS images are [row][32 channels] bf16 with an
// 80-byte pitch (16-byte fragment reads and 16-byte staging writes both conflict-free); the weight slice is staged one
// kernel row (3 taps) at a time.
// Two kernels: tconv3_tile_x3_kernel (64 couts x 128 pixel slots per block, rows at the 80-byte pitch) and the wide tconv3_tile_x3w_kernel
// (64 couts x 256 slots, swizzled 64-byte rows).  They share the staging below and differ through the row-address functor and the tile count.
// ---------------------------------------------------------------------------------------------------------------------
#define TX_PITCH 80                     // bytes per [32 x bf16] row
#define TX_A_BYTES (3 * 64 * TX_PITCH)  // one plane of the weight slice of one kernel row
#define TXW2_PITCH 64                   // the wide kernel's
#define TXW2_A_BYTES (3 * 64 * TXW2_PITCH)
// LDS byte address of 16-byte segment seg (8 channels) of row `row`, as a functor passed by value
struct TXRows80 {
    __device__ __forceinline__ int operator()(int row, int seg) const { return row * TX_PITCH + 16 * seg; }
};
// 64-byte pitch with the segment XOR-swizzled by (row >> 2) & 3: sixteen consecutive rows x one segment cover sixteen different 16-byte bank groups, for the
// staging stores and for both operands' fragment reads
struct TXRowsSwz {
    __device__ __forceinline__ int operator()(int row, int seg) const { return row * TXW2_PITCH + 16 * (seg ^ ((row >> 2) & 3)); }
};

// PN_PACK_TILE3_X3, per call: the weights in the LDS image's own order, so that staging a kernel row is six 16-byte copies per thread instead of 24 dword
// loads + the split arithmetic per thread
__global__ void wpack3_x3_kernel(const float *__restrict__ w, __bf16 *__restrict__ wpx, int Cout, int Cin, int flip) {
    t_pack_element<PN_PACK_TILE3_X3>(w, wpx, Cout, Cin, flip, (size_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// Every cached pack of a context refreshed by ONE launch (pn_train_pack_refresh): the block finds its descriptor (<= ~130 entries, bisected by
// every thread: uniform) and writes its 256 elements of that pack -- t_pack_element, as the per-call pack kernels.
struct TPackDesc { const float *w; void *dst; int Cout, Cin, flip; PnPackKind kind; unsigned first_block, pad; };
__global__ void wpack_all_kernel(const TPackDesc *__restrict__ tab, int n) {
    int e = 0, hi = n - 1;          // the last entry whose first block is <= this one (first_block ascends strictly); A2J's bf16x3 step has ~130 entries: bisect
    while (e < hi) {
        const int mid = (e + hi + 1) >> 1;
        if (blockIdx.x >= tab[mid].first_block) e = mid;
        else hi = mid - 1;
    }
    const TPackDesc d = tab[e];
    const size_t i = (size_t)(blockIdx.x - d.first_block) * blockDim.x + threadIdx.x;
    switch (d.kind) {
    case PN_PACK_C1_X3: t_pack_element<PN_PACK_C1_X3>(d.w, d.dst, d.Cout, d.Cin, d.flip, i); break;
    case PN_PACK_TILE3_X3: t_pack_element<PN_PACK_TILE3_X3>(d.w, d.dst, d.Cout, d.Cin, d.flip, i); break;
    default: t_pack_element<PN_PACK_TILE3>(d.w, d.dst, d.Cout, d.Cin, d.flip, i);
    }
}

// Weight staging role of a thread: per kernel row 3 taps x 64 couts x 4 segments of 8 channels x 2 planes = 1536 16-byte pieces, 6 per thread
struct TXPiece { int pl, kx, co, seg; };
__device__ __forceinline__ TXPiece t_x3_piece(int t, int j) {
    const int piece = t + 256 * j;                    // < 1536: plane, kx, cout, segment
    const int pl = piece / 768, rem = piece - pl * 768;
    return TXPiece{pl, rem >> 8, (rem >> 2) & 63, rem & 3};
}
// the thread's pieces of (chunk wc0 / 32, kernel row wky), from the packed planes into registers
__device__ __forceinline__ void t_x3_load_w(const TConv &c, const __bf16 *__restrict__ wpx, int co0, int t, int wc0, int wky, t_u32x4 (&wv)[6]) {
    const size_t wplane = t_pack_elems(PN_PACK_TILE3_X3, c.Cout, c.Cin);
    const __bf16 *wrow = wpx + ((size_t)(wc0 >> 5) * 9 + wky * 3) * c.Cout * 32;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const TXPiece p = t_x3_piece(t, j);
        const int ok = (int)(co0 + p.co < c.Cout);
        const size_t off = ((size_t)p.pl * wplane + ((size_t)p.kx * c.Cout + (size_t)((co0 + p.co) & -ok)) * 32 + p.seg * 8);
        wv[j] = *reinterpret_cast<const t_u32x4 *>(wrow + off);       // (rows beyond Cout read row 0: zeroed when the piece is stored -- a select here would wait for the load)
    }
}
// ... and from the registers into the slice [3 taps][64 couts][32 ch] of each plane: straight 16-byte copies
template <class Rows>
__device__ __forceinline__ void t_x3_store_w(const TConv &c, int co0, int t, const t_u32x4 (&wv)[6], unsigned char *As_hi, unsigned char *As_lo, Rows rows) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const TXPiece p = t_x3_piece(t, j);
        *reinterpret_cast<t_u32x4 *>((p.pl ? As_lo : As_hi) + rows(p.kx * 64 + p.co, p.seg)) = co0 + p.co < c.Cout ? wv[j] : t_u32x4{0u, 0u, 0u, 0u};
    }
}
// The weights are fetched one (chunk, kernel row) step AHEAD (round 5): the loads of the step after (c0, ky) are in flight under this step's MFMAs instead
// of in front of them -- three of a chunk's five exposed memory round trips gone.  ONE call site, always taken (past the last step: the current slice again,
// unused): two conditional sites merged the loaded registers through copies that waited for the loads right there.
__device__ __forceinline__ void t_x3_next_w(const TConv &c, const __bf16 *__restrict__ wpx, int co0, int t, int c0, int ky, t_u32x4 (&wv)[6]) {
    const int nc0 = ky == 2 ? c0 + 32 : c0, nky = ky == 2 ? 0 : ky + 1;
    const bool more = nc0 < c.Cin;
    t_x3_load_w(c, wpx, co0, t, more ? nc0 : c0, more ? nky : ky, wv);
}
// Halo staging role: a wave stages channels cbase = c0 + 8 wave .. + 7 (cmask: those below Cin) of halo pixels lane + 64 i.  Pixels i = I0 .. I1 - 1: all
// loads first, then -- SYNC: behind the barrier after which the previous chunk's last kernel row has been consumed -- split + two 16-byte stores per pixel.
template <int I0, int I1, bool SYNC, class Rows, int NH>
__device__ __forceinline__ void t_x3_stage_halo(const float *__restrict__ xb, int HW, int nhalo, const int (&hoff)[NH], int cbase, unsigned cmask, int lane,
                                                int wave, unsigned char *Hs_hi, unsigned char *Hs_lo, Rows rows) {
    float hv[I1 - I0][8];
#pragma unroll
    for (int i = I0; i < I1; ++i) {
        const int okp = (int)(hoff[i] >= 0);
#pragma unroll
        for (int j = 0; j < 8; ++j) hv[i - I0][j] = xb[((cbase + j) * HW + hoff[i]) & -(okp & (int)((cmask >> j) & 1u))];
    }
    if (SYNC) __syncthreads();
#pragma unroll
    for (int i = I0; i < I1; ++i) {
        const int e = lane + 64 * i;
        if (e < nhalo) {
            t_bf16x8 hi, lo;
            t_split8(hv[i - I0], hoff[i] >= 0 ? cmask : 0u, hi, lo);
            *reinterpret_cast<t_bf16x8 *>(Hs_hi + rows(e, wave)) = hi;
            *reinterpret_cast<t_bf16x8 *>(Hs_lo + rows(e, wave)) = lo;
        }
    }
}
__device__ __forceinline__ unsigned t_x3_chan_mask(const TConv &c, int cbase) {
    unsigned cmask = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) cmask |= (unsigned)(cbase + j < c.Cin) << j;
    return cmask;
}

__global__ __launch_bounds__(256, 2) void tconv3_tile_x3_kernel(TConv c, TTile g, const __bf16 *__restrict__ wpx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char t_smem8[];
    unsigned char *As_hi = t_smem8, *As_lo = t_smem8 + TX_A_BYTES;          // [3 taps][64 couts][32 ch]
    unsigned char *Hs_hi = t_smem8 + 2 * TX_A_BYTES;                        // [halo pixel][32 ch]
    unsigned char *Hs_lo = Hs_hi + g.HR * g.HC * TX_PITCH;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    T_DECODE_TILE_CB(b, cblk);
    const TBlock k = t_tile_block(g, b, cblk);
    const int co0 = k.co0, HW = c.H * c.W, nhalo = g.HR * g.HC;
    const TXRows80 rows;
    int hb[2], opix[2];                         // LDS byte offset of the slot's top-left tap (this lane's segment q), output pixel (or -1)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        t_tile_slot(c, g, k, 32 * wave + 16 * n + r, hb[n], opix[n]);
        hb[n] = rows(hb[n], q);
    }
    constexpr int NH = 5;               // ceil(320 / 64): halo tiles have at most (2 + 2) x (64 + 2) = 264 pixels
    int hoff[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) hoff[i] = t_halo_off(c, g, k, lane + 64 * i);
    const float *xb = c.x + (size_t)k.img * c.Cin * HW;

    t_f32x4 acc[4][2];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = t_f32x4{0.f, 0.f, 0.f, 0.f};

    t_u32x4 wv[6];                                     // the NEXT (chunk, kernel row) step's weight pieces of this thread
    t_x3_load_w(c, wpx, co0, t, 0, 0, wv);

    for (int c0 = 0; c0 < c.Cin; c0 += 32) {
        const int cbase = c0 + 8 * wave;
        t_x3_stage_halo<0, NH, true>(xb, HW, nhalo, hoff, cbase, t_x3_chan_mask(c, cbase), lane, wave, Hs_hi, Hs_lo, rows);
        for (int ky = 0; ky < 3; ++ky) {
            if (ky) __syncthreads();                  // the previous kernel row's fragments have been read
            t_x3_store_w(c, co0, t, wv, As_hi, As_lo, rows);
            __syncthreads();
            t_x3_next_w(c, wpx, co0, t, c0, ky, wv);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int toff = (ky * g.HC + kx) * TX_PITCH;
                t_bf16x8 bh[2], bl[2];
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    bh[n] = *reinterpret_cast<const t_bf16x8 *>(Hs_hi + hb[n] + toff);
                    bl[n] = *reinterpret_cast<const t_bf16x8 *>(Hs_lo + hb[n] + toff);
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int ao = rows(kx * 64 + 16 * m + r, q);
                    const t_bf16x8 ah = *reinterpret_cast<const t_bf16x8 *>(As_hi + ao);
                    const t_bf16x8 al = *reinterpret_cast<const t_bf16x8 *>(As_lo + ao);
#pragma unroll
                    for (int n = 0; n < 2; ++n) t_mfma_x3(acc[m][n], ah, al, bh[n], bl[n]);
                }
            }
        }
    }
    t_tile_epilogue<2>(c, k, q, acc, opix);
}

// Wide variant: 64 couts x 256 pixel slots per block, a wave owns 64 couts x 64 pixels (4 x 4 MFMA tiles): per tap 8 + 8 fragment
// reads feed 48 MFMAs (the 128-slot kernel above: 8 + 4 for 24) and a block's packed weight slice -- the larger part of its
// vector-memory bytes -- serves twice the pixels.  LDS images at TXRowsSwz's swizzled 64-byte pitch: two blocks still fit a CU (76 KB).
__global__ __launch_bounds__(256, 2) void tconv3_tile_x3w_kernel(TConv c, TTile g, const __bf16 *__restrict__ wpx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char t_smem8[];
    unsigned char *As_hi = t_smem8, *As_lo = t_smem8 + TXW2_A_BYTES;
    unsigned char *Hs_hi = t_smem8 + 2 * TXW2_A_BYTES;
    unsigned char *Hs_lo = Hs_hi + g.HR * g.HC * TXW2_PITCH;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    T_DECODE_TILE_CB(b, cblk);
    const TBlock k = t_tile_block(g, b, cblk);
    const int co0 = k.co0, HW = c.H * c.W, nhalo = g.HR * g.HC;
    const TXRowsSwz rows;
    int hbp[4], opix[4];                        // halo pixel of the slot's top-left tap, output pixel (or -1)
#pragma unroll
    for (int n = 0; n < 4; ++n) t_tile_slot(c, g, k, 64 * wave + 16 * n + r, hbp[n], opix[n]);
    constexpr int NH = 7;                       // halo tiles have at most 400 pixels (t_tile_geometry_x3w)
    int hoff[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) hoff[i] = t_halo_off(c, g, k, lane + 64 * i);
    const float *xb = c.x + (size_t)k.img * c.Cin * HW;

    t_f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = t_f32x4{0.f, 0.f, 0.f, 0.f};

    t_u32x4 wv[6];                                     // the NEXT (chunk, kernel row) step's weight pieces of this thread
    t_x3_load_w(c, wpx, co0, t, 0, 0, wv);

    for (int c0 = 0; c0 < c.Cin; c0 += 32) {
        const int cbase = c0 + 8 * wave;
        const unsigned cmask = t_x3_chan_mask(c, cbase);
        // halo of 32 channels, in two halves of the pixel range (56 prefetch registers would not fit next to 64 accumulators)
        t_x3_stage_halo<0, 4, true>(xb, HW, nhalo, hoff, cbase, cmask, lane, wave, Hs_hi, Hs_lo, rows);
        t_x3_stage_halo<4, NH, false>(xb, HW, nhalo, hoff, cbase, cmask, lane, wave, Hs_hi, Hs_lo, rows);
#pragma unroll 1
        for (int ky = 0; ky < 3; ++ky) {
            if (ky) __syncthreads();
            t_x3_store_w(c, co0, t, wv, As_hi, As_lo, rows);
            __syncthreads();
            t_x3_next_w(c, wpx, co0, t, c0, ky, wv);
#pragma unroll 1
            for (int kx = 0; kx < 3; ++kx) {          // not unrolled: with three taps' fragments hoisted the kernel spills (124 B / lane)
                t_bf16x8 bh[4], bl[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int o = rows(hbp[n] + ky * g.HC + kx, q);
                    bh[n] = *reinterpret_cast<const t_bf16x8 *>(Hs_hi + o);
                    bl[n] = *reinterpret_cast<const t_bf16x8 *>(Hs_lo + o);
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int ao = rows(kx * 64 + 16 * m + r, q);
                    const t_bf16x8 ah = *reinterpret_cast<const t_bf16x8 *>(As_hi + ao);
                    const t_bf16x8 al = *reinterpret_cast<const t_bf16x8 *>(As_lo + ao);
#pragma unroll
                    for (int n = 0; n < 4; ++n) t_mfma_x3(acc[m][n], ah, al, bh[n], bl[n]);
                }
            }
        }
    }
    t_tile_epilogue<4>(c, k, q, acc, opix);
}

// Weights for the data gradient: Wt[ci][(co, ky', kx')] = W[co][ci][KS-1-ky'][KS-1-kx']
__global__ void wflip_kernel(const float *__restrict__ w, float *__restrict__ wt, int Cout, int Cin, int KS) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int KK = KS * KS, total = Cout * Cin * KK;
    if (i >= total) return;
    const int ci = i / (Cout * KK), rem = i - ci * Cout * KK, co = rem / KK, rr = rem - co * KK;
    wt[i] = w[((size_t)co * Cin + ci) * KK + (KK - 1 - rr)];
}

// ---------------------------------------------------------------------------------------------------------------------
// The planes training engine's stem forward (round 6, late): model0.conv1 = 7x7 / 2, ONE input channel, 64 couts, on the same fp32 MFMA with the same
// k order as tconv_fwd_kernel<7> (k = tap, four taps per v_mfma_f32_16x16x4_f32, k-steps in order: bit-identical), without that kernel's staging: it
// gathers the [k][pixel] operand element by element for every 16-tap chunk and restages the weights per chunk (13.7 vector instructions per MFMA by
// SQ_INSTS_VALU / SQ_INSTS_MFMA, 82 us at the head of the step).  With one input channel the operand of tap (ky, kx) IS the input image shifted by
// (ky, kx): a block stages the 21 x 37 input patch of an 8 x 16 output tile once and every lane reads its B value at  base(pixel) + offset(tap)  --
// thirteen per-lane tap offsets for the whole kernel; the 64 x 49 weight matrix is 52 A-fragment registers per lane, loaded once per block, and a
// block walks tiles (two blocks per CU).  Alone 73 -> 41 us; beside the weight packs at the head of the step 82 -> 56 us.
// ---------------------------------------------------------------------------------------------------------------------
template <int F32>
__global__ __launch_bounds__(256) void tstem_fwd_kernel(TConv c, int tiles_x, int tiles_y, int ntiles) {
    constexpr int TR = 8, TC = 16, IR = (TR - 1) * 2 + 7, IC = (TC - 1) * 2 + 7;      // output tile, input patch (21 x 37)
    __shared__ float img[IR * IC];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    float a[4][13];
    int tapoff[13];
#pragma unroll
    for (int s = 0; s < 13; ++s) {
        const int k = 4 * s + q;
        const bool ok = k < 49;
        tapoff[s] = ok ? (k / 7) * IC + (k % 7) : 0;          // (a padding tap multiplies a zero weight with the patch's own first element)
#pragma unroll
        for (int m = 0; m < 4; ++m) a[m][s] = ok ? c.w[(16 * (r >> 2) + 4 * m + (r & 3)) * 49 + k] : 0.f;      // row r of tile m = cout 16 (r >> 2) + 4 m + (r & 3): a lane's sixteen accumulators are couts 16 q ..+15
    }
    const int base0 = (2 * (2 * wave)) * IC + 2 * r, base1 = base0 + 2 * IC;      // this wave's two output rows of the tile, pixel column r
    // the patch of tile n + 1 is fetched (four values per thread, all four loads in flight) while tile n runs: a block's round trip to the input is never exposed
    // (the first form fetched and stored them one after the other at the head of the tile: four dependent round trips, 60 us for 17 us of MFMA work)
    constexpr int NS = (IR * IC + 255) / 256;
    float sv[NS];
    unsigned sok = 0;
    auto fetch = [&](int tile) {
        const int b = tile / (tiles_x * tiles_y), rem = tile - b * (tiles_x * tiles_y), ty = rem / tiles_x, tx = rem - ty * tiles_x;
        const int iy0 = ty * TR * 2 - 3, ix0 = tx * TC * 2 - 3;
        const float *xb = c.x + (size_t)b * c.H * c.W;
        sok = 0;
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const int i = t + 256 * u, rr = i / IC, cc = i - rr * IC, iy = iy0 + rr, ix = ix0 + cc;
            const bool ok = i < IR * IC && (unsigned)iy < (unsigned)c.H && (unsigned)ix < (unsigned)c.W;
            sv[u] = xb[ok ? iy * c.W + ix : 0];
            sok |= (unsigned)ok << u;
        }
    };
    if ((int)blockIdx.x < ntiles) fetch(blockIdx.x);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = tile / (tiles_x * tiles_y), rem = tile - b * (tiles_x * tiles_y), ty = rem / tiles_x, tx = rem - ty * tiles_x;
        const int oy0 = ty * TR, ox0 = tx * TC;
        __syncthreads();                                       // the previous tile's reads are done
#pragma unroll
        for (int u = 0; u < NS; ++u)
            if (t + 256 * u < IR * IC) img[t + 256 * u] = (sok >> u) & 1u ? sv[u] : 0.f;
        __syncthreads();
        fetch(min(tile + (int)gridDim.x, ntiles - 1));         // (unconditional: a straight-line loop body keeps the compiler's wait counts exact)
        t_f32x4 acc[4][2];
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m][0] = acc[m][1] = t_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 13; ++s) {
            const float b0 = img[base0 + tapoff[s]], b1 = img[base1 + tapoff[s]];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][s], b0, acc[m][0], 0, 0, 0);
                acc[m][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][s], b1, acc[m][1], 0, 0, 0);
            }
        }
        // lane holds couts 16 q + 4 m + i of pixel (row 2 wave + n, column r): 32 contiguous bytes per plane, the four q lanes of a pixel one 128-byte line
        // (with the natural row order -- couts 16 m + 4 q + i -- a line was written by four 8-byte stores per lane quartet: 76 us, as slow as the gather kernel)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int oy = oy0 + 2 * wave + n, ox = ox0 + r;
            if (oy >= c.Ho || ox >= c.Wo) continue;
            const size_t p = ((size_t)b * c.Ho + oy) * c.Wo + ox;
            float v[16];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int i = 0; i < 4; ++i) v[4 * m + i] = acc[m][n][i] + 0.f;          // (tconv_fwd_kernel adds its zero bias: -0 becomes +0 there as well)
            if (F32) {
                float *o = (float *)c.pl + p * c.pl_cs + 16 * q;
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<t_f32x4 *>(o + 4 * j) = t_f32x4{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
            } else {
                t_bf16x8 h[2], l[2];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const __bf16 hi = (__bf16)v[j];
                    h[j >> 3][j & 7] = hi;
                    l[j >> 3][j & 7] = (__bf16)(v[j] - (float)hi);
                }
                __bf16 *o = (__bf16 *)c.pl + p * c.pl_cs + 16 * q;
                *reinterpret_cast<t_bf16x8 *>(o) = h[0];
                *reinterpret_cast<t_bf16x8 *>(o + 8) = h[1];
                *reinterpret_cast<t_bf16x8 *>(o + c.pl_split) = l[0];
                *reinterpret_cast<t_bf16x8 *>(o + c.pl_split + 8) = l[1];
            }
        }
    }
}
