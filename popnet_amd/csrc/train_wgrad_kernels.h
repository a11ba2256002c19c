// Weight-gradient kernels of the NCHW training engine (train.hip).  Every kernel writes per-slice partial sums that
// wgrad_reduce_kernel adds in slice order: deterministic, no atomics.
//   tconv_wgrad_kernel<KS>         any kernel size / stride, fp32 MFMA, slices of pixels
//   tconv3_wgrad_tile_kernel       3x3 stride 1 on halo tiles, fp32 MFMA, slices of tiles
//   tconv3_wgrad_x3 / _x3pp / _x3v_kernel   the same on split-bf16 MFMA ("bf16x3"): one group, two groups ping-ponging, vectorised staging
//   tstem_wgrad_kernel             the planes engine's stem (trainx.hip), dY from a planes tensor
// The launches, the geometry functions and the planners are in train.hip.
#pragma once
#include "train_conv_kernels.h"


// Weight gradient of the 3x3 stride-1 convolutions on the same tiles: a block owns 64 couts x (16 input channels x 9 taps) and
// walks a slice of the output tiles; per tile it stages dY [128 pixel slots][64 couts] and the halo tile of its 16 input
// channels, then 32 pixel groups x 9 taps = 288 MFMAs per wave (A = dY: row = cout, k = pixel; B = X: k = pixel, column =
// channel, one 16-column MFMA tile per tap, the tap again an LDS address offset).  Partials per slice, reduced in order.
#define TT_YP 81      // = 17 (mod 64): conflict-free pixel-major writes, near conflict-free (q * 17 + r) MFMA operand reads
#define TT_HP 17      // halo tile of the weight gradient is PIXEL-major: [halo pixel][16 channels + 1]
__global__ __launch_bounds__(256, 2) void tconv3_wgrad_tile_kernel(TConv c, TTile g, float *__restrict__ partial, int tiles_per_slice, int ntiles) {
    extern __shared__ float t_smem[];
    float *Ys = t_smem;                         // [128][TT_YP]   dY tile, pixel-major
    float *Hs = t_smem + 128 * TT_YP;           // [HR * HC][TT_HP]  halo tile of this block's 16 input channels, pixel-major
    int *hbt = (int *)(Hs + g.HR * g.HC * TT_HP);   // [128]       pixel slot -> halo pixel of its top-left tap
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    T_DECODE_XYZ(bx_, by_, slice);
    const int c0 = bx_ * 16, co0 = by_ * 64;
    const int HW = c.H * c.W, HoWo = c.Ho * c.Wo;
    // per-thread constants of the staging: the dY slot and the halo elements (same for every tile up to the tile origin)
    const int sl = t & 127, ry = sl / g.TW, rx = sl - ry * g.TW, y_c0 = t >> 7;
    int hy[TT_MAXNI], hx[TT_MAXNI], hdst[TT_MAXNI];
#pragma unroll
    for (int i = 0; i < TT_MAXNI; ++i) {
        const int e = t + 256 * i;
        hy[i] = e / g.HC;
        hx[i] = e - hy[i] * g.HC;
        hdst[i] = e < g.HR * g.HC ? e : -1;
    }
    t_f32x4 acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = t_f32x4{0.f, 0.f, 0.f, 0.f};
    const int tbeg = slice * tiles_per_slice, tend = min(tbeg + tiles_per_slice, ntiles);
    for (int tile = tbeg; tile < tend; ++tile) {
        const int tx = tile % g.tiles_x, ty = (tile / g.tiles_x) % g.tiles_y, img = tile / (g.tiles_x * g.tiles_y);
        const int y0 = ty * g.R, x0 = tx * g.TW;
        const bool sok = ry < g.R && y0 + ry < c.Ho && x0 + rx < c.Wo;
        const float *dyb = c.y + (size_t)img * c.Cout * HoWo + (sok ? (y0 + ry) * c.Wo + x0 + rx : 0);
        const float *xb = c.x + (size_t)img * c.Cin * HW;
        float rd[32], rh[16 * TT_MAXNI];
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int co = co0 + y_c0 + 2 * j;
            rd[j] = dyb[(co * HoWo) & -(int)(sok & (co < c.Cout))];
        }
        int hoff[TT_MAXNI];
#pragma unroll
        for (int i = 0; i < TT_MAXNI; ++i) {
            const int iy = y0 - c.pad + hy[i], ix = x0 - c.pad + hx[i];
            hoff[i] = (hdst[i] >= 0 && iy >= 0 && iy < c.H && ix >= 0 && ix < c.W) ? iy * c.W + ix : -1;
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
            for (int i = 0; i < TT_MAXNI; ++i) {
                const int ok = (int)(c0 + kk < c.Cin) & (int)(hoff[i] >= 0);
                rh[kk * TT_MAXNI + i] = xb[((c0 + kk) * HW + hoff[i]) & -ok];
            }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int co = co0 + y_c0 + 2 * j;
            Ys[sl * TT_YP + y_c0 + 2 * j] = (sok && co < c.Cout) ? rd[j] : 0.f;
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
            for (int i = 0; i < TT_MAXNI; ++i)
                if (hdst[i] >= 0) Hs[hdst[i] * TT_HP + kk] = (c0 + kk < c.Cin && hoff[i] >= 0) ? rh[kk * TT_MAXNI + i] : 0.f;
        if (t < 128) hbt[t] = sok ? ry * g.HC + rx : 0;
        __syncthreads();
#pragma unroll 4
        for (int pg = 0; pg < 32; ++pg) {
            const float a = Ys[(4 * pg + q) * TT_YP + 16 * wave + r];
            const int hb = hbt[4 * pg + q] * TT_HP + r;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
                acc[tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Hs[hb + ((tap / 3) * g.HC + (tap % 3)) * TT_HP], acc[tap], 0, 0, 0);
        }
    }
    float *pb = partial + (size_t)slice * c.Cout * c.Kdim;
    if (c0 + r < c.Cin) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = co0 + 16 * wave + 4 * q + i;
                if (co < c.Cout) pb[((size_t)co * c.Cin + c0 + r) * 9 + tap] = acc[tap][i];
            }
    }
}

// Weight gradient on split-bf16 MFMA.  k = pixels, so the X operand of tap (ky, kx) is the channel-major halo row shifted by kx
// ELEMENTS -- not a 16-byte-aligned fragment.  The halo rows are laid out so that every 8-slot pixel group starts 16-byte
// aligned (slots per tile row rounded up to a multiple of 8, halo column 0 = image column x0 - 1); a lane reads the aligned
// group plus the next dword once per (ky, plane) and builds the kx = 1 fragment with four v_alignbyte and the kx = 2 one by
// renaming registers.  Block = 64 couts x (16 input channels x 9 taps), 4 pixel groups of 32 slots per tile.
struct TTileW {
    int TW, SW, R, tiles_x, tiles_y;    // live columns, slots per tile row (multiple of 8), rows
    int HP, HR;                         // halo row pitch in elements (SW + 8), halo rows (R + 2)
    int CHB;                            // bytes per halo channel
};
#define TXW_YP 272                      // bytes per dY row: 128 slots x bf16 + 16

__device__ __forceinline__ t_bf16x8 t_as_bf16x8(t_u32x4 v) {
    union { t_u32x4 u; t_bf16x8 b; } x;
    x.u = v;
    return x.b;
}

#define TXW_CI 32                       // input channels per block (two 16-column MFMA tiles per tap)

// ---- building blocks of the x3 family; each kernel below is its phase structure around them ----
// One LDS image set: dY tile [64 couts][128 slots] and halo [32 channels][HR][HP], a hi and a lo plane each.
struct TXwSet { unsigned char *Yh, *Yl, *Xh, *Xl; };
__device__ __forceinline__ int t_xw_set_bytes(const TTileW &g) { return 2 * 64 * TXW_YP + 2 * TXW_CI * g.CHB; }
__device__ __forceinline__ TXwSet t_xw_set(unsigned char *base, const TTileW &g) {
    TXwSet s;
    s.Yh = base; s.Yl = base + 64 * TXW_YP;
    s.Xh = base + 2 * 64 * TXW_YP; s.Xl = s.Xh + TXW_CI * g.CHB;
    return s;
}

__device__ __forceinline__ void t_xw_origin(const TTileW &g, int tile, int &img, int &y0, int &x0) {
    const int tx = tile % g.tiles_x, ty = (tile / g.tiles_x) % g.tiles_y;
    img = tile / (g.tiles_x * g.tiles_y);
    y0 = ty * g.R;
    x0 = tx * g.TW;
}

// dY tile staging.  Thread t of the group: slot pair (2 sp, 2 sp + 1) = row ry_a, column rx_a of the tile, couts wave + 4 j.
// t_xw_dy_load issues the 2 x 16 loads, t_xw_dy_store splits them and writes one 4-byte LDS word per plane and pair; a kernel
// puts its barrier, if it needs one, between the two.
struct TXwDy { float d0[16], d1[16]; int ok0, ok1; };
__device__ __forceinline__ void t_xw_dy_load(const TConv &c, const TTileW &g, int tile, int co0, int t, int ry_a, int rx_a, TXwDy &d) {
    const int wave = t >> 6, HoWo = c.Ho * c.Wo;
    int img, y0, x0;
    t_xw_origin(g, tile, img, y0, x0);
    const bool rowok = ry_a < g.R && y0 + ry_a < c.Ho;
    d.ok0 = (int)(rowok && rx_a < g.TW && x0 + rx_a < c.Wo);
    d.ok1 = (int)(rowok && rx_a + 1 < g.TW && x0 + rx_a + 1 < c.Wo);
    const float *dyb = c.y + (size_t)img * c.Cout * HoWo + (rowok ? (y0 + ry_a) * c.Wo + x0 + rx_a : 0);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int co = co0 + wave + 4 * j;
        const int cok = (int)(co < c.Cout);
        d.d0[j] = dyb[(co * HoWo) & -(d.ok0 & cok)];
        d.d1[j] = dyb[(co * HoWo + 1) & -(d.ok1 & cok)];
    }
}
__device__ __forceinline__ void t_xw_dy_store(const TConv &c, const TXwSet &s, int co0, int t, const TXwDy &d) {
    const int wave = t >> 6, sp = t & 63;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int co = co0 + wave + 4 * j;
        const float v0 = (d.ok0 && co < c.Cout) ? d.d0[j] : 0.f, v1 = (d.ok1 && co < c.Cout) ? d.d1[j] : 0.f;
        const __bf16 h0 = (__bf16)v0, h1 = (__bf16)v1;
        const __bf16 l0 = (__bf16)(v0 - (float)h0), l1 = (__bf16)(v1 - (float)h1);
        union { __bf16 b[2]; unsigned u; } ph, pl;
        ph.b[0] = h0; ph.b[1] = h1; pl.b[0] = l0; pl.b[1] = l1;
        *reinterpret_cast<unsigned *>(s.Yh + (wave + 4 * j) * TXW_YP + 4 * sp) = ph.u;
        *reinterpret_cast<unsigned *>(s.Yl + (wave + 4 * j) * TXW_YP + 4 * sp) = pl.u;
    }
}

// Halo staging.  Thread t of the group: channel hk = t >> 3, elements (t & 7) + 8 i.
__device__ __forceinline__ void t_xw_halo_stage(const TConv &c, const TTileW &g, const TXwSet &s, int tile, int c0, int t) {
    const int hk = t >> 3, he0 = t & 7;
    const int hk_ok = (int)(c0 + hk < c.Cin);
    const int HW = c.H * c.W, nh = g.HR * g.HP;
    int img, y0, x0;
    t_xw_origin(g, tile, img, y0, x0);
    const float *xb = c.x + (size_t)img * c.Cin * HW + (size_t)(hk_ok ? c0 + hk : 0) * HW;
    // halo of channel hk, element PAIRS (2 e, 2 e + 1), e = he0 + 8 i: one 4-byte LDS store per plane and pair (2-byte stores
    // of neighbouring lanes into one bank word serialise: 64 % LDS conflict cycles in the first version); HP is even, so a
    // pair never straddles a halo row; (row, column) advance without a division; 3 pairs = 6 loads in flight (all 36
    // loads at once spilled: 22.9 instead of 17.2 ms per step)
    int hy = 0, hx = 2 * he0;
    const int iy0 = y0 - c.pad, ix0 = x0 - c.pad;
    while (hx >= g.HP) { hx -= g.HP; ++hy; }
    for (int e0 = 2 * he0; e0 < nh; e0 += 48) {
        float hv[6];
        int okv[6];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int iy = iy0 + hy, ix = ix0 + hx;
            const int rowok = hk_ok & (int)(e0 + 16 * i < nh) & (int)(iy >= 0) & (int)(iy < c.H);
            okv[2 * i] = rowok & (int)(hx < g.TW + 2) & (int)(ix >= 0) & (int)(ix < c.W);
            okv[2 * i + 1] = rowok & (int)(hx + 1 < g.TW + 2) & (int)(ix + 1 >= 0) & (int)(ix + 1 < c.W);
            hv[2 * i] = xb[(iy * c.W + ix) & -okv[2 * i]];
            hv[2 * i + 1] = xb[(iy * c.W + ix + 1) & -okv[2 * i + 1]];
            hx += 16;
            while (hx >= g.HP) { hx -= g.HP; ++hy; }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int e = e0 + 16 * i;
            if (e < nh) {
                const float v0 = okv[2 * i] ? hv[2 * i] : 0.f, v1 = okv[2 * i + 1] ? hv[2 * i + 1] : 0.f;
                const __bf16 h0 = (__bf16)v0, h1 = (__bf16)v1;
                union { __bf16 b[2]; unsigned u; } ph, pl;
                ph.b[0] = h0; ph.b[1] = h1;
                pl.b[0] = (__bf16)(v0 - (float)h0); pl.b[1] = (__bf16)(v1 - (float)h1);
                *reinterpret_cast<unsigned *>(s.Xh + hk * g.CHB + 2 * e) = ph.u;
                *reinterpret_cast<unsigned *>(s.Xl + hk * g.CHB + 2 * e) = pl.u;
            }
        }
    }
}

// byte offset (inside a channel's halo) of this lane's 8-slot group, per pixel group
__device__ __forceinline__ void t_xw_frag_offsets(const TTileW &g, int q, int (&hbq)[4]) {
#pragma unroll
    for (int pg = 0; pg < 4; ++pg) {
        const int s0 = 32 * pg + 8 * q, ry = s0 / g.SW, rx0 = s0 - ry * g.SW;
        hbq[pg] = (ry < g.R ? ry * g.HP + rx0 : 0) * 2;
    }
}

// The MFMAs of one staged image set: 4 pixel groups x 2 channel tiles x 3 kernel rows, per tap hi*hi, hi*lo, lo*hi.
__device__ __forceinline__ void t_xw_mfma_set(const TTileW &g, const TXwSet &s, const int (&hbq)[4], int wave, int q, int r, t_f32x4 (&acc)[2][9]) {
#pragma unroll
    for (int pg = 0; pg < 4; ++pg) {
        const int ao = (16 * wave + r) * TXW_YP + 64 * pg + 16 * q;
        const t_bf16x8 ah = *reinterpret_cast<const t_bf16x8 *>(s.Yh + ao), al = *reinterpret_cast<const t_bf16x8 *>(s.Yl + ao);
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int bo = (16 * n + r) * g.CHB + hbq[pg] + ky * g.HP * 2;
                const t_u32x4 vh = *reinterpret_cast<const t_u32x4 *>(s.Xh + bo), vl = *reinterpret_cast<const t_u32x4 *>(s.Xl + bo);
                const unsigned nh4 = *reinterpret_cast<const unsigned *>(s.Xh + bo + 16), nl4 = *reinterpret_cast<const unsigned *>(s.Xl + bo + 16);
                t_bf16x8 bh[3], bl[3];
                bh[0] = t_as_bf16x8(vh);
                bl[0] = t_as_bf16x8(vl);
                bh[1] = t_as_bf16x8(t_u32x4{__builtin_amdgcn_alignbyte(vh[1], vh[0], 2), __builtin_amdgcn_alignbyte(vh[2], vh[1], 2),
                                            __builtin_amdgcn_alignbyte(vh[3], vh[2], 2), __builtin_amdgcn_alignbyte(nh4, vh[3], 2)});
                bl[1] = t_as_bf16x8(t_u32x4{__builtin_amdgcn_alignbyte(vl[1], vl[0], 2), __builtin_amdgcn_alignbyte(vl[2], vl[1], 2),
                                            __builtin_amdgcn_alignbyte(vl[3], vl[2], 2), __builtin_amdgcn_alignbyte(nl4, vl[3], 2)});
                bh[2] = t_as_bf16x8(t_u32x4{vh[1], vh[2], vh[3], nh4});
                bl[2] = t_as_bf16x8(t_u32x4{vl[1], vl[2], vl[3], nl4});
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    acc[n][ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[kx], acc[n][ky * 3 + kx], 0, 0, 0);
                    acc[n][ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[kx], acc[n][ky * 3 + kx], 0, 0, 0);
                    acc[n][ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[kx], acc[n][ky * 3 + kx], 0, 0, 0);
                }
            }
    }
}

// The block's partial sums of its slice: lane holds couts 16 wave + 4 q + i of channel 16 n + r, nine taps.
__device__ __forceinline__ void t_xw_store_partial(const TConv &c, float *__restrict__ partial, int slice, int c0, int co0, int wave, int q, int r, const t_f32x4 (&acc)[2][9]) {
    float *pb = partial + (size_t)slice * c.Cout * c.Kdim;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int ci = c0 + 16 * n + r;
        if (ci >= c.Cin) continue;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = co0 + 16 * wave + 4 * q + i;
                if (co < c.Cout) pb[((size_t)co * c.Cin + ci) * 9 + tap] = acc[n][tap][i];
            }
    }
}

// Two-group kernels: add the two groups' accumulators through LDS (72 floats per thread, the image sets are free by then).
// Every thread of the block calls it; false = this thread (group 1) has handed its sums over and is done.
__device__ __forceinline__ bool t_xw_handover(float *scr, int grp, int t, t_f32x4 (&acc)[2][9]) {
    if (grp == 1) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int k9 = 0; k9 < 9; ++k9)
#pragma unroll
                for (int i = 0; i < 4; ++i) scr[((n * 9 + k9) * 4 + i) * 256 + t] = acc[n][k9][i];
    }
    __syncthreads();
    if (grp == 1) return false;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int k9 = 0; k9 < 9; ++k9)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[n][k9][i] += scr[((n * 9 + k9) * 4 + i) * 256 + t];
    return true;
}

// One group of four waves, two blocks per CU: stage a tile, barrier, multiply it, barrier.
__global__ __launch_bounds__(256, 2) void tconv3_wgrad_x3_kernel(TConv c, TTileW g, float *__restrict__ partial, int tiles_per_slice, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char t_smem8[];
    const TXwSet s = t_xw_set(t_smem8, g);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    T_DECODE_XYZ(bx_, by_, slice);
    const int c0 = bx_ * TXW_CI, co0 = by_ * 64;
    int hbq[4];
    t_xw_frag_offsets(g, q, hbq);
    const int s_a = 2 * lane, ry_a = s_a / g.SW, rx_a = s_a - ry_a * g.SW;      // this thread's dY slot pair
    t_f32x4 acc[2][9];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[n][k] = t_f32x4{0.f, 0.f, 0.f, 0.f};
    const int tbeg = slice * tiles_per_slice, tend = min(tbeg + tiles_per_slice, ntiles);
    for (int tile = tbeg; tile < tend; ++tile) {
        TXwDy d;
        t_xw_dy_load(c, g, tile, co0, t, ry_a, rx_a, d);
        __syncthreads();                          // the previous tile's fragments have been read
        t_xw_dy_store(c, s, co0, t, d);
        t_xw_halo_stage(c, g, s, tile, c0, t);
        __syncthreads();
        t_xw_mfma_set(g, s, hbq, wave, q, r, acc);
    }
    t_xw_store_partial(c, partial, slice, c0, co0, wave, q, r, acc);
}

__global__ __launch_bounds__(512, 1) void tconv3_wgrad_x3pp_kernel(TConv c, TTileW g, float *__restrict__ partial, int tiles_per_slice, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char t_smem8[];
    // two wave groups of 256 threads, each with its own LDS image set; in phase p group (p & 1) stages tile p while the other
    // group runs the MFMAs of tile p - 1: ONE block barrier per phase, staging and matrix work always overlap inside the block,
    // and the block writes ONE partial tile (the groups' accumulators are added through LDS): half the partial-sum traffic of
    // two independent 4-wave blocks per CU
    const int grp = threadIdx.x >> 8;
    const TXwSet s = t_xw_set(t_smem8 + grp * t_xw_set_bytes(g), g);
    const int t = threadIdx.x & 255, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    T_DECODE_XYZ(bx_, by_, slice);
    const int c0 = bx_ * TXW_CI, co0 = by_ * 64;
    int hbq[4];
    t_xw_frag_offsets(g, q, hbq);
    const int s_a = 2 * lane, ry_a = s_a / g.SW, rx_a = s_a - ry_a * g.SW;      // this thread's dY slot pair
    t_f32x4 acc[2][9];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[n][k] = t_f32x4{0.f, 0.f, 0.f, 0.f};
    const int tbeg = slice * tiles_per_slice, tend = min(tbeg + tiles_per_slice, ntiles), ntl = tend - tbeg;
    for (int ph = 0; ph <= ntl; ++ph) {
        if ((ph & 1) == grp) {
            if (ph < ntl) {
                TXwDy d;
                t_xw_dy_load(c, g, tbeg + ph, co0, t, ry_a, rx_a, d);
                t_xw_dy_store(c, s, co0, t, d);
                t_xw_halo_stage(c, g, s, tbeg + ph, c0, t);
            }
        } else if (ph >= 1) {
            t_xw_mfma_set(g, s, hbq, wave, q, r, acc);
        }
        __syncthreads();
    }
    if (!t_xw_handover(reinterpret_cast<float *>(t_smem8), grp, t, acc)) return;
    t_xw_store_partial(c, partial, slice, c0, co0, wave, q, r, acc);
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 5: the ping-pong weight gradient with ONE global round trip of staging per tile.  Stamps and the step's kernel stats
// (profiles/r05_train_step_*) said what bounds tconv3_wgrad_x3pp_kernel: not the matrix pipe (216 MFMAs = 3.5 k cycles per tile and
// wave) but the staging group next to it -- 32 + 30 scalar dword loads per thread, the halo ones in five dependent batches of six
// (more in flight spilled), every value split and written to LDS with 4-byte stores: ~5 memory round trips per phase against 1.6 us
// of matrix work.  Here
//   * dY never goes through LDS: a lane's A fragment IS eight consecutive pixels of its cout row (NCHW: 32 contiguous bytes, 16-byte
//     aligned when the map and tile widths are multiples of 4) -- two dwordx4 loads per pixel group, prefetched into registers by the
//     group that will multiply them in its NEXT phase, split into hi / lo right before the MFMAs;
//   * the X halo is fetched by rows: per (channel, halo row) TW / 4 aligned dwordx4 pieces + the two edge columns, <= 9 loads per
//     thread, ALL in flight at once (36 registers), each piece written with one 8-byte store per plane.  Layout per channel:
//     [16 B lead][HR rows x HP bf16], element hx of a row = image column x0 + hx, the left edge column x0 - 1 in the last slot of
//     the previous row's pitch (hx = -1): every dwordx4 piece lands 8-byte aligned, a slot group's fragment for tap kx is the
//     aligned 16-byte group shifted by kx - 1 elements (kx = 1: as read; kx = 0 / 2: five v_alignbyte with the dword before / after).
// Same tiles, same slices, same products in the same order as the x3pp kernel: bit-identical partial sums.  Shapes it does not take
// (widths that are not multiples of 4, pad != 1) stay on x3pp.
// ---------------------------------------------------------------------------------------------------------------------
#define TXV_NPI 9
__global__ __launch_bounds__(512, 1) void tconv3_wgrad_x3v_kernel(TConv c, TTileW g, float *__restrict__ partial, int tiles_per_slice, int ntiles, int ppi, int npieces) {
    extern __shared__ __attribute__((aligned(16))) unsigned char t_smem8[];
    const int set_bytes = 2 * TXW_CI * g.CHB;
    const int grp = threadIdx.x >> 8;
    unsigned char *Xh = t_smem8 + grp * set_bytes, *Xl = Xh + TXW_CI * g.CHB;       // halo [32 channels][16 + HR x HP x 2 bytes]
    const int t = threadIdx.x & 255, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    T_DECODE_XYZ(bx_, by_, slice);
    const int c0 = bx_ * TXW_CI, co0 = by_ * 64;
    const int HW = c.H * c.W, HoWo = c.Ho * c.Wo;
    {   // the images start as zeros: slots no piece ever writes (behind the right edge column) are READ by the fragments of the padding
        // slots, whose dY is zero -- the product must not be 0 x NaN
        t_u32x4 *z = reinterpret_cast<t_u32x4 *>(t_smem8);
        for (int i = threadIdx.x; i < 2 * set_bytes / 16; i += 512) z[i] = t_u32x4{0u, 0u, 0u, 0u};
    }
    // this lane's four 8-slot pixel groups: halo byte offset of the aligned fragment group (tap ky adds rows), dY pixel offset in the tile
    int hbq[4], aoff[4], arow[4], acol[4];
#pragma unroll
    for (int pg = 0; pg < 4; ++pg) {
        const int s0 = 32 * pg + 8 * q, ry = s0 / g.SW, rx0 = s0 - ry * g.SW;
        const bool in = ry < g.R;
        hbq[pg] = 16 + ((in ? ry : 0) * g.HP + rx0) * 2;
        arow[pg] = in ? ry : -1;
        acol[pg] = rx0;
        aoff[pg] = (in ? ry : 0) * c.Wo + rx0;
    }
    // tile-invariant description of this thread's X pieces: piece t + 256 i = (item = (channel, halo row), pc): pc 0 = left edge column,
    // ppi - 1 = right edge column, else the dwordx4 piece of columns 4 (pc - 1) .. + 3
    int meta[TXV_NPI];                                   // kind | row << 2 | ch << 8 | (colrel + 1) << 14 (kind 3 = none); offsets are rebuilt from it per tile
#pragma unroll
    for (int i = 0; i < TXV_NPI; ++i) {
        const int pidx = t + 256 * i;
        const int item = pidx / ppi, pc = pidx - item * ppi, ch = item / g.HR, row = item - ch * g.HR;
        const int kind = pidx < npieces ? (pc == 0 ? 0 : (pc == ppi - 1 ? 2 : 1)) : 3;
        const int colrel = kind == 0 ? -1 : (kind == 2 ? g.TW : 4 * (pc - 1));
        meta[i] = kind | (row << 2) | (ch << 8) | ((colrel + 1) << 14);
    }
    t_f32x4 acc[2][9];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[n][k] = t_f32x4{0.f, 0.f, 0.f, 0.f};
    t_f32x4 a4[4][2];                                     // this lane's dY fragments of the tile its group multiplies next
#pragma unroll
    for (int pg = 0; pg < 4; ++pg) a4[pg][0] = a4[pg][1] = t_f32x4{0.f, 0.f, 0.f, 0.f};
    const int tbeg = slice * tiles_per_slice, tend = min(tbeg + tiles_per_slice, ntiles), ntl = tend - tbeg;
    __syncthreads();
    for (int ph = 0; ph <= ntl; ++ph) {
      if ((ph & 1) == grp) {
        if (ph < ntl) {
            const int tile = tbeg + ph;
            const int tx = tile % g.tiles_x, ty = (tile / g.tiles_x) % g.tiles_y, img = tile / (g.tiles_x * g.tiles_y);
            const int y0 = ty * g.R, x0 = tx * g.TW;
            // ---- every load of the phase first: X pieces, then the dY fragments ----
            const float *xb = c.x + (size_t)img * c.Cin * HW + (size_t)c0 * HW + y0 * c.W + x0;
            t_f32x4 xv[TXV_NPI];
            unsigned okm = 0;
#pragma unroll
            for (int i = 0; i < TXV_NPI; ++i) {
                const int kind = meta[i] & 3, row = (meta[i] >> 2) & 63, ch = (meta[i] >> 8) & 63, colrel = (meta[i] >> 14) - 1;
                // every piece is ONE kind of load, a 16-byte group (the edge columns too: the group that holds column x0 - 1 / x0 + TW, one element
                // of it used): a dword load and a dwordx4 load into the same registers on two divergent paths made the compiler wait for each
                // piece before issuing the next -- nine dependent round trips per phase instead of one
                const int goff_i = ch * HW + (row - 1) * c.W + (kind == 0 ? -4 : colrel);
                const int iy = y0 - 1 + row;
                const int ok = (int)(kind != 3) & (int)(c0 + ch < c.Cin) & (int)(iy >= 0) & (int)(iy < c.H) &
                               (int)(kind == 0 ? x0 > 0 : (kind == 2 ? x0 + g.TW < c.W : true));
                okm |= (unsigned)ok << i;
                xv[i] = *reinterpret_cast<const t_f32x4 *>(xb + (goff_i & -ok));
            }
            const int cout = co0 + 16 * wave + r;
            const float *yb = c.y + ((size_t)img * c.Cout + (cout < c.Cout ? cout : 0)) * HoWo + y0 * c.Wo + x0;
            unsigned aok = 0;
#pragma unroll
            for (int pg = 0; pg < 4; ++pg) {
                const int rowok = (int)(cout < c.Cout) & (int)(arow[pg] >= 0) & (int)(y0 + arow[pg] < c.Ho);
                const int ok0 = rowok & (int)(acol[pg] + 3 < g.TW), ok1 = rowok & (int)(acol[pg] + 7 < g.TW);
                aok |= (unsigned)ok0 << (2 * pg) | (unsigned)ok1 << (2 * pg + 1);
                a4[pg][0] = *reinterpret_cast<const t_f32x4 *>(yb + (aoff[pg] & -ok0));
                a4[pg][1] = *reinterpret_cast<const t_f32x4 *>(yb + ((aoff[pg] + 4) & -ok1));
            }
            // ---- X: split and store (zeros where the piece lies outside the image / beyond Cin) ----
#pragma unroll
            for (int i = 0; i < TXV_NPI; ++i) {
                const int kind = meta[i] & 3;
                const bool ok = (okm >> i) & 1u;
                const int loff_i = ((meta[i] >> 8) & 63) * g.CHB + 16 + ((meta[i] >> 2) & 63) * g.HP * 2 + 2 * ((meta[i] >> 14) - 1);
                if (kind == 1) {
                    union { __bf16 b[4]; unsigned long long u; } ph4, pl4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float v = ok ? xv[i][j] : 0.f;
                        const __bf16 h = (__bf16)v;
                        ph4.b[j] = h;
                        pl4.b[j] = (__bf16)(v - (float)h);
                    }
                    *reinterpret_cast<unsigned long long *>(Xh + loff_i) = ph4.u;
                    *reinterpret_cast<unsigned long long *>(Xl + loff_i) = pl4.u;
                } else if (kind != 3) {
                    const float v = ok ? (kind == 0 ? xv[i][3] : xv[i][0]) : 0.f;
                    const __bf16 h = (__bf16)v;
                    *reinterpret_cast<__bf16 *>(Xh + loff_i) = h;
                    *reinterpret_cast<__bf16 *>(Xl + loff_i) = (__bf16)(v - (float)h);
                }
            }
#pragma unroll
            for (int pg = 0; pg < 4; ++pg) {             // the masked loads fetched element 0 of the row: zero them
                if (!((aok >> (2 * pg)) & 1u)) a4[pg][0] = t_f32x4{0.f, 0.f, 0.f, 0.f};
                if (!((aok >> (2 * pg + 1)) & 1u)) a4[pg][1] = t_f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
      } else if (ph >= 1) {
        // 24 items (pixel group pg, channel tile n, kernel row ky), 9 MFMAs each.  Software-pipelined by hand: the six LDS reads of item
        // it + 1 are issued before the MFMAs of item it (the compiler's own schedule waited for every item's reads right before its
        // MFMAs and separated the dependent triple of an accumulator with s_nop: 45 % matrix-pipe use inside this section), and the three
        // products of a tap are interleaved across the three taps of the row, so that no MFMA reads the accumulator the previous one
        // writes.  Per accumulator the order is still hi*hi, hi*lo, lo*hi: the sums are bit-identical.
        struct Frag { t_u32x4 vh, vl; unsigned mh, ml, nh, nl; };
        auto load_frag = [&](int it) -> Frag {
            const int pg = it / 6, n = (it % 6) / 3, ky = it % 3;
            const int bo = (16 * n + r) * g.CHB + hbq[pg] + ky * g.HP * 2;
            Frag f;
            f.vh = *reinterpret_cast<const t_u32x4 *>(Xh + bo); f.vl = *reinterpret_cast<const t_u32x4 *>(Xl + bo);
            f.mh = *reinterpret_cast<const unsigned *>(Xh + bo - 4); f.ml = *reinterpret_cast<const unsigned *>(Xl + bo - 4);
            f.nh = *reinterpret_cast<const unsigned *>(Xh + bo + 16); f.nl = *reinterpret_cast<const unsigned *>(Xl + bo + 16);
            return f;
        };
        Frag fr[2];
        fr[0] = load_frag(0);
        t_bf16x8 ah, al;
#pragma unroll
        for (int it = 0; it < 24; ++it) {
            const int pg = it / 6, n = (it % 6) / 3, ky = it % 3;
            __builtin_amdgcn_sched_barrier(0);
            if (it + 1 < 24) fr[(it + 1) & 1] = load_frag(it + 1);
            if (it % 6 == 0) {
                const float v8[8] = {a4[pg][0][0], a4[pg][0][1], a4[pg][0][2], a4[pg][0][3], a4[pg][1][0], a4[pg][1][1], a4[pg][1][2], a4[pg][1][3]};
                t_split8(v8, 0xffu, ah, al);
            }
            const Frag &f = fr[it & 1];
            const unsigned sh1 = __builtin_amdgcn_alignbyte(f.vh[1], f.vh[0], 2), sh2 = __builtin_amdgcn_alignbyte(f.vh[2], f.vh[1], 2), sh3 = __builtin_amdgcn_alignbyte(f.vh[3], f.vh[2], 2);
            const unsigned sl1 = __builtin_amdgcn_alignbyte(f.vl[1], f.vl[0], 2), sl2 = __builtin_amdgcn_alignbyte(f.vl[2], f.vl[1], 2), sl3 = __builtin_amdgcn_alignbyte(f.vl[3], f.vl[2], 2);
            t_bf16x8 bh[3], bl[3];
            bh[0] = t_as_bf16x8(t_u32x4{__builtin_amdgcn_alignbyte(f.vh[0], f.mh, 2), sh1, sh2, sh3});
            bl[0] = t_as_bf16x8(t_u32x4{__builtin_amdgcn_alignbyte(f.vl[0], f.ml, 2), sl1, sl2, sl3});
            bh[1] = t_as_bf16x8(f.vh);
            bl[1] = t_as_bf16x8(f.vl);
            bh[2] = t_as_bf16x8(t_u32x4{sh1, sh2, sh3, __builtin_amdgcn_alignbyte(f.nh, f.vh[3], 2)});
            bl[2] = t_as_bf16x8(t_u32x4{sl1, sl2, sl3, __builtin_amdgcn_alignbyte(f.nl, f.vl[3], 2)});
            __builtin_amdgcn_sched_barrier(0);          // (left to the compiler the fragment arithmetic lands between the MFMAs and the section is 6 % slower)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[n][ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[kx], acc[n][ky * 3 + kx], 0, 0, 0);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[n][ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[kx], acc[n][ky * 3 + kx], 0, 0, 0);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[n][ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[kx], acc[n][ky * 3 + kx], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
    }
    if (!t_xw_handover(reinterpret_cast<float *>(t_smem8), grp, t, acc)) return;
    t_xw_store_partial(c, partial, slice, c0, co0, wave, q, r, acc);
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient: dW[cout][k] = sum_pixels dY[cout][pixel] * X[k][pixel].  Block = 64 couts x 64 k columns over one slice of
// the pixels (grid.z slices -> partial sums, reduced in slice order by wgrad_reduce_kernel: deterministic, no atomics);
// reduction chunks of 32 pixels, lanes along the pixels for both operands.
// ---------------------------------------------------------------------------------------------------------------------
#define TW_RC 32
#define TW_P 81

template <int KS, bool DIL = false>       // DIL: taps c.dil pixels apart, as tconv_fwd_kernel's
__global__ __launch_bounds__(256) void tconv_wgrad_kernel(TConv c, float *__restrict__ partial, int pix_per_slice) {
    __shared__ float As[TW_RC][TW_P];      // dY  [pixel][cout]
    __shared__ float Bs[TW_RC][TW_P];      // X   [pixel][k column]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    T_DECODE_XYZ(bx_, by_, slice);
    const int kc0 = bx_ * 64, co0 = by_ * 64;
    const int HoWo = c.Ho * c.Wo;
    const int pl = t & 31, g = t >> 5;
    int kci[8], kky[8], kkx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = kc0 + g + 8 * j;
        if (k < c.Kdim) {
            kci[j] = k / (KS * KS);
            const int rr = k - kci[j] * (KS * KS);
            kky[j] = rr / KS;
            kkx[j] = rr - kky[j] * KS;
        } else {
            kci[j] = -1; kky[j] = 0; kkx[j] = 0;
        }
    }
    const int pbeg = slice * pix_per_slice, pend = min(pbeg + pix_per_slice, c.P);
    float ra[8], rb[8];
    unsigned okm = 0;          // bit j: rb[j] valid, bit 8 + j: ra[j] valid (the select happens when the values go to LDS)
    auto load = [&](int pc) {
        okm = 0;
        const int p = pc + pl;
        const bool ok = p < pend;
        int img = 0, rem = 0, oy = 0, ox = 0;
        if (ok) {
            img = p / HoWo;
            rem = p - img * HoWo;
            oy = rem / c.Wo;
            ox = rem - oy * c.Wo;
        }
        const float *dyb = c.y + (size_t)img * c.Cout * HoWo + rem;
        const float *xb = c.x + (size_t)img * c.Cin * c.H * c.W;
        const int iy0 = oy * c.stride - c.pad, ix0 = ox * c.stride - c.pad;
#pragma unroll
        for (int j = 0; j < 8; ++j) {            // unconditional loads + selects (see tconv_fwd_kernel)
            const int co = co0 + g + 8 * j;
            const int oka = (int)(ok & (co < c.Cout));
            ra[j] = dyb[(co * HoWo) & -oka];
            const int iy = DIL ? iy0 + kky[j] * c.dil : iy0 + kky[j], ix = DIL ? ix0 + kkx[j] * c.dil : ix0 + kkx[j];
            const int okb = (int)(ok & (kci[j] >= 0) & (iy >= 0) & (iy < c.H) & (ix >= 0) & (ix < c.W));
            rb[j] = xb[((kci[j] * c.H + iy) * c.W + ix) & -okb];
            okm |= ((unsigned)oka << (8 + j)) | ((unsigned)okb << j);
        }
    };
    t_f32x4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = t_f32x4{0.f, 0.f, 0.f, 0.f};
    if (pbeg < pend) load(pbeg);
    for (int pc = pbeg; pc < pend; pc += TW_RC) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            As[pl][g + 8 * j] = (okm >> (8 + j)) & 1u ? ra[j] : 0.f;
            Bs[pl][g + 8 * j] = (okm >> j) & 1u ? rb[j] : 0.f;
        }
        __syncthreads();
        if (pc + TW_RC < pend) load(pc + TW_RC);
#pragma unroll
        for (int ks = 0; ks < TW_RC / 4; ++ks) {
            const float a = As[4 * ks + q][16 * wave + r];
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[4 * ks + q][16 * n + r], acc[n], 0, 0, 0);
        }
    }
    float *pb = partial + (size_t)slice * c.Cout * c.Kdim;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int k = kc0 + 16 * n + r;
        if (k >= c.Kdim) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = co0 + 16 * wave + 4 * q + i;
            if (co < c.Cout) pb[(size_t)co * c.Kdim + k] = acc[n][i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The planes training engine's stem weight gradient (round 6): tconv_wgrad_kernel above -- the same block roles for the MFMAs, the same
// slices, the same order of every sum: bit-identical partials -- with
//   * dY read from a planes tensor ([pixel][cs], two bf16 planes hi | lo or one f32 plane): thread = (pixel t >> 3, couts 8 (t & 7) ..+7),
//     one 16-byte load per plane instead of eight strided 4-byte gathers of an NCHW hand-over tensor;
//   * BN = 1: dY is not read but computed -- the stem's BatchNorm backward (trainx_kernels.h::bn_bwd_apply_kernel: g = dA * ReLU'(x * scale + shift),
//     d = k1 * (g - k2 - xhat * k3), rounded to hi + lo exactly as that kernel stores it) from the activation gradient and the convolution
//     output, so the 103 MB dC0 tensor is neither written nor read;
//   * EIGHT waves per slice instead of four: the kernel is bound by its vector instructions (pixel decomposition, halo tests, the BatchNorm arithmetic, b32
//     LDS stores: ~1 600 issue cycles per wave and chunk against 1 024 of MFMA; four chunks in flight instead of one changed nothing), and 392 slices on
//     256 CUs leave 136 CUs with two blocks: with half the staging work per wave a slice takes half as long.  Wave w accumulates cout tile w & 3 x k-column
//     tiles 2 (w >> 2), 2 (w >> 2) + 1 -- every accumulator sees the MFMAs of tconv_wgrad_kernel in the same order;
//   * D chunks in flight (template parameter; every load of a slot issued unconditionally and the prologue in slot order, or the compiler closes each
//     iteration with s_waitcnt vmcnt(0)): D = 2 is the default -- 83-91 us in the step's traces against 102-163 (D = 1, unsteady) and 105 (D = 4); the
//     launch is bound by instruction issue (~270 instructions per wave and 32-pixel chunk for 16 MFMAs; SQ_INSTS_VALU / SQ_INSTS_MFMA 12.6), not by latency.
// ---------------------------------------------------------------------------------------------------------------------
struct TStemBn {
    const void *x; int x_cs, x_split;            // the convolution output (planes, as dY)
    const float *mean, *invstd, *k1, *k2, *k3, *scale, *shift;
    int act;                                     // 0 none, 1 ReLU, 2 LeakyReLU(0.1); the sign comes from x * scale + shift
};
template <int KS, int F32, int BN, int D>
__global__ __launch_bounds__(512, 1) void tstem_wgrad_kernel(TConv c, TStemBn bn, float *__restrict__ partial, int pix_per_slice) {
    // pitch 80 floats: the four pixel rows q of an MFMA operand read sit 16 banks apart (80 % 32 = 16: lanes (q, r) of a half-wave on 32 different banks; the
    // 81 of tconv_wgrad_kernel gives every such read a two-way conflict, 47 % of this kernel's LDS cycles by SQ_LDS_BANK_CONFLICT), and a thread's four
    // staged values are one aligned 16-byte store
    constexpr int TSP = 80;
    __shared__ __attribute__((aligned(16))) float As[TW_RC][TSP];      // dY  [pixel][cout]
    __shared__ __attribute__((aligned(16))) float Bs[TW_RC][TSP];      // X   [pixel][k column]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    const int mt = wave & 3, nh = wave >> 2;            // this wave's cout tile and pair of k-column tiles
    T_DECODE_XYZ(bx_, by_, slice);
    const int kc0 = bx_ * 64, co0 = by_ * 64;
    const int HoWo = c.Ho * c.Wo;
    const int pl = t & 31, g = t >> 5;                  // X staging: pixel, k columns 4 g + j
    // (the vector instructions bound this kernel: everything that does not change from chunk to chunk is decided here -- a k column's offset inside the
    // image and its (ky, kx); an invalid column gets ky = -2^20, which fails the halo test)
    int koff[4], kky[4], kkx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = kc0 + 4 * g + j;
        if (k < c.Kdim) {
            const int ci = k / (KS * KS), rr = k - ci * (KS * KS);
            kky[j] = rr / KS;
            kkx[j] = rr - kky[j] * KS;
            koff[j] = (ci * c.H + kky[j]) * c.W + kkx[j];
        } else {
            koff[j] = 0; kky[j] = -(1 << 20); kkx[j] = 0;
        }
    }
    const int pbeg = slice * pix_per_slice, pend = min(pbeg + pix_per_slice, c.P);
    const int a_px = t >> 4, a_c4 = 4 * (t & 15), a_co = co0 + a_c4;       // dY staging: pixel, couts a_c4 ..+3
    const bool a_cok = a_co < c.Cout;
    float bmean[4], binv[4], bk1[4], bk2[4], bk3[4], bsc[4], bsh[4];
    if (BN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = a_cok ? a_co + j : 0;
            bmean[j] = bn.mean[ch]; binv[j] = bn.invstd[ch]; bk1[j] = bn.k1[ch]; bk2[j] = bn.k2[ch]; bk3[j] = bn.k3[ch]; bsc[j] = bn.scale[ch]; bsh[j] = bn.shift[ch];
        }
    }
    // per prefetch slot: raw dY (and x) vectors, the gathered input values, validity bits (the selects happen when the values go to LDS)
    t_f32x4 dyv[D], xv[D];                 // f32: four floats; bf16 planes: .xy = the hi plane's 4 x bf16, .zw = the lo plane's
    float rb[D][4];
    unsigned okm[D];
    const int adv_i = TW_RC / HoWo, adv_y = (TW_RC - adv_i * HoWo) / c.Wo, adv_x = TW_RC - adv_i * HoWo - adv_y * c.Wo;
    int w_img, w_oy, w_ox;
    {
        const int p = min(pbeg + pl, c.P - 1);
        w_img = p / HoWo;
        const int rem = p - w_img * HoWo;
        w_oy = rem / c.Wo;
        w_ox = rem - w_oy * c.Wo;
    }
    auto ldplanes = [&](const void *base, size_t off, int split) -> t_f32x4 {
        if (F32) return *reinterpret_cast<const t_f32x4 *>((const float *)base + off);
        const t_f32x2 h = *reinterpret_cast<const t_f32x2 *>((const __bf16 *)base + off), l = *reinterpret_cast<const t_f32x2 *>((const __bf16 *)base + off + split);
        return t_f32x4{h[0], h[1], l[0], l[1]};
    };
    auto load = [&](int d, int pc) {
        const int pp = pc + a_px;
        const bool aok = pp < pend && a_cok;
        dyv[d] = ldplanes(c.pl, (size_t)(aok ? pp : 0) * c.pl_cs + (aok ? a_co : 0), c.pl_split);
        if (BN) xv[d] = ldplanes(bn.x, (size_t)(aok ? pp : 0) * bn.x_cs + (aok ? a_co : 0), bn.x_split);
        unsigned m = (unsigned)aok << 8;
        // this thread's pixel of the chunk: (img, oy, ox) walk along with the chunks (loads are issued in chunk order), no division per chunk
        const bool ok = pc + pl < pend;
        const int iy0 = w_oy * c.stride - c.pad, ix0 = w_ox * c.stride - c.pad;
        const float *xb = c.x + (size_t)w_img * c.Cin * c.H * c.W + (iy0 * c.W + ix0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int okb = (int)(ok & ((unsigned)(iy0 + kky[j]) < (unsigned)c.H) & ((unsigned)(ix0 + kkx[j]) < (unsigned)c.W));
            const float *src = okb ? xb + koff[j] : c.x;        // (an unconditional load + a select later, see tconv_fwd_kernel)
            rb[d][j] = *src;
            m |= (unsigned)okb << j;
        }
        okm[d] = m;
        w_ox += adv_x; w_oy += adv_y; w_img += adv_i;             // the next chunk's pixel: 32 further (one carry per digit at most)
        if (w_ox >= c.Wo) { w_ox -= c.Wo; ++w_oy; }
        if (w_oy >= c.Ho) { w_oy -= c.Ho; ++w_img; }
    };
    auto value4 = [&](const t_f32x4 raw, float (&v)[4]) {           // a planes vector as trainx_kernels.h::Lay<T>::ld reads it
        if (F32) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = raw[j];
        } else {
            const t_bf4 h = __builtin_bit_cast(t_bf4, t_f32x2{raw[0], raw[1]}), l = __builtin_bit_cast(t_bf4, t_f32x2{raw[2], raw[3]});
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (float)h[j] + (float)l[j];
        }
    };
    t_f32x4 acc[2];
    acc[0] = acc[1] = t_f32x4{0.f, 0.f, 0.f, 0.f};
    // every load of a slot is issued UNCONDITIONALLY (a chunk behind the slice's end reads dummy addresses and is never used): with the loads inside
    // `if (pc < pend)` the loop body is not straight-line and the compiler closes every iteration with s_waitcnt vmcnt(0) -- no chunk stays in flight
    // (and the prologue issues the slots IN ORDER: the scheduler had moved the loads the loop needs first to the end of the prologue, which the counter
    // of the loop's first wait then had to allow for)
#pragma unroll
    for (int d = 0; d < D; ++d) {
        load(d, pbeg + d * TW_RC);
        __builtin_amdgcn_sched_barrier(0);
    }
    for (int pc0 = pbeg; pc0 < pend; pc0 += D * TW_RC) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int pc = pc0 + d * TW_RC;
            if (pc >= pend) break;
            float a4[4];
            value4(dyv[d], a4);
            if (BN) {
                float x4[4];
                value4(xv[d], x4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float gg = a4[j];
                    if (bn.act) {
                        const float y = x4[j] * bsc[j] + bsh[j];
                        const float neg = bn.act == 2 ? 0.1f : 0.f;
                        gg = y > 0.f ? gg : gg * neg;
                    }
                    const float xh = (x4[j] - bmean[j]) * binv[j];
                    float dd = bk1[j] * (gg - bk2[j] - xh * bk3[j]);
                    if (!F32) {                                            // what Lay<bf>::st stores and Lay<bf>::ld reads back
                        const __bf16 hi = (__bf16)dd;
                        dd = (float)hi + (float)(__bf16)(dd - (float)hi);
                    }
                    a4[j] = dd;
                }
            }
            __syncthreads();
            const unsigned m = okm[d];
            {
                const bool aok = (m >> 8) & 1u;
                *reinterpret_cast<t_f32x4 *>(&As[a_px][a_c4]) = t_f32x4{aok ? a4[0] : 0.f, aok ? a4[1] : 0.f, aok ? a4[2] : 0.f, aok ? a4[3] : 0.f};
                *reinterpret_cast<t_f32x4 *>(&Bs[pl][4 * g]) = t_f32x4{m & 1u ? rb[d][0] : 0.f, m & 2u ? rb[d][1] : 0.f, m & 4u ? rb[d][2] : 0.f, m & 8u ? rb[d][3] : 0.f};
            }
            __syncthreads();
            load(d, pc + D * TW_RC);
#pragma unroll
            for (int ks = 0; ks < TW_RC / 4; ++ks) {
                const float a = As[4 * ks + q][16 * mt + r];
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[4 * ks + q][16 * (2 * nh + n) + r], acc[n], 0, 0, 0);
            }
        }
    }
    float *pb = partial + (size_t)slice * c.Cout * c.Kdim;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int k = kc0 + 16 * (2 * nh + n) + r;
        if (k >= c.Kdim) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = co0 + 16 * mt + 4 * q + i;
            if (co < c.Cout) pb[(size_t)co * c.Kdim + k] = acc[n][i];
        }
    }
}

template <int V>
__global__ void wgrad_reduce_kernel(const float *__restrict__ partial, float *__restrict__ dw, int n, int slices) {
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (i >= n) return;
    float s[V];
#pragma unroll
    for (int v = 0; v < V; ++v) s[v] = 0.f;
    // slice order: deterministic.  Round 5: eight slices' loads in flight, added IN ORDER (the same sums bit for bit): a 64 -> 64 layer's 128 slices were
    // 128 dependent round trips of 36 workgroups (30 us per launch, 0.45 ms per step over the small layers)
    int k = 0;
    for (; k + 8 <= slices; k += 8) {
        float p[8][V];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (V == 4) *reinterpret_cast<float4 *>(p[j]) = *reinterpret_cast<const float4 *>(partial + (size_t)(k + j) * n + i);
            else p[j][0] = partial[(size_t)(k + j) * n + i];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int v = 0; v < V; ++v) s[v] += p[j][v];
    }
    for (; k < slices; ++k) {
        float p[V];
        if (V == 4) *reinterpret_cast<float4 *>(p) = *reinterpret_cast<const float4 *>(partial + (size_t)k * n + i);
        else p[0] = partial[(size_t)k * n + i];
#pragma unroll
        for (int v = 0; v < V; ++v) s[v] += p[v];
    }
    if (V == 4) *reinterpret_cast<float4 *>(dw + i) = *reinterpret_cast<const float4 *>(s);
    else dw[i] = s[0];
}

static void t_wgrad_reduce(hipStream_t s, const float *partial, float *dw, size_t wn, int slices) {
    // (small tensors one element per thread: four times the workgroups, the same per-element sums)
    if ((wn & 3) == 0 && ((((size_t)partial) | ((size_t)dw)) & 15) == 0 && wn >= 256 * 256 * 4)
        hipLaunchKernelGGL(wgrad_reduce_kernel<4>, dim3((unsigned)((wn / 4 + 255) / 256)), dim3(256), 0, s, partial, dw, (int)wn, slices);
    else
        hipLaunchKernelGGL(wgrad_reduce_kernel<1>, dim3((unsigned)((wn + 255) / 256)), dim3(256), 0, s, partial, dw, (int)wn, slices);
}
