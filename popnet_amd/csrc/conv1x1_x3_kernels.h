// Split-bf16 ("bf16x3") kernels of the 1x1, stride-1, pad-0 training convolutions (conv1x1_x3.hip holds the planner and the entries).
// A 1x1 convolution on NCHW is one GEMM per image; the three roles are the same 64 x 128 x 32 block product on different operands:
//   forward        y[n][co][p]  = sum_ci w[co][ci] x[n][ci][p]        A = weight pack [co][ci],     B = x as [pixel][ci]   (k-strided in memory)
//   data gradient  dx[n][ci][p] = sum_co w[co][ci] dy[n][co][p]       A = TRANSPOSED pack [ci][co], B = dy as [pixel][co]  (the same kernel)
//   weight grad.   dw[co][ci]   = sum_np dy[n][co][p] x[n][ci][p]     A = dy rows [co][pixel],      B = x rows [ci][pixel] (both k-contiguous)
// Arithmetic, as the 3x3 x3 kernels (train_conv_kernels.h) and through the same functions (train_conv_common.h: t_split8, t_mfma_x3): every fp32
// value v is split hi = bf16(v), lo = bf16(v - hi) (round to nearest even) and a product block is three v_mfma_f32_16x16x32_bf16 into ONE fp32
// accumulator, a_hi b_hi + a_hi b_lo + a_lo b_hi; no lo * lo.  The block order is t_logical_block's, decoded with the sharing dimension fastest (the
// channel blocks of one pixel tile; the blocks of one slice); the weight-gradient slices are added by train.hip's reduction (pn_train_wgrad_reduce).
// LDS: both operands as [row][32 k] bf16 rows of 80 bytes (16-byte fragment reads and 16-byte staging writes are conflict-free at that
// pitch), one hi and one lo plane each: 2 x 64 x 80 + 2 x 128 x 80 = 30 KB, static.  The next chunk's global loads are issued before the
// MFMAs of the current one and land in registers (no second LDS buffer: several blocks per CU hide the two barriers).
// A wave owns 64 A rows x 32 B rows: fragment (m, n) is A rows 16 m .. + 15 against B rows 32 wave + 16 n .. + 15, and accumulator element
// i of lane (q = lane / 16, r = lane % 16) is (A row 16 m + 4 q + i, B row 32 wave + 16 n + r) -- B rows are pixels in the forward
// kernel, so the 16 lanes of a group store 64 contiguous bytes of one output row.
// The summation order is fixed by the shape alone (chunks in order, slices in order): repeated calls give identical bits; no atomics.
#pragma once
#include "train_conv_common.h"

#define C1_BM 64                         // A rows per block
#define C1_BN 128                        // B rows per block
#define C1_BK 32                         // k per chunk: one MFMA step
#define C1_PITCH 80                      // bytes per [32 x bf16] row
#define C1_A_BYTES (C1_BM * C1_PITCH)    // one plane
#define C1_B_BYTES (C1_BN * C1_PITCH)
#define C1_LDS (2 * C1_A_BYTES + 2 * C1_B_BYTES)

struct C1Gemm {          // forward / data gradient: y[n][m][p] (+)= bias[m] + sum_k pack[m][k] x[n][k][p]
    const float *x;
    const __bf16 *wp;    // [plane hi | lo][chunk of 32 k][M][32 k], k beyond K zero
    const float *bias;
    float *y;
    int N, K, HW, M, accumulate, P;      // P = N HW
};

struct C1Wgrad {         // partial[slice][co][ci] = sum over the slice's pixel chunks of dy[n][co][p] x[n][ci][p]
    const float *x, *dy;
    float *partial;
    int N, Cin, HW, Cout;
    int cpi, total, per;                 // 32-pixel chunks per image (the last one ragged: a chunk never straddles two images), chunks in all, chunks per slice
};

// one chunk of 32 k from the staged planes
__device__ __forceinline__ void c1_mma_chunk(const unsigned char *sm, int wave, int q, int r, t_f32x4 (&acc)[4][2]) {
    const unsigned char *Ah = sm, *Al = sm + C1_A_BYTES, *Bh = sm + 2 * C1_A_BYTES, *Bl = Bh + C1_B_BYTES;
    t_bf16x8 bh[2], bl[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int off = (32 * wave + 16 * n + r) * C1_PITCH + 16 * q;
        bh[n] = *(const t_bf16x8 *)(Bh + off);
        bl[n] = *(const t_bf16x8 *)(Bl + off);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int off = (16 * m + r) * C1_PITCH + 16 * q;
        const t_bf16x8 ah = *(const t_bf16x8 *)(Ah + off), al = *(const t_bf16x8 *)(Al + off);
#pragma unroll
        for (int n = 0; n < 2; ++n) t_mfma_x3(acc[m][n], ah, al, bh[n], bl[n]);
    }
}

// PN_PACK_C1_X3, per call: the [hi | lo] pack of w [Cout][Cin] -- flip = 0: rows M = Cout over K = Cin (forward); flip = 1: the transpose, rows
// M = Cin over K = Cout (data gradient)
__global__ void conv1x1_wpack_x3_kernel(const float *__restrict__ w, __bf16 *__restrict__ wp, int M, int K, int flip) {
    t_pack_element<PN_PACK_C1_X3>(w, wp, M, K, flip, (size_t)blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void conv1x1_x3_kernel(C1Gemm c) {
    __shared__ __attribute__((aligned(16))) unsigned char sm[C1_LDS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    const int lg = t_logical_block();
    const int p0 = (lg / (int)gridDim.y) * C1_BN, m0 = (lg % (int)gridDim.y) * C1_BM;          // (p0 < P <= INT_MAX - 128: the entry checks)
    const int chunks = (c.K + 31) / 32;
    const size_t plane = t_pack_elems(PN_PACK_C1_X3, c.M, c.K);
    // staging roles.  B: this wave stages channels 8 wave .. + 7 of the chunk for pixels lane and lane + 64 (the lanes of a load are 64
    // consecutive pixels of one channel row); A: thread t copies 16 bytes (8 k) of pack row t / 4, both planes.
    long xoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int gp = p0 + lane + 64 * i;
        const int img = gp < c.P ? gp / c.HW : 0;
        xoff[i] = gp < c.P ? (long)img * c.K * c.HW + (gp - img * c.HW) : -1;
    }
    const int arow = t >> 2, aseg = t & 3;
    const bool aok = m0 + arow < c.M;
    float xv[2][8];
    t_u32x4 wv[2];
    const t_u32x4 zero4 = {0u, 0u, 0u, 0u};
    t_f32x4 acc[4][2];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = t_f32x4{0.f, 0.f, 0.f, 0.f};

#define C1_LOAD_CHUNK(ch)                                                                                                   \
    {                                                                                                                       \
        const int ci0 = (ch) * 32 + 8 * wave;                                                                               \
        _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                                       \
            _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                                   \
                xv[i][j] = (xoff[i] >= 0 && ci0 + j < c.K) ? c.x[xoff[i] + (size_t)(ci0 + j) * c.HW] : 0.f;                 \
        const __bf16 *src = c.wp + ((size_t)(ch) * c.M + m0 + arow) * 32 + 8 * aseg;                                        \
        wv[0] = aok ? *(const t_u32x4 *)src : zero4;                                                                       \
        wv[1] = aok ? *(const t_u32x4 *)(src + plane) : zero4;                                                             \
    }

    C1_LOAD_CHUNK(0)
    for (int ch = 0; ch < chunks; ++ch) {
        __syncthreads();                 // the previous chunk's fragment reads are done
        *(t_u32x4 *)(sm + arow * C1_PITCH + 16 * aseg) = wv[0];
        *(t_u32x4 *)(sm + C1_A_BYTES + arow * C1_PITCH + 16 * aseg) = wv[1];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            t_bf16x8 hi, lo;
            t_split8(xv[i], 0xffu, hi, lo);
            const int off = (lane + 64 * i) * C1_PITCH + 16 * wave;
            *(t_bf16x8 *)(sm + 2 * C1_A_BYTES + off) = hi;
            *(t_bf16x8 *)(sm + 2 * C1_A_BYTES + C1_B_BYTES + off) = lo;
        }
        __syncthreads();
        if (ch + 1 < chunks) C1_LOAD_CHUNK(ch + 1)
        c1_mma_chunk(sm, wave, q, r, acc);
    }
#undef C1_LOAD_CHUNK

    // epilogue: bias once, then the previous output; pixels on the lanes of a group
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int gp = p0 + 32 * wave + 16 * n + r;
        if (gp >= c.P) continue;
        const int img = gp / c.HW;
        float *yb = c.y + (size_t)img * c.M * c.HW + (gp - img * c.HW);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = m0 + 16 * m + 4 * q + i;
                if (co >= c.M) continue;
                float v = acc[m][n][i];
                if (c.bias) v += c.bias[co];
                if (c.accumulate) v += yb[(size_t)co * c.HW];
                yb[(size_t)co * c.HW] = v;
            }
    }
}

// 8 consecutive pixels of one row, `rem` of them inside the image (rem <= 0: none); VEC: rows are 16-byte aligned (HW % 4 == 0 and
// aligned tensors), a whole group is two 16-byte loads; the ragged group at the end of an image and every unaligned shape load per element.
template <bool VEC>
__device__ __forceinline__ void c1_load8(const float *__restrict__ p, bool row_ok, int rem, float (&v)[8]) {
    if (VEC && row_ok && rem >= 8) {
        const t_f32x4 a = *(const t_f32x4 *)p, b = *(const t_f32x4 *)(p + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (row_ok && j < rem) ? p[j] : 0.f;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void conv1x1_wgrad_x3_kernel(C1Wgrad c) {
    __shared__ __attribute__((aligned(16))) unsigned char sm[C1_LDS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, q = lane >> 4, r = lane & 15;
    const int lg = t_logical_block(), slice = lg / (int)(gridDim.x * gridDim.y);
    const int n0 = (lg % (int)gridDim.x) * C1_BN, m0 = ((lg / (int)gridDim.x) % (int)gridDim.y) * C1_BM;          // ci block, co block
    const int k_begin = slice * c.per, k_end = min(c.total, k_begin + c.per);
    // staging: thread t splits pixels 8 (t % 4) .. + 7 of the chunk for dy row t / 4 and x rows t / 4, t / 4 + 64
    const int row = t >> 2, seg = t & 3;
    const bool aok = m0 + row < c.Cout, bok0 = n0 + row < c.Cin, bok1 = n0 + 64 + row < c.Cin;
    float av[8], bv[2][8];
    t_f32x4 acc[4][2];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = t_f32x4{0.f, 0.f, 0.f, 0.f};

#define C1_LOAD_CHUNK(kc)                                                                                                   \
    {                                                                                                                       \
        const int img = (kc) / c.cpi, pb = ((kc) - img * c.cpi) * 32 + 8 * seg, rem = c.HW - pb;                            \
        c1_load8<VEC>(c.dy + ((size_t)img * c.Cout + (aok ? m0 + row : 0)) * c.HW + pb, aok, rem, av);                      \
        c1_load8<VEC>(c.x + ((size_t)img * c.Cin + (bok0 ? n0 + row : 0)) * c.HW + pb, bok0, rem, bv[0]);                   \
        c1_load8<VEC>(c.x + ((size_t)img * c.Cin + (bok1 ? n0 + 64 + row : 0)) * c.HW + pb, bok1, rem, bv[1]);              \
    }

    if (k_begin < k_end) C1_LOAD_CHUNK(k_begin)
    for (int kc = k_begin; kc < k_end; ++kc) {
        __syncthreads();
        t_bf16x8 hi, lo;
        t_split8(av, 0xffu, hi, lo);
        *(t_bf16x8 *)(sm + row * C1_PITCH + 16 * seg) = hi;
        *(t_bf16x8 *)(sm + C1_A_BYTES + row * C1_PITCH + 16 * seg) = lo;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            t_split8(bv[i], 0xffu, hi, lo);
            const int off = (row + 64 * i) * C1_PITCH + 16 * seg;
            *(t_bf16x8 *)(sm + 2 * C1_A_BYTES + off) = hi;
            *(t_bf16x8 *)(sm + 2 * C1_A_BYTES + C1_B_BYTES + off) = lo;
        }
        __syncthreads();
        if (kc + 1 < k_end) C1_LOAD_CHUNK(kc + 1)
        c1_mma_chunk(sm, wave, q, r, acc);
    }
#undef C1_LOAD_CHUNK

    float *out = c.partial + (size_t)slice * c.Cout * c.Cin;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int ci = n0 + 32 * wave + 16 * n + r;
        if (ci >= c.Cin) continue;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = m0 + 16 * m + 4 * q + i;
                if (co < c.Cout) out[(size_t)co * c.Cin + ci] = acc[m][n][i];
            }
    }
}
