// Weight gradient of a 3x3 / 1x1 stride-1 "same" convolution on NHWC [hi | lo] bf16 planes: a pixel-K GEMM on the matrix cores.
//
//   dW[co][ci][ky][kx] = sum over (n, y, x) of dy[n, y, x, co] * x[n, y + ky - pad, x + kx - pad, ci]      (autograd of nn.Conv2d:
//   tpm/lib/network/rtpose_light3d.py:24-34,222-246 under tpm/train_rtpose_light3d_kdh3d_mpaug.py:160-180 (CR))
// with every product taken as dy_hi x_hi + dy_lo x_hi + dy_hi x_lo (split-bf16, fp32 accumulate).
//
// MFMA view: D[co][ci] += A[co][k] B[k][ci] with k = PIXEL.  Both operands are channel-minor in memory, so both fragments are
// "k-strided": they are read from LDS with ds_read_b64_tr_b16 (gfx950's transposing read: a 4-pixel x 16-channel block arrives
// pixel-minor), the one instruction that makes an NHWC weight gradient cheap -- no second (pixel-minor) copy of any tensor exists.
//   * block = 4 waves = 64 couts x 64 cins x all taps; wave = 32 x 32 x KS*KS accumulator tiles (144 VGPRs for 3x3);
//   * a k-chunk is one ROW SEGMENT of <= 30 pixels (32 slots, the surplus slots hold dy = 0): the dy fragment of a row is read once and
//     multiplied with the nine shifted x fragments (tap = an immediate LDS offset: the halo image is [row][plane][32 px][128 B]);
//   * images are filled by LDS-DMA (global_load_lds_dwordx4, no staging registers), 16-byte slots XOR-swizzled by the pixel so that the
//     eight pixels a half-wave's transposed read touches cover all 64 banks once -- for every tap shift;
//   * k -> pixel map of a fragment: lane group g, read j, row q  <->  pixel 16 j + 4 g + q (any map works as long as A and B share it;
//     this one keeps a half-wave on eight CONSECUTIVE pixels);
//   * deterministic split-K: block s of a tile pair sums its strips into partial[s], wgrad_reduce_kernel adds the slices in order and
//     scatters to the reference's [Cout][Cin][k][k] layout (undoing this engine's channel order of the stage-2 input).
#pragma once
#include <functional>
#include <vector>
#include "conv_common.h"
#include "trainx_kernels.h"

namespace tx {

typedef __attribute__((ext_vector_type(4))) __bf16 bf4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

// ---- what the two kernels share: a block walks a column strip row by row -------------------------------------------------------------------------
// A first form fetched a 3-row strip (5 halo rows of x, 3 rows of dy: 64 KB), waited, computed, and -- alone on its CU since the split-K went to one
// block per CU -- exposed that round trip once per strip (36 % of wave cycles waiting).  Here a block walks a COLUMN STRIP top-down: rings of KS + D x rows
// and 1 + D dy rows (D = 2: the same 64 KB), per row ONE group of four LDS-DMA instructions per wave for the row D ahead, ONE barrier, a counted
// `s_waitcnt vmcnt` (the D - 1 newer groups stay in flight) -- and no halo row is ever fetched twice.  A block owns `rows_per_block` consecutive rows of
// the flattened (image, column strip, row) space; where its range crosses into the next column strip the rings are re-primed.
// Each kernel keeps what is its own -- fragment addresses, DMA lane set-up, the two fetch bodies and the row body -- and reaches wg_walk through
// lambdas that capture its locals by reference (bb64_common.h's header note); everything here takes its arguments by value.
struct WgArgs {
    const void *x; int x_cs, x_split; unsigned x_zero;      // x_split / dy_split: plane distance in elements ([hi | lo] bf16 planes), 0 for fp32 tensors
    const void *dy; int dy_cs, dy_split; unsigned dy_zero;
    int B, H, W;
    int Wt, tiles_x, rows_total, rows_per_block;
    int ncit, co_pad, ci_pad;
    float *partial;
};
constexpr int WG_RING = 5;                      // both rings hold WG_RING rows: ring positions are compile-time in a body unrolled WG_RING rows deep
constexpr int WG_ROWB = 8192;                   // one ring row: 32 pixel slots x 64 channels x 4 B (fp32) or x 2 planes x 2 B
constexpr int WG_XRING = WG_RING * WG_ROWB;     // LDS is [x ring][dy ring]
// rows [ya, yb) of one column strip: columns ox0 .. ox0 + Wc - 1; bx0 / by0 = byte offset of the strip's image row 0 (row offsets are added modulo 2^32)
struct WgSeg { int ya, yb, ox0, Wc; unsigned bx0, by0; };

// zeroes the accumulators and both rings, and decodes the block's (cout, cin) tile pair.  Every LDS byte a fragment read can touch holds finite data
// from the start: a tap-shifted read of the surplus pixel slots runs a few pixels past its row (multiplied by dy = 0 there -- but 0 x NaN is NaN, and
// LDS starts as whatever the previous kernel left)
template <int KK>
__device__ __forceinline__ void wg_begin(const WgArgs a, char *smem, f4 (&acc)[2][2][KK], int &co0, int &ci0) {
    const int cot = blockIdx.y / a.ncit, cit = blockIdx.y - cot * a.ncit;
    co0 = cot * 64; ci0 = cit * 64;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int tp = 0; tp < KK; ++tp) acc[mt][nt][tp] = f4{0.f, 0.f, 0.f, 0.f};
    for (int o = threadIdx.x * 16; o < 2 * WG_XRING; o += 256 * 16) *reinterpret_cast<u32x4_t *>(smem + o) = u32x4_t{0u, 0u, 0u, 0u};
}

// The walk over the block's rows.  segment(sg): the kernel takes note of the next segment; fetch_x(n, slot) / fetch_y(n, slot): one group half each (two
// LDS-DMA instructions per wave) -- x row number n of the segment = image row ya - PAD + n, dy row number n = image row ya + n (rows past the segment are
// fetched as zeros: their group is issued only to keep the vmcnt arithmetic uniform) -- into ring slot n % WG_RING; row_body(u): the MFMAs of the row in
// dy slot u.  ES = bytes per stored element.
template <int KS, int D, int ES, class Segment, class FetchX, class FetchY, class RowBody>
__device__ __forceinline__ void wg_walk(const WgArgs a, Segment segment, FetchX fetch_x, FetchY fetch_y, RowBody row_body) {
    constexpr int RING = WG_RING;
    static_assert(KS + D <= RING && 1 + D <= RING, "ring too small for the prefetch distance");
    int row = blockIdx.x * a.rows_per_block;
    const int row_end = min(row + a.rows_per_block, a.rows_total);
    while (row < row_end) {
        // segment: rows [ya, yb) of column strip cs
        const int cs = row / a.H, ya = row - cs * a.H;
        const int yb = min(a.H, ya + (row_end - row));
        const int nrows = yb - ya;
        const int b = cs / a.tiles_x, tx_ = cs - b * a.tiles_x;
        const int ox0 = tx_ * a.Wt, Wc = min(a.Wt, a.W - ox0);
        segment(WgSeg{ya, yb, ox0, Wc, (unsigned)(((long)b * a.H * a.W + ox0) * (long)a.x_cs * ES), (unsigned)(((long)b * a.H * a.W + ox0) * (long)a.dy_cs * ES)});
        __syncthreads();                          // the previous segment's fragment reads are done: the rings may be overwritten
#pragma unroll
        for (int n = 0; n < KS - 1; ++n) fetch_x(n, n % RING);
#pragma unroll
        for (int j = 0; j < D; ++j) { fetch_x(KS - 1 + j, (KS - 1 + j) % RING); fetch_y(j, j % RING); }
        for (int k0 = 0; k0 < nrows; k0 += RING) {
#pragma unroll
            for (int u = 0; u < RING; ++u) {      // row k = k0 + u: k % RING == u
                const int k = k0 + u;
                if (k >= nrows) break;
                // group k (x row number KS - 1 + k, dy row number k) has landed once at most D - 1 newer groups (4 instructions each) are outstanding
                if (D == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else if (D == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                __syncthreads();                  // ... for every wave's pieces; and every wave has finished row k - 1, whose slots group k + D overwrites
                fetch_x(KS - 1 + k + D, (KS - 1 + u + D) % RING);
                fetch_y(k + D, (u + D) % RING);
                row_body(u);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the D surplus groups of the segment's tail
        row += nrows;
    }
}

// the block's partial tile: wave (wm, wn) holds 32 couts x 32 cins x KK taps
template <int KK>
__device__ __forceinline__ void wg_store(const WgArgs a, const f4 (&acc)[2][2][KK], int co0, int ci0, int wm, int wn, int lane) {
    const int g = lane >> 4;
    float *part = a.partial + (size_t)blockIdx.x * KK * a.co_pad * a.ci_pad;
#pragma unroll
    for (int tp = 0; tp < KK; ++tp)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int co = co0 + wm * 32 + mt * 16 + 4 * g + i, ci = ci0 + wn * 32 + nt * 16 + (lane & 15);
                    part[((size_t)tp * a.co_pad + co) * a.ci_pad + ci] = acc[mt][nt][tp][i];
                }
}

// ---- [hi | lo] bf16 planes -------------------------------------------------------------------------------------------------------------------------
template <int KS, int D>
__global__ __launch_bounds__(256, 2) void wgrad_stream_kernel(WgArgs a) {
    typedef __attribute__((address_space(3))) bf4 lds4;
    constexpr int KK = KS * KS, PAD = KS / 2, RING = WG_RING, ROWB = WG_ROWB, XRING = WG_XRING;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int pxl = 4 * g + q;
    // transposed-read addresses (bytes): lane 4q + p of group g supplies row (= pixel) q, channels 4p .. 4p + 3 of the 16-channel window
    int addrA[2], addrB[KS][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int win = wm * 2 + mt, swz = (pxl >> 1) & 3;
        addrA[mt] = XRING + pxl * 128 + ((((win ^ swz) << 1) | (p >> 1)) << 4) + ((p & 1) << 3);
    }
#pragma unroll
    for (int kx = 0; kx < KS; ++kx)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int win = wn * 2 + nt, hp = pxl + kx, swz = (hp >> 1) & 3;
            addrB[kx][nt] = hp * 128 + ((((win ^ swz) << 1) | (p >> 1)) << 4) + ((p & 1) << 3);
        }
    f4 acc[2][2][KK];
    int co0, ci0;
    wg_begin(a, smem, acc, co0, ci0);

    const int dpx = lane >> 3, dsp = lane & 7;
    const int dma_px = wave * 8 + dpx;
    const int dma_slot = (((dsp >> 1) ^ ((dma_px >> 1) & 3)) << 1) | (dsp & 1);
    const unsigned lane_x = (unsigned)(((dma_px - PAD) * a.x_cs + ci0 + dma_slot * 8) * 2);
    const unsigned lane_y = (unsigned)((dma_px * a.dy_cs + co0 + dma_slot * 8) * 2);
    const unsigned rowx = (unsigned)(a.W * a.x_cs * 2), rowy = (unsigned)(a.W * a.dy_cs * 2);
    const unsigned planex = (unsigned)(a.x_split * 2), planey = (unsigned)(a.dy_split * 2);
    const unsigned dma_lds = (unsigned)__builtin_amdgcn_readfirstlane(wave * 1024);

    WgSeg sg;
    bool okx, oky;
    auto segment = [&](const WgSeg s_) {
        sg = s_;
        okx = dma_px < sg.Wc + 2 * PAD && (unsigned)(sg.ox0 - PAD + dma_px) < (unsigned)a.W;
        oky = dma_px < sg.Wc;
    };
    auto fetch_x = [&](int n, int slot) {
        const int Y = sg.ya - PAD + n;
        const bool rowok = (unsigned)Y < (unsigned)a.H;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const unsigned off = (okx && rowok) ? sg.bx0 + (unsigned)Y * rowx + (unsigned)pl * planex + lane_x : a.x_zero;
            pn_glds16_s<0>(a.x, off, (unsigned)(slot * ROWB + pl * 4096) + dma_lds);
        }
    };
    auto fetch_y = [&](int n, int slot) {
        const int Y = sg.ya + n;
        const bool rowok = Y < sg.yb;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const unsigned off = (oky && rowok) ? sg.by0 + (unsigned)Y * rowy + (unsigned)pl * planey + lane_y : a.dy_zero;
            pn_glds16_s<0>(a.dy, off, (unsigned)(XRING + slot * ROWB + pl * 4096) + dma_lds);
        }
    };
    // the dy fragment of the row is read once and multiplied, product-major, with the KK shifted x fragments (the next tap's are requested before this tap's MFMAs)
    auto row_body = [&](int u) {
        auto load_a = [&](bf8 (&A)[2][2]) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    const bf4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4 *)(smem + addrA[mt] + u * ROWB + pl * 4096));
                    const bf4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4 *)(smem + addrA[mt] + u * ROWB + pl * 4096 + 2048));
                    A[mt][pl] = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                }
        };
        auto load_b = [&](int tp, bf8 (&Bf)[2][2]) {
            const int ky = tp / KS, kx = tp - ky * KS;
            const int xs = ((u + ky) % RING) * ROWB;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    const bf4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4 *)(smem + addrB[kx][nt] + xs + pl * 4096));
                    const bf4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4 *)(smem + addrB[kx][nt] + xs + pl * 4096 + 2048));
                    Bf[nt][pl] = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                }
        };
        bf8 A[2][2], Bq[2][2][2];
        load_a(A);
        load_b(0, Bq[0]);
#pragma unroll
        for (int tp = 0; tp < KK; ++tp) {
            const int cur = tp & 1, nxt = cur ^ 1;
            __builtin_amdgcn_sched_barrier(0);
            if (tp + 1 < KK) load_b(tp + 1, Bq[nxt]);
#pragma unroll
            for (int pr = 0; pr < 3; ++pr)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[mt][nt][tp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[mt][pr == 1 ? 1 : 0], Bq[cur][nt][pr == 2 ? 1 : 0], acc[mt][nt][tp], 0, 0, 0);
            if (tp + 1 < KK) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    wg_walk<KS, D, 2>(a, segment, fetch_x, fetch_y, row_body);
    wg_store(a, acc, co0, ci0, wm, wn, lane);
}

// ---- fp32 form (precision "fp32": exact fp32 FMA chains on v_mfma_f32_16x16x4_f32) -------------------------------------------------------------------
// K = 4 pixels per MFMA and ONE value per lane and operand: lane (m, kg) multiplies dy[pixel 4 s + kg][co m] with x[pixel 4 s + kg + tap][ci n] -- a channel-minor
// tensor needs no transpose at all here (16 lanes read 16 consecutive channels).  Same row-streaming rings (five rows of x, five of dy, 256 B per pixel: 80 KB),
// 16-byte slots XOR-swizzled by the pixel's parity so that the two pixels a half-wave's ds_read_b32 touches fall on different banks.
template <int KS, int D>
__global__ __launch_bounds__(256, 2) void wgrad_f32_kernel(WgArgs a) {
    typedef __attribute__((address_space(3))) float ldsf;
    constexpr int KK = KS * KS, PAD = KS / 2, RING = WG_RING, ROWB = WG_ROWB, XRING = WG_XRING;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int m = lane & 15, kg = lane >> 4;
    // fragment addresses: pixel 4 s + kg (+ kx), channel window of 16; the channel is XORed with 16 on odd pixels
    int addrA[2], addrB[KS][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) addrA[mt] = XRING + kg * 256 + ((((wm * 2 + mt) * 16 + m) ^ ((kg & 1) << 4)) << 2);
#pragma unroll
    for (int kx = 0; kx < KS; ++kx)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) addrB[kx][nt] = (kg + kx) * 256 + ((((wn * 2 + nt) * 16 + m) ^ (((kg + kx) & 1) << 4)) << 2);
    f4 acc[2][2][KK];
    int co0, ci0;
    wg_begin(a, smem, acc, co0, ci0);

    // DMA: one instruction = 4 pixels x 16 slots of 16 B; wave w fetches pixel groups w and w + 4 of every row
    const int dq = lane >> 4, dsp = lane & 15;
    unsigned lane_x[2], lane_y[2];
    int dpx[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        dpx[h] = (wave + 4 * h) * 4 + dq;
        const int ls = dsp ^ ((dpx[h] & 1) << 2);
        lane_x[h] = (unsigned)(((dpx[h] - PAD) * a.x_cs + ci0 + ls * 4) * 4);
        lane_y[h] = (unsigned)((dpx[h] * a.dy_cs + co0 + ls * 4) * 4);
    }
    const unsigned rowx = (unsigned)(a.W * a.x_cs * 4), rowy = (unsigned)(a.W * a.dy_cs * 4);
    const unsigned dma_lds0 = (unsigned)__builtin_amdgcn_readfirstlane(wave * 1024);

    WgSeg sg;
    bool okx[2], oky[2];
    auto segment = [&](const WgSeg s_) {
        sg = s_;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            okx[h] = dpx[h] < sg.Wc + 2 * PAD && (unsigned)(sg.ox0 - PAD + dpx[h]) < (unsigned)a.W;
            oky[h] = dpx[h] < sg.Wc;
        }
    };
    auto fetch_x = [&](int n, int slot) {
        const int Y = sg.ya - PAD + n;
        const bool rowok = (unsigned)Y < (unsigned)a.H;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned off = (okx[h] && rowok) ? sg.bx0 + (unsigned)Y * rowx + lane_x[h] : a.x_zero;
            pn_glds16_s<0>(a.x, off, (unsigned)(slot * ROWB + h * 4096) + dma_lds0);
        }
    };
    auto fetch_y = [&](int n, int slot) {
        const int Y = sg.ya + n;
        const bool rowok = Y < sg.yb;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned off = (oky[h] && rowok) ? sg.by0 + (unsigned)Y * rowy + lane_y[h] : a.dy_zero;
            pn_glds16_s<0>(a.dy, off, (unsigned)(XRING + slot * ROWB + h * 4096) + dma_lds0);
        }
    };
    // items (k-step s, tap): the two x values of item i + 1 are requested before the four MFMAs of item i
    auto row_body = [&](int u) {
        auto ld_a = [&](int s_, float (&A)[2]) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) A[mt] = *(const ldsf *)(smem + addrA[mt] + u * ROWB + s_ * 1024);
        };
        auto ld_b = [&](int s_, int tp, float (&Bv)[2]) {
            const int ky = tp / KS, kx = tp - ky * KS;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) Bv[nt] = *(const ldsf *)(smem + addrB[kx][nt] + ((u + ky) % RING) * ROWB + s_ * 1024);
        };
        float A[2][2], Bq[2][2];
        ld_a(0, A[0]);
        ld_b(0, 0, Bq[0]);
#pragma unroll
        for (int s_ = 0; s_ < 8; ++s_)
#pragma unroll
            for (int tp = 0; tp < KK; ++tp) {
                const int it = s_ * KK + tp, cur = it & 1, nxt = cur ^ 1, ac = s_ & 1;
                __builtin_amdgcn_sched_barrier(0);
                if (tp + 1 < KK) ld_b(s_, tp + 1, Bq[nxt]);
                else if (s_ + 1 < 8) { ld_b(s_ + 1, 0, Bq[nxt]); ld_a(s_ + 1, A[ac ^ 1]); }
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[mt][nt][tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[ac][mt], Bq[cur][nt], acc[mt][nt][tp], 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
    };
    wg_walk<KS, D, 4>(a, segment, fetch_x, fetch_y, row_body);
    wg_store(a, acc, co0, ci0, wm, wn, lane);
}

// dw[co][ref ci][tap] = sum over the split slices, in a fixed order; k_map: this engine's input channel -> the reference's (nullptr = identity).
// Block = 16 consecutive elements x 16 split lanes: lane l adds slices l, l + 16, ... (independent loads in flight), thread (element, lane 0) adds the
// 16 lane sums in order.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ partial, int S, int KK, int co_pad, int ci_pad, int Cout, int Cin, const int *__restrict__ k_map,
                                                            float *__restrict__ dw) {
    __shared__ float sh[16][17];
    const int el = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const size_t tap_stride = (size_t)co_pad * ci_pad, split_stride = tap_stride * KK;
    const size_t e = (size_t)blockIdx.x * 16 + el;                   // element of one slice: (tap, co, ci)
    float s = 0.f;
    if (e < split_stride) {
        const float *p = partial + e;
        int sp = sl;
        for (; sp + 48 < S; sp += 64) {
            const float v0 = p[(size_t)sp * split_stride], v1 = p[(size_t)(sp + 16) * split_stride], v2 = p[(size_t)(sp + 32) * split_stride], v3 = p[(size_t)(sp + 48) * split_stride];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; sp < S; sp += 16) s += p[(size_t)sp * split_stride];
    }
    sh[sl][el] = s;
    __syncthreads();
    if (sl != 0 || e >= split_stride) return;
    float t = 0.f;
#pragma unroll
    for (int l = 0; l < 16; ++l) t += sh[l][el];
    const int tp = (int)(e / tap_stride);
    const int rem = (int)(e - (size_t)tp * tap_stride);
    const int co = rem / ci_pad, ci = rem - co * ci_pad;
    if (co >= Cout) return;
    const int ref = k_map ? k_map[ci] : (ci < Cin ? ci : -1);
    if (ref < 0) return;
    dw[((size_t)co * Cin + ref) * KK + tp] = t;
}

// What a plan decided (diagnostics: the length of the fp32 summation chains of one output element is rows_per_block rows of <= Wt pixels in a block, then Sr slices)
struct WgPlan { int tiles_x = 0, Wt = 0, rows_per_block = 0, Sr = 0; };

// What differs between the two forms: the kernel, the stored planes per tensor and the wording of the errors.
template <class T> struct Wg;
template <> struct Wg<bf> {
    static constexpr int planes = 2;
    static constexpr const char *name = "weight gradient on planes", *operands = "planes";
    template <int KS> static void (*kernel())(WgArgs) { return wgrad_stream_kernel<KS, 2>; }
};
template <> struct Wg<float> {
    static constexpr int planes = 1;
    static constexpr const char *name = "fp32 weight gradient", *operands = "tensors";
    template <int KS> static void (*kernel())(WgArgs) { return wgrad_f32_kernel<KS, 2>; }
};

template <class T, int KS>
int launch_wgrad(pn_ctx *ctx, dim3 grid, size_t lds, hipStream_t s, const WgArgs &w) {
    static PnLdsAttr attr;                                  // one per kernel instantiation
    void (*const kern)(WgArgs) = Wg<T>::template kernel<KS>();
    if (int rc = pn_lds_attr(ctx, attr, reinterpret_cast<const void *>(kern), lds)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, w);
    return PN_OK;
}

// Plans the weight gradient of one layer and appends its two launches to `ops`.  *partial_floats grows to what the layer needs; the
// buffer itself (*partial) is allocated by the caller after every layer has been planned (the kernels read the pointer at launch time).
// T = bf: [hi | lo] bf16 planes (wgrad_stream_kernel); T = float: one fp32 plane (wgrad_f32_kernel).
template <class T>
int plan_wgrad(pn_ctx *ctx, int B, int H, int W, const T *x, int x_plane, const T *dy, int dy_plane, int Cin, int Cout, int ks, const int *k_map, float *dw,
               float *const *partial, size_t *partial_floats, std::vector<std::function<int(hipStream_t)>> &ops, WgPlan *plan = nullptr) {
    if (ks != 1 && ks != 3) return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "%s: kernel size %d not built", Wg<T>::name, ks);
    const int KK = ks * ks, pad = ks / 2;
    const int seg_max = 32 - 2 * pad;                      // a halo row holds 32 pixels
    WgArgs w;
    memset(&w, 0, sizeof w);
    w.x = x; w.x_cs = Wg<T>::planes * x_plane; w.x_zero = (unsigned)((size_t)B * H * W * w.x_cs * sizeof(T));
    w.dy = dy; w.dy_cs = Wg<T>::planes * dy_plane; w.dy_zero = (unsigned)((size_t)B * H * W * w.dy_cs * sizeof(T));
    if (Wg<T>::planes == 2) { w.x_split = x_plane; w.dy_split = dy_plane; }
    w.B = B; w.H = H; w.W = W;
    w.tiles_x = (W + seg_max - 1) / seg_max;
    w.Wt = (W + w.tiles_x - 1) / w.tiles_x;
    const int ci_my = k_map ? x_plane : Cin;               // channels of x that carry weights (the stage-2 input: the whole plane, re-ordered)
    const int ncot = (Cout + 63) / 64;
    w.ncit = (ci_my + 63) / 64;
    w.co_pad = ncot * 64; w.ci_pad = w.ncit * 64;
    if (w.co_pad > dy_plane || w.ci_pad > x_plane) return pn_set_error(ctx, PN_ERR_INVALID, "%s: channel tiles exceed the %s", Wg<T>::name, Wg<T>::operands);
    const int pairs = ncot * w.ncit;
    // split-K slices: ONE block per CU.  Every slice costs a 147 KB partial tile written and read back, and a lone 64 KB block leaves the rest of the CU to
    // the BatchNorm / data-gradient launches of the step's own stream (same box, eager step: 1/2 block per CU 7.10 ms, 1: 6.49-6.68, 1.5: 6.93, 2: 7.03, 3: 7.39)
    w.rows_total = B * w.tiles_x * H;
    int Sr = std::max(1, std::min(w.rows_total, (ctx->num_cus + pairs - 1) / pairs));
    w.rows_per_block = (w.rows_total + Sr - 1) / Sr;
    Sr = (w.rows_total + w.rows_per_block - 1) / w.rows_per_block;
    *partial_floats = std::max(*partial_floats, (size_t)Sr * KK * w.co_pad * w.ci_pad);
    if (plan) { plan->tiles_x = w.tiles_x; plan->Wt = w.Wt; plan->rows_per_block = w.rows_per_block; plan->Sr = Sr; }
    const size_t ldss = (size_t)2 * WG_XRING;              // two rings of five rows
    ops.push_back([=](hipStream_t s) {
        WgArgs ww = w;
        ww.partial = *partial;                             // the host reads the pointer when the step launches (the buffer exists by then)
        if (int rc = ks == 3 ? launch_wgrad<T, 3>(ctx, dim3(Sr, pairs), ldss, s, ww) : launch_wgrad<T, 1>(ctx, dim3(Sr, pairs), ldss, s, ww)) return rc;
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)(((size_t)KK * ww.co_pad * ww.ci_pad + 15) / 16)), dim3(256), 0, s, (const float *)ww.partial, Sr, KK, ww.co_pad, ww.ci_pad, Cout, Cin, k_map, dw);
        PN_HIP_CHECK(ctx, hipGetLastError());
        return (int)PN_OK;
    });
    return PN_OK;
}

}  // namespace tx
