// bf16 3x3 stride-1 "same" convolution on the CDNA4 matrix cores, third generation: BOTH operands through LDS.
//
// Same math as conv3_kernel.h / conv_mfma_kernel.h; block order, tile decode and epilogues are conv_common.h's (it replaces the same reference code:
// tpm/lib/network/rtpose_light3d.py:24-72,222-246; yolo_posenet.py:101-126; resnet.py:27-56) for the layers that
// dominate the conv time: 3x3, Cin >= 128, >= 64 couts, maps that split into <= 30-column strips.
//
// Why (round-1 counters, profiles/r01_final_pmc_ta_vs_mfma.txt): conv3_kernel's 128-cout x 112-pixel blocks stream their
// whole weight slice global -> VGPR per block (146 B per MFMA through the per-CU vector-memory path: TA busy 1.18x the
// matrix pipe) and every wave re-reads all 7 activation fragments per 14 MFMAs (LDS array ~100 % busy with the 2-way
// conflict of the half-major image).  Here
//   * a wave owns 64 couts x 112 pixels (4 x 7 accumulator tiles, 28 MFMAs per k-step): 11 LDS fragment reads per 28
//     MFMAs instead of 7 per 14;
//   * a block = 2 cout halves x 2 pixel strips (128 couts x 224 pixels, 4 waves); the weight fragments of a k-step
//     (8 KB) are fetched ONCE per block by LDS-DMA into a 3-slot ring and shared by the two strips: 95 B per MFMA
//     through the vector-memory path (weights + halo) instead of 146 + halo;
//   * the two strips are independent 4-row x <= 28-column tiles (own halo images), so a 28-row map wastes nothing;
//   * activations: quarter-major halo images ([2 quarters][halo row][32 px][32 B] per 32-channel half: conflict-free
//     fragment reads, see below), double-buffered
//     per HALF (12 KB per strip and buffer): the next half's image is fetched, one DMA instruction per k-step, while
//     the current half's 9 taps run -- no hand-over stall;
//   * ONE barrier per k-step (28 MFMAs per wave), LDS-DMA kept in flight across it with counted vmcnt (the guide's
//     "pipelining across barriers": raw s_barrier, never vmcnt(0) inside the loop);
//   * <= 256 VGPRs, 2 waves / SIMD, 72 KB of LDS: two blocks per CU.
// Weight pack (net.hip::pack_conv4): [cout block of 128][k-step][8 cout tiles][64 lanes][8 bf16]: one k-step of a block
// is 8 KB contiguous, each DMA instruction copies 1 KB of consecutive bytes.
// k order: (32-channel half hh, tap) -- identical to conv3's (chunk, half, tap).
#pragma once
#include "conv_common.h"

#define PN4_ASLOT 8192                  // one k-step of weight fragments: 8 cout tiles x 1 KB
constexpr int PN4_RING = 3;             // weight ring slots: the slot of a k-step is an immediate offset
constexpr int PN4_PITCH = 32;           // halo pixels per LDS row
#define PN4_ARING (PN4_RING * PN4_ASLOT)
#define PN4_BQUART (5 * PN4_PITCH * 32 + 1024)   // one 16-channel quarter plane of a strip image: 6 halo rows x PITCH px x 32 B (the last row: the 1 KiB a DMA writes)
#define PN4_BSTRIP (2 * PN4_BQUART)     // one 32-channel half image of one strip
#define PN4_BBUF (2 * PN4_BSTRIP)       // both strips
#define PN4_LDS (PN4_ARING + 2 * PN4_BBUF)

// One block of problem P; block_x = the block's index within the problem's launch (blockIdx.x of conv4_kernel).
__device__ __forceinline__ void conv4_body(const ConvProblem &P, const int block_x) {
    typedef __bf16 T;
    constexpr int KS = 3, KK = 9, PT = 7, CT = 4, PITCH = PN4_PITCH;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    if (block_x >= P.nblocks) return;
    const int bx = pn_xcd_block(block_x, P.nblocks);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = wave >> 1, wc = wave & 1;            // strip, cout half
    const int c = lane & 15, q = lane >> 4;

    const int cb = bx % P.cout_blocks;
    const int pair = bx / P.cout_blocks;
    const int nstrips = P.B * P.tiles_per_img;
    const int sid_raw = pair * 2 + wp;
    const bool strip_ok = sid_raw < nstrips;             // an odd strip count leaves the last block half empty
    const int sid = strip_ok ? sid_raw : nstrips - 1;
    const int Wo = P.Wo;
    const PnTile tl = pn_tile_decode(sid, P.tiles_per_img, P.tiles_x, P.R, P.Wt, P.Ho, Wo);      // this wave's strip
    const int b = tl.b, oy0 = tl.oy0, ox0 = tl.ox0, Wc = tl.Wc, npix = tl.npix;
    const int HC = Wc + KS - 1;
    const int iy0 = oy0 - 1, ix0 = ox0 - 1;
    const float inv_wc = tl.inv_wc;
    const int nchunks = P.cin_chunks;

    // ---- weight ring: wave w fetches cout tiles 2w, 2w+1 of every k-step (2 x 1 KB of consecutive bytes) ----
    const char *aptr = (const char *)P.wpack + ((size_t)cb * (size_t)(P.ksteps + 3) * 8 + 2 * wave) * 1024;   // + 3 spare k-steps behind every cout block
    const unsigned alane16 = (unsigned)lane * 16u;
    auto dma_a = [&](int slot) {
        const unsigned dst = (unsigned)(slot * PN4_ASLOT) + (unsigned)__builtin_amdgcn_readfirstlane(wave * 2048);
        // (no instruction offset: the immediate of an LDS-DMA is added to the LDS address as well as to the global one)
        pn_glds16_s<0>(aptr, alane16, dst);
        pn_glds16_s<0>(aptr + 1024, alane16, dst + 1024u);
        aptr += PN4_ASLOT;
    };

    // ---- halo images: this wave fetches DMA pieces n = wc*6 + j (j = 0..5) of ITS strip: halo row n >> 1, pixels 16*(n&1).. ----
    const size_t frame_b = ((size_t)b * P.H * P.W * P.in_cs + P.in_coff) * 2;
    const char *img = (const char *)P.in + frame_b;                          // + hh * 64 per half (scalar)
    const unsigned zero_rel = P.in_zero_off - (unsigned)frame_b;                // zero page (>= 64 * halves + 16 bytes of zeros) relative to img
    // QUARTER-major images ([2 quarters of 16 channels][halo row][32 px][32 B] per 32-channel half): the 16 lanes one
    // ds_read_b128 phase serves (8 with an even, 8 with an odd lane quarter) cover 8 pixels x 32 B = a whole bank row,
    // conflict-free, where the half-major image of conv3 ([row][px][64 B]) costs 2 LDS cycles per read.  One DMA
    // instruction = one 32-pixel halo row of one quarter; wave wc fetches quarter wc (6 rows).
    unsigned boff[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int px = lane >> 1;
        const int iy = iy0 + j, ix = ix0 + px;
        const bool inb = px < HC && (unsigned)ix < (unsigned)P.W && (unsigned)iy < (unsigned)P.H;
        boff[j] = inb ? (unsigned)((iy * P.W + ix) * P.in_cs * 2 + wc * 32 + (lane & 1) * 16) : zero_rel;
    }
    const int nhalves = nchunks * 2, wrap_h = P.in_wrap * 2;
    auto dma_b = [&](int j, int buf, int hh) {       // piece j of half hh -> image `buf` of this strip
        const unsigned dst = (unsigned)(PN4_ARING + buf * PN4_BBUF + j * (PITCH * 32)) +
                             (unsigned)__builtin_amdgcn_readfirstlane(wp * PN4_BSTRIP + wc * PN4_BQUART);
        const int hs = hh < nhalves ? (hh >= wrap_h ? hh - wrap_h : hh) : 0;        // bf16x3: the third plane pair reads the hi plane again; past the last half: a harmless refetch into the idle image
        pn_glds16_s<0>(img + (size_t)hs * 64, boff[j], dst);
    };

    // ---- prologue: image of half 0, weight k-steps 0..2 ----
#pragma unroll
    for (int j = 0; j < 6; ++j) dma_b(j, 0, 0);
    dma_a(0); dma_a(1); dma_a(2);

    // per-lane LDS read addresses: tap / buffer / slot are immediates
    int baddr[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
        const int slot = pt * 16 + c;
        const int s = slot < npix ? slot : 0;
        int ry, rx;
        pn_slot_pixel(s, inv_wc, Wc, ry, rx);
        baddr[pt] = PN4_ARING + wp * PN4_BSTRIP + (q >> 1) * PN4_BQUART + (q & 1) * 16 + (ry * PITCH + rx) * 32;
    }
    const int aaddr = wc * 4096 + lane * 16;
    f32x4 acc[CT][PT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // a wave whose 64 couts lie beyond the layer's cout (a 64-cout conv sharing the launch of a 128-cout sibling) only
    // takes part in the DMA and the barriers
    const bool active = (cb * 2 + wc) * 64 < P.cout;

    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");

    // item j = (phase ph, pixel tile pt): B fragment of tap ph % 9 from image (ph / 9) & 1
#define PN4_BOFF(j) (((((j) / PT) / KK) & 1) * PN4_BBUF + (((((j) / PT) % KK) / KS) * PITCH + ((((j) / PT) % KK) % KS)) * 32)
    // B fragments are read BQ - 1 items (4 MFMAs each) ahead of their use: with 2 ahead a lone wave on its SIMD spent
    // 147 of 717 cycles per k-step waiting for LDS (profiles/README.md, conv4 ablations)
    constexpr int BQ = 6;
    static_assert((2 * KK * PT) % BQ == 0, "queue slot of an item must not depend on the chunk");
    bf16x8 aq[2][CT], bq[BQ];
    if (active) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) aq[0][ct] = *reinterpret_cast<const bf16x8 *>(smem + aaddr + ct * 1024);
#pragma unroll
        for (int j = 0; j < BQ - 1; ++j) bq[j] = *reinterpret_cast<const bf16x8 *>(smem + baddr[j % PT] + PN4_BOFF(j));
    }
    // phase 0 refills ring slot 0: every wave's reads of k-step 0's fragments must have returned first
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // the K loop, instantiated with and without the arithmetic (an inactive wave keeps the DMA schedule and the barriers)
    auto kloop = [&](auto mathc) {
        constexpr bool MATH = decltype(mathc)::value;
        for (int chunk = 0; chunk < nchunks; ++chunk) {
#pragma clang loop unroll(full)
            for (int ph = 0; ph < 2 * KK; ++ph) {            // k-step s = chunk * 18 + ph
                const int tap = ph % KK, half = ph / KK;
                const int hh = chunk * 2 + half;
                const int anext = aaddr + ((ph + 1) % 3) * PN4_ASLOT;
                // (1) staging for later steps: one halo piece of the NEXT half (taps 0..5), the weight fragments of step s + 3
                if (tap < 6) dma_b(tap, (half + 1) & 1, hh + 1);
                dma_a(ph % 3);
                // (2) this step's 28 MFMAs; fragment reads for the next step / the next items between them
                if (MATH) {
                    __builtin_amdgcn_sched_barrier(0);
#pragma clang loop unroll(full)
                    for (int pt = 0; pt < PT; ++pt) {
                        const int j = ph * PT + pt, jr = j + BQ - 1;
                        if (pt < CT)
                            aq[(ph + 1) & 1][pt] = *reinterpret_cast<const bf16x8 *>(smem + anext + pt * 1024);
                        bq[jr % BQ] = *reinterpret_cast<const bf16x8 *>(smem + baddr[jr % PT] + PN4_BOFF(jr % (2 * KK * PT)));
#pragma unroll
                        for (int ct = 0; ct < CT; ++ct)
                            acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq[ph & 1][ct], bq[j % BQ], acc[ct][pt], 0, 0, 0);
                        if (pt < CT) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                        else __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008, CT, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                // (3) everything older than the newest weight step (and this phase's halo piece) has landed; every fragment
                // read issued so far has returned (the slot / image it came from may be overwritten after the barrier)
                if (tap < 6) asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)\n\ts_barrier" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
        }
    };
    if (active) kloop(std::true_type{});
    else kloop(std::false_type{});
#undef PN4_BOFF
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the surplus prefetches must not land in LDS after this block has exited
    if (!active || !strip_ok) return;

    // ---- epilogue (conv_common.h): a lane holds 16 CONSECUTIVE couts of each of its pixels (net.hip packs the rows with
    // pn_conv_row_channel(tile, row, 4)): bias + residual + activation + two 16-B NHWC stores per pixel tile and plane; the four
    // lane quarters cover one whole 128-B line of the pixel ----
    constexpr int LC = CT * 4;
    const int wave_c0 = (cb * 2 + wc) * 64;
    const int cw = wave_c0 + LC * q;
    const int cout = P.cout, act = P.act, naf = P.yolo_naf;
    float bias[LC];
    pn_load_bias<LC>(P.bias, cw, bias);
    const int res_cs = P.res_cs, out_cs = P.out_cs, Ho = P.Ho;
    const int split = P.split, res_split = P.res_split;
    const int pix0 = (b * Ho + oy0) * Wo + ox0;
    if (wave_c0 + 64 <= cout && P.out && !P.out_nchw) {      // wave-uniform: the fast epilogue, pixel = (baddr - plane base) / 32 B
        const int plane0 = PN4_ARING + wp * PN4_BSTRIP + (q >> 1) * PN4_BQUART;
        pn_with_act<true>(act, P.res != nullptr, [&](auto actc, auto resc) {
            pn_conv_epilogue_fast<decltype(actc)::value, decltype(resc)::value, false, T, CT, PT>(
                acc, bias, baddr, [plane0](int a) { return (unsigned)(a - plane0) >> 5; }, c, npix, (unsigned)pix0, (unsigned)Wo,
                (PN_GLOBAL T *)P.out + P.out_coff + wave_c0, (const PN_GLOBAL T *)P.res + P.res_coff + wave_c0, (unsigned)(LC * q),
                (unsigned)res_cs, res_split, (unsigned)out_cs, split, act, cw, naf);
        });
        return;
    }
    // ragged cout, NCHW f32 export
    const PN_GLOBAL T *res_base = P.res ? (const PN_GLOBAL T *)P.res + P.res_coff + cw : nullptr;
    PN_GLOBAL T *out_base = P.out ? (PN_GLOBAL T *)P.out + P.out_coff + cw : nullptr;
    pn_with_act<true>(act, [&](auto actc) {
        pn_conv_epilogue<decltype(actc)::value, T, CT, PT>(acc, bias, c, npix, inv_wc, Wc, cw, cout, act, naf, res_base, res_cs, res_split, out_base,
                                                           out_cs, split, (PN_GLOBAL float *)P.out_nchw, b, Ho, Wo, oy0, ox0, pix0);
    });
}

__global__ __launch_bounds__(256, 2) void conv4_kernel(const ConvProblem *__restrict__ probs) {
    conv4_body(probs[blockIdx.y], (int)blockIdx.x);
}

static int conv4_launch(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream) {
    const size_t lds = PN4_LDS;
    static PnLdsAttr attr;
    if (int rc = pn_lds_attr(ctx, attr, reinterpret_cast<const void *>(conv4_kernel), lds)) return rc;
    hipLaunchKernelGGL(conv4_kernel, dim3(L.max_blocks, L.nprob), dim3(256), lds, stream, L.probs_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}
