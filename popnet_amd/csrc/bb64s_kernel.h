// Fused ResNet BasicBlock(64), bf16, walking COLUMN SEGMENTS top-down (the "strip kernel"): bb64_kernel<1> (bb64_kernel.h: LDS images, weight ring,
// loader-wave roles, barrier cadence, epilogues -- read that header first; bb64_common.h: the code the two kernels share) without most of its conv1
// recompute.
//
// bb64_kernel evaluates conv1 on the 10 x 30 intermediate halo of every 8 x 28 output tile: 20 MFMAs per k-step and compute wave where conv2 takes 14.
// Rows 0 and 1 of that halo are rows 8 and 9 of the tile above.  Here a workgroup takes SEGMENTS of consecutive row tiles of one column instead of
// single tiles and keeps those two rows:
//   * a column (frame, strip of <= 28 output columns) of T = ceil(H / 8) row tiles is cut into S segments whose lengths differ by at most one, the longer
//     ones on top (net_run.hip chooses S: the smallest count that gives every CU a segment, at most T / 2 -- a segment has at least two tiles);
//   * the FIRST tile of a segment runs bb64_kernel's conv1: 10 rows, PT1 = 5;
//   * every further tile is CARRIED: after the end-of-tile barrier the two image-loader waves copy rows 8, 9 of the intermediate image to rows 0, 1
//     (pixel columns 0..29 of the four quarter planes: 480 x 16 B through registers; columns 30, 31 hold the biases and the ticket slot), and conv1
//     covers rows 2..9 only: 8 x 30 = 240 pixels = 15 pixel tiles, PT1 = 4, 16 MFMAs per k-step and wave.  The copy is complete before the loaders
//     reach the first barrier of the tile; conv1 writes rows 8, 9 in its last phase and conv2 reads rows 0, 1 after the "publish" barrier;
//   * conv2, the residual and the stores are bb64_kernel's (the k-step-outer loop and the output epilogue through bb64_common.h).  The tile loop holds two unrolled conv1 bodies behind a wave-uniform branch and ONE conv2 body;
//   * the first segment of a workgroup is its position; where there are more segments than workgroups the further ones come through the ticket counter
//     (claimed during a segment's first tile, published at that tile's end, looked at from its last tile on), with bb64_kernel's sign-off: the workgroup
//     that signs off last leaves both counters at zero.
// A carried row is the same sum in the same k order from the same MFMA as the row the tile would have recomputed: bit-identical to bb64_kernel and to
// the two-launch plan (tests/test_gpu_bb64_strip.py).
#pragma once
#include <type_traits>
#include "bb64_common.h"

__global__ __launch_bounds__(512, 1) void bb64s_strip_kernel(const BBProblem P) {
    constexpr int CT = 4, NCW = 4, NP = 2, PT2 = 4, BQ = BB_BQ, NKO = 16;
    constexpr bool SPLIT = true, XCH = true;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, q = lane >> 4;
    const int W = P.W, H = P.H;
    const int nseg = P.nseg, grid = (int)gridDim.x;

    // ticket slot (as bb64_kernel's): pixel column 31 of row 0 of the intermediate image's first quarter plane is never written nor read as pixels
    volatile int *s_next = reinterpret_cast<volatile int *>(smem + BB_OFF_TICKET);
    const bool dyn = P.tickets != nullptr;
    // the segment after `seg` of this workgroup; the slot is valid from the end of the segment's first tile on, and is looked at in its last tile (>= second)
    auto next_seg_raw = [&](int seg) -> int { return dyn ? s_next[0] : seg + grid; };
    // segment -> frame, column strip, first row tile, number of row tiles
    auto seg_geom = [&](int seg, int &b, int &ox0, int &Wc, int &ty0, int &len) {
        const int col = seg / P.strip_S, si = seg - col * P.strip_S;
        b = col / P.tiles_x;
        const int tx = col - b * P.tiles_x;
        ox0 = tx * P.Wt; Wc = min(P.Wt, W - ox0);
        const int base = P.strip_T / P.strip_S, rem = P.strip_T - base * P.strip_S;
        ty0 = si * base + min(si, rem);
        len = base + (si < rem ? 1 : 0);
    };

    int seg = blockIdx.x;
    if (seg >= nseg) return;
    int sb_, sox0, sWc, sty0, slen, j = 0;              // this workgroup's segment and the tile of it (wave-uniform)
    seg_geom(seg, sb_, sox0, sWc, sty0, slen);

    if (wave >= NCW) {
        // ================= loader waves: LDS-DMA only =================
        const int lw = wave - NCW;
        const unsigned lane16 = (unsigned)lane * 16u;
        if (lw < 2) {
            // ---- weight loaders (the 36-step stream does not depend on the conv1 body) ----
            const char *wsrc = (const char *)P.wpack + lw * 2048;
            auto dma_a = [&](int kstep) { bb_dma_a(wsrc, lane16, lw, kstep); };
            bb_weights_prologue(dma_a);
            while (seg < nseg) {
                const int snx = next_seg_raw(seg);
                bb_weights_tile(dma_a);
                if (++j == slen) {
                    seg = __builtin_amdgcn_readfirstlane(snx);
                    j = 0;
                    seg_geom(seg, sb_, sox0, sWc, sty0, slen);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            return;
        }
        // ---- image loaders: the next tile's input image (all 12 rows: the four shared ones were read a tile ago), the carry, the tickets ----
        auto dma_in = [&](int b, int oy0, int ox0, int Wc, int buf, int n) { bb_dma_in(P, H, W, lane, b, oy0, ox0, Wc, buf, n); };
        const int n0 = (lw - 2) * 24;
        const bool ticketer = dyn && lw == 2 && lane == 0;
        int ticket = 0;
        // the carry: 16-byte piece i = (lw - 2) * 64 + lane + 128 n of the 480 = 4 quarter planes x rows 8, 9 x 60 pieces (pixel columns 0..29)
        int cpy[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int i = (lw - 2) * 64 + lane + 128 * n;
            const int qp = i / 120, r = (i - qp * 120) / 60, w = i - qp * 120 - r * 60;
            cpy[n] = i < 480 ? BB_OFF_MID + qp * BB_MIDQ + (8 + r) * 1024 + w * 16 : -1;
        }
#pragma unroll
        for (int n = 0; n < 24; ++n) dma_in(sb_, sty0 * 8, sox0, sWc, 0, n0 + n);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_barrier" ::: "memory");
        asm volatile("s_barrier" ::: "memory");
        int cur = 0;
        while (seg < nseg) {
            if (j > 0) {                                 // a carried tile: rows 8, 9 of the tile above become its rows 0, 1
                u32x4 v[4];
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    if (cpy[n] >= 0) v[n] = *reinterpret_cast<const u32x4 *>(smem + cpy[n]);
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    if (cpy[n] >= 0) *reinterpret_cast<u32x4 *>(smem + cpy[n] - 8 * 1024) = v[n];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // landed before this wave reaches the tile's first barrier
            }
            // the tile after this one: the next of the segment, the first of the next segment, or none (a harmless refetch into the idle image)
            const bool lastj = j == slen - 1;
            int nsg = seg, nb = sb_, nox0 = sox0, nWc = sWc, nty0 = sty0, nlen = slen, nj = j + 1;
            if (lastj) {
                nsg = __builtin_amdgcn_readfirstlane(next_seg_raw(seg));
                nj = 0;
                if (nsg < nseg) seg_geom(nsg, nb, nox0, nWc, nty0, nlen);
                else nj = j;
            }
            const int noy0 = (nty0 + nj) * 8;
            // tickets: a segment's successor is claimed during its first tile.  Once a claim has come back past the last segment this workgroup makes
            // no further claim: it signs off during the second tile.  The workgroup that signs off last knows every claim has been made and leaves
            // both counters at zero for the next launch (graph replay).
            int signed_off = -1;
            if (ticketer) {
                if (j == 0) ticket = grid + atomicAdd(P.tickets, 1);
                else if (j == 1 && ticket >= nseg) signed_off = atomicAdd(P.tickets + 1, 1);
            }
#pragma clang loop unroll(full)
            for (int p = 0; p < 18; ++p) {
                if (p < 12) { dma_in(nb, noy0, nox0, nWc, cur ^ 1, n0 + 2 * p); dma_in(nb, noy0, nox0, nWc, cur ^ 1, n0 + 2 * p + 1); }
                asm volatile("s_barrier" ::: "memory");
                if (p == 8) asm volatile("s_barrier" ::: "memory");
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                           // end of tile: the next image is complete (and the atomic is back)
            if (ticketer) {
                if (j == 0) s_next[0] = ticket;
                bb_sign_off(P.tickets, signed_off, grid);
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            cur ^= 1;
            if (lastj) { seg = nsg; sb_ = nb; sox0 = nox0; sWc = nWc; sty0 = nty0; slen = nlen; j = 0; }
            else j = nj;
        }
        return;
    }

    // ================= compute waves =================
    const int pw = wave;
    if (wave == 0) {                                    // lane = channel 16 q + c; published by the second prologue barrier
        *reinterpret_cast<float *>(smem + BB_BIAS(0, q) + c * 4) = P.bias1[lane];
        *reinterpret_cast<float *>(smem + BB_BIAS(1, q) + c * 4) = P.bias2[lane];
    }
    // bb64_kernel's split of conv2's fourteen pixel tiles: three whole ones per wave plus half of tile 12 + (pw >> 1); odd waves hold the cout tiles in
    // the order 2, 3, 0, 1 (slot i is cout tile i ^ 2 h, conv1 too)
    const int h = pw & 1;
    auto pct = [&](int i) -> int { return i ^ (2 * h); };       // cout tile of slot i
    auto pc = [&](int k) -> int { return k ^ h; };              // 16-byte piece (8 channels) of slot pair k
    const int biasaddr = BB_BIAS(0, q);
    float b1[4 * CT], b2[4 * CT];                       // live in an epilogue only
    int aaddr0 = BB_OFF_A + lane * 16 + pct(0) * 1024, aaddr1 = aaddr0 ^ 2048;
    asm volatile("" : "+v"(aaddr0), "+v"(aaddr1));
    bf16x8 aq[2][CT], bq[BQ];
    asm volatile("s_barrier" ::: "memory");             // prologue: first image + weight k-steps 0..2 landed
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) aq[0][ct] = *reinterpret_cast<const bf16x8 *>(smem + (ct < 2 ? aaddr0 : aaddr1) + (ct & 1) * 1024);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    int cur = 0;
    while (seg < nseg) {
        const int snx = next_seg_raw(seg);
        const int b = sb_, ox0 = sox0, Wc = sWc, oy0 = (sty0 + j) * 8, R = min(8, H - oy0);
        const int MC = Wc + 2, nout = R * Wc;
        const float inv_mc = 1.0f / (float)MC, inv_wc = 1.0f / (float)Wc;
        const int inb = cur * BB_IN;
        auto out_tile = [&](int pt) -> int { return pt < 3 ? pw * 3 + pt : 12 + (pw >> 1); };
        int cc = c;
        asm volatile("" : "+v"(cc));
        const float fc = (float)cc + 0.5f;
        const int ba1base = inb + (q >> 1) * BB_INQ + (q & 1) * 16, ba2base = BB_OFF_MID + (q >> 1) * BB_MIDQ + (q & 1) * 16;
        // conv1 slots past the tile compute pixel (3, 30 + (c & 1)): a real address of the input image to read, spare bytes of the intermediate to write
        const int dumppix = (3 * 32 + 30 + (cc & 1)) * 32;
        int ba2[PT2];
#pragma unroll
        for (int pt = 0; pt < PT2; ++pt) {
            const int sb = out_tile(pt) * 16, s = sb + cc;
            const int r = (int)((fc + (float)sb) * inv_wc), x = s - r * Wc;
            ba2[pt] = ba2base + (s < nout ? (r * 32 + x) * 32 : 0);
        }
        f32x4 acc[CT][5];
        const bool border = oy0 == 0 || ox0 == 0 || oy0 + R >= H || ox0 + Wc >= W;        // wave-uniform
        const int midw = BB_OFF_MID + q * BB_MIDQ + 16 * pc(0);
        // ---------------- conv1: 18 k-steps on the input image, intermediate rows ROW0..9 in PT1 pixel tiles per wave ----------------
        // (aq[0] holds k-step 0's weight fragments: read in the prologue / prefetched by the previous tile's last phase)
        auto conv1 = [&](auto pt1c) __attribute__((always_inline)) {
            constexpr int PT1 = decltype(pt1c)::value;
            constexpr int ROW0 = PT1 == 5 ? 0 : 2;       // 5: the whole 10-row halo (first tile of a segment); 4: rows 2..9, rows 0, 1 carried
            const int nmid = (R + 2 - ROW0) * MC;
            int ba1[PT1];
#pragma unroll
            for (int pt = 0; pt < PT1; ++pt) {
                const int sb = (pw * PT1 + pt) * 16, s = sb + cc;
                const int r = (int)((fc + (float)sb) * inv_mc), x = s - r * MC;
                ba1[pt] = ba1base + (s < nmid ? ((r + ROW0) * 32 + x) * 32 : dumppix);
            }
            // intermediate: bias + ReLU -> bf16 -> LDS image (zero outside the map = conv2's padding); (r, x) of a slot come back out of its image address
            auto epi1 = [&](int pt) {
                const int pix = ba1[pt] - ba1base, r = pix >> 10, x = (pix >> 5) & 31;
                const bool inside = (unsigned)(oy0 - 1 + r) < (unsigned)H && (unsigned)(ox0 - 1 + x) < (unsigned)W;
                const unsigned keep = !border || inside ? 0xffffffffu : 0u;
                u32x4 o[NP];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    f32x2 lo = {acc[ct][pt][0] + b1[4 * ct + 0], acc[ct][pt][1] + b1[4 * ct + 1]};
                    f32x2 hi = {acc[ct][pt][2] + b1[4 * ct + 2], acc[ct][pt][3] + b1[4 * ct + 3]};
                    o[ct >> 1][2 * (ct & 1)] = bb_relu_pk(__builtin_bit_cast(unsigned, __builtin_convertvector(lo, bf16x2))) & keep;
                    o[ct >> 1][2 * (ct & 1) + 1] = bb_relu_pk(__builtin_bit_cast(unsigned, __builtin_convertvector(hi, bf16x2))) & keep;
                }
                const int dsta = midw + pix;                  // (slots past nmid: spare bytes)
                *reinterpret_cast<u32x4 *>(smem + dsta) = o[0];
                *reinterpret_cast<u32x4 *>(smem + (dsta ^ 16)) = o[1];
            };
            bb_kouter<PT1, NKO, 0, BB_INQ, false>(smem, aaddr0, aaddr1, ba1, acc, aq, bq);
#pragma unroll
            for (int i = 0; i < CT; ++i) *reinterpret_cast<f32x4 *>(b1 + 4 * i) = *reinterpret_cast<const f32x4 *>(smem + biasaddr + 16 * pct(i));
            // last phase, pixel tile outer (bb_item_*): the epilogue of a finished tile among the MFMAs of the tiles after it; the last tile's is exposed
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) aq[1][ct] = BB_A(17, ct);
#pragma clang loop unroll(full)
            for (int m = 0; m < 2 * PT1; ++m) {
                const int n = 16 * PT1 + m, nr = n + BQ - 1, pt = bb_item_pt(n, PT1, true), ks = bb_item_ks(n, PT1, true);
                if (nr < 18 * PT1) bq[nr % BQ] = BB_B1(nr);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq[ks & 1][ct], bq[n % BQ], acc[ct][pt], 0, 0, 0);
                if (m == 2 * PT1 - 2) {                  // k-step 16's fragments have been used up: conv2's first k-step
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) aq[0][ct] = BB_A(18, ct);
                }
                if (ks == 17 && pt < PT1 - 1) epi1(pt);
                if (m == 0) __builtin_amdgcn_sched_group_barrier(0x100, CT + 1, 0);
                else if (nr < 18 * PT1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if (m >= 3) __builtin_amdgcn_sched_group_barrier(0x206, BB_FILL1, 0);
                }
                if (m == 2 * PT1 - 2) __builtin_amdgcn_sched_group_barrier(0x100, CT, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_barrier" ::: "memory");      // end of the phase
            epi1(PT1 - 1);
        };
        if (j == 0) conv1(std::integral_constant<int, 5>());
        else conv1(std::integral_constant<int, 4>());
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");       // the intermediate image is published
        // ---------------- conv2: 18 k-steps on the intermediate image (bb64_kernel's, unchanged) ----------------
        // output: bias + residual (centre of the input image) + ReLU, 16-B stores (two per pixel; one for the half tile)
        const int resw = inb + q * BB_INQ + (2 * 32 + 2) * 32 + 16 * pc(0);
        __amdgpu_buffer_rsrc_t orsrc;
        auto epi2 = [&](int pt) {
            bb_epi2<CT, SPLIT>(smem, acc, b2, pt, ba2[pt] - ba2base, out_tile(pt) * 16 + cc < nout, resw, orsrc, oy0, ox0, W, P.out_cs, q, pc);
        };
        bb_kouter<PT2, NKO, 18, BB_MIDQ, SPLIT>(smem, aaddr0, aaddr1, ba2, acc, aq, bq);
#pragma unroll
        for (int i = 0; i < CT; ++i) *reinterpret_cast<f32x4 *>(b2 + 4 * i) = *reinterpret_cast<const f32x4 *>(smem + biasaddr + 1024 + 16 * pct(i));
        orsrc = __builtin_amdgcn_make_buffer_rsrc((char *)P.out + ((size_t)b * H * W * P.out_cs + P.out_coff) * 2, 0, (int)((size_t)H * W * P.out_cs * 2), 0x00020000);
        // last phase as in conv1, with the output epilogue (residual read, stores) among the MFMAs; the exposed last epilogue is the half tile's.
        // aq[0] = k-step 34, aq[1] = k-step 35; the next tile's k-step 0 follows into aq[0]
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) aq[1][ct] = BB_A(35, ct);
#pragma clang loop unroll(full)
        for (int m = 0; m < 2 * PT2; ++m) {
            const int n = 16 * PT2 + m, nr = n + BQ - 1, pt = bb_item_pt(n, PT2, true), ks = bb_item_ks(n, PT2, true);
            const int nct = pt == 3 ? 2 : CT;
            if (nr < 18 * PT2) bq[nr % BQ] = BB_B2(nr);
#pragma unroll
            for (int ct = 0; ct < nct; ++ct)
                acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq[ks & 1][ct], bq[n % BQ], acc[ct][pt], 0, 0, 0);
            if (m == 2 * PT2 - 2) {
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) aq[0][ct] = BB_A(36, ct);
            }
            if (ks == 17 && pt < PT2 - 1) epi2(pt);
            if (m == 0) __builtin_amdgcn_sched_group_barrier(0x100, CT + 1, 0);
            else if (nr < 18 * PT2) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
            for (int ct = 0; ct < nct; ++ct) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (m >= 3) __builtin_amdgcn_sched_group_barrier(0x146, BB_FILL2, 0);
            }
            if (m == 2 * PT2 - 2) __builtin_amdgcn_sched_group_barrier(0x100, CT, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_barrier" ::: "memory");      // end of the phase
        epi2(PT2 - 1);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");       // end of tile: the loaders may refill this image's buffer and carry rows 8, 9
        cur ^= 1;
        if (++j == slen) {
            seg = __builtin_amdgcn_readfirstlane(snx);
            j = 0;
            seg_geom(seg, sb_, sox0, sWc, sty0, slen);
        }
    }
}

static int bb64s_launch(pn_ctx *ctx, const BBProblem &P, int num_cus, hipStream_t stream) {
    static PnLdsAttr attr;
    if (P.strip_S < 1 || P.strip_T < 2 * P.strip_S || P.nseg != P.B * P.tiles_x * P.strip_S)
        return pn_set_error(ctx, PN_ERR_INVALID, "bb64s: %d segments per column of %d row tiles (every segment needs two tiles)", P.strip_S, P.strip_T);
    if (int rc = pn_lds_attr(ctx, attr, reinterpret_cast<const void *>(bb64s_strip_kernel), BB_LDS)) return rc;
    const int grid = P.nseg < num_cus ? P.nseg : num_cus;
    hipLaunchKernelGGL(bb64s_strip_kernel, dim3(grid), dim3(512), BB_LDS, stream, P);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}
