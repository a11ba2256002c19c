// Fused ResNet BasicBlock(64) on the CDNA4 matrix cores (bf16 storage, fp32 accumulate):
//     y = relu( conv3x3(relu(conv3x3(x, W1) + b1), W2) + b2 + x )            64 -> 64 -> 64 channels, stride 1
// replaces the two launches per block of tpm/lib/network/rtpose_light3d.py:48-72 (BasicBlock.forward) for model0.layer1
// (tpm/lib/network/rtpose_light3d.py:145-152) and resnet.BasicBlock (tpm/lib/network/resnet.py:27-56) for YoloPoseNet's
// layer1.  BatchNorm is folded into W / b on the host (net.hip).
//
// Why: at 112x112 these layers are not arithmetic: unfused, a BasicBlock moves 297 MB per 32 frames (conv1 reads x with
// its halo and writes the 51 MB intermediate, conv2 reads it back with halo, reads x again as the residual and writes
// y) in memory-bound prologue / epilogue phases that every resident block runs in lockstep (45 us per conv for 12 us of
// MFMA work, profiles/README.md r01 v21).  Here the intermediate never leaves the CU and x is read once:
//   * one PERSISTENT workgroup per CU walks its share of the 8-row x <=28-column output tiles;
//   * per tile the 12 x 32-pixel input halo (48 KB, quarter-major [quarter][row][32 px][32 B]) sits in LDS, conv1 is evaluated on
//     the 10 x 30 intermediate halo (1.34x recompute) straight into a second LDS image (40 KB, zero outside the map =
//     conv2's padding), conv2 reads that image, the residual comes from the CENTRE of the input image (no second read
//     of x), and y leaves with 16-B stores;
//   * the input image is double-buffered: the next tile's image is fetched during this tile's conv1, the stores of
//     this tile drain under the next tile's conv1 -- no lockstep memory phases;
//   * 8 waves (HV = 1) with FIXED ROLES: waves 0-3 compute (each 64 couts x 5 / 3 1/2 pixel tiles: 20 / 14 MFMAs per k-step, B
//     fragments from the images, A fragments from a 6-slot LDS ring), waves 4-7 only issue LDS-DMA and count their own
//     vmcnt -- a compute wave's instruction stream is MFMA + ds_read only (conv4_kernel's ablations: DMA issue and its
//     waits cost a lone wave 80 of 717 cycles per k-step).  Round 3: the loaders are split by STREAM -- waves 4, 5 fetch
//     weights (W1 | W2 as one periodic 36-step stream, L2-resident: one 4 KB k-step each per phase, landed one phase later),
//     waves 6, 7 the next tile's input image (HBM / Infinity Cache latency) and wait for it only at the end of the tile.
//     vmcnt retires in issue order, so with both streams on one wave (round 2) every phase of conv1 waited for an image
//     piece issued one phase earlier: 530 cycles per 320-cycle phase against 355 per 256 in conv2 (lab timeline);
//   * one barrier per TWO k-steps (a bare s_barrier for the compute waves: their fragment reads stay in flight across it):
//     20 barriers per tile instead of 38; 160 KB of LDS, one workgroup per CU.
//   * round 5: the tiles are handed out by TICKET (one atomic per tile, fetched a tile ahead by an image-loader wave and published through sixteen spare
//     bytes of the intermediate image), not by blockIdx.x + k * gridDim.x: a persistent workgroup can only start on a CU that holds no other wave, so among
//     the other in-flight batches' launches some workgroups start late -- with the static schedule the launch ended when the LATEST starter had walked its
//     seven tiles; now the early ones take its share.  Which workgroup computes which tile changes, nothing else.
//   * conv2 has no padding pixel tiles: a full tile's 224 outputs are 14 pixel tiles, three whole ones per compute wave plus tiles 12 and 13 split
//     by cout-tile pairs (wave 0: tile 12, cout tiles 0-1; wave 1: tile 12, 2-3; wave 2: tile 13, 0-1; wave 3: tile 13, 2-3).  Four tiles per wave
//     were 16: one MFMA in eight of conv2 computed on padding.  Odd waves hold the cout tiles in the order 2, 3, 0, 1 (addresses only);
//   * the last phase of each convolution (k-steps 16, 17: both in the weight ring) runs PIXEL TILE OUTER: a tile's accumulators are final while
//     the tiles after it still have MFMAs to issue, and its epilogue (bias + ReLU + pack + ds_write, or residual + bias + ReLU + pack + store) is
//     placed among those MFMAs with sched_group_barrier.  Only the last tile's epilogue (conv2: the half tile's) runs with the matrix pipe idle.
//     The epilogues are branch-free for that (a branch ends the scheduling region): conv1 slots past the tile compute a spare pixel of the images;
//   * the folded biases sit in spare bytes of the intermediate image, not in 32 registers: 242 VGPRs, no scratch (tests/test_bb64_resources.py).
// Every (cout tile, pixel tile) accumulator keeps its k order and its MFMA whichever wave owns it: bit-identical to the two-launch plan
// (tests/test_gpu_bb64_tiles.py, tests/test_gpu_parity.py).
// Weight pack (net.hip): [36 k-steps = (conv, half, tap)][4 cout tiles][64 lanes][8 bf16], rows permuted with
// pn_conv_row_channel(tile, row, 4) so that a lane's 16 accumulators are 16 consecutive channels.
// bb64s_kernel.h is this kernel (HV = 1) handing out column segments instead of tiles and carrying the intermediate's two overlap rows down a segment;
// net_run.hip chooses between the two per launch.
// bb64_common.h holds what the two kernels share, each piece described at its code: the LDS layout, the weight-loader stream, the image-piece DMA, the
// ticket sign-off, the fragment reads, the k-step-outer MFMA loop and the output epilogue.
#pragma once
#include "bb64_common.h"


// HV = 1 (default): four compute waves of 64 couts.  HV = 2 (round 5, POPNET_BB64_HALVES=2): EIGHT compute waves -- the four pixel groups times two
// cout halves, two per SIMD, so that one wave's fragment reads and barrier waits hide behind the other's MFMAs.  Same LDS images, same weight ring,
// same k order per output: bit-identical.  Measured (lab timeline, 32 x 112 x 112): the third tile takes 17 877 shader cycles instead of 19 595
// (the intermediate write 1 944 instead of 3 057), the whole kernel 126 k instead of 136 k -- and 73.2-74.2 us instead of 71.8-72.1: the in-kernel
// clock read 1.56 GHz against 1.71.  The package draws 1 370 W of its 1 400 W limit under this kernel (rocm-smi, profiles/r05_power.txt): twelve
// waves and 55 % more LDS bytes per k-step (both halves read every B fragment) cost the clock what they save in cycles.  Kept as a switch.
template <int HV>
__global__ __launch_bounds__((4 * HV + 4) * 64, 1) void bb64_kernel(const BBProblem P) {
    constexpr int CT = 4 / HV, NCW = 4 * HV, NP = CT / 2, PT1 = 5, PT2 = 4, BQ = BB_BQ;
    constexpr bool SPLIT = HV == 1;                      // conv2 without padding tiles (below)
    constexpr bool XCH = HV == 1;                        // last phase of each convolution pixel tile outer, epilogues among its MFMAs
    constexpr int NKO = XCH ? 16 : 18;                   // k-steps that run k-step outer
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, q = lane >> 4;
    const int W = P.W, H = P.H;

    // ticket slots: pixel column 31 of row 0 of the intermediate image's first quarter plane is never written (MC <= 30) nor read (x + kx <= 29)
    volatile int *s_tile = reinterpret_cast<volatile int *>(smem + BB_OFF_TICKET);
    const bool dyn = P.tickets != nullptr;
    // tile k + 1 of this workgroup, as every wave sees it at the start of tile k (static schedule: t + gridDim.x)
    auto next_tile = [&](int t, int k) -> int { return dyn ? __builtin_amdgcn_readfirstlane(s_tile[(k + 1) & 3]) : t + (int)gridDim.x; };
    // (the compute and weight-loader waves need it at the END of tile k only: they issue the LDS read at the start and look at it there)
    auto next_tile_raw = [&](int t, int k) -> int { return dyn ? s_tile[(k + 1) & 3] : t + (int)gridDim.x; };
    auto tile_geom = [&](int t, int &b, int &oy0, int &ox0, int &R, int &Wc) {
        b = t / P.tiles_per_img;
        const int rem = t - b * P.tiles_per_img;
        const int ty = rem / P.tiles_x, tx = rem - ty * P.tiles_x;
        oy0 = ty * 8; ox0 = tx * P.Wt;
        R = min(8, H - oy0); Wc = min(P.Wt, W - ox0);
    };

    if (wave >= NCW) {
        // ================= loader waves: LDS-DMA only =================
        const int lw = wave - NCW;
        const unsigned lane16 = (unsigned)lane * 16u;
        int t = blockIdx.x;
        if (t >= P.ntiles) return;
        if (lw < 2) {
            // ---- weight loaders ----
            const char *wsrc = (const char *)P.wpack + lw * 2048;
            auto dma_a = [&](int kstep) { bb_dma_a(wsrc, lane16, lw, kstep); };
            bb_weights_prologue(dma_a);
            for (int k = 0; t < P.ntiles; ++k) {
                const int tnx = next_tile_raw(t, k);
                bb_weights_tile(dma_a);
                t = __builtin_amdgcn_readfirstlane(tnx);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            return;
        }
        // ---- image loaders: wave 6 / 7 fetches pieces 0..23 / 24..47 of the NEXT tile's input image, two per phase ----
        auto dma_in = [&](int tt, int buf, int n) {            // piece n of tile tt
            int b, oy0, ox0, R, Wc;
            tile_geom(tt, b, oy0, ox0, R, Wc);
            bb_dma_in(P, H, W, lane, b, oy0, ox0, Wc, buf, n);
        };
        const int n0 = (lw - 2) * 24;
        const bool ticketer = dyn && lw == 2 && lane == 0;      // this lane fetches the tickets: tile k + 2 during tile k
        int ticket = 0;
        // (hybrids -- the first tiles of a workgroup by position, only its last 1, 2 or 3 by ticket -- measured no better than the static schedule:
        //  profiles/r05_notes.txt)
        // The first TWO tiles of a workgroup are its position (the prologue waits for no atomic).  Launches with fewer than four tiles per workgroup
        // (56 x 56 maps: 448 tiles on 256 workgroups) keep the static schedule altogether (net.hip passes no counters): with the second tile a ticket
        // YoloPoseNet lost 1.5 % (96.1 / 95.9 / 96.3 k against 98.0 / 97.7 / 96.4 k frames/s, same box, profiles/r05_notes.txt).
        auto claim = [&]() -> int { return 2 * (int)gridDim.x + atomicAdd(P.tickets, 1); };
        if (ticketer) ticket = t + (int)gridDim.x;
#pragma unroll
        for (int j = 0; j < 24; ++j) dma_in(t, 0, n0 + j);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (ticketer) s_tile[1] = ticket;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        asm volatile("s_barrier" ::: "memory");
        int cur = 0;
        for (int k = 0; t < P.ntiles; ++k) {
            const int tnx = next_tile(t, k);
            const int tn = tnx < P.ntiles ? tnx : t;             // past the last tile: a harmless refetch into the idle image
            // a workgroup on its LAST tile has no use for another ticket: it signs off instead (looked at after the end-of-tile wait, ten microseconds
            // later: the kernel's end does not wait for an atomic's round trip)
            int signed_off = -1;
            if (ticketer) {
                if (tnx < P.ntiles) ticket = claim();
                else signed_off = atomicAdd(P.tickets + 1, 1);
            }
#pragma clang loop unroll(full)
            for (int p = 0; p < 18; ++p) {
                if (p < 12) { dma_in(tn, cur ^ 1, n0 + 2 * p); dma_in(tn, cur ^ 1, n0 + 2 * p + 1); }
                asm volatile("s_barrier" ::: "memory");
                if (p == 8) asm volatile("s_barrier" ::: "memory");
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                           // end of tile: the next image is complete (and the ticket is back)
            if (ticketer) {
                s_tile[(k + 2) & 3] = ticket;
                bb_sign_off(P.tickets, signed_off, (int)gridDim.x);
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            cur ^= 1;
            t = tnx;
        }
        return;
    }

    // ================= compute waves =================
    int t = blockIdx.x;
    if (t >= P.ntiles) return;
    const int pw = HV == 2 ? (wave & 3) : wave, hv = HV == 2 ? (wave >> 2) : 0;            // pixel group, cout half
    if (wave == 0) {                                    // lane = channel 16 q + c; published by the second prologue barrier
        *reinterpret_cast<float *>(smem + BB_BIAS(0, q) + c * 4) = P.bias1[lane];
        *reinterpret_cast<float *>(smem + BB_BIAS(1, q) + c * 4) = P.bias2[lane];
    }
    // HV = 1: a full 8 x 28 tile has 14 pixel tiles of conv2 outputs; four per wave would be 16, two of them padding on the critical path of every
    // k-step.  Each wave takes three whole pixel tiles (3 pw ..) and HALF of a leftover one: tile 12 + (pw >> 1), cout tiles 2 h, 2 h + 1 with
    // h = pw & 1 -- 14 MFMAs per k-step instead of 16, the same four A and four B fragment reads.  So that the half tile's cout tiles are
    // compile-time registers, a wave with h = 1 holds the cout tiles in the order 2, 3, 0, 1: fragment / accumulator slot i is cout tile i ^ 2 h
    // everywhere (conv1 too), which only moves addresses -- the A fragment, the bias and the 16-byte piece of a pixel's quarter entry.
    const int h = SPLIT ? (pw & 1) : 0;
    auto pct = [&](int i) -> int { return SPLIT ? (i ^ (2 * h)) : hv * CT + i; };       // cout tile of slot i
    auto pc = [&](int k) -> int { return SPLIT ? (k ^ h) : hv * NP + k; };              // 16-byte piece (8 channels) of slot pair k
    const int biasaddr = BB_BIAS(0, q);                 // this lane's quarter: channels 16 q ..
    float b1[4 * CT], b2[4 * CT];                       // live in an epilogue only
    // two bases reach every weight fragment with an immediate offset (slots 0, 1 and slots 2, 3: cout tiles 2 h .. and 2 - 2 h ..); opaque, or the
    // compiler folds BB_OFF_A into per-ring-slot bases of its own, a dozen registers held for the whole kernel
    int aaddr0 = BB_OFF_A + lane * 16 + pct(0) * 1024, aaddr1 = aaddr0 ^ 2048;
    asm volatile("" : "+v"(aaddr0), "+v"(aaddr1));
    bf16x8 aq[2][CT], bq[BQ];
    asm volatile("s_barrier" ::: "memory");             // prologue: first image + weight k-steps 0..2 landed
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) aq[0][ct] = *reinterpret_cast<const bf16x8 *>(smem + (ct < 2 ? aaddr0 : aaddr1) + (ct & 1) * 1024);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    int cur = 0;
    for (int it = 0; t < P.ntiles; ++it) {
        const int tnx = next_tile_raw(t, it);
        int b, oy0, ox0, R, Wc;
        tile_geom(t, b, oy0, ox0, R, Wc);
        const int MC = Wc + 2, nmid = (R + 2) * MC, nout = R * Wc;
        const float inv_mc = 1.0f / (float)MC, inv_wc = 1.0f / (float)Wc;
        const int inb = cur * BB_IN;
        // conv2's pixel tile of slot pt (SPLIT: slot 3 is the half tile)
        auto out_tile = [&](int pt) -> int { return !SPLIT ? pw * PT2 + pt : pt < 3 ? pw * 3 + pt : 12 + (pw >> 1); };
        // per-lane image addresses (tap and half are immediates).  A tile-local copy of c: what is derived from it is recomputed per tile (one or two VALU per slot) instead of being held in eighteen
        // registers for the whole kernel.  (float)s + 0.5f == fc + (float)(s - c) exactly: small half-integers.
        int cc = c;
        asm volatile("" : "+v"(cc));
        const float fc = (float)cc + 0.5f;
        const int ba1base = inb + (q >> 1) * BB_INQ + (q & 1) * 16, ba2base = BB_OFF_MID + (q >> 1) * BB_MIDQ + (q & 1) * 16;
        // conv1 slots past nmid compute pixel (3, 30 + (c & 1)) instead: a real address of the input image to read, and in the intermediate image spare
        // bytes (pixel columns 30, 31) to write -- their epilogue needs no branch round the write, which would end the scheduling region it is placed in
        const int dumppix = (3 * 32 + 30 + (cc & 1)) * 32;
        int ba1[PT1], ba2[PT2];
#pragma unroll
        for (int pt = 0; pt < PT1; ++pt) {
            const int sb = (pw * PT1 + pt) * 16, s = sb + cc;
            const int r = (int)((fc + (float)sb) * inv_mc), x = s - r * MC;
            ba1[pt] = ba1base + (s < nmid ? (r * 32 + x) * 32 : dumppix);
        }
#pragma unroll
        for (int pt = 0; pt < PT2; ++pt) {
            const int sb = out_tile(pt) * 16, s = sb + cc;
            const int r = (int)((fc + (float)sb) * inv_wc), x = s - r * Wc;
            ba2[pt] = ba2base + (s < nout ? (r * 32 + x) * 32 : 0);
        }
        f32x4 acc[CT][PT1];
        // ---------------- the two epilogues, one pixel tile each, branch-free (a branch would end the scheduling region they are placed in) ----------------
        // (r, x) of a slot come back out of its image address
        const bool border = oy0 == 0 || ox0 == 0 || oy0 + R >= H || ox0 + Wc >= W;        // wave-uniform
        // intermediate: bias + ReLU -> bf16 -> LDS image (zero outside the map).  Piece pc(0) of the lane's quarter entry; with NP = 2 piece pc(1) is ^ 16
        const int midw = BB_OFF_MID + q * BB_MIDQ + 16 * pc(0);
        auto epi1 = [&](int pt) {
            const int pix = ba1[pt] - ba1base, r = pix >> 10, x = (pix >> 5) & 31;
            const bool inside = (unsigned)(oy0 - 1 + r) < (unsigned)H && (unsigned)(ox0 - 1 + x) < (unsigned)W;
            const unsigned keep = !border || inside ? 0xffffffffu : 0u;       // conv2's zero padding
            // bias + ReLU as add + max, two channels per v_cvt_pk_bf16_f32; the zero padding outside the map is applied to the
            // 8 packed dwords (per pixel), not per channel: a lone wave pays every VALU instruction of this block in full
            // ReLU on the PACKED bf16 pair (a negative bf16 is a negative int16: one v_pk_max_i16 per two channels; rounding is
            // monotonic, so relu(bf16(v)) == bf16(relu(v)))
            u32x4 o[NP];                                 // this lane's 8 * NP channels of the pixel
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                f32x2 lo = {acc[ct][pt][0] + b1[4 * ct + 0], acc[ct][pt][1] + b1[4 * ct + 1]};
                f32x2 hi = {acc[ct][pt][2] + b1[4 * ct + 2], acc[ct][pt][3] + b1[4 * ct + 3]};
                o[ct >> 1][2 * (ct & 1)] = bb_relu_pk(__builtin_bit_cast(unsigned, __builtin_convertvector(lo, bf16x2))) & keep;
                o[ct >> 1][2 * (ct & 1) + 1] = bb_relu_pk(__builtin_bit_cast(unsigned, __builtin_convertvector(hi, bf16x2))) & keep;
            }
            const int dsta = midw + pix;                  // (slots past nmid: spare bytes)
            *reinterpret_cast<u32x4 *>(smem + dsta) = o[0];
            if (NP == 2) *reinterpret_cast<u32x4 *>(smem + (dsta ^ 16)) = o[NP - 1];
        };
        // output: bias + residual (centre of the input image) + ReLU, 16-B stores (two per pixel; one for the half tile)
        const int resw = inb + q * BB_INQ + (2 * 32 + 2) * 32 + 16 * pc(0);
        __amdgpu_buffer_rsrc_t orsrc;
        auto epi2 = [&](int pt) {
            bb_epi2<CT, SPLIT>(smem, acc, b2, pt, ba2[pt] - ba2base, out_tile(pt) * 16 + cc < nout, resw, orsrc, oy0, ox0, W, P.out_cs, q, pc);
        };
        // (aq[0] holds k-step 0's weight fragments: read in the prologue / prefetched by the previous tile's last phase)
        // ---------------- conv1: 18 k-steps on the input image ----------------
        bb_kouter<PT1, NKO, 0, BB_INQ, false>(smem, aaddr0, aaddr1, ba1, acc, aq, bq);
#pragma unroll
        for (int i = 0; i < CT; ++i) *reinterpret_cast<f32x4 *>(b1 + 4 * i) = *reinterpret_cast<const f32x4 *>(smem + biasaddr + 16 * pct(i));
        if constexpr (XCH) {
            // last phase, pixel tile outer (bb_item_*): the intermediate epilogue of a finished tile is issued among the MFMAs of the tiles after it
            // (BB_FILL1 VALU / SALU / ds_write per MFMA); only the last tile's epilogue is exposed.  aq[0] = k-step 16, aq[1] = k-step 17, read here.
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
        } else {
#pragma clang loop unroll(full)
            for (int pt = 0; pt < PT1; ++pt) epi1(pt);
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        // ---------------- conv2: 18 k-steps on the intermediate image ----------------
        bb_kouter<PT2, NKO, 18, BB_MIDQ, SPLIT>(smem, aaddr0, aaddr1, ba2, acc, aq, bq);
#pragma unroll
        for (int i = 0; i < CT; ++i) *reinterpret_cast<f32x4 *>(b2 + 4 * i) = *reinterpret_cast<const f32x4 *>(smem + biasaddr + 1024 + 16 * pct(i));
        orsrc = __builtin_amdgcn_make_buffer_rsrc((char *)P.out + ((size_t)b * H * W * P.out_cs + P.out_coff) * 2, 0, (int)((size_t)H * W * P.out_cs * 2), 0x00020000);
        if constexpr (XCH) {
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
        } else {
#pragma clang loop unroll(full)
            for (int pt = 0; pt < PT2; ++pt) epi2(pt);
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");       // the loader may now refill this image's buffer
        cur ^= 1;
        t = __builtin_amdgcn_readfirstlane(tnx);
    }
}

static int bb64_launch(pn_ctx *ctx, const BBProblem &P, int num_cus, hipStream_t stream) {
    static PnLdsAttr attr[2];
    const int halves = P.halves == 2 ? 2 : 1;        // 2 (POPNET_BB64_HALVES=2 when the net was compiled): the eight-compute-wave form -- 7 % fewer cycles, 2-3 % MORE time
    if (int rc = pn_lds_attr(ctx, attr[halves - 1], halves == 2 ? reinterpret_cast<const void *>(bb64_kernel<2>) : reinterpret_cast<const void *>(bb64_kernel<1>), BB_LDS)) return rc;
    const int grid = P.ntiles < num_cus ? P.ntiles : num_cus;
    if (halves == 2) hipLaunchKernelGGL(bb64_kernel<2>, dim3(grid), dim3(768), BB_LDS, stream, P);
    else hipLaunchKernelGGL(bb64_kernel<1>, dim3(grid), dim3(512), BB_LDS, stream, P);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}
