// Direct (im2col-free) convolution on CDNA4 matrix cores.
//
// Replaces the cuDNN calls behind nn.Conv2d + BatchNorm2d(eval) + (Leaky)ReLU / residual add /
// sigmoid range casts of the reference networks:
//   conv3x3 / conv1x1 / BasicBlock      tpm/lib/network/rtpose_light3d.py:24-72
//   make_stages Conv2d+BN+LeakyReLU     tpm/lib/network/rtpose_light3d.py:222-246
//   forward() sigmoid casts             tpm/lib/network/rtpose_light3d.py:335-337,348-350
//   YoloPoseNet neck/head + slice casts tpm/lib/network/yolo_posenet.py:101-126,146-156
//   resnet.BasicBlock (stride-2 + 1x1)  tpm/lib/network/resnet.py:27-56,134-148
//
// Formulation: D[cout][pixel] = sum_k W[cout][k] * X[k][pixel], k = (cin-chunk, tap, cin).
//   * MFMA "A" operand = weights, streamed global -> VGPR.  They are pre-packed on the host in
//     exactly the per-lane fragment order, so one wave-load is 1 KiB (bf16) of contiguous memory.
//   * MFMA "B" operand = activations.  A block owns R full output rows of one image; the input
//     halo tile ((R-1)*stride+KS rows x Wo*stride+KS-1 cols x 64 channels) is staged once per
//     64-channel chunk into LDS and re-read by all KS*KS taps and all cout tiles.
//   * LDS image: [halo pixel][64 ch], 128 B (bf16) / 256 B (f32) per pixel, row pitch a multiple
//     of 8 pixels, 16-B (bf16) / 32-B (f32) slots XOR-swizzled with (pixel & 7) so that the 16
//     lanes ds_read_b128 services together hit 16 different slots of the 256-B bank row.
//   * bf16: v_mfma_f32_16x16x32_bf16, fp32 accumulate.  f32 ("parity" mode):
//     v_mfma_f32_16x16x4_f32, bit-exact fp32 FMA chains (no xf32 on gfx950).
//   * C/D layout (col = lane&15 -> pixel, row = 4*(lane>>4)+reg -> cout): each lane ends up
//     with 4 consecutive output channels of one pixel = one 8-B / 16-B NHWC store.
//   * Epilogue fuses folded-BN bias, residual add, ReLU / LeakyReLU(0.1) / sigmoid casts, and
//     can emit NHWC (next layer) and/or NCHW f32 (API boundary) in the same pass.
#pragma once
#include "conv_common.h"
#include "conv_inst_table.h"

template <int CFG> struct TileCfg;
template <> struct TileCfg<PN_CFG_C128> { static constexpr int WC = 4, WP = 1, CT = 2, PT = 7; };
template <> struct TileCfg<PN_CFG_C64>  { static constexpr int WC = 2, WP = 2, CT = 2, PT = 4; };
template <> struct TileCfg<PN_CFG_C32>  { static constexpr int WC = 1, WP = 4, CT = 2, PT = 2; };
template <> struct TileCfg<PN_CFG_C16>  { static constexpr int WC = 1, WP = 4, CT = 1, PT = 2; };
template <> struct TileCfg<PN_CFG_C64W> { static constexpr int WC = 2, WP = 2, CT = 2, PT = 7; };

template <int PREC> __device__ __forceinline__ typename Elem<PREC>::Frag load_a_frag(gcptr p);
template <> __device__ __forceinline__ Elem<PN_PREC_BF16>::Frag load_a_frag<PN_PREC_BF16>(gcptr p) {
    Elem<PN_PREC_BF16>::Frag f;
    f.v = *reinterpret_cast<const PN_GLOBAL bf16x8 *>(p);
    return f;
}
template <> __device__ __forceinline__ Elem<PN_PREC_F32>::Frag load_a_frag<PN_PREC_F32>(gcptr p) {
    Elem<PN_PREC_F32>::Frag f;   // packed as [half][lane][4 floats]: both halves lane-contiguous
    f.lo = *reinterpret_cast<const PN_GLOBAL f32x4 *>(p);
    f.hi = *reinterpret_cast<const PN_GLOBAL f32x4 *>(p + 1024);
    return f;
}

// Register-prefetched halo staging: MAXST = 16-B pieces per thread needed to hold the largest halo
// tile of this geometry (pn_conv_stage_maxpx is the host-side mirror used when R is chosen);
// 0 = too many registers, stage with the plain load->store loop instead.
constexpr int pn_stage_maxpx_c(int ks, int stride, int pitch) {
    return stride != 1 ? 0 : (ks == 1 ? 128 : (pitch <= 32 ? 192 : (pitch <= 64 ? 288 : 360)));
}
template <int PREC, int KS, int STRIDE, int PITCH, int CFG> struct StageCfg {
    static constexpr int NCH = Elem<PREC>::PIXB / 16;
    static constexpr int RAW = (pn_stage_maxpx_c(KS, STRIDE, PITCH) * NCH + 255) / 256;
    static constexpr int MAXST = (RAW <= 12 && CFG != PN_CFG_C64W) ? RAW : 0;
};

// Weight fragments are addressed as (wave-uniform 64-bit base in SGPRs) + (32-bit lane offset): the
// compiler then emits the saddr form of global_load and bumps the base with scalar adds -- no vector
// ALU work per k-step.
// acc += t as four v_add_f32 the compiler may not move: written as plain C++ the 252 block additions of a chunk were all sunk behind its last MFMA,
// every block sum parked in scratch until then and the MFMA pipeline drained at every item to store it.  t was produced one item (16 MFMAs) earlier.
// `after` is a register the CURRENT item's last MFMA writes: named as an operand and not read, it keeps the additions behind that item's MFMAs, so
// what they do read is at least 16 MFMAs old whatever the hazard recogniser knows about inline assembly.
__device__ __forceinline__ void pn_block_add(f32x4 &a, const f32x4 &t, float after) {
    float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
    asm volatile("v_add_f32 %0, %0, %4\n\tv_add_f32 %1, %1, %5\n\tv_add_f32 %2, %2, %6\n\tv_add_f32 %3, %3, %7"
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(t[0]), "v"(t[1]), "v"(t[2]), "v"(t[3]), "v"(after));
    a = f32x4{a0, a1, a2, a3};
}

template <int PREC> __device__ __forceinline__ typename Elem<PREC>::Frag load_a_frag2(gcptr base, unsigned voff) {
    return load_a_frag<PREC>(base + voff);
}
// Same stream through a buffer resource: fragment offset in an SGPR, 32-bit lane offset -- hipcc otherwise widens
// the lane offset to 64 bits and rebuilds a VGPR address pair per load (2 VALU + 6 VGPRs per k-step, measured:
// profiles/README.md v23).
template <int PREC> __device__ __forceinline__ typename Elem<PREC>::Frag load_a_frag_buf(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff);
template <> __device__ __forceinline__ Elem<PN_PREC_BF16>::Frag load_a_frag_buf<PN_PREC_BF16>(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(Elem<PN_PREC_BF16>::Frag, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0));
}
template <> __device__ __forceinline__ Elem<PN_PREC_F32>::Frag load_a_frag_buf<PN_PREC_F32>(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    Elem<PN_PREC_F32>::Frag f;
    f.lo = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0));
    f.hi = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff + 1024u, 0));
    return f;
}

// DIL: distance of the taps in input pixels (A2J's ResNet-50 layer4 blocks 1 and 2: 3x3, dilation 2, padding 2 -- taps at 0, +-2, a halo of 5 rows
// and columns; third_party_methods/A2J_experiments/resnet.py:112,145).  DIL = 1 is every other convolution: each expression below reduces to what it was.
// ACC (fp32 only): 1 = blocked accumulation.  The default fp32 path adds every 4-product MFMA onto ONE running sum, a serial chain of K / 4 roundings whose
// error grows like K; with ACC = 1 the eight MFMAs of a k-step (32 products) start from zero and their sum is added to the running sum once, so the long
// chain has K / 32 links -- about a third of the rounding error on the K = 4608 .. 18432 convolutions of the A2J net, which is what puts its fp32 heads
// within the reference's own fp32 error of the fp64 run.  ACC = 0 is every other fp32 net: the bit-exact FMA chain they are tested for.
template <int PREC, int KS, int STRIDE, int PITCH, int CFG, int DIL = 1, int ACC = 0>
__global__ __launch_bounds__(256, 2) void conv_mfma_kernel(const ConvProblem *__restrict__ probs) {
    typedef Elem<PREC> E;
    typedef typename E::T T;
    typedef typename E::Frag Frag;
    constexpr int PIXB = E::PIXB, FRAGB = E::FRAGB, SUBX = E::SUBX;
    constexpr int WC = TileCfg<CFG>::WC, WP = TileCfg<CFG>::WP, CT = TileCfg<CFG>::CT, PT = TileCfg<CFG>::PT;
    constexpr int KK = KS * KS, PAD = DIL * (KS / 2), KSD = (KS - 1) * DIL + 1;      // KSD: rows / columns the taps span
    constexpr int NCH = PIXB / 16;      // 16-B pieces per halo pixel
    constexpr int PPI = 256 / NCH;      // halo pixels staged per block pass
    constexpr int ES = (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const ConvProblem &P = probs[blockIdx.y];
    if ((int)blockIdx.x >= P.nblocks) return;
    const int bx = pn_xcd_block(blockIdx.x, P.nblocks);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wc = wave / WP, wp = wave % WP;
    const int c = lane & 15, q = lane >> 4;

    const int cb = bx % P.cout_blocks;
    const int Wo = P.Wo;
    const PnTile tl = pn_tile_decode(bx / P.cout_blocks, P.tiles_per_img, P.tiles_x, P.R, P.Wt, P.Ho, Wo);
    const int b = tl.b, oy0 = tl.oy0, ox0 = tl.ox0, R = tl.R, Wc = tl.Wc, npix = tl.npix;
    const int HRa = (R - 1) * STRIDE + KSD;      // halo rows actually needed
    const int HC = (Wc - 1) * STRIDE + KSD;      // halo columns
    const int iy0 = oy0 * STRIDE - PAD, ix0 = ox0 * STRIDE - PAD;
    const float inv_wc = tl.inv_wc;

    // ---- per-lane LDS addresses of tap (ky=0,kx) for each pixel tile, current 32-channel half ----
    int baddr[PT][KS];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
        int slot = (wp * PT + pt) * 16 + c;
        int s = slot < npix ? slot : 0;
        int ry, rx;
        pn_slot_pixel(s, inv_wc, Wc, ry, rx);
        int hp0 = ry * STRIDE * PITCH + rx * STRIDE;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            int hp = hp0 + kx * DIL;
            baddr[pt][kx] = hp * PIXB + ((q ^ (hp & 7)) << (PREC == PN_PREC_BF16 ? 4 : 5));
        }
    }

    f32x4 acc[CT][PT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- software pipeline -------------------------------------------------------------------
    //  * k order inside a 64-channel chunk: (32-channel half, tap): the swizzled LDS address of the
    //    second half is the first half's XOR SUBX, so the XOR is applied once per half (not per read);
    //  * weights (A): NA-slot register queue, loads run NA-1 k-steps ahead of their MFMAs;
    //  * activations (B): DB fragments in flight, read between the MFMAs of earlier pixel tiles;
    //  * halo staging: the NEXT chunk is fetched global -> registers before this chunk's MFMAs and
    //    written to the other LDS image after them (one barrier per chunk).
    // No branch inside the K loop: pixel tiles beyond the tile's valid pixels compute on clamped
    // addresses and are masked in the epilogue only.
    constexpr int NSTEP = KK * 2;                       // k32 steps per 64-channel chunk
    constexpr int NA = (PREC == PN_PREC_BF16) ? ((NSTEP % 6 == 0) ? 6 : 2) : ((NSTEP % 3 == 0) ? 3 : 2);
    constexpr int NITEM = NSTEP * PT;                   // (k-step, pixel tile) items per chunk
    constexpr int DB = (PREC == PN_PREC_BF16) ? ((NITEM % 3 == 0) ? 3 : 2) : 1;   // B fragments in flight
    // 0: stage without register prefetch (ACC = 1 always: the 48 prefetch registers are what the block sums need -- with them the 128-cout instances,
    // already at 256 VGPRs, kept the accumulators in scratch and drained the MFMA pipeline at every item)
    constexpr int MAXST = (ACC == 1) ? 0 : StageCfg<PREC, KS, STRIDE, PITCH, CFG>::MAXST;
    const int nchunks = P.cin_chunks;
    const int in_wrap = P.in_wrap;

    // weight stream: scalar base per cout tile + lane offset
    const int ctile0 = (cb * WC + wc) * CT;
    const __amdgpu_buffer_rsrc_t wrsrc = pn_weight_rsrc(P.wpack);
    unsigned wbase[CT];
    pn_weight_bases<CT>(ctile0, P.ksteps, FRAGB, wbase);
    const unsigned wlane = (unsigned)lane * 16u;
    // bf16: buffer loads (fewer VGPRs); fp32 parity mode: the flat form measured 2 % faster (two loads per fragment)
    auto load_w = [&](unsigned off) {
        if constexpr (PREC == PN_PREC_F32) return load_a_frag2<PREC>((gcptr)P.wpack + off, wlane);
        else return load_a_frag_buf<PREC>(wrsrc, wlane, off);
    };

    // halo staging: thread -> 16-B piece `ch` of halo pixels p0, p0+PPI, ...; coordinates advance
    // incrementally (no division per piece), global offsets are 32-bit from a scalar image base.
    const int ch = tid % NCH;
    const int p0 = tid / NCH;
    const int npx = HRa * HC;
    const int hy_first = (int)(((float)p0 + 0.5f) / (float)HC);
    const int hx_first = p0 - hy_first * HC;
    const int wrap1 = PPI / HC, wrap_rem = PPI - wrap1 * HC;         // one staging step = wrap1 rows + wrap_rem columns
    gcptr img = (gcptr)P.in + ((size_t)b * P.H * P.W * P.in_cs + P.in_coff) * ES + ch * 16;
    const int row_b = P.W * P.in_cs * ES, col_b = P.in_cs * ES;
    auto piece = [&](int hy, int hx, int &soff, int &dst, bool &inb) {
        const int iy = iy0 + hy, ix = ix0 + hx;
        inb = (unsigned)iy < (unsigned)P.H && (unsigned)ix < (unsigned)P.W;
        const int iyc = min(max(iy, 0), P.H - 1), ixc = min(max(ix, 0), P.W - 1);   // always a valid address
        soff = iyc * row_b + ixc * col_b;
        const int hp = hy * PITCH + hx;
        dst = hp * PIXB + (PREC == PN_PREC_BF16 ? ((ch ^ (hp & 7)) << 4) : ((((ch >> 1) ^ (hp & 7)) << 5) | ((ch & 1) << 4)));
    };
    auto advance = [&](int &hy, int &hx) {
        hx += wrap_rem;
        hy += wrap1;
        if (hx >= HC) { hx -= HC; ++hy; }
    };
    u32x4 st[MAXST > 0 ? MAXST : 1];
    auto stage_load = [&](int chunk) {                   // all loads issued back to back, no waits
        int hy = hy_first, hx = hx_first;
        gcptr src = img + (size_t)(chunk >= in_wrap ? chunk - in_wrap : chunk) * 64 * ES;      // bf16x3: the third plane pair reads the hi plane again
#pragma unroll
        for (int it = 0; it < MAXST; ++it) {
            int soff, dst; bool inb;
            piece(hy, hx, soff, dst, inb);
            st[it] = *reinterpret_cast<const PN_GLOBAL u32x4 *>(src + (unsigned)soff);
            advance(hy, hx);
        }
    };
    auto stage_store = [&](char *buf) {                  // zero padding is applied here, not at load time
        int hy = hy_first, hx = hx_first;
#pragma unroll
        for (int it = 0; it < MAXST; ++it) {
            int soff, dst; bool inb;
            piece(hy, hx, soff, dst, inb);
            if (p0 + it * PPI < npx) *reinterpret_cast<u32x4 *>(buf + dst) = inb ? st[it] : u32x4{0u, 0u, 0u, 0u};
            advance(hy, hx);
        }
    };
    auto stage_direct = [&](int chunk, char *buf) {      // large halos: batches of 4 loads, then 4 stores
        int hy = hy_first, hx = hx_first;
        gcptr src = img + (size_t)(chunk >= in_wrap ? chunk - in_wrap : chunk) * 64 * ES;      // bf16x3: the third plane pair reads the hi plane again
        for (int pb = p0; pb < npx; pb += 4 * PPI) {
            u32x4 v[4];
            int dst[4]; bool inb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int soff;
                piece(hy, hx, soff, dst[k], inb[k]);
                v[k] = *reinterpret_cast<const PN_GLOBAL u32x4 *>(src + (unsigned)soff);
                advance(hy, hx);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (pb + k * PPI < npx) *reinterpret_cast<u32x4 *>(buf + dst[k]) = inb[k] ? v[k] : u32x4{0u, 0u, 0u, 0u};
        }
    };

    char *buf0 = smem, *buf1 = P.lds_two ? smem + P.lds_buf_bytes : smem;
    Frag aq[NA][CT];
    pn_weight_prime<CT, NA>(FRAGB, wbase, aq, load_w);
    if (MAXST > 0) { stage_load(0); stage_store(buf0); }
    else stage_direct(0, buf0);
    __syncthreads();

    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const char *sm = (chunk & 1) ? buf1 : buf0;
        char *nbuf = (chunk & 1) ? buf0 : buf1;
        const bool more = chunk + 1 < nchunks;
        if (MAXST > 0 && more) stage_load(chunk + 1);

        // item j = (k-step s = half * KK + tap, pixel tile pt); the half is selected by the XOR state of baddr
#define PN_BADDR(j) (baddr[(j) % PT][(((j) / PT) % KK) % KS] + ((((j) / PT) % KK) / KS) * DIL * PITCH * PIXB)
        Frag bq[DB];
        f32x4 tq[2][CT];                                 // ACC = 1: the blocks of the current and the previous item
        (void)tq;
        if (DB > 1) {
#pragma unroll
            for (int j = 0; j < DB - 1; ++j) bq[j] = read_b_frag<PREC>(sm, PN_BADDR(j));
            __builtin_amdgcn_sched_barrier(0);          // keep the primed reads out of the pinned sequence below
        }
#define PN_BADDRX(j) ((baddr[(j) % PT][(((j) / PT) % KK) % KS] ^ SUBX) + ((((j) / PT) % KK) / KS) * DIL * PITCH * PIXB)
#pragma unroll
        for (int h = 0; h < 2; ++h) {                    // the two 32-channel halves of the chunk
#pragma unroll
            for (int i = 0; i < KK * PT; ++i) {
                const int j = h * KK * PT + i, s = j / PT, pt = j % PT;
                if (pt == 0) {
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {    // wpack ends with NA-1 spare fragments
                        aq[(s + NA - 1) % NA][ct] = load_w(wbase[ct]);
                        wbase[ct] += FRAGB;
                    }
                }
                const int jr = (DB > 1) ? j + DB - 1 : j;                // item whose B fragment is read now
                if (jr < NITEM) {
                    // the few prefetches that already belong to the other half take the XOR explicitly
                    if (jr / (KK * PT) != h) bq[jr % DB] = read_b_frag<PREC>(sm, PN_BADDRX(jr));
                    else bq[jr % DB] = read_b_frag<PREC>(sm, PN_BADDR(jr));
                }
                if constexpr (ACC == 1 && PREC == PN_PREC_F32) {
                    // blocked accumulation: this item's 32 products summed from zero; the PREVIOUS item's block, long finished, joins its running sum
                    // while these MFMAs run.  The fence keeps MFMAs and adds in item order (global loads may cross, LDS reads may not: hoisted, they are what fills the registers): without it the
                    // scheduler interleaves the blocks of many items and spills.
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) tq[j & 1][ct] = mma(aq[s % NA][ct], bq[j % DB], f32x4{0.f, 0.f, 0.f, 0.f});
                    if (j > 0) {
#pragma unroll
                        for (int ct = 0; ct < CT; ++ct) pn_block_add(acc[ct][(j - 1) % PT], tq[(j - 1) & 1][ct], tq[j & 1][CT - 1][3]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                } else {
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) acc[ct][pt] = mma(aq[s % NA][ct], bq[j % DB], acc[ct][pt]);
                }
                if (DB > 1) {
                    // pin the issue order (the scheduler otherwise sinks every prefetch down to its use)
                    if (pt == 0) __builtin_amdgcn_sched_group_barrier(0x020, CT, 0);             // weight loads
                    if (jr < NITEM) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);           // one LDS read
                    __builtin_amdgcn_sched_group_barrier(0x008, CT, 0);                          // CT MFMAs
                }
            }
#pragma unroll
            for (int p2 = 0; p2 < PT; ++p2)              // switch half (and back to the first one after the second)
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) baddr[p2][kx] ^= SUBX;
        }
#undef PN_BADDRX
#undef PN_BADDR
        if constexpr (ACC == 1 && PREC == PN_PREC_F32) {      // the chunk's last block
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) acc[ct][(NITEM - 1) % PT] = acc[ct][(NITEM - 1) % PT] + tq[(NITEM - 1) & 1][ct];
        }
        if (more) {
            if (!P.lds_two) __syncthreads();             // single LDS image: wait for every wave's reads
            if (MAXST > 0) stage_store(nbuf);
            else stage_direct(chunk + 1, nbuf);
            __syncthreads();
        }
    }

    // ---- epilogue (conv_common.h) ----------------------------------------------------------------
    constexpr int LC = CT * 4;
    const int cw = (cb * WC + wc) * (CT * 16) + LC * q;          // first output channel of this lane
    const int cout = P.cout, act = P.act;
    float bias[LC];
    pn_load_bias<LC>(P.bias, cw, bias);
    const PN_GLOBAL T *res_base = P.res ? (const PN_GLOBAL T *)P.res + P.res_coff + cw : nullptr;
    PN_GLOBAL T *out_base = P.out ? (PN_GLOBAL T *)P.out + P.out_coff + cw : nullptr;
    PN_GLOBAL float *nchw = (PN_GLOBAL float *)P.out_nchw;
    const int res_cs = P.res_cs, out_cs = P.out_cs, Ho = P.Ho, naf = P.yolo_naf;
    const int split = P.split, res_split = P.res_split;
    const int pix0 = (b * Ho + oy0) * Wo + ox0;
    pn_with_act<true>(act, [&](auto actc) {                   // -1: dispatch at run time (sigmoid casts: last layers only)
        pn_conv_epilogue<decltype(actc)::value, T, CT, PT>(acc, bias, wp * PT * 16 + c, npix, inv_wc, Wc, cw, cout, act, naf, res_base, res_cs, res_split,
                                                           out_base, out_cs, split, nchw, b, Ho, Wo, oy0, ox0, pix0);
    });
}


template <int PREC, int KS, int STRIDE, int PITCH, int CFG, int DIL = 1, int ACC = 0>
static int conv_launch_one(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream) {
    auto kern = conv_mfma_kernel<PREC, KS, STRIDE, PITCH, CFG, DIL, ACC>;
    if (L.lds_bytes > PN_CONV_LDS_MAX)
        return pn_set_error(ctx, PN_ERR_UNSUPPORTED, "conv halo tile needs %zu B of LDS", L.lds_bytes);
    if (L.lds_bytes > 48 * 1024) {
        static PnLdsAttr attr;          // per instantiation, per device
        if (int rc = pn_lds_attr(ctx, attr, reinterpret_cast<const void *>(kern), L.lds_bytes)) return rc;
    }
    dim3 grid(L.max_blocks, L.nprob), block(256);
    hipLaunchKernelGGL(kern, grid, block, L.lds_bytes, stream, L.probs_dev);
    PN_HIP_CHECK(ctx, hipGetLastError());
    return PN_OK;
}

#define PN_CASE(PREC, KS, ST, PITCH, CFG)                                                       \
    if (L.prec == PREC && L.ks == KS && L.stride == ST && L.pitch == PITCH && L.cfg == CFG)     \
        return conv_launch_one<PREC, KS, ST, PITCH, CFG>(ctx, L, stream);
// the dilation-2 rows (PN_CONV_INSTANCES_D2_*): pn_launch_conv sends a launch with L.dil == 2 to these shares only
#define PN_CASE_D2(PREC, KS, ST, PITCH, CFG)                                                    \
    if (L.prec == PREC && L.ks == KS && L.stride == ST && L.pitch == PITCH && L.cfg == CFG)     \
        return conv_launch_one<PREC, KS, ST, PITCH, CFG, 2>(ctx, L, stream);
// the fp32 blocked-accumulation instances (ConvLaunch::acc, conv_inst_acc_*.hip): every row of the table, dilation 1 and 2
#define PN_CASE_ACC(KS, ST, PITCH, CFG)                                                         \
    if (L.ks == KS && L.stride == ST && L.pitch == PITCH && L.cfg == CFG)                       \
        return conv_launch_one<PN_PREC_F32, KS, ST, PITCH, CFG, 1, 1>(ctx, L, stream);
#define PN_CASE_ACC_D2(KS, ST, PITCH, CFG)                                                      \
    if (L.ks == KS && L.stride == ST && L.pitch == PITCH && L.cfg == CFG)                       \
        return conv_launch_one<PN_PREC_F32, KS, ST, PITCH, CFG, 2, 1>(ctx, L, stream);
#define PN_CASES_PREC_D2(KS, ST, PITCH, CFG) \
    PN_CASE_D2(PN_PREC_BF16, KS, ST, PITCH, CFG) PN_CASE_D2(PN_PREC_F32, KS, ST, PITCH, CFG)
#define PN_CASES_PREC(KS, ST, PITCH, CFG) \
    PN_CASE(PN_PREC_BF16, KS, ST, PITCH, CFG) PN_CASE(PN_PREC_F32, KS, ST, PITCH, CFG)

// each conv_inst_*.hip implements one of these for its share of the instantiations -- PN_CONV_INSTANCES_<n>(PN_CASES_PREC), the rows of
// conv_inst_table.h and nothing else; returns 1 when the launch description is not one of its cases
int pn_launch_conv_part0(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_part1(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_part2(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_part3(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_d2_part0(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
int pn_launch_conv_d2_part1(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream);
