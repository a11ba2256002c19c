// What the fused BasicBlock(64) kernels share: bb64_kernel.h (tile tickets) and bb64s_kernel.h (column segments).  LDS layout and k-step order, the
// weight-loader stream, the image-piece DMA, the ticket sign-off, the fragment reads, the k-step-outer MFMA loop of both convolutions and the output
// epilogue.  bb64_kernel.h's header describes the design (roles, ring, barrier cadence); each shared mechanism is described here, at its code.
//
// The kernels reach this code through lambdas that capture their locals by reference, as the code did before it was shared, and everything here takes
// its arguments by value: the compiler folds a captured local later than a plain one, and the instruction streams of bb64_kernel<1> and
// bb64s_strip_kernel are pinned to what they were (profiles/bb64_shared_ab.txt).  The compute-wave prologue, the per-tile set-up, the intermediate
// epilogue and the pixel-tile-outer last phases are still written out in both kernels: every way of sharing them that was tried changed those streams.
#pragma once
#include "conv_common.h"


// LDS images are QUARTER-major: [4 quarters of 16 channels][row][32 px][32 B].  A lane's 16-B B fragment (8 channels) is
// half of a pixel's 32-B quarter entry, so the 16 lanes one ds_read_b128 phase serves (8 with an even, 8 with an odd lane
// quarter q) cover 8 consecutive pixels x 32 B = one whole 256-B bank row: conflict-free, where the half-major image of
// conv3 / conv4 ([row][px][64 B]) costs 2 LDS cycles per read -- this kernel's 4 compute waves would keep the LDS array
// ~100 % busy with it (20 MFMAs per 9 fragment reads).  One DMA instruction = one 32-pixel row of one quarter.
#define BB_INQ (12 * 32 * 32)
#define BB_IN (4 * BB_INQ)                    // 48 KB
#define BB_MIDQ (10 * 32 * 32)
#define BB_MID (4 * BB_MIDQ)                  // 40 KB
#define BB_ASLOT 4096
#define BB_OFF_MID (2 * BB_IN)
#define BB_OFF_A (BB_OFF_MID + BB_MID)
#define BB_NSLOT 6                              // weight ring: a phase = 2 k-steps; phase p + 2 lands in the slots of phase p - 1
#define BB_LDS (BB_OFF_A + BB_NSLOT * BB_ASLOT) // 163840 B = all of a CU's LDS
// The folded biases live in LDS, not in 32 VGPRs per compute wave: pixel columns 30, 31 of the intermediate image are never written (MC <= 30) nor
// read (x + kx <= 29), so rows 1 (b1) and 2 (b2) of quarter plane q hold that quarter's 16 floats there (64 B); the epilogues read them back.
#define BB_BIAS(cv, q) (BB_OFF_MID + (q) * BB_MIDQ + (((cv) + 1) * 32 + 30) * 32)
// Ticket slots: pixel column 31 of row 0 of the intermediate image's first quarter plane is never written (MC <= 30) nor read (x + kx <= 29) as pixels
#define BB_OFF_TICKET (BB_OFF_MID + 31 * 32)

// The (k-step, pixel tile) order of the 18 * PT MFMA groups ("items") of a convolution; the B-fragment queue runs BQ - 1 items ahead of the MFMAs.
// k-steps 0..15 go k-step outer.  With xch the last phase (k-steps 16, 17: both in the weight ring for the whole phase) goes pixel tile outer, so that
// a tile's accumulators are final while the tiles after it still have MFMAs to issue -- except that tiles 0 and 1 go (0, 16) (1, 16) (0, 17) (1, 17):
// k-step 17's weight fragments are read at the head of the phase and have not arrived for the second item.  Every accumulator keeps its k order.
__host__ __device__ constexpr int bb_item_ks(int n, int PT, bool xch) { return !xch || n < 16 * PT ? n / PT : n - 16 * PT < 4 ? 16 + ((n - 16 * PT) >> 1) : 16 + ((n - 16 * PT) & 1); }
__host__ __device__ constexpr int bb_item_pt(int n, int PT, bool xch) { return !xch || n < 16 * PT ? n % PT : n - 16 * PT < 4 ? (n - 16 * PT) & 1 : (n - 16 * PT) >> 1; }
constexpr int BB_BQ = 6;                        // depth of the B-fragment queue
// Epilogue instructions (VALU / SALU / LDS write or store) placed behind each MFMA of a last phase.  Chosen from the cross-compiled instruction
// stream, not tuned on a GPU: conv1 has 28 MFMAs after its first finished tile for four epilogues of about 45 instructions, conv2 16 for three of
// about 58; with a smaller number the compiler leaves the rest in one lump at the end of the phase.  An MFMA hides only two VALU, so these
// regions are VALU-bound either way.
constexpr int BB_FILL1 = 7, BB_FILL2 = 11;             // conv1, conv2

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) short i16x2;
// ReLU of two packed bf16: the sign bit of a bf16 is the sign bit of the int16 with the same bits
__device__ __forceinline__ unsigned bb_relu_pk(unsigned w) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(i16x2, w), i16x2{0, 0}));
}

// ================= loader waves: LDS-DMA only =================
// ---- weight loaders (lw = 0, 1): each fetches half (two 1 KB instructions) of both k-steps of a phase ----
// Ring of 6 slots, k-step k in slot k % 6; the compute waves read the fragments of k-step k during k - 1.  In phase q
// (k-steps 2q, 2q + 1) the loaders issue k-step 2q + 4 and then 2q + 5 into the slots phase q - 1 has just released;
// 2q + 4 is read in phase q + 1 and must have landed by the barrier that ends phase q (vmcnt leaves only the two
// newer instructions = 2q + 5 in flight), 2q + 5 is read in phase q + 2 and gets a phase of slack.
// this wave's half of a k-step of the periodic 36-step stream; wsrc = the weight pack + lw * 2048
__device__ __forceinline__ void bb_dma_a(const char *wsrc, unsigned lane16, int lw, int kstep) {
    pn_glds16_s<0>(wsrc + (size_t)kstep * BB_ASLOT, lane16, (unsigned)(BB_OFF_A + (kstep % BB_NSLOT) * BB_ASLOT) + (unsigned)__builtin_amdgcn_readfirstlane(lw * 2048));
    pn_glds16_s<0>(wsrc + (size_t)kstep * BB_ASLOT + 1024, lane16, (unsigned)(BB_OFF_A + (kstep % BB_NSLOT) * BB_ASLOT + 1024) + (unsigned)__builtin_amdgcn_readfirstlane(lw * 2048));
}
// the prologue (k-steps 0..3) and the pass over a tile; dma_a(kstep) = the kernel's bb_dma_a call
template <class DmaA>
__device__ __forceinline__ void bb_weights_prologue(DmaA dma_a) {
    dma_a(0); dma_a(1); dma_a(2); dma_a(3);             // phases 0 and 1
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    asm volatile("s_barrier" ::: "memory");              // (the compute waves have read k-step 0's fragments)
}
template <class DmaA>
__device__ __forceinline__ void bb_weights_tile(DmaA dma_a) {
#pragma clang loop unroll(full)
    for (int p = 0; p < 18; ++p) {                   // phase p = k-steps 2p, 2p + 1 of the tile's 36
        dma_a((2 * p + 4) % 36);
        dma_a((2 * p + 5) % 36);
        asm volatile("s_waitcnt vmcnt(2)\n\ts_barrier" ::: "memory");
        if (p == 8) asm volatile("s_barrier" ::: "memory");          // the compute waves publish the intermediate image
    }
    asm volatile("s_barrier" ::: "memory");                             // end of tile
}

// ---- image loaders (lw = 2, 3): pieces 0..23 / 24..47 of the NEXT tile's input image, two per phase ----
// piece n = (quarter n / 12, halo row n % 12) of the tile at (b, oy0, ox0), Wc columns wide, into image buffer buf: 32 pixels x 32 B.  Pixels outside
// the map come from the zero page.
__device__ __forceinline__ void bb_dma_in(const BBProblem &P, int H, int W, int lane, int b, int oy0, int ox0, int Wc, int buf, int n) {
    const int qu = n / 12, row = n % 12;
    const int px = lane >> 1;
    const int iy = oy0 - 2 + row, ix = ox0 - 2 + px;
    const size_t frame_b = ((size_t)b * H * W * P.in_cs + P.in_coff) * 2;
    const bool inb = px < Wc + 4 && (unsigned)ix < (unsigned)W && (unsigned)iy < (unsigned)H;
    const unsigned off = inb ? (unsigned)((iy * W + ix) * P.in_cs * 2 + qu * 32 + (lane & 1) * 16) : P.in_zero_off - (unsigned)frame_b;
    pn_glds16_s<0>((const char *)P.in + frame_b, off, (unsigned)__builtin_amdgcn_readfirstlane(buf * BB_IN + qu * BB_INQ + row * 1024));
}
// Ticket sign-off: a workgroup that will make no further claim has added one to tickets[1] (signed_off = the count before it).  The workgroup that signs
// off last knows every claim has been made and leaves both counters at zero for the next launch (graph replay).
__device__ __forceinline__ void bb_sign_off(int *tickets, int signed_off, int grid) {
    if (signed_off == grid - 1) {
        __hip_atomic_store(tickets, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(tickets + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ================= compute waves =================
// Fragment reads, in terms of the kernels' locals (smem; aaddr0, aaddr1; ba1[], ba2[]; PT1, PT2, XCH).
#define BB_TAPOFF(tap) ((((tap) / 3) * 32 + ((tap) % 3)) * 32)
#define BB_A(k, ct) (*reinterpret_cast<const bf16x8 *>(smem + ((ct) < 2 ? aaddr0 : aaddr1) + ((k) % BB_NSLOT) * BB_ASLOT + ((ct) & 1) * 1024))                    /* weight fragment of k-step k of the tile's 36 */
#define BB_KOFF1(ks) (((ks) / 9) * 2 * BB_INQ + BB_TAPOFF((ks) % 9))
#define BB_B1(n) (*reinterpret_cast<const bf16x8 *>(smem + ba1[bb_item_pt(n, PT1, XCH)] + BB_KOFF1(bb_item_ks(n, PT1, XCH))))         /* B fragment of item n of conv1 */
#define BB_KOFF2(ks) (((ks) / 9) * 2 * BB_MIDQ + BB_TAPOFF((ks) % 9))
#define BB_B2(n) (*reinterpret_cast<const bf16x8 *>(smem + ba2[bb_item_pt(n, PT2, XCH)] + BB_KOFF2(bb_item_ks(n, PT2, XCH))))         /* B fragment of item n of conv2 */

// output: bias + residual (centre of the input image, resw = its pixel (0, 0)) + ReLU, 16-B stores (two per pixel; one for the half tile = slot 3 with
// SPLIT); valid = the slot is an output pixel; pc(k) = the 16-byte piece of slot pair k
template <int CT, bool SPLIT, class Pc>
__device__ __forceinline__ void bb_epi2(char *smem, const f32x4 (&acc)[CT][5], const float (&b2)[4 * CT], int pt, int pix, bool valid, int resw, __amdgpu_buffer_rsrc_t orsrc,
                                        int oy0, int ox0, int W, int out_cs, int q, Pc pc) {
    constexpr int NP = CT / 2;
    const int nct = SPLIT && pt == 3 ? 2 : CT, np = nct / 2;
    const int r = pix >> 10, x = (pix >> 5) & 31;
    u32x4 rr[NP], o[NP];
    rr[0] = *reinterpret_cast<const u32x4 *>(smem + resw + pix);
    if (np == 2) rr[NP - 1] = *reinterpret_cast<const u32x4 *>(smem + ((resw + pix) ^ 16));
#pragma unroll
    for (int ct = 0; ct < nct; ++ct) {
        const unsigned ra = rr[ct >> 1][2 * (ct & 1)], rb = rr[ct >> 1][2 * (ct & 1) + 1];
        // a bf16 is the upper half of its float: residual channels by shift / mask, no conversion instruction
        f32x2 lo = {acc[ct][pt][0] + b2[4 * ct + 0] + __builtin_bit_cast(float, ra << 16),
                    acc[ct][pt][1] + b2[4 * ct + 1] + __builtin_bit_cast(float, ra & 0xffff0000u)};
        f32x2 hi = {acc[ct][pt][2] + b2[4 * ct + 2] + __builtin_bit_cast(float, rb << 16),
                    acc[ct][pt][3] + b2[4 * ct + 3] + __builtin_bit_cast(float, rb & 0xffff0000u)};
        o[ct >> 1][2 * (ct & 1)] = bb_relu_pk(__builtin_bit_cast(unsigned, __builtin_convertvector(lo, bf16x2)));
        o[ct >> 1][2 * (ct & 1) + 1] = bb_relu_pk(__builtin_bit_cast(unsigned, __builtin_convertvector(hi, bf16x2)));
    }
    // out-of-range offset for the unused slots: the store is issued unconditionally and dropped by the hardware
    unsigned vin = (unsigned)(((oy0 + r) * W + ox0 + x) * out_cs * 2 + 32 * q);
    asm volatile("" : "+v"(vin));                  // computed for every slot: the compiler otherwise branches round the multiply
    const unsigned voff = valid ? vin : 0x80000000u;
#pragma unroll
    for (int k = 0; k < np; ++k) __builtin_amdgcn_raw_buffer_store_b128(o[k], orsrc, voff + 16u * (unsigned)pc(k), 0, 0);
}

// ---------------- the k-step-outer MFMA loop of a convolution: PT pixel tiles per wave, B fragments at ba[] in an image of PLANE bytes per quarter.
// HALF (conv2 with SPLIT): pixel tile 3 is the half tile, slots 0 and 1 only ----------------
// Zeroes the accumulators, then k-steps PH0 .. PH0 + NKO - 1 of the tile's 36 (NKO = 16: the last phase follows pixel tile outer, bb_item_*).
// aq[PH0 & 1] holds k-step PH0's weight fragments: read in the prologue / prefetched by the phase before
template <int PT, int NKO, int PH0, int PLANE, bool HALF, int CT>
__device__ __forceinline__ void bb_kouter(char *smem, int aaddr0, int aaddr1, const int (&ba)[PT], f32x4 (&acc)[CT][5], bf16x8 (&aq)[2][CT], bf16x8 (&bq)[BB_BQ]) {
    constexpr int BQ = BB_BQ;
    constexpr bool XCH = NKO == 16;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
#define BB_B(n) (*reinterpret_cast<const bf16x8 *>(smem + ba[bb_item_pt(n, PT, XCH)] + ((bb_item_ks(n, PT, XCH) / 9) * 2 * PLANE + BB_TAPOFF(bb_item_ks(n, PT, XCH) % 9))))
#pragma unroll
    for (int j = 0; j < BQ - 1; ++j) bq[j] = BB_B(j);
#pragma clang loop unroll(full)
    for (int p = 0; p < NKO; ++p) {
        const int ph = PH0 + p;
        __builtin_amdgcn_sched_barrier(0);
#pragma clang loop unroll(full)
        for (int pt = 0; pt < PT; ++pt) {
            const int j = p * PT + pt, jr = j + BQ - 1;
            if (pt < CT) aq[(ph + 1) & 1][pt] = BB_A(ph + 1, pt);
            if (jr < 18 * PT) bq[jr % BQ] = BB_B(jr);
            const int nct = HALF && pt == 3 ? 2 : CT;           // the half tile: slots 0, 1
#pragma unroll
            for (int ct = 0; ct < nct; ++ct)
                acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq[ph & 1][ct], bq[j % BQ], acc[ct][pt], 0, 0, 0);
            if (pt < CT && jr < 18 * PT) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            else if (pt < CT || jr < 18 * PT) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            if (HALF && pt == 3) __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            else __builtin_amdgcn_sched_group_barrier(0x008, CT, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        // one barrier per two k-steps (no lgkmcnt wait: the ring slots refilled after it were last read a phase ago, the
        // images are stable)
        if (ph & 1) asm volatile("s_barrier" ::: "memory");
    }
#undef BB_B
}
