// What the inference convolution kernels share: conv_mfma_kernel.h (the generic kernel), conv3_kernel.h, conv4_kernel.h, and the helpers the fused
// BasicBlock kernels (bb64_common.h, bb64x3_kernel.h) take from them.  No kernel lives here: vector types and the address-space macro, the MFMA
// operand types, the LDS-DMA instruction, and ONE copy of everything the kernels' "same contract" consists of -- block order, tile decode, the
// slot -> pixel rule, the folded-bias load, the activation dispatch, the two output epilogues and the LDS parking step of the fused tails.
// Each kernel header keeps its own K loop, staging, LDS layout and launch.
//
// Everything here is __device__ __forceinline__, takes scalars by value (arrays of registers by reference: they cannot be passed otherwise) and is
// called from lambdas that capture the kernel's locals by reference -- the form that left scheduling and register use alone when the bb64 kernels
// were folded (profiles/bb64_shared_ab.txt, section 2; this fold: profiles/conv_common_ab.txt).
#pragma once
#include <type_traits>
#include "pn_internal.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
// Pointers read out of the ConvProblem record are "generic" to the compiler, which then emits flat_*
// memory ops (they tick vmcnt AND lgkmcnt and can only be waited for with 0/0, serialising against
// the LDS pipeline).  Everything that touches HBM goes through explicit global-address-space pointers.
#define PN_GLOBAL __attribute__((address_space(1)))
typedef const PN_GLOBAL char *gcptr;
typedef PN_GLOBAL char *gptr;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;   // native vector: loadable through address-space pointers
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;   // native vector: storable through address-space pointers

template <int PREC> struct Elem;
template <> struct Elem<PN_PREC_BF16> {
    typedef __bf16 T;
    static constexpr int PIXB = 128;   // LDS bytes per halo pixel (64 channels)
    static constexpr int FRAGB = 1024; // bytes of one packed A fragment (16 couts x 32 k)
    static constexpr int SUBX = 64;    // address XOR selecting the second 32-channel half
    struct Frag { bf16x8 v; };
};
template <> struct Elem<PN_PREC_F32> {
    typedef float T;
    static constexpr int PIXB = 256;
    static constexpr int FRAGB = 2048;
    static constexpr int SUBX = 128;
    struct Frag { f32x4 lo, hi; };
};

__device__ __forceinline__ float pn_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float pn_activate(float v, int act, int co, int naf) {
    switch (act) {
        case PN_ACT_RELU: return v > 0.f ? v : 0.f;
        case PN_ACT_LEAKY: return v > 0.f ? v : v * 0.1f;
        case PN_ACT_SIG_PM2: return (pn_sigmoid(v) - 0.5f) * 4.f;
        case PN_ACT_SIG: return pn_sigmoid(v);
        case PN_ACT_YOLO: {
            int f = co % naf;
            float s = pn_sigmoid(v);
            if (f < 2) return (s - 0.5f) * 2.f;
            if (f < 4) return s * 2.f;
            if (f == 4) return s;
            return (s - 0.5f) * 4.f;
        }
        default: return v;
    }
}

template <int PREC> __device__ __forceinline__ typename Elem<PREC>::Frag read_b_frag(const char *smem, int addr);
template <> __device__ __forceinline__ Elem<PN_PREC_BF16>::Frag read_b_frag<PN_PREC_BF16>(const char *smem, int addr) {
    Elem<PN_PREC_BF16>::Frag f;
    f.v = *reinterpret_cast<const bf16x8 *>(smem + addr);
    return f;
}
template <> __device__ __forceinline__ Elem<PN_PREC_F32>::Frag read_b_frag<PN_PREC_F32>(const char *smem, int addr) {
    Elem<PN_PREC_F32>::Frag f;
    f.lo = *reinterpret_cast<const f32x4 *>(smem + addr);
    f.hi = *reinterpret_cast<const f32x4 *>(smem + addr + 16);
    return f;
}

__device__ __forceinline__ f32x4 mma(const Elem<PN_PREC_BF16>::Frag &a, const Elem<PN_PREC_BF16>::Frag &b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma(const Elem<PN_PREC_F32>::Frag &a, const Elem<PN_PREC_F32>::Frag &b, f32x4 c) {
    // k-slot s of lane-quarter q is channel 8q+s for BOTH operands (any consistent k order is valid)
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo[0], b.lo[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo[1], b.lo[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo[2], b.lo[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo[3], b.lo[3], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi[0], b.hi[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi[1], b.hi[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi[2], b.hi[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi[3], b.hi[3], c, 0, 0, 0);
    return c;
}

// LDS-DMA: 64 lanes x 16 B from per-lane global addresses to LDS [lds_dst, lds_dst + 1024).
// M0 is written in the same statement that uses it (the compiler does not preserve it around asm).
__device__ __forceinline__ void pn_glds16(gcptr src, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
}

// LDS-DMA, scalar base + 32-bit lane offset: no 64-bit address registers, the per-step pointer bump is scalar.
template <int IMM>
__device__ __forceinline__ void pn_glds16_s(const void *sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 offset:%4\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst), "n"(IMM) : "memory");
}

// ---- block set-up ---------------------------------------------------------------------------------------------------------------------

// XCD-aware remap (speed only): hardware deals consecutive block ids round-robin over the 8
// XCDs; give each XCD a contiguous range of logical blocks so that blocks sharing an input
// halo / a weight slice hit the same L2.  Bijective for any nblocks.
template <class I>      // the caller's own index type (blockIdx.x is unsigned, a flattened grid index an int): no conversion, the same instructions as written in place
__device__ __forceinline__ int pn_xcd_block(I block_x, int nblocks) {
    const int xcd = block_x & 7, idx = block_x >> 3;
    const int qq = nblocks >> 3, rr = nblocks & 7;
    return (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + idx;
}

// The output tile of a block: tt = (image, tile) index, i.e. the logical block id without its cout block (conv4 pairs two of them per block and
// passes each strip's own).  A block owns R (<= rows_per_block) full-width rows x Wc (<= Wt) columns of image b, origin (oy0, ox0); a pixel
// "slot" is its row-major index within those R x Wc pixels.
struct PnTile {
    int b, ty, tx, oy0, ox0, R, Wc, npix;
    float inv_wc;
};
__device__ __forceinline__ PnTile pn_tile_decode(int tt, int tiles_per_img, int tiles_x, int rows_per_block, int Wt, int Ho, int Wo) {
    PnTile t;
    const int tile = tt % tiles_per_img;
    t.b = tt / tiles_per_img;
    t.ty = tile / tiles_x, t.tx = tile - t.ty * tiles_x;
    t.oy0 = t.ty * rows_per_block, t.ox0 = t.tx * Wt;
    t.R = min(rows_per_block, Ho - t.oy0);
    t.Wc = min(Wt, Wo - t.ox0);          // output columns of this tile
    t.npix = t.R * t.Wc;
    t.inv_wc = 1.0f / (float)t.Wc;
    return t;
}

// slot -> (row, column) of the tile without an integer division: exact for every slot < 2^22 / Wc (tiles hold <= 512 pixels)
__device__ __forceinline__ void pn_slot_pixel(int slot, float inv_wc, int Wc, int &ry, int &rx) {
    ry = (int)(((float)slot + 0.5f) * inv_wc);
    rx = slot - ry * Wc;
}

// the LC consecutive folded biases of a lane, first channel cw (a multiple of 4; the bias vector is padded to whole cout tiles)
template <int LC>
__device__ __forceinline__ void pn_load_bias(const float *bias_vec, int cw, float (&bias)[LC]) {
#pragma unroll
    for (int ct = 0; ct < LC / 4; ++ct) {
        const f32x4 b4 = *reinterpret_cast<const PN_GLOBAL f32x4 *>((const PN_GLOBAL float *)bias_vec + cw + 4 * ct);
        bias[4 * ct + 0] = b4[0]; bias[4 * ct + 1] = b4[1]; bias[4 * ct + 2] = b4[2]; bias[4 * ct + 3] = b4[3];
    }
}

// ---- activation: run time -> compile time ---------------------------------------------------------------------------------------------
// f(std::integral_constant<int, ACT>) with the common activations as compile-time constants.  RUNTIME: a fourth case, ACT = -1 = dispatch per value
// with pn_activate (the sigmoid casts: last layers only).  Without it every other code runs as PN_ACT_NONE: for callers whose problems hold
// RELU / LEAKY / NONE only (the fused tails, net.hip::fuse_1x1_tails; conv3's fast epilogue) -- their bodies must not contain the run-time switch.
template <bool RUNTIME, class F>
__device__ __forceinline__ void pn_with_act(int act, F f) {
    if (act == PN_ACT_RELU) f(std::integral_constant<int, PN_ACT_RELU>{});
    else if (act == PN_ACT_LEAKY) f(std::integral_constant<int, PN_ACT_LEAKY>{});
    else if constexpr (!RUNTIME) f(std::integral_constant<int, PN_ACT_NONE>{});
    else {
        if (act == PN_ACT_NONE) f(std::integral_constant<int, PN_ACT_NONE>{});
        else f(std::integral_constant<int, -1>{});
    }
}
// f(activation constant, std::bool_constant<has_res>)
template <bool RUNTIME, class F>
__device__ __forceinline__ void pn_with_act(int act, bool has_res, F f) {
    if (has_res) pn_with_act<RUNTIME>(act, [&](auto actc) { f(actc, std::true_type{}); });
    else pn_with_act<RUNTIME>(act, [&](auto actc) { f(actc, std::false_type{}); });
}
template <int ACT>
__device__ __forceinline__ float pn_act_ct(float v, int act, int co, int naf) {
    if constexpr (ACT == PN_ACT_NONE) return v;
    else if constexpr (ACT == PN_ACT_RELU) return v > 0.f ? v : 0.f;
    else if constexpr (ACT == PN_ACT_LEAKY) return v > 0.f ? v : v * 0.1f;
    else return pn_activate(v, act, co, naf);
}

// ---- epilogues ------------------------------------------------------------------------------------------------------------------------
// The MFMA C layout gives a lane 4 consecutive rows (couts) of one pixel per accumulator.  The
// packed weight rows are permuted on the host (net.hip::prepare_conv, pn_conv_row_channel) so
// that the CT accumulators of a lane together are LC = 4*CT CONSECUTIVE output channels: each
// lane adds the folded bias, the residual, applies the activation and writes LC values per pixel
// tile straight from registers as 16-B pieces (bf16 CT = 2: one, bf16 CT = 4 / fp32 CT = 2: two)
// -- no LDS transpose, no barrier; the four lane quarters of a wave cover one contiguous run of a pixel's line.
// The arithmetic on a value, the same in every kernel and both epilogues: acc + bias, + residual hi, + residual lo (bf16x3), activation,
// then hi = (T)v and, for a split (bf16x3) output, lo = (T)(v - (float)hi) in a second plane `split` channels behind the first.

// LC contiguous values <-> memory as 16-B pieces (LC * sizeof(T) = 16 or 32), else element by element
template <class T, int LC>
__device__ __forceinline__ void pn_load_line(const PN_GLOBAL T *p, T (&rv)[LC]) {
    if constexpr ((LC * sizeof(T)) % 16 == 0) {
#pragma unroll
        for (int i = 0; i < (int)(LC * sizeof(T)) / 16; ++i) reinterpret_cast<u32x4 *>(rv)[i] = reinterpret_cast<const PN_GLOBAL u32x4 *>(p)[i];
    } else {
#pragma unroll
        for (int k = 0; k < LC; ++k) rv[k] = p[k];
    }
}
template <class T, int LC>
__device__ __forceinline__ void pn_store_line(PN_GLOBAL T *p, T (&ov)[LC]) {
    if constexpr ((LC * sizeof(T)) % 16 == 0) {
#pragma unroll
        for (int i = 0; i < (int)(LC * sizeof(T)) / 16; ++i) reinterpret_cast<PN_GLOBAL u32x4 *>(p)[i] = reinterpret_cast<u32x4 *>(ov)[i];
    } else {
#pragma unroll
        for (int k = 0; k < LC; ++k) p[k] = ov[k];
    }
}
// plane pl of the output values: 0 = hi (the whole value of a plain tensor), 1 = lo
template <class T, int LC>
__device__ __forceinline__ void pn_plane(const float (&v)[LC], int pl, T (&ov)[LC]) {
#pragma unroll
    for (int k = 0; k < LC; ++k) {
        const T hi = (T)v[k];
        ov[k] = pl == 1 ? (T)(v[k] - (float)hi) : hi;
    }
}

// General epilogue, any problem: ragged cout (element stores for the lane that straddles cout), residual hi (+ lo), split output planes, NCHW f32
// export, run-time activation (ACT = -1).  slot0 = the lane's pixel slot in pixel tile 0; cw = the lane's first output channel;
// res_base / out_base include cw (nullptr = none); pix0 = pixel index of the tile origin in the NHWC output.
template <int ACT, class T, int CT, int PT>
__device__ __forceinline__ void pn_conv_epilogue(const f32x4 (&acc)[CT][PT], const float (&bias)[4 * CT], int slot0, int npix, float inv_wc, int Wc,
                                                 int cw, int cout, int act, int naf, const PN_GLOBAL T *res_base, int res_cs, int res_split,
                                                 PN_GLOBAL T *out_base, int out_cs, int split, PN_GLOBAL float *nchw, int b, int Ho, int Wo,
                                                 int oy0, int ox0, int pix0) {
    constexpr int LC = CT * 4;
    const bool full = cw + LC <= cout;
#pragma clang loop unroll(full)                          // a rolled loop would index acc[] dynamically = scratch memory
    for (int pt = 0; pt < PT; ++pt) {
        const int slot = slot0 + pt * 16;
        if (slot >= npix || cw >= cout) continue;
        int ry, rx;
        pn_slot_pixel(slot, inv_wc, Wc, ry, rx);
        const int opix = pix0 + ry * Wo + rx;
        float v[LC];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int i = 0; i < 4; ++i) v[4 * ct + i] = acc[ct][pt][i] + bias[4 * ct + i];
        for (int pl = 0; pl < (res_base ? (res_split ? 2 : 1) : 0); ++pl) {      // bf16x3: residual = hi plane + lo plane
            const PN_GLOBAL T *rp = res_base + (unsigned)(opix * res_cs + pl * res_split);
            if (full) {
                T rv[LC];
                pn_load_line<T, LC>(rp, rv);
#pragma unroll
                for (int k = 0; k < LC; ++k) v[k] += (float)rv[k];
            } else {
                for (int k = 0; k < LC; ++k)
                    if (cw + k < cout) v[k] += (float)rp[k];
            }
        }
#pragma unroll
        for (int k = 0; k < LC; ++k) v[k] = pn_act_ct<ACT>(v[k], act, cw + k, naf);
        if (out_base) {
            for (int pl = 0; pl < (split ? 2 : 1); ++pl) {
                PN_GLOBAL T *op = out_base + (unsigned)(opix * out_cs + pl * split);
                T ov[LC];
                pn_plane<T, LC>(v, pl, ov);
                if (full) {
                    pn_store_line<T, LC>(op, ov);
                } else {
                    for (int k = 0; k < LC; ++k)
                        if (cw + k < cout) op[k] = ov[k];
                }
            }
        }
        if (nchw) {                                       // API-boundary layout: 16 lanes = 16 consecutive pixels of a plane
            const size_t hw = (size_t)Ho * Wo;
            PN_GLOBAL float *np = nchw + ((size_t)b * cout + cw) * hw + (size_t)(oy0 + ry) * Wo + (ox0 + rx);
            for (int k = 0; k < LC; ++k)
                if (cw + k < cout) np[(size_t)k * hw] = v[k];
        }
    }
}

// Fast epilogue, chosen per WAVE (the caller's condition is wave-uniform, so no exec-mask branching): every cout of the wave exists and the output
// is NHWC only.  The pixel of a slot is recovered from its LDS read address instead of being divided out again: pixof(ba[pt]) = ry * 32 + rx for
// the 32-pixel LDS rows of conv3 / conv4.  Same arithmetic on the values as pn_conv_epilogue, so the results are bit-identical.
// ob / rb: the wave's first channel; lane_c = the lane's first channel within the wave.  A caller that excludes split planes passes the literals
// split = res_split = 0 and the plane loops fold away.  PREFETCH: every residual (hi plane) load is issued before the first value is finished.
template <int ACT, bool RES, bool PREFETCH, class T, int CT, int PT, class PixOf>
__device__ __forceinline__ void pn_conv_epilogue_fast(const f32x4 (&acc)[CT][PT], const float (&bias)[4 * CT], const int (&ba)[PT], PixOf pixof, int slot0,
                                                      int npix, unsigned pix0, unsigned Wo, PN_GLOBAL T *ob, const PN_GLOBAL T *rb, unsigned lane_c,
                                                      unsigned res_cs, int res_split, unsigned out_cs, int split, int act, int cw, int naf) {
    constexpr int LC = CT * 4;
    T rq[PREFETCH && RES ? PT : 1][LC];
    if constexpr (PREFETCH && RES) {
#pragma clang loop unroll(full)
        for (int pt = 0; pt < PT; ++pt) {
            const unsigned t = pixof(ba[pt]);
            const unsigned opix = pix0 + (t >> 5) * Wo + (t & 31u);
            pn_load_line<T, LC>(rb + (opix * res_cs + lane_c), rq[pt]);
        }
    }
#pragma clang loop unroll(full)
    for (int pt = 0; pt < PT; ++pt) {
        const int slot = slot0 + pt * 16;
        const unsigned t = pixof(ba[pt]);
        const unsigned opix = pix0 + (t >> 5) * Wo + (t & 31u);
        float v[LC];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int i = 0; i < 4; ++i) v[4 * ct + i] = acc[ct][pt][i] + bias[4 * ct + i];
        if constexpr (RES) {
            for (int pl = 0; pl < (res_split ? 2 : 1); ++pl) {       // bf16x3: residual = hi plane + lo plane
                T rv[LC];
                if (!PREFETCH || pl > 0) pn_load_line<T, LC>(rb + (opix * res_cs + lane_c + (unsigned)(pl * res_split)), rv);
#pragma unroll
                for (int k = 0; k < LC; ++k) v[k] += (float)(PREFETCH && pl == 0 ? rq[PREFETCH ? pt : 0][k] : rv[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < LC; ++k) v[k] = pn_act_ct<ACT>(v[k], act, cw + k, naf);
        for (int pl = 0; pl < (split ? 2 : 1); ++pl) {
            T ov[LC];
            pn_plane<T, LC>(v, pl, ov);
            if (slot < npix) pn_store_line<T, LC>(ob + (opix * out_cs + lane_c + (unsigned)(pl * split)), ov);
        }
    }
}

// Fused tails (conv3_kernel.h, TAIL = 1 / 2): a lane's finished values of every pixel tile (bias + activation + bf16: exactly what the epilogue would
// store) parked in LDS as the B fragments of a second convolution: fragment (wc, pt) at ((wc * PT + pt) * 64 + lane) * 16.  LO: with lo_off != 0
// (bf16x3) the lo plane bf16(v - hi) goes lo_off bytes behind.  ACT is a compile-time RELU / LEAKY / NONE (pn_with_act<false>).
template <int ACT, bool LO, int CT, int PT>
__device__ __forceinline__ void pn_park_tile(const f32x4 (&acc)[CT][PT], const float (&bias)[4 * CT], char *smem, int wc, int lane, int lo_off) {
    constexpr int LC = CT * 4;
    static_assert(LC * sizeof(__bf16) == 16, "one 16-byte fragment per lane and pixel tile");
#pragma clang loop unroll(full)
    for (int pt = 0; pt < PT; ++pt) {
        float v[LC];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int i = 0; i < 4; ++i) v[4 * ct + i] = pn_act_ct<ACT>(acc[ct][pt][i] + bias[4 * ct + i], ACT, 0, 0);
        __bf16 ov[LC];
        pn_plane<__bf16, LC>(v, 0, ov);
        *reinterpret_cast<u32x4 *>(smem + ((wc * PT + pt) * 64 + lane) * 16) = *reinterpret_cast<u32x4 *>(ov);
        if constexpr (LO) {
            if (lo_off) {
                pn_plane<__bf16, LC>(v, 1, ov);
                *reinterpret_cast<u32x4 *>(smem + lo_off + ((wc * PT + pt) * 64 + lane) * 16) = *reinterpret_cast<u32x4 *>(ov);
            }
        }
    }
}

// ---- weight stream of the kernels that take their A operand global -> VGPR (generic kernel, conv3) ----------------------------------------
// One buffer resource for the whole pack, a wave-uniform fragment offset per cout tile (SGPR) and a 32-bit lane offset: no vector ALU work and
// no 64-bit address registers per k-step (the flat form cost 2 v_lshl_add_u64 + 6 VGPRs, profiles/README.md v23).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pn_weight_rsrc(const void *wpack) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(wpack), 0, 0x7fffffff, 0x00020000);
}
// byte offsets of the first fragment of cout tiles ctile0 .. ctile0 + CT - 1
template <int CT>
__device__ __forceinline__ void pn_weight_bases(int ctile0, int ksteps, int fragb, unsigned (&wbase)[CT]) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) wbase[ct] = (unsigned)__builtin_amdgcn_readfirstlane((ctile0 + ct) * ksteps * fragb);
}
// the first NA - 1 k-steps into the queue (load_w(offset) -> Frag); wbase moves on to the next fragment to load
template <int CT, int NA, class Frag, class LoadW>
__device__ __forceinline__ void pn_weight_prime(int fragb, unsigned (&wbase)[CT], Frag (&aq)[NA][CT], LoadW load_w) {
#pragma unroll
    for (int d = 0; d < NA - 1; ++d)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) aq[d][ct] = load_w(wbase[ct] + d * fragb);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) wbase[ct] += (NA - 1) * fragb;
}
