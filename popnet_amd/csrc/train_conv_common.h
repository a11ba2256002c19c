// Device-inline pieces shared by the NCHW training convolutions: train.hip (train_conv_kernels.h, train_wgrad_kernels.h) and conv1x1_x3.hip
// (conv1x1_x3_kernels.h).  Only typedefs, macros, __device__ __forceinline__ functions and templates live here, so that any translation unit
// can include it: the vector types, the reuse-aware block order, pinned loads, the bf16 split, the split-bf16 MFMA triple, and the FORMAT of
// every weight pack -- per kind one element-count function and one element function, called by the per-call pack kernels, by
// pn_train_pack_refresh's wpack_all_kernel and by every launch that sizes a pack.
#pragma once
#include "conv_common.h"      // pn_xcd_block: the one copy of the remap

typedef float t_f32x4 __attribute__((ext_vector_type(4)));
typedef float t_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 t_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 t_bf4 __attribute__((ext_vector_type(4)));
typedef unsigned t_u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------
// Reuse-aware block order (round 5).  The dispatcher deals the workgroups of a launch round-robin over the 8 XCDs in linear-id order
// (x fastest) and every XCD has its own 4 MB L2.  With the plain (tile, cout block) / (ci block, cout block, slice) grids the blocks
// that read the SAME operand tile -- the cout blocks of one input tile in the forward / data-gradient kernels, the (ci, cout) blocks of
// one pixel slice in the weight gradient -- sat on different XCDs or ran a whole grid apart in time: every operand tile crossed the
// fabric once per sharer (a 256 -> 256 weight gradient staged 444 MB for 51 MB of tensors).  t_logical_block() maps the hardware id to
// a LOGICAL id such that each XCD owns one contiguous range of logical ids (a bijection: pn_xcd_block, the inference kernels' remap); the
// kernels decode the logical id with the sharing dimension fastest, so sharers run at the same time behind the same L2.  Which block
// computes which tile changes, nothing else: results are bit-identical.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int t_logical_block() {
    const int nb = (int)(gridDim.x * gridDim.y * gridDim.z);
    const int L = (int)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
    return pn_xcd_block(L, nb);
}
// forward-type grids (tiles, cout blocks): the cout blocks of a tile are neighbours in logical order
#define T_DECODE_TILE_CB(tile, cb) const int _lg = t_logical_block(), cb = _lg % (int)gridDim.y, tile = _lg / (int)gridDim.y
// weight-gradient grids (column blocks, cout blocks, slices): a slice's blocks are one contiguous logical range
#define T_DECODE_XYZ(bx, by, bz) const int _lg = t_logical_block(), bx = _lg % (int)gridDim.x, by = (_lg / (int)gridDim.x) % (int)gridDim.y, bz = _lg / (int)(gridDim.x * gridDim.y)

// Sixteen loaded values pinned in registers at this point of the program: every one of their loads has been issued before the first is
// waited for.  Without it the compiler sinks each load to its single use (legal: the addresses are provably distinct from the stores in
// between) and waits for it there -- a dependent memory round trip per element.
#define T_PIN16(a) do { _Pragma("unroll") for (int _k = 0; _k < 16; ++_k) asm volatile("" : "+v"((a)[_k])); } while (0)

// ---- split bf16 ("bf16x3") -------------------------------------------------------------------------------------------------------------
// Every fp32 value v is staged as hi = bf16(v), lo = bf16(v - hi) (round to nearest even; 16 mantissa bits together).  Elements whose
// bit in okmask is clear are staged as zero.
__device__ __forceinline__ void t_split8(const float (&v)[8], unsigned okmask, t_bf16x8 &hi, t_bf16x8 &lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x = (okmask >> j) & 1u ? v[j] : 0.f;
        const __bf16 h = (__bf16)x;
        hi[j] = h;
        lo[j] = (__bf16)(x - (float)h);
    }
}
// One product block of 32 k into ONE fp32 accumulator, in this order: a_hi b_hi + a_hi b_lo + a_lo b_hi (the dropped lo * lo term is 2^-16 relative)
__device__ __forceinline__ void t_mfma_x3(t_f32x4 &acc, const t_bf16x8 &ah, const t_bf16x8 &al, const t_bf16x8 &bh, const t_bf16x8 &bl) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
}

// ---- weight packs: the format, in one place --------------------------------------------------------------------------------------------
// A pack is the weight tensor w in the order its kernel stages it.  (Cout, Cin) is the shape of the convolution the pack SERVES; flip = 1
// reads w as the tensor of the convolution this one is the data gradient of ([Cin][Cout]...: transposed, and rotated for 3x3).
//   PN_PACK_TILE3      f32   wp[tap][ci][co]                                        tconv3_tile_kernel
//   PN_PACK_TILE3_X3   bf16  wp[plane][chunk of 32 ci][tap][co][32 ci]              tconv3_tile_x3 / _x3w_kernel
//   PN_PACK_C1_X3      bf16  wp[plane][chunk of 32 k][m][32 k], m = Cout, k = Cin   conv1x1_x3_kernel
// The split kinds hold two planes (0 = hi, 1 = lo) of t_pack_elems elements each; channels beyond Cin are zero.
__host__ __device__ inline bool t_pack_split(PnPackKind kind) { return kind != PN_PACK_TILE3; }
// elements of one plane
__host__ __device__ inline size_t t_pack_elems(PnPackKind kind, int Cout, int Cin) {
    const size_t chunks = (size_t)((Cin + 31) / 32);
    return kind == PN_PACK_C1_X3 ? chunks * Cout * 32 : kind == PN_PACK_TILE3_X3 ? chunks * 9 * Cout * 32 : (size_t)9 * Cin * Cout;
}
__host__ __device__ inline size_t t_pack_bytes(PnPackKind kind, int Cout, int Cin) {
    return t_pack_elems(kind, Cout, Cin) * (t_pack_split(kind) ? 2 * sizeof(__bf16) : sizeof(float));
}
inline unsigned t_pack_blocks(PnPackKind kind, int Cout, int Cin) { return (unsigned)((t_pack_elems(kind, Cout, Cin) + 255) / 256); }     // 256 threads, one element each

// the value of 3x3 weight (co, ci, tap) of the served convolution
__device__ __forceinline__ float t_pack_w3(const float *__restrict__ w, int Cout, int Cin, int flip, int co, int ci, int tap) {
    return flip ? w[((size_t)ci * Cout + co) * 9 + (8 - tap)] : w[((size_t)co * Cin + ci) * 9 + tap];
}
// Element i of the pack of kind KIND, written to dst (both planes for the split kinds); i beyond the pack writes nothing.
template <PnPackKind KIND>
__device__ __forceinline__ void t_pack_element(const float *__restrict__ w, void *__restrict__ dst, int Cout, int Cin, int flip, size_t i) {
    const size_t plane = t_pack_elems(KIND, Cout, Cin);
    if (i >= plane) return;
    if (KIND == PN_PACK_TILE3) {
        const int co = (int)(i % Cout), ci = (int)((i / Cout) % Cin), tap = (int)(i / ((size_t)Cout * Cin));
        ((float *)dst)[i] = t_pack_w3(w, Cout, Cin, flip, co, ci, tap);
        return;
    }
    float v = 0.f;
    if (KIND == PN_PACK_TILE3_X3) {
        const int ch = (int)(i & 31), co = (int)((i >> 5) % Cout), tap = (int)(((i >> 5) / Cout) % 9), chunk = (int)((i >> 5) / Cout / 9);
        const int ci = chunk * 32 + ch;
        if (ci < Cin) v = t_pack_w3(w, Cout, Cin, flip, co, ci, tap);
    } else {
        const int k = (int)((i >> 5) / Cout) * 32 + (int)(i & 31), m = (int)((i >> 5) % Cout);
        if (k < Cin) v = flip ? w[(size_t)k * Cout + m] : w[(size_t)m * Cin + k];
    }
    const __bf16 h = (__bf16)v;
    ((__bf16 *)dst)[i] = h;
    ((__bf16 *)dst)[plane + i] = (__bf16)(v - (float)h);
}
