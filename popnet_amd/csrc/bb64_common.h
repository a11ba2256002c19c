// LDS layout, k-step order and small helpers shared by the fused BasicBlock(64) kernels: bb64_kernel.h (tile tickets) and bb64s_kernel.h (column segments).
#pragma once
#include "conv3_kernel.h"


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

// The (k-step, pixel tile) order of the 18 * PT MFMA groups ("items") of a convolution; the B-fragment queue runs BQ - 1 items ahead of the MFMAs.
// k-steps 0..15 go k-step outer.  With xch the last phase (k-steps 16, 17: both in the weight ring for the whole phase) goes pixel tile outer, so that
// a tile's accumulators are final while the tiles after it still have MFMAs to issue -- except that tiles 0 and 1 go (0, 16) (1, 16) (0, 17) (1, 17):
// k-step 17's weight fragments are read at the head of the phase and have not arrived for the second item.  Every accumulator keeps its k order.
__host__ __device__ constexpr int bb_item_ks(int n, int PT, bool xch) { return !xch || n < 16 * PT ? n / PT : n - 16 * PT < 4 ? 16 + ((n - 16 * PT) >> 1) : 16 + ((n - 16 * PT) & 1); }
__host__ __device__ constexpr int bb_item_pt(int n, int PT, bool xch) { return !xch || n < 16 * PT ? n % PT : n - 16 * PT < 4 ? (n - 16 * PT) & 1 : (n - 16 * PT) >> 1; }

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) short i16x2;
// ReLU of two packed bf16: the sign bit of a bf16 is the sign bit of the int16 with the same bits
__device__ __forceinline__ unsigned bb_relu_pk(unsigned w) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(i16x2, w), i16x2{0, 0}));
}
