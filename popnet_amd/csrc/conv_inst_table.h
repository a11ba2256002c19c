// The instantiation table of the generic MFMA convolution (conv_mfma_kernel.h), in ONE place.  Every row is
// X(kernel size, stride, LDS pitch class, tile configuration) and stands for the bf16 and the fp32 instance.  The four shares are what
// conv_inst_0..3.hip compile (PN_CONV_INSTANCES_<n>(PN_CASES_PREC) is the whole body of a share's dispatch); pn_conv_has_instance
// (conv_mfma.hip) expands the same rows into the predicate the planner asks (conv_plan.h::pn_plan_conv_tiles), so a row added or removed
// here changes the dispatch and the predicate together.
#pragma once

#define PN_CONV_INST_ALLCFG(X, KS, ST, PITCH) \
    X(KS, ST, PITCH, PN_CFG_C128) X(KS, ST, PITCH, PN_CFG_C64) X(KS, ST, PITCH, PN_CFG_C32) X(KS, ST, PITCH, PN_CFG_C16)

#define PN_CONV_INSTANCES_0(X)       \
    PN_CONV_INST_ALLCFG(X, 3, 1, 32) \
    PN_CONV_INST_ALLCFG(X, 1, 1, 32)

#define PN_CONV_INSTANCES_1(X)       \
    PN_CONV_INST_ALLCFG(X, 3, 1, 64) \
    PN_CONV_INST_ALLCFG(X, 1, 1, 64) \
    X(3, 1, 64, PN_CFG_C64W)

#define PN_CONV_INSTANCES_2(X)        \
    PN_CONV_INST_ALLCFG(X, 3, 1, 120) \
    PN_CONV_INST_ALLCFG(X, 1, 1, 120) \
    X(3, 1, 120, PN_CFG_C64W)

// (no 1x1 instance at pitch 16, no stride-2 instance at pitch 16 / 32 or for the 32- / 16-cout blocks: the planner takes the next wider class or refuses)
#define PN_CONV_INSTANCES_3(X)       \
    PN_CONV_INST_ALLCFG(X, 3, 1, 16) \
    X(3, 2, 64, PN_CFG_C128)         \
    X(3, 2, 64, PN_CFG_C64)          \
    X(1, 2, 64, PN_CFG_C128)         \
    X(1, 2, 64, PN_CFG_C64)          \
    X(3, 2, 120, PN_CFG_C128)        \
    X(3, 2, 120, PN_CFG_C64)         \
    X(1, 2, 120, PN_CFG_C128)        \
    X(1, 2, 120, PN_CFG_C64)

// Dilation 2 (conv_mfma_kernel<..., DIL = 2>): A2J's dilated 3x3 layer4 convolutions, 512 -> 512 channels at stride 1 -- the 128-cout block and the
// 64-cout block the planner takes on small maps, every pitch class.  Rows of their own: the rows above are the DIL = 1 instances they always were.
#define PN_CONV_INSTANCES_D2_0(X) \
    X(3, 1, 16, PN_CFG_C128) X(3, 1, 16, PN_CFG_C64) X(3, 1, 32, PN_CFG_C128) X(3, 1, 32, PN_CFG_C64)
#define PN_CONV_INSTANCES_D2_1(X) \
    X(3, 1, 64, PN_CFG_C128) X(3, 1, 64, PN_CFG_C64) X(3, 1, 120, PN_CFG_C128) X(3, 1, 120, PN_CFG_C64)
#define PN_CONV_INSTANCES_D2(X) PN_CONV_INSTANCES_D2_0(X) PN_CONV_INSTANCES_D2_1(X)

#define PN_CONV_INSTANCES(X) PN_CONV_INSTANCES_0(X) PN_CONV_INSTANCES_1(X) PN_CONV_INSTANCES_2(X) PN_CONV_INSTANCES_3(X)
