// MFMA convolution instantiations with dilation 2, share 0 of 2: the rows PN_CONV_INSTANCES_D2_0 of conv_inst_table.h.
#include "conv_mfma_kernel.h"

int pn_launch_conv_d2_part0(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream) {
    PN_CONV_INSTANCES_D2_0(PN_CASES_PREC_D2)
    return 1;
}
