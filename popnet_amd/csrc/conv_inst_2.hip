// MFMA convolution instantiations, share 2 of 4 (see conv_mfma.hip): the rows PN_CONV_INSTANCES_2 of conv_inst_table.h.
#include "conv_mfma_kernel.h"

int pn_launch_conv_part2(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream) {
    PN_CONV_INSTANCES_2(PN_CASES_PREC)
    return 1;
}
