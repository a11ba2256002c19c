// MFMA convolution instantiations, share 0 of 4 (see conv_mfma.hip): the rows PN_CONV_INSTANCES_0 of conv_inst_table.h.
#include "conv_mfma_kernel.h"

int pn_launch_conv_part0(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream) {
    PN_CONV_INSTANCES_0(PN_CASES_PREC)
    return 1;
}
