// fp32 MFMA convolution instantiations with blocked accumulation (conv_mfma_kernel<..., ACC = 1>), share 2 of 3: rows of conv_inst_table.h.
#include "conv_mfma_kernel.h"

int pn_launch_conv_acc_part2(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream) {
    if (L.dil == 1) { PN_CONV_INSTANCES_2(PN_CASE_ACC) }
    if (L.dil == 2) { PN_CONV_INSTANCES_D2(PN_CASE_ACC_D2) }
    return 1;
}
