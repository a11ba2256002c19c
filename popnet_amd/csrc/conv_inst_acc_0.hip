// fp32 MFMA convolution instantiations with blocked accumulation (conv_mfma_kernel<..., ACC = 1>), share 0 of 3: rows of conv_inst_table.h.
#include "conv_mfma_kernel.h"

int pn_launch_conv_acc_part0(pn_ctx *ctx, const ConvLaunch &L, hipStream_t stream) {
    if (L.dil == 1) { PN_CONV_INSTANCES_0(PN_CASE_ACC) PN_CONV_INSTANCES_3(PN_CASE_ACC) }
    return 1;
}
