// bb64s_strip_kernel (fused BasicBlock(64) walking column segments top-down, the intermediate's overlap rows carried; bb64s_kernel.h) and its launcher.
#include "bb64s_kernel.h"

int pn_launch_bb64s(pn_ctx *ctx, const BBProblem &P, hipStream_t stream) { return bb64s_launch(ctx, P, ctx->num_cus, stream); }
