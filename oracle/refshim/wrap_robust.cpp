/* oracle/refshim/wrap_robust.cpp -- host entry point for the reference's RobustnessModell.cu.
 * TEST INFRASTRUCTURE ONLY.  Argument list of orc_ComputeRobustnessMask, then the block shape
 * and the packed texture configuration. */
#include "refshim_launch.h"

#include "RobustnessModell.cu"   /* the reference's file, from the directory the Makefile names */

/* `extern __shared__ float3 pixelsRef[]`: 3 x 3 float3 per thread of the block */
float3 pixelsRef[(refshim::kSharedBytes + refshim::kGuardBytes) / sizeof(float3) + 1];

using refshim::cdiv;

REFSHIM_EXPORT int ref_ComputeRobustnessMask(const float3* rawImgRef, const float3* rawImgMoved, float4* robustnessMask, const void* uvPtr,
                                             int uvPitch, int uvW, int uvH, int imgWidth, int imgHeight, int imgPitch, int maskPitch,
                                             float alpha, float beta, float thresholdM, int bx, int by, int bz, int texCfg)
{
    (void)bz;
    refshim_tex texUV = refshim::make_tex(uvPtr, uvPitch, uvW, uvH, texCfg, 0);
    refshim::shared_mem sm;
    sm.base = pixelsRef;
    sm.bytes = (size_t)bx * (size_t)by * 9 * sizeof(float3);
    return refshim::run(dim3(cdiv(imgWidth, bx), cdiv(imgHeight, by)), dim3(bx, by), sm, [&] {
        ComputeRobustnessMask(rawImgRef, rawImgMoved, robustnessMask, refshim::handle(texUV), imgWidth, imgHeight, imgPitch, maskPitch,
                              alpha, beta, thresholdM);
    });
}
