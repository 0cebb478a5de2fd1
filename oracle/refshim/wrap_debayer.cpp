/* oracle/refshim/wrap_debayer.cpp -- host entry points for the kernels of the reference's
 * DeBayerKernels.cu (demosaic and the accumulate kernels).  TEST INFRASTRUCTURE ONLY.
 * Argument lists are those of orc_<kernel> followed by the block shape and, where the kernel
 * reads textures, the packed texture configuration (refshim::make_tex). */
#include "refshim_launch.h"

#include "DeBayerKernels.cu"   /* the reference's file, from the directory the Makefile names */

/* the file only declares its constant-memory CFA table; this is its storage (RGGB until set) */
extern "C" {
BayerColor c_cfaPattern[2][2] = {{(BayerColor)0, (BayerColor)1}, {(BayerColor)1, (BayerColor)2}};
}

using refshim::cdiv;

static inline float3 f3(const float* v) { return make_float3(v[0], v[1], v[2]); }

REFSHIM_EXPORT int ref_set_cfa_pattern(const int32_t* p)
{
    for (int i = 0; i < 4; i++) c_cfaPattern[i / 2][i % 2] = (BayerColor)p[i];
    return 0;
}

REFSHIM_EXPORT int ref_deBayersSubSample3(const uint16_t* dataIn, float3* imgOut, float maxVal, int dimX, int dimY, int strideOut, int bx,
                                          int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(dimX, bx), cdiv(dimY, by)), dim3(bx, by),
                        [&] { deBayersSubSample3(const_cast<uint16_t*>(dataIn), imgOut, maxVal, dimX, dimY, strideOut); });
}

REFSHIM_EXPORT int ref_deBayerGreenKernel(int width, int height, const float* imgIn, int strideIn, float3* outImage, int strideOut,
                                          const float* blackPoint, const float* scale, int bx, int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(width, bx), cdiv(height, by)), dim3(bx, by),
                        [&] { deBayerGreenKernel(width, height, imgIn, strideIn, outImage, strideOut, f3(blackPoint), f3(scale)); });
}

REFSHIM_EXPORT int ref_deBayerRedBlueKernel(int width, int height, const float* imgIn, int strideIn, float3* outImage, int strideOut,
                                            const float* blackPoint, const float* scale, int bx, int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(width, bx), cdiv(height, by)), dim3(bx, by),
                        [&] { deBayerRedBlueKernel(width, height, imgIn, strideIn, outImage, strideOut, f3(blackPoint), f3(scale)); });
}

REFSHIM_EXPORT int ref_accumulateImages(const uint16_t* dataIn, float3* imgOut, float3* totalWeights, const float4* certaintyMask,
                                        const float3* kernelParam, const float2* shifts, const float* whiteLevel, const float* blackLevel,
                                        int dimX, int dimY, int strideOut, int strideMask, int strideShift, int bx, int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(dimX, bx), cdiv(dimY, by)), dim3(bx, by), [&] {
        accumulateImages(const_cast<uint16_t*>(dataIn), imgOut, totalWeights, certaintyMask, kernelParam, shifts, f3(whiteLevel),
                         f3(blackLevel), dimX, dimY, strideOut, strideMask, strideShift);
    });
}

REFSHIM_EXPORT int ref_accumulateImagesSuperRes(const uint16_t* dataIn, float3* imgOut, float3* totalWeights, const float4* certaintyMask,
                                                const void* kpPtr, int kpPitch, int kpW, int kpH, const void* shPtr, int shPitch, int shW,
                                                int shH, const float* whiteLevel, const float* blackLevel, int dimX, int dimY,
                                                int strideOut, int strideMask, int bx, int by, int bz, int texCfg)
{
    (void)bz;
    refshim_tex texK = refshim::make_tex(kpPtr, kpPitch, kpW, kpH, texCfg, 0);
    refshim_tex texS = refshim::make_tex(shPtr, shPitch, shW, shH, texCfg, 1);
    return refshim::run(dim3(cdiv(dimX, bx), cdiv(dimY, by)), dim3(bx, by), [&] {
        accumulateImagesSuperRes(const_cast<uint16_t*>(dataIn), imgOut, totalWeights, certaintyMask, refshim::handle(texK),
                                 refshim::handle(texS), f3(whiteLevel), f3(blackLevel), dimX, dimY, strideOut, strideMask, kpPitch,
                                 shPitch);
    });
}
