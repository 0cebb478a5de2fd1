/* oracle/refshim/wrap_flow.cpp -- host entry points for the kernels of the reference's
 * opticalFlow.cu.  TEST INFRASTRUCTURE ONLY.  Argument lists are those of orc_<kernel>
 * followed by the block shape and the packed texture configuration (refshim::make_tex, textures
 * numbered in argument order). */
#include "refshim_launch.h"

#include "opticalFlow.cu"   /* the reference's file, from the directory the Makefile names */

using refshim::cdiv;

REFSHIM_EXPORT int ref_WarpingKernel(int width, int height, int stride, const void* uvPtr, int uvPitch, int uvW, int uvH, float* out,
                                     const void* imgPtr, int imgPitch, int imgW, int imgH, int bx, int by, int bz, int texCfg)
{
    (void)bz;
    refshim_tex texUV = refshim::make_tex(uvPtr, uvPitch, uvW, uvH, texCfg, 0);
    refshim_tex texImg = refshim::make_tex(imgPtr, imgPitch, imgW, imgH, texCfg, 1);
    return refshim::run(dim3(cdiv(width, bx), cdiv(height, by)), dim3(bx, by),
                        [&] { WarpingKernel(width, height, stride, refshim::handle(texUV), out, refshim::handle(texImg)); });
}

REFSHIM_EXPORT int ref_CreateFlowFieldFromTiles(float2* outImg, const void* tsPtr, int tsPitch, int tsW, int tsH, int tileSize,
                                                int tileCountX, int tileCountY, int imgWidth, int imgHeight, int imgPitch,
                                                float baseShiftX, float baseShiftY, float baseRotation, int bx, int by, int bz, int texCfg)
{
    (void)bz;
    refshim_tex texShift = refshim::make_tex(tsPtr, tsPitch, tsW, tsH, texCfg, 0);
    return refshim::run(dim3(cdiv(imgWidth, bx), cdiv(imgHeight, by)), dim3(bx, by), [&] {
        CreateFlowFieldFromTiles(outImg, refshim::handle(texShift), tileSize, tileCountX, tileCountY, imgWidth, imgHeight, imgPitch,
                                 make_float2(baseShiftX, baseShiftY), baseRotation);
    });
}

REFSHIM_EXPORT int ref_ComputeDerivativesKernel(int width, int height, int stride, float* Ix, float* Iy, float* Iz, const void* srcPtr,
                                                int srcPitch, int srcW, int srcH, const void* tgtPtr, int tgtPitch, int tgtW, int tgtH,
                                                int bx, int by, int bz, int texCfg)
{
    (void)bz;
    refshim_tex texSource = refshim::make_tex(srcPtr, srcPitch, srcW, srcH, texCfg, 0);
    refshim_tex texTarget = refshim::make_tex(tgtPtr, tgtPitch, tgtW, tgtH, texCfg, 1);
    return refshim::run(dim3(cdiv(width, bx), cdiv(height, by)), dim3(bx, by), [&] {
        ComputeDerivativesKernel(width, height, stride, Ix, Iy, Iz, refshim::handle(texSource), refshim::handle(texTarget));
    });
}

REFSHIM_EXPORT int ref_ComputeDerivatives2Kernel(int width, int height, int stride, float* Ix, float* Iy, const void* texPtr, int texPitch,
                                                 int texW, int texH, int bx, int by, int bz, int texCfg)
{
    (void)bz;
    refshim_tex tex = refshim::make_tex(texPtr, texPitch, texW, texH, texCfg, 0);
    return refshim::run(dim3(cdiv(width, bx), cdiv(height, by)), dim3(bx, by),
                        [&] { ComputeDerivatives2Kernel(width, height, stride, Ix, Iy, refshim::handle(tex)); });
}

REFSHIM_EXPORT int ref_lucasKanadeOptim(float2* shifts, const float* imFx, const float* imFy, const float* imFt, int pitchShift,
                                        int pitchImg, int width, int height, int halfWindowSize, float minDet, int bx, int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(width, bx), cdiv(height, by)), dim3(bx, by),
                        [&] { lucasKanadeOptim(shifts, imFx, imFy, imFt, pitchShift, pitchImg, width, height, halfWindowSize, minDet); });
}
