/* oracle/refshim/wrap_kernel.cpp -- host entry points for the kernels of the reference's
 * kernel.cu (tile tracker, finishing, kernel parameters, Fourier helpers).
 * TEST INFRASTRUCTURE ONLY.  Every ref_<kernel> takes the argument list of orc_<kernel>
 * (oracle/bindings.py) followed by the block shape, and returns refshim::take_error(). */
#include "refshim_launch.h"

#include "kernel.cu"   /* the reference's file, from the directory the Makefile names */

/* `extern __shared__ float shared[]` of the two box filters */
alignas(16) float shared[(refshim::kSharedBytes + refshim::kGuardBytes) / sizeof(float)];

using refshim::cdiv;

REFSHIM_EXPORT int ref_squaredSum(const float* inTiles, float* outValues, int maxShift, int tileSize, int tileCount, int bx, int by,
                                  int bz)
{
    (void)by; (void)bz;
    return refshim::run(dim3(cdiv(tileCount, bx)), dim3(bx), [&] { squaredSum(inTiles, outValues, maxShift, tileSize, tileCount); });
}

/* block = (T + 2S, 1, bz) for X and (1, T + 2S, bz) for Y: the kernels index the shared row by the pixel
 * coordinate, so the block must span the tile side */
REFSHIM_EXPORT int ref_boxFilterWithBorderX(const float* inTiles, float* outTiles, int maxShift, int tileSize, int tileCount, int bx,
                                            int by, int bz)
{
    const int side = tileSize + 2 * maxShift;
    refshim::shared_mem sm;
    sm.base = shared;
    sm.bytes = (size_t)bz * (size_t)side * sizeof(float);
    return refshim::run_threads(dim3(cdiv(side, bx), cdiv(side, by), cdiv(tileCount, bz)), dim3(bx, by, bz), sm,
                                [&] { boxFilterWithBorderX(inTiles, outTiles, maxShift, tileSize, tileCount); });
}

REFSHIM_EXPORT int ref_boxFilterWithBorderY(const float* inTiles, float* outTiles, int maxShift, int tileSize, int tileCount, int bx,
                                            int by, int bz)
{
    const int side = tileSize + 2 * maxShift;
    refshim::shared_mem sm;
    sm.base = shared;
    sm.bytes = (size_t)bz * (size_t)side * sizeof(float);
    return refshim::run_threads(dim3(cdiv(side, bx), cdiv(side, by), cdiv(tileCount, bz)), dim3(bx, by, bz), sm,
                                [&] { boxFilterWithBorderY(inTiles, outTiles, maxShift, tileSize, tileCount); });
}

REFSHIM_EXPORT int ref_normalizedCC(const float* ccImage, const float* squaredTemplate, const float* boxFilteredImage, float* shiftImage,
                                    int maxShift, int tileSize, int tileCount, int bx, int by, int bz)
{
    const int side = 2 * maxShift + 1;
    return refshim::run(dim3(cdiv(side, bx), cdiv(side, by), cdiv(tileCount, bz)), dim3(bx, by, bz),
                        [&] { normalizedCC(ccImage, squaredTemplate, boxFilteredImage, shiftImage, maxShift, tileSize, tileCount); });
}

REFSHIM_EXPORT int ref_convertToTilesOverlapBorder(const float* inImg, float* outTiles, int imgWidth, int imgHeight, int imgPitch,
                                                   int maxShift, int tileSize, int tileCountX, int tileCountY, float baseShiftX,
                                                   float baseShiftY, float baseRotation, int bx, int by, int bz)
{
    const int side = tileSize + 2 * maxShift;
    return refshim::run(dim3(cdiv(side, bx), cdiv(side, by), cdiv(tileCountX * tileCountY, bz)), dim3(bx, by, bz), [&] {
        convertToTilesOverlapBorder(inImg, outTiles, imgWidth, imgHeight, imgPitch, maxShift, tileSize, tileCountX, tileCountY,
                                    make_float2(baseShiftX, baseShiftY), baseRotation);
    });
}

REFSHIM_EXPORT int ref_convertToTilesOverlapPreShift(const float* inImg, float* outTiles, const float2* preShift, int preShiftPitch,
                                                     int imgWidth, int imgHeight, int imgPitch, int maxShift, int tileSize,
                                                     int tileCountX, int tileCountY, float baseShiftX, float baseShiftY,
                                                     float baseRotation, int bx, int by, int bz)
{
    const int side = tileSize + 2 * maxShift;
    return refshim::run(dim3(cdiv(side, bx), cdiv(side, by), cdiv(tileCountX * tileCountY, bz)), dim3(bx, by, bz), [&] {
        convertToTilesOverlapPreShift(inImg, outTiles, preShift, preShiftPitch, imgWidth, imgHeight, imgPitch, maxShift, tileSize,
                                      tileCountX, tileCountY, make_float2(baseShiftX, baseShiftY), baseRotation);
    });
}

REFSHIM_EXPORT int ref_GammasRGB(float3* inOutImg, int imgWidth, int imgHeight, int imgPitch, int bx, int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(imgWidth, bx), cdiv(imgHeight, by)), dim3(bx, by), [&] { GammasRGB(inOutImg, imgWidth, imgHeight, imgPitch); });
}

REFSHIM_EXPORT int ref_ApplyWeighting(float3* inOutImg, const float3* finalImg, const float3* weight, int imgWidth, int imgHeight,
                                      int imgPitch, float threshold, int bx, int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(imgWidth, bx), cdiv(imgHeight, by)), dim3(bx, by),
                        [&] { ApplyWeighting(inOutImg, finalImg, weight, imgWidth, imgHeight, imgPitch, threshold); });
}

REFSHIM_EXPORT int ref_conjugateComplexMulKernel(const float2* aIn, float2* bInOut, int maxElem, int bx, int by, int bz)
{
    (void)by; (void)bz;
    return refshim::run(dim3(cdiv(maxElem, bx)), dim3(bx), [&] { conjugateComplexMulKernel(aIn, bInOut, maxElem); });
}

REFSHIM_EXPORT int ref_findMinimum(const float* shiftImage, float2* coordinates, int coordinatesPitch, int maxShift, int tileCount,
                                   int tileCountX, float threshold, int bx, int by, int bz)
{
    (void)by; (void)bz;
    return refshim::run(dim3(cdiv(tileCount, bx)), dim3(bx),
                        [&] { findMinimum(shiftImage, coordinates, coordinatesPitch, maxShift, tileCount, tileCountX, threshold); });
}

REFSHIM_EXPORT int ref_UpSampleShifts(const float2* inShift, float2* outShift, int inPitch, int outPitch, int oldLevel, int newLevel,
                                      int oldCountX, int oldCountY, int newCountX, int newCountY, int oldTileSize, int newTileSize, int bx,
                                      int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(newCountX, bx), cdiv(newCountY, by)), dim3(bx, by), [&] {
        UpSampleShifts(inShift, outShift, inPitch, outPitch, oldLevel, newLevel, oldCountX, oldCountY, newCountX, newCountY, oldTileSize,
                       newTileSize);
    });
}

REFSHIM_EXPORT int ref_ComputeStructureTensor(const float* imgDx, const float* imgDy, float3* outImg, int imgWidth, int imgHeight,
                                              int imgDxDyPitch, int imgOutPitch, int bx, int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(imgWidth, bx), cdiv(imgHeight, by)), dim3(bx, by),
                        [&] { ComputeStructureTensor(imgDx, imgDy, outImg, imgWidth, imgHeight, imgDxDyPitch, imgOutPitch); });
}

REFSHIM_EXPORT int ref_ComputeKernelParam(float3* kernelImg, int imgWidth, int imgHeight, int imgOutPitch, float Dth, float Dtr,
                                          float kDetail, float kDenoise, float kStretch, float kShrink, int bx, int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(imgWidth, bx), cdiv(imgHeight, by)), dim3(bx, by), [&] {
        ComputeKernelParam(kernelImg, imgWidth, imgHeight, imgOutPitch, Dth, Dtr, kDetail, kDenoise, kStretch, kShrink);
    });
}

REFSHIM_EXPORT int ref_fourierFilter(float2* img, size_t stride, int width, int height, float lp, float hp, float lps, float hps,
                                     int clearAxis, int bx, int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(width / 2 + 1, bx), cdiv(height, by)), dim3(bx, by),
                        [&] { fourierFilter(img, stride, width, height, lp, hp, lps, hps, clearAxis); });
}

REFSHIM_EXPORT int ref_fftshift(float2* fft, int width, int height, int bx, int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(width, bx), cdiv(height, by)), dim3(bx, by), [&] { fftshift(fft, width, height); });
}
