/* oracle/refshim/wrap_shift.cpp -- host entry points for the kernels of the reference's
 * ShiftMinimizerKernels.cu.  TEST INFRASTRUCTURE ONLY.  Argument lists are those of
 * orc_<kernel> followed by the block shape. */
#include "refshim_launch.h"

#include "ShiftMinimizerKernels.cu"   /* the reference's file, from the directory the Makefile names */

using refshim::cdiv;

REFSHIM_EXPORT int ref_copyShiftMatrix(float* matrices, int tileCount, int imageCount, int shiftCount, int bx, int by, int bz)
{
    (void)by; (void)bz;
    return refshim::run(dim3(cdiv(tileCount, bx)), dim3(bx), [&] { copyShiftMatrix(matrices, tileCount, imageCount, shiftCount); });
}

REFSHIM_EXPORT int ref_setPointers(float** shiftMatrixArray, float** shiftMatrixSafeArray, float** matrixSquareArray,
                                   float** matrixInvertedArray, float** solvedMatrixArray, float2** shiftOneToOneArray,
                                   float2** shiftMeasuredArray, float2** shiftOptimArray, float* shiftMatrices, float* shiftSafeMatrices,
                                   float* matricesSquared, float* matricesInverted, float* solvedMatrices, float2* shiftsOneToOne,
                                   float2* shiftsMeasured, float2* shiftsOptim, int tileCount, int imageCount, int shiftCount, int bx,
                                   int by, int bz)
{
    (void)by; (void)bz;
    return refshim::run(dim3(cdiv(tileCount, bx)), dim3(bx), [&] {
        setPointers(shiftMatrixArray, shiftMatrixSafeArray, matrixSquareArray, matrixInvertedArray, solvedMatrixArray, shiftOneToOneArray,
                    shiftMeasuredArray, shiftOptimArray, shiftMatrices, shiftSafeMatrices, matricesSquared, matricesInverted,
                    solvedMatrices, shiftsOneToOne, shiftsMeasured, shiftsOptim, tileCount, imageCount, shiftCount);
    });
}

REFSHIM_EXPORT int ref_checkForOutliers(float2* measuredShifts, const float* optimShiftsT, float* shiftMatrix, int* status,
                                        const int* inversionInfo, int tileCount, int imageCount, int shiftCount, int bx, int by, int bz)
{
    (void)by; (void)bz;
    return refshim::run(dim3(cdiv(tileCount, bx)), dim3(bx), [&] {
        checkForOutliers(measuredShifts, optimShiftsT, shiftMatrix, status, const_cast<int*>(inversionInfo), tileCount, imageCount,
                         shiftCount);
    });
}

REFSHIM_EXPORT int ref_transposeShifts(float2* measuredShifts, const float* measuredShiftsT, const float* shiftsOneToOneT,
                                       float2* shiftsOneToOne, int tileCount, int imageCount, int shiftCount, int bx, int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(tileCount, bx), cdiv(shiftCount, by)), dim3(bx, by), [&] {
        transposeShifts(measuredShifts, measuredShiftsT, shiftsOneToOneT, shiftsOneToOne, tileCount, imageCount, shiftCount);
    });
}

REFSHIM_EXPORT int ref_getOptimalShifts(float2* optimalShifts, const float2* bestShifts, int imageCount, int tileCountX, int tileCountY,
                                        int optimalShiftsPitch, int referenceImage, int imageToTrack, int bx, int by, int bz)
{
    (void)bz;
    return refshim::run(dim3(cdiv(tileCountX, bx), cdiv(tileCountY, by)), dim3(bx, by), [&] {
        getOptimalShifts(optimalShifts, bestShifts, imageCount, tileCountX, tileCountY, optimalShiftsPitch, referenceImage, imageToTrack);
    });
}

/* thread x = shift, y = tile column, z = tile row */
REFSHIM_EXPORT int ref_concatenateShifts(const float2* const* shiftIn, const int* shiftInPitch, float2* shiftOut, int shiftCount,
                                         int tileCountX, int tileCountY, int bx, int by, int bz)
{
    return refshim::run(dim3(cdiv(shiftCount, bx), cdiv(tileCountX, by), cdiv(tileCountY, bz)), dim3(bx, by, bz), [&] {
        concatenateShifts(shiftIn, const_cast<int*>(shiftInPitch), shiftOut, shiftCount, tileCountX, tileCountY);
    });
}

REFSHIM_EXPORT int ref_separateShifts(const float2* shiftIn, float2* const* shiftOut, const int* shiftOutPitch, int shiftCount,
                                      int tileCountX, int tileCountY, int bx, int by, int bz)
{
    return refshim::run(dim3(cdiv(shiftCount, bx), cdiv(tileCountX, by), cdiv(tileCountY, bz)), dim3(bx, by, bz), [&] {
        separateShifts(shiftIn, shiftOut, const_cast<int*>(shiftOutPitch), shiftCount, tileCountX, tileCountY);
    });
}
