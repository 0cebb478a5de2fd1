/*
 * mfsr.h -- C-ABI of the MI355X-native multi-frame super-resolution hot path.
 *
 * Drop-in boundary for the align -> fuse -> upsample path of
 * zhongzisha/multi_frame_super_resolution (the ImageStackAlignator CUDA
 * kernels in test_opencv, the five .cu files).  The reference exposes that path as
 * unmangled `extern "C" __global__` symbols loaded by name by a host that is
 * not in the repository, and its own host-side FFI convention is
 * `extern "C" void f(T* devPtr..., int width, int height...)`
 * (test_opencv/myKernels.cu:114-120,156-165; decls test_opencv/main.cpp:763-767).
 * Each entry point below replaces the launch of ONE reference kernel: same
 * name (prefixed mfsr_), same argument order, same units (pitches in BYTES,
 * dims in elements, raw device pointers), with
 *   - cudaTextureObject_t  ->  mfsr_tex2d {ptr, pitch, width, height} by value
 *     (linear filtering, normalised coordinates; MIRROR addressing for images,
 *     CLAMP for flow / parameter fields -- stated per function),
 *   - the module constant c_cfaPattern -> mfsr_set_cfa_pattern(), read by these
 *     reference-shaped entry points only (bursts and frame streams take cfg.cfa),
 *   - grid/block shapes chosen by the library,
 *   - one trailing mfsr_stream_t (a hipStream_t; NULL = default stream).
 *
 * Conventions (reference error convention: cudaError_t return + fprintf(stderr),
 * test_opencv/kernel.cu:36-114):
 *   - every function returns int: 0 = success, >0 = hipError_t, <0 = MFSR_E_*;
 *     nothing throws; failures are logged to stderr;
 *   - all calls are asynchronous on `stream` unless named *_sync;
 *   - the caller allocates and frees every buffer; kernels never allocate;
 *     accumulators are zero-initialised by the caller and accumulated across
 *     calls (DeBayerKernels.cu:306-307,374-375);
 *   - untouched border rings (caller initialises): deBayer* 2 px,
 *     accumulate* 1 px, lucasKanadeOptim halfWindowSize px,
 *     ComputeRobustnessMask 1 px.
 *   - there is NO CPU fallback: without a HIP device every call fails.
 */
#ifndef MFSR_H
#define MFSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFSR_VERSION 100
#define MFSR_MAX_FUSE_GROUP 4 /* frames one warp+fuse call takes (mfsr_accumulateSuperResFullN, cfg.pairFrames) */
#define MFSR_MAX_BURST_FUSE 16 /* frames the burst form takes: up to four such groups (mfsr_accumulateSuperResBurst) */

typedef void* mfsr_stream_t; /* hipStream_t */

typedef struct { float x, y; } mfsr_float2;
typedef struct { float x, y, z; } mfsr_float3;
typedef struct { float x, y, z, w; } mfsr_float4;

/* stand-in for cudaTextureObject_t: pitched 2-D array in device memory */
typedef struct {
    const void* ptr;
    int32_t pitch; /* bytes */
    int32_t width; /* texels */
    int32_t height;
} mfsr_tex2d;

enum {
    MFSR_OK = 0,
    MFSR_E_INVALID = -1,   /* bad argument (null pointer, non-positive size, pitch too small) */
    MFSR_E_UNSUPPORTED = -2, /* parameter outside what the kernels are built for */
    MFSR_E_NODEVICE = -3,  /* no usable HIP device */
    MFSR_E_WORKSPACE = -4  /* workspace too small */
};

/* enum BayerColor, DeBayerKernels.cu:28-37 */
enum { MFSR_RED = 0, MFSR_GREEN = 1, MFSR_BLUE = 2, MFSR_CYAN = 3, MFSR_MAGENTA = 4, MFSR_YELLOW = 5, MFSR_WHITE = 6 };

const char* mfsr_error_string(int code);
int mfsr_version(void);
/* number of visible HIP devices (0 if none); never fails */
int mfsr_device_count(void);

/* ---- A0: c_cfaPattern[2][2], DeBayerKernels.cu:40-41 ---------------------- */
/* pattern[0..3] = {[0][0],[0][1],[1][0],[1][1]}; RGGB = {0,1,1,2}; entries 0 .. MFSR_WHITE, else MFSR_E_INVALID.
 * Process-wide state like the reference's module constant, read at launch time by the reference-shaped entry points
 * (mfsr_deBayer*, mfsr_prepareFrame*, mfsr_accumulate*, mfsr_robustnessMaskGroup).  A burst (mfsr_burst_*) or frame stream
 * (mfsr_stream_*) takes cfg.cfa instead, checked the same way by its create call, and neither reads nor writes this one. */
int mfsr_set_cfa_pattern(const int32_t pattern[4]);
int mfsr_get_cfa_pattern(int32_t pattern[4]);

/* ---- A: DeBayerKernels.cu ------------------------------------------------- */
/* A1 deBayersSubSample3 :244 -- dimX,dimY = OUTPUT (half-res) dims; dataIn is
 * dense u16 with row stride 2*dimX elements. */
int mfsr_deBayersSubSample3(const uint16_t* dataIn, mfsr_float3* imgOut, float maxVal, int dimX, int dimY, int strideOut,
                            mfsr_stream_t stream);
/* A2 deBayerGreenKernel :55 */
int mfsr_deBayerGreenKernel(int width, int height, const float* imgIn, int strideIn, mfsr_float3* outImage,
                            int strideOut, mfsr_float3 blackPoint, mfsr_float3 scale, mfsr_stream_t stream);
/* A3 deBayerRedBlueKernel :153 (run after A2 has completed on the stream) */
int mfsr_deBayerRedBlueKernel(int width, int height, const float* imgIn, int strideIn, mfsr_float3* outImage,
                              int strideOut, mfsr_float3 blackPoint, mfsr_float3 scale, mfsr_stream_t stream);
/* G1 accumulateImages :290 (x1 merge; kernelParam rows use strideOut, :308) */
int mfsr_accumulateImages(const uint16_t* dataIn, mfsr_float3* imgOut, mfsr_float3* totalWeights,
                          const mfsr_float4* certaintyMask, const mfsr_float3* kernelParam, const mfsr_float2* shifts,
                          mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int dimX, int dimY, int strideOut,
                          int strideMask, int strideShift, mfsr_stream_t stream);
/* G2 accumulateImagesSuperRes :379 (x2 merge, output grid dimX x dimY covering
 * the central half of the frame).  kernelParam: float4 texture, shifts: float2
 * texture, both CLAMP.  strideKernelParam/strideShift of the reference are
 * carried inside the descriptors. */
int mfsr_accumulateImagesSuperRes(const uint16_t* dataIn, mfsr_float3* imgOut, mfsr_float3* totalWeights,
                                  const mfsr_float4* certaintyMask, mfsr_tex2d kernelParam, mfsr_tex2d shifts,
                                  mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int dimX, int dimY, int strideOut,
                                  int strideMask, mfsr_stream_t stream);
/* G2 generalised to integer scale s (1..8) on the FULL frame: output grid
 * (s*dimX) x (s*dimY); the build's extension of :379-468. */
int mfsr_accumulateSuperResFull(const uint16_t* dataIn, mfsr_float3* imgOut, mfsr_float3* totalWeights,
                                const mfsr_float4* certaintyMask, mfsr_tex2d kernelParam, mfsr_tex2d shifts,
                                mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int dimX, int dimY, int scale,
                                int strideOut, int strideMask, mfsr_stream_t stream);

/* Two frames in one call (frame 0, then frame 1): what two mfsr_accumulateSuperResFull calls compute,
 * with the accumulators read and written once where the x2 tile kernel applies.  Equal to the
 * two-call sequence to fp32 rounding (the two per-pixel sums are added to each other first). */
int mfsr_accumulateSuperResFull2(const uint16_t* dataIn0, const uint16_t* dataIn1, mfsr_float3* imgOut,
                                 mfsr_float3* totalWeights, const mfsr_float4* certaintyMask0,
                                 const mfsr_float4* certaintyMask1, mfsr_tex2d kernelParam, mfsr_tex2d shifts0,
                                 mfsr_tex2d shifts1, mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int dimX, int dimY,
                                 int scale, int strideOut, int strideMask, mfsr_stream_t stream);

/* nFrames (1 .. MFSR_MAX_FUSE_GROUP) frames in one call (dataIn / certaintyMask / shifts: host arrays of nFrames entries);
 * the frames add in call order.  At scale 2 / 4 with the fields at a quarter / an eighth of the HR size (the Bayer pipeline)
 * the whole group is ONE pass over the accumulators; other geometries take it two frames at a time.
 * accumulatorsUndefined != 0: imgOut / totalWeights are OVERWRITTEN as if they had been zeroed before
 * the call -- the first launch of a burst needs neither the memset nor the read of the two planes. */
int mfsr_accumulateSuperResFullN(int nFrames, const uint16_t* const* dataIn, mfsr_float3* imgOut, mfsr_float3* totalWeights,
                                 const mfsr_float4* const* certaintyMask, mfsr_tex2d kernelParam, const mfsr_tex2d* shifts,
                                 mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int dimX, int dimY, int scale,
                                 int strideOut, int strideMask, int accumulatorsUndefined, mfsr_stream_t stream);

/* mfsr_accumulateSuperResFullN restricted to HR rows [rowBegin, rowEnd) (rowBegin % 16 == 0; rowEnd % 16 == 0 or
 * rowEnd == scale*dimY): a burst whose fuse stage is sharded over HR row stripes (multi-GPU, mfsr_dist_*) calls it once
 * per stripe; every pixel of the window gets exactly the whole-frame result.  Raw / certainty / shift buffers keep their
 * whole-frame addressing -- only the rows the window's taps reach are read. */
int mfsr_accumulateSuperResFullRows(int nFrames, const uint16_t* const* dataIn, mfsr_float3* imgOut, mfsr_float3* totalWeights,
                                    const mfsr_float4* const* certaintyMask, mfsr_tex2d kernelParam, const mfsr_tex2d* shifts,
                                    mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int dimX, int dimY, int scale,
                                    int strideOut, int strideMask, int accumulatorsUndefined, int rowBegin, int rowEnd,
                                    mfsr_stream_t stream);

/* Zoom window: mfsr_accumulateSuperResFullRows on the HR rectangle [x0, x0+w) x [y0, y0+h) of the (scale*dimX) x (scale*dimY)
 * grid, with imgOut / totalWeights holding THAT RECTANGLE ONLY (pointers = its pixel (x0, y0), pitch strideOut >= 12*w bytes,
 * 16-byte aligned).  Every pixel of it gets exactly the whole-frame result; raw / certainty / shift buffers keep their
 * whole-frame addressing and are read around the window.  x0, y0 multiples of 16; w, h multiples of 16 or reaching the
 * frame's right / bottom edge; x0 = y0 = w = h = 0: the whole frame.  accumulatorsUndefined as for FullN (only the window's
 * bytes are written).  Rows outside [0, h) and columns outside [0, w) of the buffers are never touched. */
int mfsr_accumulateSuperResFullWindow(int nFrames, const uint16_t* const* dataIn, mfsr_float3* imgOut, mfsr_float3* totalWeights,
                                      const mfsr_float4* const* certaintyMask, mfsr_tex2d kernelParam, const mfsr_tex2d* shifts,
                                      mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int dimX, int dimY, int scale,
                                      int strideOut, int strideMask, int accumulatorsUndefined, int x0, int y0, int w, int h,
                                      mfsr_stream_t stream);

/* The burst form of mfsr_accumulateSuperResFullN: nFrames = 8, 12 or 16 frames (whole groups of MFSR_MAX_FUSE_GROUP, at most
 * MFSR_MAX_BURST_FUSE) in ONE pass over the accumulators -- both plane-sets are read (not at all with accumulatorsUndefined)
 * and written once for the whole burst instead of once per group.  Bit for bit the result of nFrames / 4 successive FullN
 * calls of four frames each on the same inputs, accumulatorsUndefined given to the first.  Only where the x2 Bayer tile kernel
 * applies: scale 2, a Bayer pattern (mfsr_set_cfa_pattern), kernelParam and shifts at half the raw size, raw dimensions
 * multiples of 4; everything else returns MFSR_E_UNSUPPORTED and touches nothing (other frame counts: MFSR_E_INVALID).
 * The images are given as descriptors: imgOut / totalWeights float3, (scale*rawWidth) x (scale*rawHeight), 16-byte aligned rows;
 * certaintyMasks float4 at half the raw size, all with one row pitch; dataIn dense uint16_t rows. */
int mfsr_accumulateSuperResBurst(int nFrames, const uint16_t* const* dataIn, mfsr_tex2d imgOut, mfsr_tex2d totalWeights,
                                 const mfsr_tex2d* certaintyMasks, mfsr_tex2d kernelParam, const mfsr_tex2d* shifts,
                                 mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int scale, int accumulatorsUndefined,
                                 mfsr_stream_t stream);

/* mfsr_accumulateSuperResBurst followed by the plain uint16_t finish of the whole frame, without the finish pass: the tile
 * launch finishes its pixels from the sums it still holds on chip and a small launch finishes the 16-pixel ring after the
 * margin launch.  Both accumulators are written as by mfsr_accumulateSuperResBurst, and out16 (dense RGB, out16Width x
 * out16Height = the accumulators' size, 8-byte aligned) is bit for bit what mfsr_finishFusedWindow with the same finish
 * arguments writes from them.  The finish arguments are mfsr_finishFusedWindow's, the fallback image (float3) as a descriptor
 * like the others (fallback.ptr may be NULL: no fallback).  The refusals of mfsr_accumulateSuperResBurst apply; in addition
 * everything but the plain finish of the whole frame -- applyGamma != 0, maxOut != 65535, a window (colOffset, rowOffset != 0
 * or out16Width, out16Height != fullWidth, fullHeight != the accumulators' size) -- returns MFSR_E_UNSUPPORTED.  A refusal
 * touches nothing. */
int mfsr_accumulateSuperResBurstFinish(int nFrames, const uint16_t* const* dataIn, mfsr_tex2d imgOut, mfsr_tex2d totalWeights,
                                       const mfsr_tex2d* certaintyMasks, mfsr_tex2d kernelParam, const mfsr_tex2d* shifts,
                                       mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int scale, int accumulatorsUndefined,
                                       mfsr_tex2d fallback, float u0, float u1, float v0, float v1, float threshold,
                                       uint16_t* out16, int out16Width, int out16Height, int applyGamma, float maxOut,
                                       int colOffset, int rowOffset, int fullWidth, int fullHeight, mfsr_stream_t stream);

/* ---- B/E/H/I: kernel.cu --------------------------------------------------- */
int mfsr_squaredSum(const float* inTiles, float* outValues, int maxShift, int tileSize, int tileCount,
                    mfsr_stream_t stream); /* :119 */
int mfsr_boxFilterWithBorderX(const float* inTiles, float* outTiles, int maxShift, int tileSize, int tileCount,
                              mfsr_stream_t stream); /* :149 */
int mfsr_boxFilterWithBorderY(const float* inTiles, float* outTiles, int maxShift, int tileSize, int tileCount,
                              mfsr_stream_t stream); /* :186 */
int mfsr_normalizedCC(const float* ccImage, const float* squaredTemplate, const float* boxFilteredImage,
                      float* shiftImage, int maxShift, int tileSize, int tileCount, mfsr_stream_t stream); /* :227 */
int mfsr_convertToTilesOverlapBorder(const float* inImg, float* outTiles, int imgWidth, int imgHeight, int imgPitch,
                                     int maxShift, int tileSize, int tileCountX, int tileCountY, mfsr_float2 baseShift,
                                     float baseRotation, mfsr_stream_t stream); /* :265 */
int mfsr_convertToTilesOverlapPreShift(const float* inImg, float* outTiles, const mfsr_float2* preShift,
                                       int preShiftPitch, int imgWidth, int imgHeight, int imgPitch, int maxShift,
                                       int tileSize, int tileCountX, int tileCountY, mfsr_float2 baseShift,
                                       float baseRotation, mfsr_stream_t stream); /* :324 */
int mfsr_GammasRGB(mfsr_float3* inOutImg, int imgWidth, int imgHeight, int imgPitch, mfsr_stream_t stream); /* :393 */
int mfsr_ApplyWeighting(mfsr_float3* inOutImg, const mfsr_float3* finalImg, const mfsr_float3* weight, int imgWidth,
                        int imgHeight, int imgPitch, float threshold, mfsr_stream_t stream); /* :426 */
int mfsr_conjugateComplexMulKernel(const mfsr_float2* aIn, mfsr_float2* bInOut, int maxElem,
                                   mfsr_stream_t stream); /* :485 */
int mfsr_findMinimum(const float* shiftImage, mfsr_float2* coordinates, int coordinatesPitch, int maxShift,
                     int tileCount, int tileCountX, float threshold, mfsr_stream_t stream); /* :512 */
int mfsr_UpSampleShifts(const mfsr_float2* inShift, mfsr_float2* outShift, int inPitch, int outPitch, int oldLevel,
                        int newLevel, int oldCountX, int oldCountY, int newCountX, int newCountY, int oldTileSize,
                        int newTileSize, mfsr_stream_t stream); /* :642 */
int mfsr_ComputeStructureTensor(const float* imgDx, const float* imgDy, mfsr_float3* outImg, int imgWidth,
                                int imgHeight, int imgDxDyPitch, int imgOutPitch, mfsr_stream_t stream); /* :691 */
int mfsr_ComputeKernelParam(mfsr_float3* kernelImg, int imgWidth, int imgHeight, int imgOutPitch, float Dth, float Dtr,
                            float kDetail, float kDenoise, float kStretch, float kShrink,
                            mfsr_stream_t stream); /* :718 */
int mfsr_fourierFilter(mfsr_float2* img, size_t stride, int width, int height, float lp, float hp, float lps,
                       float hps, int clearAxis, mfsr_stream_t stream);                             /* :794 */
int mfsr_fftshift(mfsr_float2* fft, int width, int height, mfsr_stream_t stream); /* :873 */

/* ---- C: ShiftMinimizerKernels.cu ------------------------------------------ */
int mfsr_copyShiftMatrix(float* matrices, int tileCount, int imageCount, int shiftCount,
                         mfsr_stream_t stream); /* :29 */
int mfsr_setPointers(float** shiftMatrixArray, float** shiftMatrixSafeArray, float** matrixSquareArray,
                     float** matrixInvertedArray, float** solvedMatrixArray, mfsr_float2** shiftOneToOneArray,
                     mfsr_float2** shiftMeasuredArray, mfsr_float2** shiftOptimArray, float* shiftMatrices,
                     float* shiftSafeMatrices, float* matricesSquared, float* matricesInverted, float* solvedMatrices,
                     mfsr_float2* shiftsOneToOne, mfsr_float2* shiftsMeasured, mfsr_float2* shiftsOptim, int tileCount,
                     int imageCount, int shiftCount, mfsr_stream_t stream); /* :51 */
int mfsr_checkForOutliers(mfsr_float2* measuredShifts, const float* optimShiftsT, float* shiftMatrix, int* status,
                          int* inversionInfo, int tileCount, int imageCount, int shiftCount,
                          mfsr_stream_t stream); /* :81 */
int mfsr_transposeShifts(mfsr_float2* measuredShifts, const float* measuredShiftsT, const float* shiftsOneToOneT,
                         mfsr_float2* shiftsOneToOne, int tileCount, int imageCount, int shiftCount,
                         mfsr_stream_t stream); /* :143 */
int mfsr_getOptimalShifts(mfsr_float2* optimalShifts, const mfsr_float2* bestShifts, int imageCount, int tileCountX,
                          int tileCountY, int optimalShiftsPitch, int referenceImage, int imageToTrack,
                          mfsr_stream_t stream); /* :179 */
int mfsr_concatenateShifts(const mfsr_float2* const* shiftIn, int* shiftInPitch, mfsr_float2* shiftOut, int shiftCount,
                           int tileCountX, int tileCountY, mfsr_stream_t stream); /* :223 */
int mfsr_separateShifts(const mfsr_float2* shiftIn, mfsr_float2* const* shiftOut, int* shiftOutPitch, int shiftCount,
                        int tileCountX, int tileCountY, mfsr_stream_t stream); /* :242 */
/* C4: the batched least-squares solve the reference leaves to a missing host
 * (batched cuBLAS upstream): per tile d = (A^T A)^-1 A^T b, o = A d.  A is
 * column-major m x (imageCount-1) per tile; optimShiftsT is planar
 * [x(m) | y(m)] per tile (what checkForOutliers reads, :114-115);
 * inversionInfo = 0 or (index of the zero pivot)+1.  imageCount-1 <= 63. */
int mfsr_solveShiftsBatched(const float* shiftMatrix, const mfsr_float2* measuredShifts, mfsr_float2* shiftsOneToOne,
                            float* optimShiftsT, int* inversionInfo, int tileCount, int imageCount, int shiftCount,
                            mfsr_stream_t stream);

/* C driver: iterate solve -> checkForOutliers until every tile's status is -1
 * (at most shiftCount+1 rounds; synchronises the stream once per round to read
 * the status array back).  status / inversionInfo: device int[tileCount]. */
int mfsr_minimizeShifts(float* shiftMatrix, mfsr_float2* measuredShifts, mfsr_float2* shiftsOneToOne,
                        float* optimShiftsT, int* status, int* inversionInfo, int tileCount, int imageCount,
                        int shiftCount, int* roundsOut, mfsr_stream_t stream);

/* the same loop inside one launch (the tiles are independent: one wavefront per tile iterates solve -> checkForOutliers
 * until its tile converges): no host synchronisation, graph-capturable, bit-identical to mfsr_minimizeShifts */
int mfsr_minimizeShiftsFused(float* shiftMatrix, mfsr_float2* measuredShifts, mfsr_float2* shiftsOneToOne, float* optimShiftsT,
                             int* status, int* inversionInfo, int tileCount, int imageCount, int shiftCount,
                             mfsr_stream_t stream);

/* ---- D/E: opticalFlow.cu -------------------------------------------------- */
/* texUV: CLAMP; texToWarp: MIRROR */
int mfsr_WarpingKernel(int width, int height, int stride, mfsr_tex2d texUV, float* out, mfsr_tex2d texToWarp,
                       mfsr_stream_t stream); /* :28 */
/* texObjShiftXY: CLAMP, tileCountX x tileCountY texels */
int mfsr_CreateFlowFieldFromTiles(mfsr_float2* outImg, mfsr_tex2d texObjShiftXY, int tileSize, int tileCountX,
                                  int tileCountY, int imgWidth, int imgHeight, int imgPitch, mfsr_float2 baseShift,
                                  float baseRotation, mfsr_stream_t stream); /* :48 */
/* texSource/texTarget: MIRROR, width x height */
int mfsr_ComputeDerivativesKernel(int width, int height, int stride, float* Ix, float* Iy, float* Iz,
                                  mfsr_tex2d texSource, mfsr_tex2d texTarget, mfsr_stream_t stream); /* :97 */
int mfsr_ComputeDerivatives2Kernel(int width, int height, int stride, float* Ix, float* Iy, mfsr_tex2d tex,
                                   mfsr_stream_t stream); /* :151 */
/* the same for image rows [row0, row0 + rows) only (Ix, Iy are the full-size images) */
int mfsr_ComputeDerivatives2Rows(int width, int height, int stride, float* Ix, float* Iy, mfsr_tex2d tex, int row0, int rows,
                                 mfsr_stream_t stream);
int mfsr_lucasKanadeOptim(mfsr_float2* shifts, const float* imFx, const float* imFy, const float* imFt, int pitchShift,
                          int pitchImg, int width, int height, int halfWindowSize, float minDet,
                          mfsr_stream_t stream); /* :190 */

/* ---- F: RobustnessModell.cu ----------------------------------------------- */
/* texUV: CLAMP */
int mfsr_ComputeRobustnessMask(const mfsr_float3* rawImgRef, const mfsr_float3* rawImgMoved,
                               mfsr_float4* robustnessMask, mfsr_tex2d texUV, int imgWidth, int imgHeight, int imgPitch,
                               int maskPitch, float alpha, float beta, float thresholdM,
                               mfsr_stream_t stream); /* :29 */

/* ---- host helpers of the reference ---------------------------------------- */
/* gaussin_filter_1D, test_opencv/main.cpp:370-391; taps must hold 99 floats;
 * returns the tap count (host function, no device work). */
int mfsr_gaussin_filter_1D(float sigma, float* taps);
/* sharpenImg2, finalProject/Project/multi_frame_sr.cpp:90-119 on DEVICE u8
 * interleaved images (step in bytes); never-written pixels are 0. */
int mfsr_sharpenImg2(const uint8_t* img, uint8_t* result, int rows, int cols, int ch, int stepIn, int stepOut,
                     mfsr_stream_t stream);

/* sharpenImg, test_opencv/main.cpp:525-534: unsharp mask (sigma 1, threshold 5, amount 1) on DEVICE u8 interleaved
 * images; tmp: rows*cols*ch device bytes.  The Gaussian blur is third-party there (cv::GaussianBlur): restated from its
 * published definition, parity unpinned (oracle/glue.c). */
int mfsr_sharpenImg(const uint8_t* img, uint8_t* result, uint8_t* tmp, int rows, int cols, int ch, int stepIn, int stepOut,
                    mfsr_stream_t stream);

/* ---- glue stages between the reference kernels (the build's own; the
 *      reference has no host for this path -- DESIGN.md "Pipeline glue") ---- */
int mfsr_rgbToGray(const mfsr_float3* in, int inPitch, float* out, int outPitch, int width, int height,
                   mfsr_stream_t stream);
int mfsr_u16ToFloat(const uint16_t* in, float* out, int outPitch, int width, int height, float factor,
                    mfsr_stream_t stream);
/* separable filter, clamped borders, chan = 1 or 3, ntaps <= 99 (taps on HOST) */
int mfsr_separableFilter(const float* in, int inPitch, float* tmp, float* out, int outPitch, int width, int height,
                         int chan, const float* taps, int ntaps, mfsr_stream_t stream);
int mfsr_downsample2x(const float* in, int inPitch, float* out, int outPitch, int outW, int outH, mfsr_stream_t stream);
/* direct correlation replacing FFT -> conjugateComplexMulKernel -> IFFT; output
 * in the wrapped layout normalizedCC reads (kernel.cu:248-254) */
int mfsr_crossCorrelateTiles(const float* refTiles, const float* movedTiles, float* ccImage, int maxShift, int tileSize,
                             int tileCount, mfsr_stream_t stream);
int mfsr_addRoundedPreShift(const mfsr_float2* preShift, int prePitch, mfsr_float2* found, int foundPitch, int countX,
                            int countY, mfsr_stream_t stream);
int mfsr_scaleFlow(mfsr_float2* flow, int pitch, int width, int height, float factor, mfsr_stream_t stream);
int mfsr_float3ToFloat4(const mfsr_float3* in, int inPitch, mfsr_float4* out, int outPitch, int width, int height,
                        mfsr_stream_t stream);
int mfsr_resampleFloat3(const mfsr_float3* in, int inPitch, int inW, int inH, mfsr_float3* out, int outPitch, int outW,
                        int outH, float u0, float u1, float v0, float v1, mfsr_stream_t stream);
/* exactly one of out16/out8 non-NULL; dense interleaved RGB */
int mfsr_quantize(const mfsr_float3* in, int inPitch, uint16_t* out16, uint8_t* out8, int width, int height,
                  float maxOut, mfsr_stream_t stream);
int mfsr_fill_f32(float* dst, size_t count, float value, mfsr_stream_t stream);
/* deBayersSubSample3 (A1) + mfsr_rgbToGray + mfsr_separableFilter + the first mfsr_downsample2x in one
 * launch (what the burst driver does to every Bayer frame before tracking); bit-identical to the chain.
 * dimX x dimY is the half-resolution size; pyr1 may be NULL; ntaps odd, <= 17. */
int mfsr_prepareFrameFused(const uint16_t* dataIn, mfsr_float3* halfOut, int halfPitch, float maxVal, int dimX, int dimY,
                           float* pyr0, int pyr0Pitch, float* pyr1, int pyr1Pitch, const float* taps, int ntaps,
                           mfsr_stream_t stream);
/* one-pixel border ring of a float4 image := 0: what ComputeRobustnessMask (:37) leaves unwritten */
int mfsr_zeroRing_f32x4(mfsr_float4* img, int pitch, int width, int height, mfsr_stream_t stream);
/* variant selector of the accumulate kernels (tests, A/B benchmarks):
 * 0 = straight kernel, exp(-w/2) with the ocml expf (tight parity against the oracle);
 * 1 = straight kernel, v_exp_f32; 2 (default) = additionally the restructured x2
 * strip kernel where it applies (scale 2, Bayer/mono CFA, 16-byte aligned accumulators). */
int mfsr_set_accumulate_fast_exp(int enable);
/* the selector's value (process-wide: a test that changes it puts back what it found) */
int mfsr_get_accumulate_fast_exp(void);

/* ---- fused MI355X kernels (same results as the chains they replace, within
 *      the tolerances stated in DESIGN.md) --------------------------------- */
/* B1+B2+B3+B4+cc+B6+B7 in one launch, one workgroup per tile: gathers the
 * reference tile and the pre-shifted moved patch into LDS, evaluates the L2
 * distance image directly and reduces it with wavefront shuffles. */
int mfsr_trackTilesFused(const float* refImg, const float* movedImg, const mfsr_float2* preShift, int preShiftPitch,
                         mfsr_float2* coordinates, int coordinatesPitch, int imgWidth, int imgHeight, int imgPitch,
                         int maxShift, int tileSize, int tileCountX, int tileCountY, float threshold,
                         const float* refSquaredSums, mfsr_stream_t stream);
/* sum(ref^2) of every reference tile in the serial order of squaredSum (B3, kernel.cu:119): it does
 * not depend on the moved frame, so a burst takes it once per reference and hands it to
 * mfsr_trackTilesFused (refSquaredSums; NULL = taken inside the tracker). */
int mfsr_tileSquaredSums(const float* refImg, float* outValues, int imgWidth, int imgHeight, int imgPitch, int maxShift,
                         int tileSize, int tileCountX, int tileCountY, mfsr_stream_t stream);
/* ... of every tracker level in one launch (the kernel's time is one lane's chain of tileSize^2 dependent adds, which a
 * launch per level pays per level): levels <= 4; the arrays are host memory, one entry per level; refImgs[l] = level l's
 * image, outValues[l] = its tileCountX[l] * tileCountY[l] sums.  Bit-identical to mfsr_tileSquaredSums level by level. */
int mfsr_tileSquaredSumsLevels(int levels, const mfsr_tex2d* refImgs, float* const* outValues, const int* maxShift,
                               const int* tileSize, const int* tileCountX, const int* tileCountY, mfsr_stream_t stream);
/* D2+D3+D4 for one Lucas-Kanade iteration in one launch (LDS-tiled warp,
 * derivative and separable window sums).  Flow is double-buffered: shiftsOut
 * must not alias shiftsIn (tile halos read neighbouring tiles' flow).  outScale
 * multiplies the flow written (1 = plain iteration; the last iteration of a
 * pipeline passes its tracking->raw pixel factor instead of a mfsr_scaleFlow pass). */
int mfsr_lucasKanadeIterationFused(const mfsr_float2* shiftsIn, mfsr_float2* shiftsOut, int pitchShift,
                                   const float* refImg, const float* movedImg, int pitchImg, int width, int height,
                                   int halfWindowSize, float minDet, float outScale, mfsr_stream_t stream);
/* F1 (ComputeRobustnessMask, RobustnessModell.cu:29) + its zero ring (:48-49) in one launch: reference patch through an
 * LDS tile, hardware sqrt / rcp / exp (mask within 2e-6 of the straight kernel; the roundings and the M threshold keep
 * their exact arithmetic).  mfsr_set_robustness_fast(0) routes it to ring + mfsr_ComputeRobustnessMask. */
int mfsr_robustnessMaskFused(const mfsr_float3* rawImgRef, const mfsr_float3* rawImgMoved, mfsr_float4* robustnessMask,
                             mfsr_tex2d texUV, int imgWidth, int imgHeight, int imgPitch, int maskPitch, float alpha, float beta,
                             float thresholdM, mfsr_stream_t stream);
int mfsr_set_robustness_fast(int enable);
/* E1+E2 (derivatives + structure tensor) in one launch */
int mfsr_structureTensorFused(const float* img, int imgPitch, mfsr_float3* outImg, int outPitch, int width, int height,
                              mfsr_stream_t stream);
/* A2+A3 (+u16 -> float) in one launch through an LDS green tile */
int mfsr_deBayerFused(const uint16_t* raw, mfsr_float3* outImage, int strideOut, int width, int height,
                      mfsr_float3 blackPoint, mfsr_float3 scale, mfsr_stream_t stream);
/* ... which also stores zero in the 2-pixel ring of the image that A2 / A3 (and mfsr_deBayerFused) leave untouched: every
 * pixel of outImage (float3; its width and height are those of the dense raw image) is written, as a cleared image followed
 * by mfsr_deBayerFused holds it */
int mfsr_deBayerFusedRing(const uint16_t* raw, mfsr_tex2d outImage, mfsr_float3 blackPoint, mfsr_float3 scale,
                          mfsr_stream_t stream);
/* E1 + E2 + the separable smoothing of the tensor + E3 + the float4 packing in one launch: rows [row0, row0 + rows) of the
 * kernel-shape field (float4, .w = 0; `field` has the size of the tracking image `tex`) hold, bit for bit, what the
 * whole-image chain mfsr_ComputeDerivatives2Kernel -> mfsr_ComputeStructureTensor -> mfsr_separableFilter(chan = 3) ->
 * mfsr_ComputeKernelParam -> mfsr_float3ToFloat4 gives for them (mirror for the stencil and clamp for the smoothing at the
 * IMAGE border, whatever the window); other rows are not touched.  MFSR_E_UNSUPPORTED (nothing launched) for ntaps / 2 > 5
 * and for images smaller than one 64 x 16 tile. */
int mfsr_kernelParamField(mfsr_tex2d tex, mfsr_tex2d field, int row0, int rows, const float* taps, int ntaps, float Dth,
                          float Dtr, float kDetail, float kDenoise, float kStretch, float kShrink, mfsr_stream_t stream);
/* For tests: the number of workgroups of all mfsr_kernelParamField launches since the last reset that took their derivatives
 * from global memory instead of the LDS tile (same bits, slower; expected: 0 for every image size).  Synchronises with the
 * device; reset != 0 zeroes the count after reading it. */
int mfsr_kernelParamFieldFallbacks(int* count, int reset);
/* 1 (default): mfsr_burst_set_reference makes the reference's products with mfsr_kernelParamField,
 * mfsr_tileSquaredSumsLevels and mfsr_deBayerFusedRing (cfg.fused = 1); 0: with the kernel chain and a cleared fallback
 * image.  Same bits either way.  Process-wide, like mfsr_set_robustness_fast. */
int mfsr_set_reference_fused(int enable);
/* H1 (+fallback resample) + H2 + quantise in one launch */
int mfsr_finishFused(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgPitch, const mfsr_float3* fallback,
                     int fbPitch, int fbW, int fbH, float u0, float u1, float v0, float v1, mfsr_float3* outImg,
                     int outPitch, uint16_t* out16, int width, int height, float threshold, int applyGamma,
                     float maxOut, mfsr_stream_t stream);

/* ---- global pre-alignment.  The reference has the slot -- `class PreAlignment`,
 *      boxFilterNPP.cpp:102-166; baseShift / baseRotation of kernel.cu:265,324 and opticalFlow.cu:48 -- but no finished
 *      estimator (test_opencv/main.cpp:861-1194 returns nothing).  Model fixed by those kernels: reference pixel p maps
 *      to moved pixel q = c + R(rotation) * (p - c - shift), c = (width/2, height/2).  The estimator is the build's own
 *      (csrc/prealign.hip): exhaustive coarse-to-fine search on 2x2-mean pyramids, integer scores, angles on a 1/16
 *      degree grid; no host round trip, the result stays in device memory. ---------------------------------------- */
typedef struct {
    float shiftX, shiftY;   /* base shift in pixels of the image the pyramids were built from */
    float rotation;         /* base rotation in radians (= angleIndex * pi/2880) */
    float cosRotation, sinRotation; /* cosf/sinf(rotation) of the host's libm */
    int32_t angleIndex, tx, ty, level; /* raw search result: angle in 1/16 degree, shift at pyramid level `level` */
    int32_t reserved[3];
} mfsr_prealign;
/* device bytes of one image's search pyramid / of the search workspace (trig table, scores, per-level state) */
size_t mfsr_preAlign_pyramid_bytes(int width, int height);
size_t mfsr_preAlign_workspace_bytes(float maxAngleDeg);
/* uploads the trig table for |angle| <= maxAngleDeg into the workspace (once per workspace) */
int mfsr_preAlign_init(void* workspace, float maxAngleDeg, mfsr_stream_t stream);
/* 2x2-mean pyramid of img (float, pitched) down to a long side <= 64, quantised to 8 bit */
int mfsr_preAlignPyramid(const float* img, int width, int height, int pitch, void* pyramid, mfsr_stream_t stream);
/* search: *result (DEVICE memory) := base shift / rotation of the moved image against the reference image */
int mfsr_preAlign(const void* refPyramid, const void* movedPyramid, int width, int height, float maxAngleDeg,
                  void* workspace, mfsr_prealign* result, mfsr_stream_t stream);
int mfsr_preAlign_identity(mfsr_prealign* result, mfsr_stream_t stream);
/* mfsr_trackTilesFused with B2's baseShift / baseRotation taken from *base (device; NULL = none); the base shift is
 * multiplied by baseInvScale (1 / down-sampling factor of this pyramid level) */
int mfsr_trackTilesFusedBase(const float* refImg, const float* movedImg, const mfsr_float2* preShift, int preShiftPitch,
                             mfsr_float2* coordinates, int coordinatesPitch, int imgWidth, int imgHeight, int imgPitch,
                             int maxShift, int tileSize, int tileCountX, int tileCountY, float threshold,
                             const float* refSquaredSums, const mfsr_prealign* base, float baseInvScale,
                             mfsr_stream_t stream);
/* mfsr_trackTilesFusedBase with UpSampleShifts (B8, kernel.cu:642) folded in: every tile's pre-shift is taken inside the
 * kernel from the previous level's shifts (oldCountX x oldCountY tiles of oldTileSize at down-sampling factor oldLevel)
 * with B8's own arithmetic: same bits, one launch and one buffer less per pyramid level */
int mfsr_trackTilesFusedUp(const float* refImg, const float* movedImg, const mfsr_float2* coarseShifts, int coarsePitch,
                           int oldLevel, int newLevel, int oldCountX, int oldCountY, int oldTileSize, mfsr_float2* coordinates,
                           int coordinatesPitch, int imgWidth, int imgHeight, int imgPitch, int maxShift, int tileSize,
                           int tileCountX, int tileCountY, float threshold, const float* refSquaredSums,
                           const mfsr_prealign* base, float baseInvScale, mfsr_stream_t stream);
/* mfsr_CreateFlowFieldFromTiles (opticalFlow.cu:48) with baseShift / baseRotation taken from *base (device) */
int mfsr_CreateFlowFieldFromTilesBase(mfsr_float2* outImg, mfsr_tex2d texObjShiftXY, int imgWidth, int imgHeight,
                                      int imgPitch, const mfsr_prealign* base, mfsr_stream_t stream);
/* The same iteration with the warped moved image handed over between launches instead of re-gathered for every tile halo:
 * sumIn / diffIn = (warped + ref) / (warped - ref) of every pixel under shiftsIn (made by mfsr_CreateFlowFieldWarped or by
 * the previous call's sumOut / diffOut); sumOut / diffOut (both NULL on the last iteration) receive them under shiftsOut,
 * taken by the thread that has just updated the pixel.  Bit-identical to mfsr_lucasKanadeIterationFused. */
int mfsr_lucasKanadeIterationWarped(const mfsr_float2* shiftsIn, mfsr_float2* shiftsOut, int pitchShift, const float* refImg,
                                    const float* movedImg, int pitchImg, const float* sumIn, const float* diffIn, float* sumOut,
                                    float* diffOut, int pitchSD, int width, int height, int halfWindowSize, float minDet,
                                    float outScale, mfsr_stream_t stream);
/* ---- frame batches: the per-frame stages of the alignment for 1 .. 4 moved frames against one reference in ONE launch each
 * (gridDim.z = frame; the single-frame entry points launch the same kernels with a table of one frame, so a frame's result
 * does not depend on the batch it is in).  mfsr_burst_add_frame aligns the frames of a fuse group this way. */
typedef struct {
    const uint16_t* dataIn;
    mfsr_float3* halfOut;
    float* pyr0;
    float* pyr1; /* NULL for all frames: no second pyramid level */
} mfsr_prepare_frame;
int mfsr_prepareFrameFusedBatch(int nFrames, const mfsr_prepare_frame* frames, int halfPitch, float maxVal, int dimX, int dimY,
                                int pyr0Pitch, int pyr1Pitch, const float* taps, int ntaps, mfsr_stream_t stream);
typedef struct {
    const float* movedImg;
    const mfsr_float2* coarseShifts; /* this frame's shifts of the coarser level (mfsr_trackTilesFusedUp); NULL for all: none */
    mfsr_float2* coordinates;
    const mfsr_prealign* base; /* or NULL */
} mfsr_track_frame;
int mfsr_trackTilesFastSupported(int tileSize, int maxShift); /* 1: mfsr_trackTilesFusedBatch takes this (tile size, search range) */
int mfsr_trackTilesFusedBatch(int nFrames, const mfsr_track_frame* frames, const float* refImg, int coarsePitch, int oldLevel,
                              int newLevel, int oldCountX, int oldCountY, int oldTileSize, int coordinatesPitch, int imgWidth,
                              int imgHeight, int imgPitch, int maxShift, int tileSize, int tileCountX, int tileCountY, float threshold,
                              const float* refSquaredSums, float baseInvScale, mfsr_stream_t stream);
typedef struct {
    mfsr_float2* outImg;
    const mfsr_float2* tileShifts;
    const mfsr_prealign* base; /* NULL for all frames, or set for all */
    const float* movedImg;
    float* sumOut;
    float* diffOut;
} mfsr_flowfield_frame;
int mfsr_CreateFlowFieldWarpedBatch(int nFrames, const mfsr_flowfield_frame* frames, int tilePitch, int tileCountX, int tileCountY,
                                    int imgWidth, int imgHeight, int imgPitch, const float* refImg, int pitchImg, int pitchSD,
                                    mfsr_stream_t stream);
typedef struct {
    const mfsr_float3* movedHalf;
    mfsr_float4* mask;
    const mfsr_float2* flow;
} mfsr_robustness_frame;
int mfsr_robustnessMaskFusedBatch(int nFrames, const mfsr_robustness_frame* frames, const mfsr_float3* rawImgRef, int flowPitch,
                                  int flowWidth, int flowHeight, int imgWidth, int imgHeight, int imgPitch, int maskPitch, float alpha,
                                  float beta, float thresholdM, mfsr_stream_t stream);
/* ---- the robustness masks of a group in one pass over the reference (csrc/robustness.hip, k_robustnessGroup) ----
 * mfsr_prepareFrameFusedBatch whose halfOut receives, instead of the half-resolution pixel, that pixel's 3 x 3 patch mean as
 * the robustness mask forms it: per channel div9(sum of half(clamp(x + dx), clamp(y + dy))), summed from 0.0f row-major, the
 * division exact.  Both pyramid outputs are bit-identical to mfsr_prepareFrameFusedBatch.  meansRowBytes >= 12 * w.
 * MFSR_E_UNSUPPORTED (nothing launched) for ntaps < 3 (the tile has no halo) and for ntaps / 2 > 8. */
int mfsr_prepareFrameMeansBatch(int nFrames, const mfsr_prepare_frame* frames, int meansRowBytes, float maxVal, int w, int h,
                                int pyr0RowBytes, int pyr1RowBytes, const float* taps, int ntaps, mfsr_stream_t stream);
/* The masks of 1 .. 4 moved frames against one reference, bit-identical to mfsr_robustnessMaskFusedBatch: what depends on the
 * reference alone is computed once per pixel and kept across the frames, and a frame's moved side is one gather from its
 * patch-mean image (movedMeans: mfsr_prepareFrameMeansBatch).  Where the displaced position leaves the image the nine
 * individually clamped pixels are rebuilt from the frame's dense raw samples (movedRaw: 2 * w samples per row, 2 * h rows;
 * maxVal and the CFA pattern as given to the prepare call).  Every flow field has the image's resolution (w x h texels of
 * flowRowBytes rows).  MFSR_E_UNSUPPORTED (nothing launched) after mfsr_set_robustness_fast(0). */
typedef struct {
    const mfsr_float3* movedMeans;
    const uint16_t* movedRaw;
    mfsr_float4* mask;
    const mfsr_float2* flow;
} mfsr_robustness_group_frame;
int mfsr_robustnessMaskGroup(int nFrames, const mfsr_robustness_group_frame* frames, const mfsr_float3* refHalf, int refRowBytes,
                             int flowRowBytes, int meansRowBytes, int maskRowBytes, int w, int h, float maxVal, float alpha,
                             float beta, float thresholdM, mfsr_stream_t stream);
/* process-wide switch for A/B (default 1; MFSR_ROBUST_GROUP=0 in the environment): 1 = the burst driver makes the masks of an
 * aligned group with the two calls above, 0 = with mfsr_prepareFrameFusedBatch + mfsr_robustnessMaskFusedBatch.  Same bits. */
int mfsr_set_robustness_group(int enable);
/* The iteration of mfsr_lucasKanadeIterationWarped for 1 .. 4 frames against one reference in ONE launch (csrc/lk_fused.hip,
 * k_lkSweep: one wavefront per 64 columns sweeping down a band of rows, vertical state in registers, horizontal window sums
 * through whole-wave DPP shifts, no LDS).  Agrees with mfsr_lucasKanadeIterationWarped to fp32 rounding (another
 * summation order of the row sums).  MFSR_E_UNSUPPORTED (nothing launched) for half windows outside 1..7 or width < 64:
 * call the per-frame entry point then. */
typedef struct {
    const mfsr_float2* shiftsIn;
    mfsr_float2* shiftsOut;
    const float* movedImg;
    const float* sumIn;
    const float* diffIn;
    float* sumOut;  /* NULL (with diffOut) on the last iteration */
    float* diffOut;
} mfsr_lk_frame;
int mfsr_lucasKanadeSweepBatch(int nFrames, const mfsr_lk_frame* frames, const float* refImg, int pitchShift, int pitchImg,
                               int pitchSD, int width, int height, int halfWindowSize, float minDet, float outScale,
                               mfsr_stream_t stream);
/* The band height, in rows, that mfsr_lucasKanadeSweepBatch gives each wavefront at this geometry (the launcher calls this very
 * function; MFSR_LK_BAND=rows in the environment, >= 8, overrides the rule), or 0 where that entry point refuses the geometry
 * (half window outside 1..7, width < 64, height < 2 (halfWindowSize + 2), nFrames outside 1..4).  Host arithmetic, no GPU call.
 * A pixel's flow and warped planes do not depend on the band it falls in: bit-identical at every band height. */
int mfsr_lucasKanadeSweepBand(int width, int height, int halfWindowSize, int nFrames);
/* D1 (mfsr_CreateFlowFieldFromTiles; base != NULL: mfsr_CreateFlowFieldFromTilesBase) + the warp of every pixel under the flow
 * it writes: outImg and the first iteration's sumIn / diffIn in one launch (opticalFlow.cu:48 + :28) */
int mfsr_CreateFlowFieldWarped(mfsr_float2* outImg, mfsr_tex2d texObjShiftXY, int imgWidth, int imgHeight, int imgPitch,
                               mfsr_float2 baseShift, float baseRotation, const mfsr_prealign* base, const float* refImg,
                               const float* movedImg, int pitchImg, float* sumOut, float* diffOut, int pitchSD,
                               mfsr_stream_t stream);

/* mfsr_finishFused on rows [rowOffset, rowOffset + height) of a fullHeight-row image (pointers = first row of the stripe;
 * u/v window = that of the WHOLE image): bit-identical to the rows of the whole-image call */
int mfsr_finishFusedRows(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgPitch, const mfsr_float3* fallback,
                         int fbPitch, int fbW, int fbH, float u0, float u1, float v0, float v1, mfsr_float3* outImg,
                         int outPitch, uint16_t* out16, int width, int height, float threshold, int applyGamma, float maxOut,
                         int rowOffset, int fullHeight, mfsr_stream_t stream);
/* mfsr_finishFused on the window [colOffset, colOffset + width) x [rowOffset, rowOffset + height) of a fullWidth x fullHeight
 * image (pointers = the window's first pixel; u/v window = that of the WHOLE image): bit-identical to that rectangle of the
 * whole-image call */
int mfsr_finishFusedWindow(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgPitch, const mfsr_float3* fallback,
                           int fbPitch, int fbW, int fbH, float u0, float u1, float v0, float v1, mfsr_float3* outImg,
                           int outPitch, uint16_t* out16, int width, int height, float threshold, int applyGamma, float maxOut,
                           int colOffset, int rowOffset, int fullWidth, int fullHeight, mfsr_stream_t stream);

/* ---- burst pipeline (the L3 driver the reference lacks; mirrors the CLI
 *      contract of finalProject/Project/multi_frame_sr.cpp:122-210) ---------- */
typedef struct {
    int32_t width, height;   /* raw / LR frame size (even) */
    int32_t frames;          /* N */
    int32_t reference;       /* index of the reference frame */
    int32_t scale;           /* output scale s (1..8) */
    int32_t mono;            /* 0: Bayer mosaic per cfa; 1: monochrome (config 1) */
    int32_t cfa[4];          /* CFA pattern (ignored when mono) */
    float black[3], white[3]; /* per-channel levels: norm = (raw - black)/white */
    float maxVal;            /* deBayersSubSample3's maxVal */
    /* tile tracker */
    int32_t levels;          /* pyramid levels (1..4), coarsest first */
    int32_t levelFactor[4];  /* down-sampling factor per level (power of two) */
    int32_t tileSize[4];
    int32_t maxShift[4];
    float minimumThreshold;  /* findMinimum threshold */
    float sigmaTracking;     /* gaussin_filter_1D sigma of the tracking prefilter (main.cpp:1868) */
    /* Lucas-Kanade refinement */
    int32_t lkIterations;
    int32_t lkHalfWindow;
    float lkMinDet;
    /* robustness */
    float alpha, beta, thresholdM;
    /* kernel shape */
    float sigmaTensor;
    float Dth, Dtr, kDetail, kDenoise, kStretch, kShrink;
    /* finish */
    float weightThreshold;
    int32_t applyGamma;
    int32_t fused;           /* 1: fused MI355X kernels; 0: one launch per reference kernel */
    int32_t pairFrames;      /* frames per warp+fuse launch of add_frame (see mfsr_burst_add_frame): 0 = one, like the
                                reference; 1 (default) = as many as one launch takes (MFSR_MAX_FUSE_GROUP at scale 2 and 4 Bayer, else 2);
                                2 .. MFSR_MAX_FUSE_GROUP = that many */
    int32_t asyncFuse;       /* 1: the warp+fuse launches run on a stream owned by the burst, beside the alignment of the
                                following frames on the caller's stream (see mfsr_burst_add_frame); 0 (default since round 4:
                                the four-workgroup fuse kernel leaves no room on a CU for the alignment to run beside it, so
                                one stream is 1 % faster): everything on the caller's stream.  Same bits either way. */
    int32_t preAlign;        /* 1: estimate a global base shift + rotation per moved frame (mfsr_preAlign) and feed it to
                                the tile tracker and the flow field (baseShift / baseRotation of kernel.cu:324, opticalFlow.cu:48) */
    float preAlignMaxAngle;  /* search range of the base rotation in degrees (default 20) */
    int32_t uploadRing;      /* > 0: the workspace holds this many device raw-frame slots (>= 3) + 2 reference slots and the
                                burst owns a copy stream: mfsr_burst_*_host take frames from (pinned) HOST memory and upload
                                them ahead of the compute (BASELINE configs[4]: double-buffered H2D) */
    int32_t maskErode;       /* 0 (default): off; 1, 2: radius of the erosion of every moved frame's certainty mask between
                                stage F and stage G (mfsr_erodeMaskBatch; ghost suppression) */
    int32_t rawPacking;      /* 0 (default, MFSR_PACK_NONE): the host frames of mfsr_burst_*_host are uint16_t samples; MFSR_PACK_*:
                                they are packed 10 / 12-bit rows (mfsr_unpackRaw), uploaded packed into one staging slot per upload
                                slot and unpacked on the device.  Needs uploadRing > 0 and the packing's width rule (the last of
                                the reserved ints: sizeof and every other offset are unchanged) */
} mfsr_config;

typedef struct mfsr_burst mfsr_burst;

/* fill *cfg with the build's defaults for a width x height x frames burst */
int mfsr_config_default(mfsr_config* cfg, int width, int height, int frames, int scale, int mono);
/* device scratch the pipeline needs for cfg (bytes) */
size_t mfsr_burst_workspace_bytes(const mfsr_config* cfg);
/* bytes of ONE accumulator plane-set (imgOut or totalWeights): float3, pitch = 12*scale*width */
size_t mfsr_burst_accumulator_bytes(const mfsr_config* cfg);
int mfsr_burst_create(mfsr_burst** out, const mfsr_config* cfg, void* workspace, size_t workspaceBytes);
void mfsr_burst_destroy(mfsr_burst* b);

/* ---- zoom windows: super-resolve the HR rectangle [x0, x0+w) x [y0, y0+h) of the (scale*width) x (scale*height) grid only.
 * The windowed burst's accumulators, float image and u16 image are bit for bit that rectangle cut from the whole-frame burst
 * (same config, frames and calls); its buffers are dense window-sized images: accumulators and outImg pitch 12*w bytes,
 * out16 w*h*3.  The alignment stays whole-frame.  Constraints: x0, y0 multiples of 16; w, h multiples of 16 or reaching
 * the right / bottom edge; inside the frame, not empty; x0 = y0 = w = h = 0 = the whole frame (the default).
 * mfsr_window_check: host arithmetic only (no device call): MFSR_OK, MFSR_E_INVALID, MFSR_E_UNSUPPORTED (cfg->fused == 0). */
int mfsr_window_check(const mfsr_config* cfg, int x0, int y0, int w, int h);
/* between bursts only (MFSR_E_INVALID while frames are pending); takes effect from the next set_reference* on: add_frame,
 * begin, flush, finish, the *_host calls, process_source and process_joint then work on window-sized buffers.  A window
 * needs cfg.fused = 1 (MFSR_E_UNSUPPORTED otherwise). */
int mfsr_burst_set_window(mfsr_burst* b, int x0, int y0, int w, int h);
/* the window in effect (the whole frame: 0, 0, scale*width, scale*height) */
int mfsr_burst_get_window(const mfsr_burst* b, int* x0, int* y0, int* w, int* h);
/* Prepare the reference frame (tracking pyramid, half-res RGB, kernel
 * parameters, fallback image).  rawRef: dense u16 width x height on device. */
int mfsr_burst_set_reference(mfsr_burst* b, const uint16_t* rawRef, mfsr_stream_t stream);
/* mfsr_burst_set_reference for a burst whose fuse and finish touch HR rows [hrRow0, hrRow1) only (a stripe of a multi-GPU
 * burst): the products the alignment reads (half-resolution RGB, tracking pyramid, tile sums) are complete, the kernel
 * parameters and the debayered fallback image are made for the rows that stripe's mfsr_burst_fuse_rows /
 * mfsr_burst_finish_rows read -- bit-identical there to mfsr_burst_set_reference's, undefined elsewhere. */
int mfsr_burst_set_reference_rows(mfsr_burst* b, const uint16_t* rawRef, int hrRow0, int hrRow1, mfsr_stream_t stream);
/* Align + robustness + accumulate ONE frame into the caller's accumulators
 * (float3 HR, pitch 12*scale*width; zeroed by the caller before the first
 * call).  isReference != 0: identity flow, certainty 1.
 * With cfg.pairFrames the warp+fuse of a frame is deferred until its group (2 .. MFSR_MAX_FUSE_GROUP frames,
 * mfsr_burst_group_size) is aligned and the whole group is fused in one pass over the accumulators (a fraction of the
 * accumulator traffic, and everything that depends on the reference only -- kernel parameters, tap weights -- once
 * per pixel): between groups up to group - 1 frames are still waiting -- their raw buffers must stay untouched and
 * the accumulators do not contain them -- until the next add_frame, mfsr_burst_flush, finish or finish_rows has been
 * issued on the stream.  With mfsr_burst_hold_fuse(b, 1) whole groups wait as well, until flush / finish (see there).
 * With cfg.asyncFuse the warp+fuse launches go to a high-priority stream the burst owns (ordered by
 * events after the alignment on the caller's stream), so the fuse of frames k, k+1 overlaps the
 * alignment of k+2, k+3.  The caller's stream sees the accumulators complete only after
 * mfsr_burst_flush / finish / finish_rows / set_reference (they join the two streams), and every raw
 * buffer handed to add_frame must stay untouched until one of those has been issued. */
int mfsr_burst_add_frame(mfsr_burst* b, const uint16_t* raw, int isReference, mfsr_float3* imgOut,
                         mfsr_float3* totalWeights, mfsr_stream_t stream);
/* Start a new burst on these accumulators WITHOUT zeroing them: the first warp+fuse launch that follows
 * overwrites them (as if zeroed), which saves the memset and the first read of both planes.  If no frame
 * is added before flush / finish, they are zeroed then.  Without this call the caller zeroes them. */
int mfsr_burst_begin(mfsr_burst* b, mfsr_float3* imgOut, mfsr_float3* totalWeights, mfsr_stream_t stream);
/* fuse the frames that are still waiting -- for the rest of their group, or, with the burst hold, for the burst launch -- and
 * make the caller's stream wait for every fuse issued so far */
int mfsr_burst_flush(mfsr_burst* b, mfsr_stream_t stream);
/* Burst hold (opt-in per context, off by default).  enable != 0: a complete group is still ALIGNED when its last frame
 * arrives, but its warp+fuse is HELD and leaves together with the burst's other complete groups as ONE launch
 * (mfsr_accumulateSuperResBurst: the accumulators are read and written once per burst instead of once per group) at
 * mfsr_burst_flush / finish / finish_rows / set_reference, or when the next frame needs a held frame's ring slot (the ring
 * has max(8, min(cfg.frames, 16)) slots).  A remainder of 1 .. 3 frames follows as an ordinary launch; fewer than two held
 * groups take the ordinary launches, so bursts of at most 7 frames behave exactly as without the hold.  Results are bit for
 * bit those of the group-by-group launches.
 * THE CONTRACT IT CHANGES: the raw buffers of ALL frames added since the last flush / finish must stay untouched, and the
 * accumulators are incomplete, until flush / finish / finish_rows / set_reference has been issued (without the hold: until
 * the next add_frame).  Every library call that reads the accumulators or takes ring slots flushes the hold itself.
 * Only the plain resident path is held: whole-frame x2 Bayer bursts on the caller's stream.  cfg.asyncFuse, zoom windows,
 * host bursts (add_frame_host), mfsr_burst_fuse_rows, streams and the joint mode are unchanged. */
int mfsr_burst_hold_fuse(mfsr_burst* b, int enable);
/* burst launches since mfsr_burst_begin and the four-frame groups they fused (host-side counters; not an mfsr_path counter:
 * a burst launch needs eight frames) */
int mfsr_burst_fuse_stats(const mfsr_burst* b, int* burstLaunches, int* groupsFused);
/* process-wide switch of the burst hold for A/B (default 1; MFSR_BURST_FUSE=0 in the environment): 0 = every context fuses
 * group by group whatever mfsr_burst_hold_fuse said */
int mfsr_set_burst_fuse(int enable);
/* process-wide switch of the x2 margin kernels' body for A/B (default 1; MFSR_MARGIN_SITES=0 in the environment): 1 = raw
 * samples and certainty texels once per site (3 x 3 sites, 2 x 2 texels), tap weights once per pixel and workgroup; 0 = the
 * per-tap body (25 loads of each).  Both give the same accumulators bit for bit. */
int mfsr_set_margin_sites(int enable);
/* process-wide switch of the finish inside the burst launch for A/B (default 1; MFSR_FINISH_FUSE=0 in the environment):
 * 0 = mfsr_burst_finish always runs its finish pass.  Both give the same image bit for bit. */
int mfsr_set_finish_fuse(int enable);
/* *finishes = the finishes this burst has taken inside its burst launch (mfsr_accumulateSuperResBurstFinish) since
 * mfsr_burst_begin: host-side counter */
int mfsr_burst_debug_finish_fused(const mfsr_burst* b, int* finishes);
/* ApplyWeighting (+fallback) + optional gamma; outImg float3 HR (may be NULL),
 * out16 dense interleaved u16 HR (may be NULL).  Fuses whatever is still waiting first (mfsr_burst_flush), the groups of
 * the burst hold included.  Where the burst hold's launch is the burst's last fuse (8, 12 or 16 held frames and nothing
 * after them) and the call asks for the plain whole-frame uint16_t image only (out16 without outImg, no gamma, render,
 * sharpen, denoise or window), that launch writes out16 itself and no finish pass runs; the accumulators are written as
 * ever.  With timing on, the events around that launch then include the finish. */
int mfsr_burst_finish(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights, mfsr_float3* outImg,
                      uint16_t* out16, mfsr_stream_t stream);
/* finish restricted to HR rows [row0, row0+rows) (pointers are those of the
 * full images): each rank of a reduce-scattered burst normalises its stripe.
 * Fused kernels only. */
int mfsr_burst_finish_rows(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights,
                           mfsr_float3* outImg, uint16_t* out16, int row0, int rows, mfsr_stream_t stream);
/* ---- bursts whose frames live in HOST memory (cfg.uploadRing > 0).  Same semantics as set_reference / add_frame /
 * finish, with the H2D copy of every frame enqueued by the library on a copy stream it owns, into a ring of device
 * slots inside the workspace, so that the upload of frame k+1.. overlaps the align+fuse of frame k (the reference
 * uploads its frames one blocking copy at a time, multi_frame_sr.cpp:167-174).  hostRaw must stay valid and unchanged
 * until the stream has passed the call's work; pinned memory (hipHostMalloc) is what makes the copies asynchronous.
 * add_frame_host(isReference) with the pointer last given to set_reference_host re-uses the uploaded reference.
 * A host frame is `height` rows, mfsr_burst_set_host_row_bytes apart (default: dense).  With cfg.rawPacking != 0 the host
 * pointers of set_reference_host / add_frame_host / prefetch_host mean PACKED BYTES in the layout of that packing (rows of
 * mfsr_packed_row_bytes(cfg.rawPacking, width) bytes; the declarations keep their uint16_t type, cast the pointer): the
 * library uploads the packed bytes and unpacks them on the device (mfsr_unpackRaw) before the first kernel that reads the
 * frame; the result is bit for bit that of the burst of the unpacked samples.  Bytes of a row beyond the dense row size
 * (line padding) do not cross the link. */
int mfsr_burst_set_reference_host(mfsr_burst* b, const uint16_t* hostRaw, mfsr_stream_t stream);
int mfsr_burst_add_frame_host(mfsr_burst* b, const uint16_t* hostRaw, int isReference, mfsr_float3* imgOut,
                              mfsr_float3* totalWeights, mfsr_stream_t stream);
/* Optional: enqueue the uploads of the next nFrames frames (in the order they will be handed to add_frame_host) right
 * away, before any of their kernels.  add_frame_host enqueues a frame's ~10 alignment launches after its copy, so the NEXT
 * frame's copy reaches the copy engine only when the host is through with those -- 16 us between copies most of the time,
 * 70-300 us at group boundaries (one burst at 4K x 16: the uploads end at 5.7 instead of 5.0 ms).  With the copies queued up
 * front the engine runs them back to back and every add_frame_host finds its frame already on its way (matched by the
 * host pointer; a frame that was not announced is uploaded as before).  At most cfg.uploadRing frames are taken, the
 * pointer of the current host reference is skipped; call it after set_reference_host. */
int mfsr_burst_prefetch_host(mfsr_burst* b, const uint16_t* const* hostRaws, int nFrames, mfsr_stream_t stream);
/* mfsr_burst_finish into out16Dev (device), then its D2H copy into out16Host on a stream the burst owns, so that the next
 * burst's uploads and kernels overlap the download (full-duplex PCIe).  out16Host is complete after
 * mfsr_burst_host_sync(b) (blocks the HOST on the download); out16Dev must not be written by the caller before that.
 * A host burst (set_reference_host .. finish_host, packed or not) may be captured into a graph on `stream`: the uploads, the
 * unpack and the download become nodes of it, finish_host joins the download back into `stream` (the image is in out16Host when
 * a replay has completed; host_sync has nothing to wait for), and the host buffers are the graph's inputs and output.  Call
 * mfsr_burst_host_sync and synchronise `stream` before the capture, and before a replay that follows eager host bursts of the
 * same handle: a graph cannot wait for their copies. */
int mfsr_burst_finish_host(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights, uint16_t* out16Dev,
                           uint16_t* out16Host, mfsr_stream_t stream);
int mfsr_burst_host_sync(mfsr_burst* b);
/* Row stride in bytes of the host frames of the following mfsr_burst_*_host calls; 0 = dense (the default).  The dense row is
 * 2*width bytes of uint16_t samples, or mfsr_packed_row_bytes(cfg.rawPacking, width) of packed bytes; a larger stride is a host
 * frame with padded lines (the padding is not uploaded).  Between bursts only: MFSR_E_INVALID while frames are pending, for a
 * stride below the dense row size, for an odd stride of uint16_t rows, for a burst without an upload ring, and for a non-dense
 * stride when the environment asks for 1-D uploads (MFSR_UPLOAD_1D=1).  Host arithmetic only, no device call. */
int mfsr_burst_set_host_row_bytes(mfsr_burst* b, int rowBytes);
/* ---- building blocks of stripe-sharded bursts (multi-GPU, include/mfsr_dist.h): a frame is ALIGNED on the rank that
 * holds it (flow field + certainty mask into caller buffers, no accumulation), the ranks exchange the rows of raw / flow /
 * mask their stripes need, and every rank FUSES all frames, in frame order, onto its own stripe of HR rows -- the
 * summation order of the single-GPU burst, so the result is bit-identical to it. */
/* flow field: float2 flowW x flowH (tracking resolution, raw-pixel units); certainty mask: float4 maskW x maskH */
int mfsr_burst_field_dims(const mfsr_burst* b, int* flowW, int* flowH, int* maskW, int* maskH);
/* stages A1, (I), B, D, F of mfsr_burst_add_frame without G; results copied to flowOut / maskOut (byte pitches) */
int mfsr_burst_align_frame(mfsr_burst* b, const uint16_t* raw, int isReference, mfsr_float2* flowOut, int flowPitch,
                           mfsr_float4* maskOut, int maskPitch, mfsr_stream_t stream);
/* frames per warp+fuse launch cfg.pairFrames stands for with this configuration (1 .. MFSR_MAX_FUSE_GROUP) */
/* mfsr_burst_align_frame for nFrames frames (isReference: per-frame flags or NULL): groups of up to mfsr_burst_group_size
 * frames share their launches (one per stage and Lucas-Kanade iteration); same results as frame by frame */
int mfsr_burst_align_frames(mfsr_burst* b, int nFrames, const uint16_t* const* raws, const int* isReference,
                            mfsr_float2* const* flowOut, int flowPitch, mfsr_float4* const* maskOut, int maskPitch,
                            mfsr_stream_t stream);
int mfsr_burst_group_size(const mfsr_config* cfg);
/* stage G for 1 .. MFSR_MAX_FUSE_GROUP aligned frames on HR rows [rowBegin, rowEnd) (see mfsr_accumulateSuperResFullRows), with the kernel
 * parameters of the burst's reference */
int mfsr_burst_fuse_rows(mfsr_burst* b, int nFrames, const uint16_t* const* raws, const mfsr_float2* const* flows, int flowPitch,
                         const mfsr_float4* const* masks, int maskPitch, mfsr_float3* imgOut, mfsr_float3* totalWeights,
                         int accumulatorsUndefined, int rowBegin, int rowEnd, mfsr_stream_t stream);

/* rows rank `rank` of `worldSize` owns and reads (host arithmetic only): HR rows [rowBegin, rowEnd) (multiples of 16), and
 * of every frame's products the flow rows, certainty rows and raw rows its fuse can touch as long as the vertical flow
 * stays within maxFlowY raw pixels (rawHalo - 3); mfsr_checkFlowBound verifies that on the device. */
typedef struct {
    int32_t rowBegin, rowEnd;
    int32_t flowRow0, flowRows;
    int32_t maskRow0, maskRows;
    int32_t rawRow0, rawRows;
    float maxFlowY;
    int32_t reserved[3];
} mfsr_stripe_plan;
int mfsr_dist_stripe_plan(const mfsr_config* cfg, int worldSize, int rank, int rawHalo, mfsr_stripe_plan* out);
/* *flag |= 1 (device int) if any |flow.y| of the `rows` flow rows starting at `flow` exceeds bound (NaN passes: it
 * rounds to a zero shift) */
int mfsr_checkFlowBound(const mfsr_float2* flow, int pitch, int width, int rows, float bound, int* flag, mfsr_stream_t stream);
/* *maxBits = max(*maxBits, bit pattern of |flow.y|) over the rows (device int, zero it first; non-negative floats order
 * like their bit patterns; NaN is skipped): the measured vertical flow a multi-GPU caller sizes the raw-row halo of the
 * next bursts from (mfsr_dist_measured_flow) */
int mfsr_maxAbsFlowY(const mfsr_float2* flow, int pitch, int width, int rows, int* maxBits, mfsr_stream_t stream);
/* Host-only diagnostic (no device call): 1 if the kernels divide by `d` -- an image dimension, the divisor of the reference's
 * normalised texture coordinates (opticalFlow.cu:38-39, :88; RobustnessModell.cu:59-77) -- with the reciprocal sequence
 * q = x (1/d), q' = fma(fma(-d, q, x), 1/d, q), which this library takes only after checking on the host, over all 2^23
 * significands, that it IS the correctly rounded x / d for every x; 0 if they keep the division (check failed, d outside
 * (0, 2^24), or MFSR_EXACT_DIV=0). */
int mfsr_exactDivisionOk(float d);

/* ---- frame streams (BASELINE configs[4]): a sliding window of 2*radius+1 frames around every
 * frame, the reference's setTemporalAreaRadius(1) (finalProject/Project/multi_frame_sr.cpp:182).  Output t fuses frames
 * [t-radius, t+radius] (clipped to the stream) with frame t as the reference -- exactly what one mfsr_burst_* burst per
 * window gives -- but every frame is uploaded and PREPARED once (A1 half-resolution RGB, tracking pyramid, pre-alignment
 * search pyramid), not once per window it takes part in.  cfg->frames is ignored.  framesInHostMemory: frames are
 * (pinned) host pointers, uploaded on a copy stream the context owns, ahead of the compute. */
typedef struct mfsr_stream mfsr_stream;
size_t mfsr_stream_workspace_bytes(const mfsr_config* cfg, int radius);
int mfsr_stream_create(mfsr_stream** out, const mfsr_config* cfg, int radius, int framesInHostMemory, void* workspace,
                       size_t workspaceBytes);
void mfsr_stream_destroy(mfsr_stream* s);
/* hand over frame t = 0, 1, 2, ... (copied: the caller may reuse its buffer once the stream has passed the call).  From
 * t = radius on each call also produces output t - radius into outImg (float3 HR, may be NULL) / out16 (u16 HR, may be
 * NULL) and sets *produced to its index; before that *produced = -1. */
int mfsr_stream_push(mfsr_stream* s, const uint16_t* frame, mfsr_float3* outImg, uint16_t* out16, long long* produced,
                     mfsr_stream_t stream);
/* end of the stream: each call produces the next outstanding output (windows clipped at the last frame); *produced = -1
 * when none is left */
int mfsr_stream_drain(mfsr_stream* s, mfsr_float3* outImg, uint16_t* out16, long long* produced, mfsr_stream_t stream);
int mfsr_stream_reset(mfsr_stream* s);
/* every output of the stream is the window (see mfsr_burst_set_window): before the first push or after mfsr_stream_reset.  The
 * workspace is sized for the whole frame, so any window fits. */
int mfsr_stream_set_window(mfsr_stream* s, int x0, int y0, int w, int h);

/* ---- whole burst with the JOINT SHIFT MINIMISER (stage C; ShiftMinimizerKernels.cu:81-258) in the loop.  Besides every
 * (reference, k) pair the tracker measures every neighbouring pair (k, k+1); per tile the frame-to-frame shifts are the
 * least-squares solution of all measurements with the worst outlier dropped until every residual is below 1 px^2, and
 * the reference->k shifts (getOptimalShifts) replace the tracker's in the per-frame chain.  frames: cfg.frames device
 * pointers; jointWorkspace: mfsr_burst_joint_workspace_bytes(cfg) device bytes; accumulators as for add_frame (a
 * mfsr_burst_begin is issued inside); finish with mfsr_burst_finish.  Needs cfg.fused = 1, cfg.preAlign = 0. */
size_t mfsr_burst_joint_workspace_bytes(const mfsr_config* cfg);
int mfsr_burst_process_joint(mfsr_burst* b, const uint16_t* const* frames, void* jointWorkspace, size_t jointBytes,
                             mfsr_float3* imgOut, mfsr_float3* totalWeights, mfsr_stream_t stream);

/* ---- frame-source plug-in: the pull model of the reference's cv::superres::FrameSource subclass
 * (MultiFrameSource_CUDA, finalProject/Project/multi_frame_sr.cpp:18-49: nextFrame copies the next device-resident frame
 * into the caller's buffer and leaves it empty when exhausted; reset rewinds).  Same ownership: the library owns the
 * destination (a slot of the burst's upload ring, cfg.uploadRing >= 3), the callee fills it. */
typedef struct {
    /* copy the next frame (dense u16, width x height) into dst (DEVICE memory) with work enqueued on `stream`;
     * return 1 = delivered, 0 = source exhausted, < 0 = error (returned to the caller of process_source) */
    int (*next_frame)(void* user, uint16_t* dst, mfsr_stream_t stream);
    void (*reset)(void* user);   /* may be NULL */
    void* user;
} mfsr_frame_source;
/* reset, then pull up to cfg.frames frames (the first one is the reference: cfg.reference must be 0), fuse them and
 * finish into outImg / out16 (either may be NULL); *framesUsed = frames delivered.  imgOut / totalWeights: accumulators.
 * MFSR_E_INVALID for a burst created with cfg.rawPacking != 0: the source writes uint16_t samples into the slots itself. */
int mfsr_burst_process_source(mfsr_burst* b, const mfsr_frame_source* src, mfsr_float3* imgOut, mfsr_float3* totalWeights,
                              mfsr_float3* outImg, uint16_t* out16, int* framesUsed, mfsr_stream_t stream);

/* ---- frame selection: score every frame of a burst by sharpness, take the sharpest as the reference and drop frames much
 * softer than it (the base-frame choice of the handheld multi-frame SR method).
 * Score of a raw frame: G(i, j) = raw(2i+ay, 2j+ax) + raw(2i+by, 2j+bx) with (ay, ax), (by, bx) the two quad positions whose
 * CFA entry is MFSR_GREEN ((0,1) and (1,0) for mono; any other count of greens is invalid), gx / gy its 3x3 Sobel gradients,
 * S = sum of gx^2 + gy^2 over the half-resolution rectangle rect = {x0, y0, x1, y1}: [x0, x1) x [y0, y1) with
 * 1 <= x0 < x1 <= width/2 - 1, 1 <= y0 < y1 <= height/2 - 1 and at most 2^23 pixels.  Exact 64-bit integer arithmetic:
 * bit-for-bit reproducible.
 * mfsr_frameSharpness: frames = host array of nFrames DEVICE pointers (u16, rows `pitch` bytes apart, width and height even);
 * sumsDev[0 .. nFrames) (device) := S of each frame (zeroed on the stream first).  Every argument is checked on the host
 * before any device call (MFSR_E_INVALID).  cfa is ignored (may be NULL) when mono != 0. */
int mfsr_frameSharpness(int nFrames, const uint16_t* const* frames, int pitch, int width, int height, const int32_t cfa[4],
                        int mono, const int32_t rect[4], long long* sumsDev, mfsr_stream_t stream);
/* Host only (no device call).  reference := argmax of sums over frames [0, candidates) (candidates 0 or >= n: all frames;
 * ties: the lowest index); keep[k] (may be NULL) := 1 iff k == reference or (double)sums[k] >= (double)keepRatio *
 * (double)sums[reference], else 0.  keepRatio in [0, 1] (0 keeps every frame); anything else, NaN included, is invalid. */
int mfsr_select_frames(int n, const long long* sums, int candidates, float keepRatio, int* reference, int32_t* keep);
/* Score the burst's frames (device-resident, dense rows as for mfsr_burst_add_frame; 1 <= nFrames <= cfg.frames; CFA, mono and
 * size from the burst's config), wait for the stream once and select (mfsr_select_frames).  sumsDev: nFrames device entries
 * of caller scratch.  Host outputs: reference (required), keep[nFrames], sums[nFrames] and the scored rectangle rect[4]
 * (each may be NULL).  Scored rectangle: without a zoom window [8, W/2-8) x [8, H/2-8), or [1, W/2-1) x [1, H/2-1) if that
 * margin leaves nothing; with the window (x, y, w, h) of the next set_reference (mfsr_burst_set_window) at scale s its raw
 * footprint in half resolution, [floor(x/2s), ceil((x+w)/2s)) and likewise in y, clipped to [1, W/2-1) x [1, H/2-1) (a
 * footprint that the clip empties becomes the nearest scorable column / row).  Processes nothing: the caller then runs
 * mfsr_burst_begin / set_reference(frames[reference]) / add_frame(kept frames in index order) / finish. */
int mfsr_burst_select_frames(mfsr_burst* b, int nFrames, const uint16_t* const* frames, int candidates, float keepRatio,
                             long long* sumsDev, int* reference, int32_t* keep, long long* sums, int32_t rect[4],
                             mfsr_stream_t stream);

/* ---- defective pixels: hot / dead sensor pixels found by a vote over the frames of a burst, and repaired in the raw domain
 * before anything else looks at the frames.  A deviation that stays on the same sensor pixel in most
 * frames of a hand-held burst is the sensor, not the scene.  Exact integer arithmetic: bit-for-bit reproducible.
 * Let d = 1 for mono, d = 2 for a Bayer mosaic (the same-colour lattice of every quad position).  For pixel (x, y) of a
 * frame with value v: N8 = the up to eight pixels (x + i*d, y + j*d), i, j in {-1, 0, 1}, not both 0, inside the frame;
 * hi = max N8, lo = min N8, margin = threshold + (((hi - lo) * spread) >> 2) in 32-bit integers; the frame casts a HOT vote
 * if v > hi + margin and a COLD vote if v + margin < lo.  map(x, y) = 1 (hot) if the hot votes of all frames >= minVotes,
 * else 2 (cold) if the cold votes >= minVotes, else 0.
 * Arguments: 1 <= nFrames <= 64, 0 <= threshold <= 65535, 0 <= spread <= 16, nFrames/2 < minVotes <= nFrames (a pixel
 * cannot be both), width and height >= 2d+1, pitch >= 2*width and even, mapPitch >= width; everything is checked on the
 * host before any device call (MFSR_E_INVALID).  frames = host array of nFrames DEVICE pointers (u16, rows `pitch` bytes
 * apart).
 * mfsr_detectDefects: mapDev (device, rows mapPitch bytes apart; only the width bytes of a row are written) := the map;
 * countsDev (device, may be NULL) := {hot pixels, cold pixels} of the map, zeroed on the stream first.  Frames are read only.
 * mfsr_repairDefects, in place, under ANY map (a camera's calibration map is as good as a detected one): every pixel whose
 * map entry is not 0 becomes, in each frame, the median of those of its N8 whose own map entry is 0: with n of them sorted
 * ascending as s, s[n/2] for odd n, (s[n/2-1] + s[n/2] + 1) >> 1 for even n; unchanged for n = 0.  Pixels whose map entry
 * is 0 are never written (flagged pixels are only written, unflagged ones only read: in place is safe). */
int mfsr_detectDefects(int nFrames, const uint16_t* const* frames, int pitch, int width, int height, int mono, int threshold,
                       int spread, int minVotes, uint8_t* mapDev, int mapPitch, uint32_t* countsDev, mfsr_stream_t stream);
int mfsr_repairDefects(int nFrames, uint16_t* const* frames, int pitch, int width, int height, int mono, const uint8_t* mapDev,
                       int mapPitch, mfsr_stream_t stream);
/* Detect and repair the defects of a burst's frames (device-resident, dense rows as for mfsr_burst_add_frame; size and mono
 * from the burst's config; 1 <= nFrames <= 64), in place.  mapDev: width * height bytes of caller scratch (the dense map, left
 * there for the caller); countsDev: 2 device entries of caller scratch, required if counts is given; counts (host, may be
 * NULL) := {hot, cold} after one wait for the stream.  Processes nothing: the caller then runs the usual
 * begin / set_reference / add_frame / finish, or mfsr_burst_select_frames first (repair goes before selection). */
int mfsr_burst_repair_defects(mfsr_burst* b, int nFrames, uint16_t* const* frames, int threshold, int spread, int minVotes,
                              uint8_t* mapDev, uint32_t* countsDev, uint32_t counts[2], mfsr_stream_t stream);

/* ---- exposure matching: equalise the brightness of a burst's frames in the raw domain before alignment looks at them
 * (auto-exposure drift, flicker of mains-powered light).  A global gain per frame (or per frame and
 * colour) about the black level, measured from plain channel sums and applied in place.  Exact integer arithmetic:
 * bit-for-bit reproducible.  Order of the raw-domain steps: repair defects, select the reference, match exposure to that
 * reference, process.
 * Let q = 2*(y&1) + (x&1) number the position of sample (x, y) inside its 2x2 quad (for mono too); black[q] integer black
 * levels, 0 <= black[q] <= 65535; 0 < sat <= maxValue <= 65535; rect = {x0, y0, x1, y1} a half-resolution rectangle of quads
 * [x0, x1) x [y0, y1) with the bounds of mfsr_frameSharpness (1 <= x0 < x1 <= width/2 - 1, likewise y; at most 2^23 quads).
 * MEASURE.  A quad of frame k is usable if all four of its samples are < sat.  C[k] = number of usable quads in rect;
 * S[k][q] = sum over the usable quads of max(v_q - black[q], 0).  64-bit integers, independent of the reduction order and of
 * the launch shape.  (A quad, not a pixel, is the unit, so that the four sums always cover the same scene area.)
 * GAIN (host only, unsigned 128-bit intermediates, no floating point).  colour(q) = cfa[q], which must be MFSR_RED, MFSR_GREEN
 * or MFSR_BLUE; mono: all four positions are one class and perColour is ignored.  Common mode (perColour = 0): T[k][c] =
 * S[k][0] + S[k][1] + S[k][2] + S[k][3] for every c; per-colour mode: T[k][c] = sum of S[k][q] over the positions with
 * colour(q) = c.  gain[k][c] = floor((T[ref][c] * C[k] * 65536 + den/2) / den), den = T[k][c] * C[ref]: Q16, 65536 = 1.0,
 * saturated at 2^31 - 1.  In common mode the three entries of gain[k] are equal; in per-colour mode the entry of a colour the
 * CFA does not have is 65536 and takes no part below.
 * status[k], tested in this order:
 *   the reference: 1, gains 65536, never written;
 *   2 unmeasurable: C[k] == 0, C[ref] == 0, or a T[k][c] or T[ref][c] that is needed is 0; gains reported as 65536;
 *   1 within the deadband: every |gain[k][c] - 65536| <= deadband; gains reported as 65536;
 *   3 out of range: some gain[k][c] outside [minGain, maxGain]; gains reported as computed;
 *   0 matched.
 * Only frames with status 0 are ever written.  0 <= deadband < 65536, 4096 <= minGain <= 65536 <= maxGain <= 1048576.
 * APPLY (in place, frames with status 0 only).  Sample v at position q with b = black[q], g = gain[k][colour(q)] (mono:
 * gain[k][0]): unchanged if v <= b or v >= sat (a clipped sample stays clipped: a darkened highlight would read as grey);
 * otherwise min(b + (((v - b) * g + 32768) >> 16), maxValue) (the product needs more than 32 bits).
 * Every argument is checked on the host before any device call (MFSR_E_INVALID).  frames = host array of nFrames DEVICE
 * pointers (u16, rows `pitch` bytes apart, pitch >= 2*width and even, width and height even), 1 <= nFrames <= 64.
 * mfsr_frameLevels: levelsDev[5*k + q] := S[k][q], levelsDev[5*k + 4] := C[k] (device, zeroed on the stream first).  Frames
 * are read only. */
int mfsr_frameLevels(int nFrames, const uint16_t* const* frames, int pitch, int width, int height, const int32_t black[4], int sat,
                     const int32_t rect[4], long long* levelsDev, mfsr_stream_t stream);
/* Host only (no device call).  levels[5*n] as mfsr_frameLevels leaves them (each entry in [0, 2^48)); gains[3*n], status[n]. */
int mfsr_exposure_gains(int n, const long long* levels, int reference, const int32_t cfa[4], int mono, int perColour, int deadband,
                        int minGain, int maxGain, int32_t* gains, int32_t* status);
/* gains[3*nFrames] and status[nFrames] are HOST arrays (they travel in the launch's argument table, like the frame
 * pointers); the gains of a status-0 frame must lie in [4096, 1048576].  One launch for all status-0 frames; frames with
 * status != 0, and the bytes of a row beyond its width samples, are never written. */
int mfsr_applyGains(int nFrames, uint16_t* const* frames, int pitch, int width, int height, const int32_t cfa[4], int mono,
                    const int32_t black[4], int sat, int maxValue, const int32_t* gains, const int32_t* status, mfsr_stream_t stream);
/* The levels and bounds a burst uses when the caller has none of their own (host only): black[q] = cfg.black[colour(q)] rounded
 * to nearest (mono: cfg.black[0]); sat = the smallest floor(cfg.black[c] + cfg.white[c]) over the three channels; maxValue =
 * (int)cfg.maxVal; deadband = 164 (0.25 %, twice what a constant-exposure burst measures: DESIGN.md section 2.14); minGain =
 * 16384, maxGain = 262144 (+-2 EV: beyond it a frame is no flicker victim); perColour = 0.  Every output may be NULL. */
int mfsr_exposure_defaults(const mfsr_config* cfg, int32_t black[4], int32_t* sat, int32_t* maxValue, int32_t* deadband,
                           int32_t* minGain, int32_t* maxGain, int32_t* perColour);
/* Match the exposure of a burst's frames (device-resident, dense rows as for mfsr_burst_add_frame; 1 <= nFrames <= 64) to
 * frames[reference], in place: mfsr_frameLevels, one wait for the stream, mfsr_exposure_gains, mfsr_applyGains.  black, sat and
 * maxValue are those of mfsr_exposure_defaults; CFA, mono and size come from the burst's config; the rectangle is exactly the
 * one mfsr_burst_select_frames scores (the window's footprint when a zoom window is set).  levelsDev: 5 * nFrames device
 * entries of caller scratch.  Host outputs (each may be NULL): gains[3*nFrames], status[nFrames], levels[5*nFrames].
 * Processes nothing: the caller then runs the usual begin / set_reference(frames[reference]) / add_frame / finish. */
int mfsr_burst_match_exposure(mfsr_burst* b, int nFrames, uint16_t* const* frames, int reference, int perColour, int deadband,
                              int minGain, int maxGain, long long* levelsDev, int32_t* gains, int32_t* status, long long* levels,
                              mfsr_stream_t stream);

/* ---- lens shading: vignetting and colour shading of the lens corrected in the raw domain with a flat-field gain map, before
 * anything else but the defect repair looks at the frames.  Exact integer arithmetic: bit-for-bit
 * reproducible.  Order of the raw-domain steps: repair defects, correct shading, select the reference, match exposure, process.
 * THE MAP.  q = 2*(y&1) + (x&1) numbers the position of sample (x, y) inside its 2x2 quad (for mono too); X = x>>1, Y = y>>1 are
 * its quad's half-resolution coordinates, hw = width/2, hh = height/2.  cell = 1<<k quads, 3 <= k <= 8.  The grid has gw =
 * (hw - 2 + cell)/cell + 1 by gh = (hh - 2 + cell)/cell + 1 points (integer division); point (i, j) sits at quad (i*cell,
 * j*cell), so the last point lies at or beyond the last quad.  map = int32 [4][gh][gw] in DEVICE memory, dense, 4-byte aligned:
 * Q16 gains (65536 = 1.0), each in [4096, 1048576], G[q][j][i] the gain of position q at grid point (i, j).  The values are the
 * caller's responsibility (they are not read back to be checked; a value outside the range gives an unspecified sample value,
 * never an access outside the frame or the map); mfsr_shading_fit produces none outside it.
 * Gain of quad (X, Y) at position q, with i = X>>k, fx = X & (cell-1), j = Y>>k, fy = Y & (cell-1), in 64-bit integers (the
 * sum is below 2^37):
 *   g = ((cell-fx)*(cell-fy)*G[q][j][i] + fx*(cell-fy)*G[q][j][i+1] + (cell-fx)*fy*G[q][j+1][i] + fx*fy*G[q][j+1][i+1]
 *        + (1 << (2k-1))) >> 2k
 * A term whose weight is 0 is not read: at X = (gw-1)*cell (fx = 0) column i+1 does not exist, likewise row j+1.
 * APPLY (in place).  Sample v at position q with b = black[q]: unchanged if v <= b; otherwise min(b + (((v - b) * g + 32768)
 * >> 16), maxValue), the arithmetic of mfsr_applyGains.  Unlike there, a clipped sample is multiplied too (there is no sat): a
 * blown corner is "at least sat * g", and left at sat beside neighbours lifted above it a highlight would turn into a dark spot.
 * Bytes of a row beyond its width samples are never written.  frames = host array of nFrames DEVICE pointers with the rules of
 * mfsr_applyGains (1 <= nFrames <= 64, u16, rows `pitch` bytes apart, pitch >= 2*width and even, width and height even);
 * 0 <= black[q] <= 65535, 0 < maxValue <= 65535.  Every argument is checked on the host before any device call
 * (MFSR_E_INVALID). */
int mfsr_applyShading(int nFrames, uint16_t* const* frames, int pitch, int width, int height, const int32_t* mapDev, int cell,
                      const int32_t black[4], int maxValue, mfsr_stream_t stream);
/* MEASURE a map from flat-field frames (a uniformly lit diffuser).  The BOX of grid point (i, j) is the quads with
 * i*cell - cell/2 <= X < i*cell + cell/2 and likewise in Y, clipped to the frame: the boxes tile the frame, edge boxes are half
 * or quarter size.  A quad is usable iff all four of its samples are < sat (the quad is the unit, as for mfsr_frameLevels).
 * Over all frames of the call: sumsDev[q][j][i] = sum over the usable quads of the box of max(v_q - black[q], 0) (int64
 * [4][gh][gw]), countsDev[j][i] = number of usable quads of the box (int64 [gh][gw]); device memory, 8-byte aligned, zeroed on
 * the stream first.  Integers: independent of the reduction order and of the launch shape.  Frames as above, read only;
 * 0 < sat <= 65535.  Every argument is checked on the host before any device call (MFSR_E_INVALID). */
int mfsr_shadingStats(int nFrames, const uint16_t* const* frames, int pitch, int width, int height, int cell, const int32_t black[4],
                      int sat, long long* sumsDev, long long* countsDev, mfsr_stream_t stream);
/* FIT (host only, no device call, unsigned 128-bit intermediates, no floating point).  sums[4][gh][gw] and counts[gh][gw] as
 * mfsr_shadingStats leaves them, in HOST memory (each entry in [0, 2^48)); map[4][gh][gw] (host) := the gains.  With p a grid
 * point, S_q[p] and C[p] its sums and count: the ANCHOR a is the point with the largest mean level (S_0 + S_1 + S_2 + S_3)[p] /
 * C[p], compared exactly by cross-multiplication, ties to the lowest index j*gw + i; map[q][p] = clamp(floor((S_q[a] * C[p] *
 * 65536 + den/2) / den), 65536, maxGain), den = S_q[p] * C[a].  One anchor for all four positions: colour shading is corrected
 * relative to the same spot.  *status: 2 unmeasurable (some C[p] < minQuads or some S_q[p] == 0: every gain 65536); 3 some gain
 * was clamped at maxGain (the map is still returned); else 0.  minQuads >= 1, 65536 <= maxGain <= 1048576. */
int mfsr_shading_fit(const long long* sums, const long long* counts, int gw, int gh, int minQuads, int maxGain, int32_t* map,
                     int32_t* status);
/* The levels and bounds a burst uses when the caller has none of their own (host only): black, sat and maxValue as
 * mfsr_exposure_defaults; cell = the largest 1<<k, k <= 6, with cell <= min(width/2, height/2) - 1 (so that gw, gh >= 2), never
 * below 8: frames smaller than 18 x 18 are refused when cell is asked for; minQuads = 64; maxGain = 524288 (3 stops).  Every
 * output may be NULL. */
int mfsr_shading_defaults(const mfsr_config* cfg, int32_t black[4], int32_t* sat, int32_t* maxValue, int32_t* cell, int32_t* minQuads,
                          int32_t* maxGain);
/* mfsr_applyShading on a burst's frames (device-resident, dense rows as for mfsr_burst_add_frame; 1 <= nFrames <= 64), in
 * place, with black and maxValue of mfsr_shading_defaults and the size of the burst's config; cell <= 0: the cell of
 * mfsr_shading_defaults.  Processes nothing: the caller then runs mfsr_burst_select_frames, mfsr_burst_match_exposure and the
 * usual begin / set_reference / add_frame / finish (shading goes after the defect repair and before the selection). */
int mfsr_burst_correct_shading(mfsr_burst* b, int nFrames, uint16_t* const* frames, const int32_t* mapDev, int cell,
                               mfsr_stream_t stream);

/* ---- packed raw frames: the 10 / 12-bit packings sensors and raw files deliver, widened on the device to the uint16_t samples
 * every other entry point takes.  P is a sample and B a byte of ONE ROW; rows are independent and
 * a row starts at a byte boundary (its first byte is B0 of its first group).
 *   MFSR_PACK_MIPI10  4 samples in 5 bytes (CSI-2 RAW10):  B0 = P0>>2, B1 = P1>>2, B2 = P2>>2, B3 = P3>>2,
 *                     B4 = (P0&3) | (P1&3)<<2 | (P2&3)<<4 | (P3&3)<<6
 *   MFSR_PACK_MIPI12  2 samples in 3 bytes (CSI-2 RAW12):  B0 = P0>>4, B1 = P1>>4, B2 = (P0&15) | (P1&15)<<4
 *   MFSR_PACK_BE10    4 samples in 5 bytes, big-endian bit stream (DNG / TIFF), first sample in the most significant bits:
 *                     B0 = P0>>2, B1 = (P0&3)<<6 | P1>>4, B2 = (P1&15)<<4 | P2>>6, B3 = (P2&63)<<2 | P3>>8, B4 = P3&255
 *   MFSR_PACK_BE12    2 samples in 3 bytes, big-endian bit stream:  B0 = P0>>4, B1 = (P0&15)<<4 | P1>>8, B2 = P1&255
 * Samples come out as they are (0..1023 / 0..4095): no shift, no scaling; a burst's cfg.black / white / maxVal describe that
 * range.  width is a multiple of 4 (10 bits) or 2 (12 bits); the dense row is width*bits/8 bytes.
 * mfsr_packed_row_bytes: that size; host arithmetic; MFSR_E_INVALID (< 0) for an unknown packing (MFSR_PACK_NONE included) or
 * a width that is not positive or breaks the rule.
 * mfsr_unpackRaw: packed = host array of nFrames DEVICE pointers to packed frames (any alignment), rows rowBytes >= the dense
 * row size apart (bytes of a row beyond the dense size are never read); frames = host array of nFrames DEVICE pointers (u16,
 * 2-byte aligned, rows `pitch` bytes apart, pitch >= 2*width and even; bytes of a row beyond 2*width are never written);
 * 1 <= nFrames <= 64, height >= 1.  One launch for all frames.  Source and destination must not overlap.  Every argument is
 * checked on the host before any device call (MFSR_E_INVALID).  Exact: integers only. */
#define MFSR_PACK_NONE 0
#define MFSR_PACK_MIPI10 1
#define MFSR_PACK_MIPI12 2
#define MFSR_PACK_BE10 3
#define MFSR_PACK_BE12 4
int mfsr_packed_row_bytes(int packing, int width);
int mfsr_unpackRaw(int nFrames, const uint8_t* const* packed, int rowBytes, int packing, uint16_t* const* frames, int pitch,
                   int width, int height, mfsr_stream_t stream);

/* ---- noise-model calibration: measure the affine noise model var = alpha * I + beta of the robustness model (cfg.alpha,
 * cfg.beta) from raw frames of the sensor at the gain in use.  An exact-integer device stage and a small
 * host fit.  Frames are read only; nothing here runs unless it is called.
 * q = 2*(y&1) + (x&1) numbers the position of sample (x, y) inside its 2x2 quad (for mono too).  A BLOCK is 4x4 quads = 8x8
 * raw samples; the block grid starts at the frame origin and has (width/8) x (height/8) blocks (a partial block at the right
 * or bottom edge is not part of it).  Per position a block holds 16 samples p[r][c], r, c = 0..3.  rect = {bx0, by0, bx1, by1}
 * is a rectangle of blocks [bx0, bx1) x [by0, by1) inside the grid, not empty.  0 < sat <= 65535, 0 <= black[q] < sat.
 * STATS.  A block is usable iff all of its 64 samples are < sat.  Per usable block and position q:
 *   S = sum of p;   D = sum over r of (p[r][0] - p[r][1])^2 + (p[r][2] - p[r][3])^2   (8 disjoint same-colour pairs; E[D] = 16 var)
 *   level bin l = clamp(S - 16*black[q], 0, span - 1) * 64 / span (integer division), span = 16 * (sat - black[q]);
 *   variance bin v = D for D < 16, else 16 + 8*(e - 4) + ((D >> (e - 3)) & 7) with e = floor(log2 D): 8 bins per octave, v <= 271.
 * Summed over all frames of the call: hist[q][l][v] (u32, 4 x 64 x 272), levelSum[q][l] = sum of S, count[q][l] (both 64-bit,
 * 4 x 64).  Integer arithmetic: independent of the reduction order and of the launch shape.  The three tables are device
 * memory, zeroed on the stream first.  frames = host array of nFrames DEVICE pointers (u16, rows `pitch` bytes apart, pitch >=
 * 2*width and even, width and height even), 1 <= nFrames <= 64; nFrames * blocks of rect < 2^31.  Every argument is checked on
 * the host before any device call (MFSR_E_INVALID). */
#define MFSR_NOISE_HIST_ENTRIES (4 * 64 * 272)
#define MFSR_NOISE_LEVEL_ENTRIES (4 * 64)
#define MFSR_NOISE_SCRATCH_BYTES (4 * MFSR_NOISE_HIST_ENTRIES + 16 * MFSR_NOISE_LEVEL_ENTRIES)
int mfsr_noiseStats(int nFrames, const uint16_t* const* frames, int pitch, int width, int height, const int32_t black[4], int sat,
                    const int32_t rect[4], uint32_t* histDev, long long* levelSumDev, long long* countDev, mfsr_stream_t stream);
/* FIT (host only, no device call, double precision).  The three tables as HOST arrays; white[q] > 0 the white level of
 * position q; minBlocks >= 1.  Every (q, l) with count >= minBlocks gives one point: median = the value at rank count/2 of the
 * row's histogram, linear inside the bin between the bin's lowest D and the next bin's; var = median / 14.6882 (D / (2 var) is
 * chi-square with 8 degrees of freedom on a flat block, whose median is 7.3441); x = (levelSum / (16 count) - black[q]) /
 * white[q]; y = max(var - 1/12, 0) / white[q]^2 (1/12: the quantiser's own variance).  One least-squares line y = alpha x + beta
 * over the points of all four positions, weighted by count.  A negative beta is set to 0 and alpha refitted through the origin.
 * *status: 0 ok; 2 unmeasurable (fewer than 4 points, or max x - min x < 1/8: alpha = beta = 0); 3 alpha <= 0 (values as
 * fitted).  *points (may be NULL): the number of points. */
int mfsr_noise_fit(const uint32_t* hist, const long long* levelSum, const long long* count, const int32_t black[4],
                   const float white[4], int minBlocks, double* alpha, double* beta, int32_t* status, int32_t* points);
/* The levels and bounds a burst uses (host only): black[q] and sat as mfsr_exposure_defaults; white[q] = cfg.white[colour(q)]
 * (mono: cfg.white[0]); minBlocks = 200; rect = the whole block grid less one block of border (needs width, height >= 24).
 * Every output may be NULL. */
int mfsr_noise_defaults(const mfsr_config* cfg, int32_t black[4], float white[4], int32_t* sat, int32_t* minBlocks, int32_t rect[4]);
/* mfsr_noiseStats over the given device frames (dense rows, the burst's size; 1 <= nFrames <= 64) with the defaults above, one
 * wait for the stream, mfsr_noise_fit.  scratchDev: MFSR_NOISE_SCRATCH_BYTES of device memory, 8-byte aligned.  Changes nothing
 * in the burst or in the frames: alpha and beta are construction-time configuration, so the caller writes them into the
 * mfsr_config of the burst it creates next.  *alpha, *beta: as fitted (0 when *status is 2).  The frames should show flat areas
 * at many levels (a chart, or a natural image with flat regions): pixel-scale texture reads as noise (section 2.15, limits). */
int mfsr_burst_calibrate_noise(mfsr_burst* b, int nFrames, const uint16_t* const* frames, void* scratchDev, float* alpha,
                               float* beta, int32_t* status, mfsr_stream_t stream);

/* ---- burst noise calibration: the noise model measured on the DIFFERENCES of the frames of a burst.
 * Two frames whose displacement relative to each other is, at some place, within tol of a whole number of quads sample the
 * scene there at the same sub-quad phase: their same-colour samples differ by noise only, texture and aliasing cancel.  No
 * interpolation, so the device stage is exact integer arithmetic like mfsr_noiseStats; blocks, positions q, level and variance
 * bins, rect, black, sat and the three tables are those of mfsr_noiseStats.
 * frames: host array of nFrames DEVICE pointers (u16, w x h samples, rows rowBytes bytes apart), 2 <= nFrames <= 64, checked as
 * mfsr_noiseStats checks its frames, pitch, width and height.  flows: host array of nFrames DEVICE pointers, flows[i] = the flow
 * field of frame i in the burst's convention (float2 texels, flowW x flowH, rows flowRowBytes bytes apart, flowRowBytes >= 8*flowW
 * and a multiple of 8, pointer 8-byte aligned; raw-pixel units; reference pixel p corresponds to pixel p + flow of frame i), or
 * NULL = zero flow (the reference).  (flowW, flowH) is (w/2, h/2) or (w, h), the two sizes mfsr_burst_field_dims gives.
 * 0 <= tol <= 0.25.
 * PER BLOCK (bx, by) of rect:
 *   frame i: f = the texel ((8bx+4)*flowW / w, (8by+4)*flowH / h) (integer division, a plain load); h_i = 0.5f * f;
 *     the frame is PLACED at the block iff both components are finite and |h| <= 16384; s_i = (int)roundf(h_i) per axis;
 *   pair j < k of placed frames: d = h_k - h_j (float), s = (int)roundf(d), r = d - (float)s; ACCEPTED iff |r.x| <= tol and
 *     |r.y| <= tol;
 *   block A = the 8x8 samples of frame j at (8bx + 2 s_j.x, 8by + 2 s_j.y), block B = those of frame k at A's origin + 2s; both
 *     wholly inside the frame and all 128 samples < sat, otherwise the pair contributes nothing at this block;
 *   per position q, p = A, t = A - B:  S = sum of p;  D = sum over r of ((t[r][0] - t[r][1])^2 + (t[r][2] - t[r][3])^2) (64-bit:
 *     it can reach 2^38); level bin from S as mfsr_noiseStats; variance bin min(bin(D), 271): the last bin saturates.
 * The tables are summed over all accepted (block, j, k); count[q][l] counts those terms.  Integer arithmetic: independent of
 * the launch shape and order.  nFrames*(nFrames-1)/2 * blocks of rect < 2^31.  Every argument is checked on the host before
 * any device call (MFSR_E_INVALID). */
int mfsr_noiseStatsTemporal(int nFrames, const uint16_t* const* frames, int rowBytes, int w, int h,
                            const mfsr_float2* const* flows, int flowRowBytes, int flowW, int flowH, const int32_t black[4], int sat,
                            const int32_t rect[4], float tol, uint32_t* histDev, long long* levelSumDev, long long* countDev,
                            mfsr_stream_t stream);
/* mfsr_noise_fit for the tables of mfsr_noiseStatsTemporal: the same operations with var = median / 29.3764 (t[.][0] - t[.][1]
 * has four times the variance of a sample, so D / (4 var) is chi-square with 8 degrees of freedom).  The 1/12 of the quantiser
 * is unchanged. */
int mfsr_noise_fit_temporal(const uint32_t* hist, const long long* levelSum, const long long* count, const int32_t black[4],
                            const float white[4], int minBlocks, double* alpha, double* beta, int32_t* status, int32_t* points);
/* bytes of device scratch mfsr_burst_calibrate_noise_temporal needs for nFrames frames of cfg's size (the tables, nFrames - 1
 * flow fields, one certainty mask); 0 for an invalid cfg or nFrames outside 2 .. 64.  Host arithmetic only. */
size_t mfsr_noise_temporal_scratch_bytes(const mfsr_config* cfg, int nFrames);
/* The noise model of the burst `frames` (nFrames device frames, dense rows, the burst's size), measured on the burst itself.
 * Between bursts only (MFSR_E_INVALID while frames are pending).  Starts a burst on b (as mfsr_burst_begin does, with no
 * accumulators attached), makes frames[reference] the reference (mfsr_burst_set_reference), aligns the other frames with
 * mfsr_burst_align_frames (flows into the scratch, one mask buffer for all: the masks are ignored, so cfg.alpha and cfg.beta
 * have no part in the result), one mfsr_noiseStatsTemporal over all frames (the reference with a NULL flow) with black, sat and
 * rect of mfsr_noise_defaults, one wait for the stream, mfsr_noise_fit_temporal with white of mfsr_noise_defaults.  tol <= 0 =
 * 1/16; minBlocks <= 0 = mfsr_noise_defaults' 200.  scratchDev: scratchBytes >= mfsr_noise_temporal_scratch_bytes(cfg, nFrames)
 * of device memory, 256-byte aligned.  Fuses nothing and changes neither the frames nor cfg: the caller writes *alpha and *beta
 * into the mfsr_config of the burst it creates next (doubles, as mfsr_noise_fit gives them).  The handle is left as mfsr_burst_begin and mfsr_burst_set_reference leave
 * it: the next burst starts with its own begin / set_reference as always.  *status as mfsr_noise_fit; 2 is the ordinary answer
 * for a burst without a phase-matched pair.  *points (may be NULL): points of the fit.  *blocks (may be NULL): the accepted
 * (block, pair) terms, the sum of count[0][.]. */
int mfsr_burst_calibrate_noise_temporal(mfsr_burst* b, int nFrames, const uint16_t* const* frames, int reference, float tol,
                                        int minBlocks, void* scratchDev, size_t scratchBytes, double* alpha, double* beta,
                                        int32_t* status, int32_t* points, long long* blocks, mfsr_stream_t stream);

/* ---- ghost suppression: erosion of the certainty mask between stage F and stage G.  Stage F decides
 * every cell on its own; at the rim of a moving object single cells pass although their neighbours fail, and the merge shows
 * a faint outline of the object there.  The erosion replaces every colour certainty by its minimum over a (2r+1) x (2r+1)
 * neighbourhood (r = 2: the 5x5 "additional robustness refinement" of the hand-held multi-frame super-resolution method).
 * Mask: float4 cells, width x height, .x .y .z the colour certainties, .w the motion measure M, the one-cell ring zero.  For
 * interior cells 1 <= x <= width-2, 1 <= y <= height-2:
 *   out.c(x, y) = min over |i| <= r, |j| <= r of in.c(clamp(x+i, 1, width-2), clamp(y+j, 1, height-2)),  c = x, y, z, each alone
 *   out.w(x, y) = in.w(x, y)
 * The window is clamped to the interior (the zero ring takes part in no window: it would reject the frame's outer r cells);
 * ring cells of the output are zero in all four components; bytes of a row beyond 16*width are never written.  Plain fminf
 * semantics: stage F never writes a NaN into .x .y .z (fmaxf(fminf(.., 1), 0)), so the result is defined bit for bit and does
 * not depend on the launch shape.
 * One launch for nFrames (1 .. MFSR_MAX_FUSE_GROUP) masks; in[k] != out[k], no output overlaps an input or another output
 * (not in place: a tile's halo would read cells a neighbour has already eroded); every argument is checked on the host before
 * any device call (MFSR_E_INVALID: radius outside 1..2, width or height < 3, a pitch < 16*width or not a multiple of 16, null,
 * misaligned or overlapping pointers, nFrames out of range).  Asynchronous on `stream`, allocates nothing: capturable.
 * cfg.maskErode = r makes the burst pipeline do this to every moved frame's mask (the reference frame's all-ones mask is not
 * touched); everything that consumes masks -- zoom windows, frame streams, the joint mode, stripe-sharded multi-GPU bursts --
 * then gets the eroded ones. */
int mfsr_erodeMaskBatch(int nFrames, const mfsr_float4* const* in, mfsr_float4* const* out, int width, int height,
                        int inPitch, int outPitch, int radius, mfsr_stream_t stream);

/* ---- rendered output: colour matrix, tone curve and a display-format store inside the finish.
 * A render description is something a burst carries; without one every entry point produces the bits and the launches it
 * always did.  All arithmetic is float32, no contraction.  For an HR pixel, p is the value the plain finish holds after
 * ApplyWeighting (with the fallback) and before its gamma:
 *   1. matrix (useMatrix != 0):  c_k = isnan(p_k) ? 0 : fminf(fmaxf(p_k, 0), 65536);
 *      q_i = (matrix[3i] * c_0 + matrix[3i+1] * c_1) + matrix[3i+2] * c_2  (row-major, this order of operations).  The nine
 *      coefficients must be finite with |m| <= 256 (MFSR_E_INVALID otherwise): no inf or NaN can arise.  Else q = p.
 *   2. tone.  toneLut != NULL: toneSize + 1 floats of DEVICE memory (4-byte aligned), 1 <= toneSize = N <= 65536:
 *      v = isnan(q) ? 0 : clamp(q, 0, 1);  t = v * (float)N;  i = min((int)t, N - 1);  f = t - (float)i;
 *      o = lut[i] + (lut[i+1] - lut[i]) * f.   Else with applyGamma the fixed sRGB curve of mfsr_GammasRGB; else o = q.
 *   3. quantise, Q(o, max) = (int)(clamp(o, 0, 1) * max + 0.5f), NaN -> 0:
 *      MFSR_OUT_RGB16    three uint16_t, max 65535, 6 bytes per pixel (rows and `out` 2-byte aligned)
 *      MFSR_OUT_RGB8     three bytes, max 255, 3 bytes per pixel (any byte alignment of `out`, any row bytes >= 3 * w)
 *      MFSR_OUT_RGBA8    bytes R, G, B, 255; 4 bytes per pixel (`out` 4-byte aligned, row bytes a multiple of 4)
 *      MFSR_OUT_RGB10A2  one little-endian dword r | g<<10 | b<<20 | 3u<<30, max 1023 (alignment as RGBA8)
 * The float image receives o, so the integer output is always the quantisation of the float output.  {MFSR_OUT_RGB16, no
 * matrix, no LUT} is bit for bit the plain finish.  The LUT stays the caller's and must stay valid until the stream has
 * passed the finish; the matrix is copied.  reserved: write zeros.
 * mfsr_render_row_bytes: bytes of a dense row of widthPx pixels; host arithmetic; MFSR_E_INVALID (< 0) for an unknown format
 * or a width that is not positive.
 * mfsr_renderImage: steps 1-3 on an existing float image (rows inRowBytes apart); outImg may be NULL or == in (in place), out
 * may be NULL when outImg is not.  mfsr_finishRendered: mfsr_finishFusedWindow with steps 1-3 in the same launch; it evaluates
 * the same float expressions for the fallback coordinates, so a stripe or window of it is the crop of the whole.  Both check
 * every argument on the host before any device call (MFSR_E_INVALID), are asynchronous on `stream` and allocate nothing. */
#define MFSR_OUT_RGB16 0
#define MFSR_OUT_RGB8 1
#define MFSR_OUT_RGBA8 2
#define MFSR_OUT_RGB10A2 3
typedef struct {
    int32_t format;       /* MFSR_OUT_* */
    int32_t useMatrix;    /* 0: matrix[] is ignored */
    float matrix[9];      /* row-major 3x3, display RGB = matrix * camera RGB */
    const float* toneLut; /* device memory, toneSize + 1 floats; NULL: cfg.applyGamma decides */
    int32_t toneSize;
    int32_t reserved[3];
} mfsr_render;
int mfsr_render_row_bytes(int format, int widthPx);
int mfsr_renderImage(const mfsr_float3* in, int inRowBytes, mfsr_float3* outImg, int outImgRowBytes, void* out, int outRowBytes,
                     int w, int h, const mfsr_render* render, int applyGamma, mfsr_stream_t stream);
int mfsr_finishRendered(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                        int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, mfsr_float3* outImg,
                        int outImgRowBytes, void* out, int outRowBytes, const mfsr_render* render, int w, int h, float threshold,
                        int applyGamma, int colOffset, int rowOffset, int fullWidth, int fullHeight, mfsr_stream_t stream);
/* The burst's render description (copied; NULL = off, the default).  Between bursts only: refused (MFSR_E_INVALID) while frames
 * are pending, as mfsr_burst_set_host_row_bytes is.  With one set, the out16 / out16Dev / out16Host arguments of
 * mfsr_burst_finish, _finish_rows, _finish_host, mfsr_burst_process_source, mfsr_burst_process_joint, mfsr_stream_push and
 * mfsr_stream_drain mean rendered bytes with dense rows of mfsr_render_row_bytes(format, output width): the declarations keep
 * their type and the caller casts.  finish_host downloads rows of that size.  cfg.fused = 0 runs its chain up to
 * ApplyWeighting and then mfsr_renderImage.  The multi-GPU layer (mfsr_dist.h) never sets one. */
int mfsr_burst_set_render(mfsr_burst* b, const mfsr_render* render);
/* the same for every output of a frame stream (between outputs: any time, a push completes its window before it returns) */
int mfsr_stream_set_render(mfsr_stream* s, const mfsr_render* render);

/* ---- two-plane YUV 4:2:0 output of the rendered finish: NV12 and P010.  Two more values of
 * mfsr_render.format; for them reserved[0] carries the colour description: bits 0-1 the standard (MFSR_YUV_BT709 / _BT601 /
 * _BT2020), bit 2 (MFSR_YUV_FULL) full range instead of limited range.  Any other bit, the standard value 3 or a non-zero
 * reserved[1] / reserved[2] is MFSR_E_INVALID; zeros mean BT.709 limited range.  (For the four formats above reserved stays
 * ignored.)  All arithmetic is float32, no contraction, in the order written; o is the pixel after steps 1-2 of the rendered
 * output (matrix, tone), which is still what the float image receives:
 *   1. c_k = isnan(o_k) ? 0 : fminf(fmaxf(o_k, 0), 1)
 *   2. Y = (Kr*c0 + Kg*c1) + Kb*c2;  Cb = (c2 - Y) * Sb;  Cr = (c0 - Y) * Sr.  The five constants are the float32 roundings of
 *      doubles: (Kr, Kb) = (0.2126, 0.0722) BT.709, (0.299, 0.114) BT.601, (0.2627, 0.0593) BT.2020; Kg = 1 - Kr - Kb,
 *      Sb = 0.5 / (1 - Kb), Sr = 0.5 / (1 - Kr).
 *   3. chroma of the 2 x 2 block with top-left pixel (x, y), x and y even:
 *      C = ((C(x, y) + C(x+1, y)) + (C(x, y+1) + C(x+1, y+1))) * 0.25f.  This is the box mean, i.e. the chroma sample is sited
 *      at the CENTRE of its four pixels (MPEG-1 / JPEG siting); left-cosited (MPEG-2) or filtered chroma is not offered.
 *   4. codes, N = 8 (NV12) or 10 (P010), m = 2^(N-8), M = 2^N - 1: limited range yq = 16m + 219m*Y, cq = 128m + 224m*C; full
 *      range yq = M*Y, cq = 2^(N-1) + M*C;  code = (int)(fminf(fmaxf(v, 0), M) + 0.5f).
 *      MFSR_OUT_NV12 stores the byte, MFSR_OUT_P010 stores code << 6 as a little-endian uint16_t.
 * Layout: a Y plane of h rows of w samples, and a chroma plane of h/2 rows of w/2 interleaved (Cb, Cr) pairs, so a chroma row
 * has the bytes of a Y row: mfsr_render_row_bytes gives w (NV12) or 2w (P010).  w and h must be even and positive
 * (MFSR_E_INVALID otherwise, also from mfsr_render_row_bytes for an odd width).  NV12 planes may have any byte alignment and
 * any row bytes >= w; P010 planes are 2-byte aligned with even row bytes >= 2w.
 * mfsr_render_image_bytes: the dense size of a rendered w x h image of any of the six formats, rowBytes * h or
 * rowBytes * h * 3 / 2; host arithmetic; < 0 for an unknown format or an extent the format does not take.
 * mfsr_renderImageYuv / mfsr_finishRenderedYuv: mfsr_renderImage / mfsr_finishRendered with the two plane pointers, each at
 * the launch's first row (chroma row r/2 goes with Y rows r, r+1), in place of out.  outImg may be NULL or in place; outY and
 * outUV are both given or both NULL, and at least one of outImg and the pair is given.  They refuse the four single-plane
 * formats, as mfsr_renderImage, mfsr_finishRendered, mfsr_sharpenImage and mfsr_finishSharpened refuse these two.  Every
 * argument is checked on the host before any device call (MFSR_E_INVALID); asynchronous on `stream`, nothing is allocated.
 * Bursts and streams (mfsr_burst_set_render / mfsr_stream_set_render): wherever one output buffer is taken, the chroma plane
 * follows the Y plane immediately -- chroma row r is "row" h + r of the same dense pitch, mfsr_render_image_bytes in all.
 * mfsr_burst_finish_rows needs even row0 and rows and fills both row ranges; mfsr_burst_finish_host downloads each band's Y
 * rows and chroma rows (one copy of 3h/2 rows when there is one band).  A window (x0, y0 multiples of 16) must have even
 * extents, so its 2 x 2 blocks are the whole frame's and its output is the crop of both planes; an odd output width or height
 * is refused at the finish.  A sharpen description together with a two-plane format is refused by whichever of
 * mfsr_burst_set_render / mfsr_burst_set_sharpen comes second. */
#define MFSR_OUT_NV12 16   /* 8-bit  Y plane, then interleaved Cb,Cr plane at half resolution in x and y */
#define MFSR_OUT_P010 17   /* 16-bit little-endian words, the 10-bit code in bits 15..6 (code << 6), same planes */
#define MFSR_YUV_BT709 0
#define MFSR_YUV_BT601 1
#define MFSR_YUV_BT2020 2
#define MFSR_YUV_FULL 4
long long mfsr_render_image_bytes(int format, int w, int h);
int mfsr_renderImageYuv(const mfsr_float3* in, int inRowBytes, mfsr_float3* outImg, int outImgRowBytes, void* outY, int yRowBytes,
                        void* outUV, int uvRowBytes, int w, int h, const mfsr_render* render, int applyGamma, mfsr_stream_t stream);
int mfsr_finishRenderedYuv(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                           int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, mfsr_float3* outImg,
                           int outImgRowBytes, void* outY, int yRowBytes, void* outUV, int uvRowBytes, const mfsr_render* render,
                           int w, int h, float threshold, int applyGamma, int colOffset, int rowOffset, int fullWidth,
                           int fullHeight, mfsr_stream_t stream);

/* ---- sharpening inside the finish: an unsharp mask on the linear float value, before matrix and tone (DESIGN.md section
 * 2.20).  Off unless asked for; without a sharpen description every entry point produces the bits and the launches it always
 * did.  All arithmetic is float32, no contraction.  For an HR pixel and each channel alone, p is the value section 2.19 calls
 * p (after ApplyWeighting with the fallback, before gamma):
 *   1. s = isnan(p) ? 0 : p
 *   2. horizontal: h(x, y) = k0 * s(x, y); then for d = 1 .. R in this order  h = h + kd * (s(x-d, y) + s(x+d, y))
 *   3. vertical:   the same expression on h along y gives b
 *   4. e = s - b;  a = fabsf(e) - threshold;  g = a > 0 ? copysignf(a, e) : 0;  o = s + amount * g
 *   5. o takes the place of p in steps 1-3 of the rendered output (matrix, tone, quantise); with no render description the
 *      steps are those of {MFSR_OUT_RGB16, no matrix, no table}.
 * Borders replicate: a coordinate outside the valid extent reads the nearest valid pixel (the extent is stated per entry point).
 * An inf in the input is not cleaned: s - b can then be inf - inf = NaN (which step 4 treats as "no edge": g = 0) or +-inf in
 * the R-neighbourhood of that pixel; the quantiser maps NaN to 0 and clamps inf as it always did.
 * Every value of a description must be finite, 0 <= radius <= 4, |taps[d]| <= 4, 0 <= amount <= 16, threshold >= 0, reserved
 * zero-filled; otherwise MFSR_E_INVALID.  radius == 0 or amount == 0 means off wherever a description is set on a handle.
 * mfsr_sharpen_gaussian (host only) fills a description with Gaussian taps: w_d = exp(-d^2 / (2 sigma^2)) in double, divided by
 * w_0 + 2 sum w_d in double, rounded to float; radius == 0 chooses min(4, max(1, (int)ceilf(2.5f * sigma))); sigma > 0, finite.
 * mfsr_sharpen_tile: the output tile one workgroup owns (the sizes at which the kernels take another path). */
typedef struct {
    int32_t radius;      /* R, 1..4; 0 = off */
    float taps[5];       /* k[0] centre, k[1..R]; k[d] for d > R ignored */
    float amount;        /* 0 <= amount <= 16; 0 = off */
    float threshold;     /* coring, >= 0, linear units */
    int32_t reserved[4]; /* zeros */
} mfsr_sharpen;
int mfsr_sharpen_gaussian(float sigma, int radius, float amount, float threshold, mfsr_sharpen* out);
int mfsr_sharpen_validate(const mfsr_sharpen* sharpen);
int mfsr_sharpen_tile(int* tileW, int* tileH);
/* Steps 1-5 on an existing float image; the valid extent is the image.  Neither outImg (the float value the integers quantise)
 * nor out may overlap `in` (MFSR_E_INVALID: a stencil cannot run in place); outImg or out may be NULL, not both.  render may be NULL
 * ({MFSR_OUT_RGB16, no matrix, no table}).  A description that is off (radius or amount 0) is refused: call mfsr_renderImage.
 * mfsr_finishSharpened: mfsr_finishRendered with steps 1-4 in the same launch.  Columns are valid in [0, w) of the launch, rows
 * in [-rowsAbove, h + rowsBelow) relative to the launch's first row (0 <= rowsAbove <= rowOffset, 0 <= rowsBelow <= fullHeight
 * - rowOffset - h): the accumulator and weight rows in that range must be complete, finalImg / weight point at the launch's
 * first row, and neither outImg nor out may overlap those rows (MFSR_E_INVALID; unlike mfsr_finishRendered, not in place).  So a
 * stripe with rowsAbove = rowsBelow = R is the crop of the whole in its rows, and a window (w < fullWidth)
 * clamps at its own left and right edges.  Both check every argument on the host before any device call, are asynchronous on
 * `stream` and allocate nothing. */
int mfsr_sharpenImage(const mfsr_float3* in, int inRowBytes, mfsr_float3* outImg, int outImgRowBytes, void* out, int outRowBytes,
                      int w, int h, const mfsr_sharpen* sharpen, const mfsr_render* render, int applyGamma, mfsr_stream_t stream);
int mfsr_finishSharpened(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                         int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, mfsr_float3* outImg,
                         int outImgRowBytes, void* out, int outRowBytes, const mfsr_render* render, int w, int h, float threshold,
                         int applyGamma, int colOffset, int rowOffset, int fullWidth, int fullHeight, const mfsr_sharpen* sharpen,
                         int rowsAbove, int rowsBelow, mfsr_stream_t stream);
/* The burst's sharpen description (copied; NULL, radius == 0 or amount == 0 = off, the default).  Between bursts only, as
 * mfsr_burst_set_render.  With one set, every finish of the burst goes through mfsr_finishSharpened: mfsr_burst_finish,
 * _finish_rows, _finish_host, mfsr_burst_process_source, mfsr_burst_process_joint and the outputs of a stream; without a render
 * description the integer output stays uint16_t RGB.  cfg.fused = 0 takes the same launch (the value the fused finish holds before
 * its gamma is bit for bit the chain's resampleFloat3 + ApplyWeighting; a stencil cannot run in place on the chain's image, and
 * the workspace holds no second one).  mfsr_burst_finish_rows passes rowsAbove = min(R, row0) and rowsBelow = min(R, H -
 * row0 - rows): the caller must have fused those rows of the accumulators too.  mfsr_burst_finish_host finishes band i - 1
 * after band i has been fused (the band count, the events and the download per band stay).  A window (mfsr_burst_set_window) is
 * the image at this level: it clamps at the window's own edges, so pixels within R of a window edge that is not a frame edge
 * differ from the whole-frame result (the Python layer grows the window by one 16-pixel ring and crops).  The multi-GPU layer
 * (mfsr_dist.h) never sets one. */
int mfsr_burst_set_sharpen(mfsr_burst* b, const mfsr_sharpen* sharpen);
int mfsr_stream_set_sharpen(mfsr_stream* s, const mfsr_sharpen* sharpen);
/* *finishes = the launches of mfsr_finishSharpened this burst has made since mfsr_burst_begin (host-side, as the counters of
 * mfsr_burst_debug_paths: 1 for a resident burst, one per band for a host burst, 0 when off).  It is
 * not an mfsr_path: those count branches that a configuration (mfsr_config) chooses, this one follows a setter. */
int mfsr_burst_debug_sharpened(const mfsr_burst* b, int* finishes);

/* ---- merge-aware denoise inside the finish: a range filter on the linear float value whose tolerance is the variance the
 * merge left at the pixel.  Off unless asked for; without a denoise description every entry point
 * produces the bits and the launches it always did.  All arithmetic is float32, no contraction, in the order written.  For an
 * HR pixel i, p is the value section 2.19 calls p (after ApplyWeighting with the fallback, before gamma), three channels k;
 * w is its accumulated weight (the totalWeights accumulator), threshold is cfg.weightThreshold:
 *   1. s_k = isnan(p_k) ? 0 : fminf(fmaxf(p_k, -65536), 65536)
 *   2. effective count, by the finish's own rule: n_k = (w_k < threshold) ? w_k + 1 : w_k;  n_k = isnan(n_k) ? 0 : n_k
 *   3. fade: wHi <= wLo (the default, both 0): lambda_k = 1; otherwise lambda_k = fminf(fmaxf((wHi - n_k) * rSpan, 0), 1) with
 *      rSpan = 1.0f / (wHi - wLo), formed once on the host in float
 *   4. tolerance: v_k = fmaxf((gain * (alpha * fmaxf(s_k, 0) + beta)) / fmaxf(n_k, 1e-6f), 1e-20f);  r_k = 1.0f / (hh * v_k)
 *      with hh = strength * strength, formed once on the host in float
 *   5. for dy = -R .. R and inside it dx = -R .. R, the neighbour j at the coordinate clamped to the valid extent (borders
 *      replicate; the extent is stated per entry point):
 *        d_k = s_jk - s_ik;  t = ((d_0*d_0)*r_0 + (d_1*d_1)*r_1) + (d_2*d_2)*r_2;  u = fmaxf(1.0f - t, 0);  g = u*u
 *      row sums start at 0 and add in dx order: G_dy = G_dy + g, S_dy,k = S_dy,k + g * s_jk; G and S_k start at 0 and the rows
 *      are added in dy order from row -R: G = G + G_dy, S_k = S_k + S_dy,k.  The centre contributes g = 1, so G >= 1.
 *   6. f_k = S_k / G;  o_k = (lambda_k == 0) ? s_k : s_k + lambda_k * (f_k - s_k)
 *   7. o takes the place of p in steps 1-3 of the rendered output (matrix, tone, quantise); with no render description the
 *      steps are those of {MFSR_OUT_RGB16, no matrix, no table}.
 * The tolerance is the expected variance (alpha p + beta) / n of a pixel that averaged n samples, times gain (a merge's
 * measured variance was about twice the prediction: the weights are not equal and the samples are interpolated) and times
 * strength^2: the filter is wide where few samples were merged and narrows by itself where many were.  The range kernel is a
 * polynomial, max(1 - t, 0)^2, so that no exp is evaluated and a float32 restatement is exact.
 * A description: radius 1..3 (0 = off), strength in [1/16, 16] (0 = off), gain in (0, 1024], alpha and beta in [0, 1], wLo and
 * wHi finite with 0 <= wLo and either wHi <= wLo or wHi - wLo >= 2^-10, reserved zero-filled; anything else is MFSR_E_INVALID.
 * With these bounds no inf or NaN arises in steps 3-6: |s| <= 2^16 and n is not NaN, so lambda is fmaxf / fminf of a product
 * with rSpan in (0, 1024] (fmaxf returns its other argument for a NaN: lambda lies in [0, 1] whatever n is); the numerator of
 * v is at most 1024 * (2^16 + 1) < 2^27 and its denominator at least 1e-6 (an infinite n gives 0, then 1e-20), so
 * 1e-20 <= v < 2^47; hh lies in [2^-8, 2^8], so 2^-55 < r < 2.6e22; |d| <= 2^17, so (d*d)*r < 2^34 * 2.6e22 < 5e32 and
 * t < 1.5e33 is finite; u and g lie in [0, 1]; G lies in [1, 49] (the centre has d = 0, t = 0, g = 1) and |S_k| <= 49 * 2^16;
 * f_k = S_k / G is a weighted mean of values of s, and |lambda (f - s)| <= 2^17.
 * mfsr_denoise_defaults (host only): radius 2, strength 3, gain 2, wLo = wHi = 0 and the caller's alpha, beta (the noise
 * model of one raw sample, cfg.alpha / cfg.beta, which mfsr_burst_calibrate_noise* can measure).
 * mfsr_denoise_tile: the output tile one workgroup owns (the sizes at which the kernels take another path). */
typedef struct {
    int32_t radius;      /* R, 1..3; 0 = off */
    float strength;      /* 1/16 .. 16; 0 = off */
    float gain;          /* measured / predicted variance of the merge, (0, 1024] */
    float alpha, beta;   /* variance of one raw sample = alpha * p + beta; each in [0, 1] */
    float wLo, wHi;      /* fade: full strength at n <= wLo, none at n >= wHi; wHi <= wLo = no fade */
    int32_t reserved[5]; /* zeros */
} mfsr_denoise;
int mfsr_denoise_defaults(float alpha, float beta, mfsr_denoise* out);
int mfsr_denoise_validate(const mfsr_denoise* denoise);
int mfsr_denoise_tile(int* tileW, int* tileH);
/* Steps 1 and 3-7 on an existing float image; the valid extent is the image.  count: a float3 image of n (rows countRowBytes
 * apart), or NULL for n = 1 everywhere, the single-frame case.  A count image IS n: the threshold rule of step 2 is skipped and
 * only its NaN cleaning applies.  Neither outImg nor out may overlap `in` or `count` (MFSR_E_INVALID: a stencil cannot run in
 * place); outImg or out may be NULL, not both.  render may be NULL ({MFSR_OUT_RGB16, no matrix, no table}); the two-plane
 * formats are refused.  A description that is off (radius or strength 0) is refused: call mfsr_renderImage.
 * mfsr_finishDenoised: mfsr_finishRendered with steps 1-6 in the same launch.  Columns are valid in [0, w) of the launch, rows
 * in [-rowsAbove, h + rowsBelow) relative to the launch's first row, exactly as for mfsr_finishSharpened: the accumulator and
 * weight rows in that range must be complete, and neither outImg nor out may overlap them.  A stripe with rowsAbove =
 * rowsBelow = R is the crop of the whole in its rows; a window clamps at its own left and right edges.  A wave whose pixels
 * all have lambda_k == 0 skips the stencil (step 6 makes that value-preserving).  Both check every argument on the host before
 * any device call, are asynchronous on `stream` and allocate nothing. */
int mfsr_denoiseImage(const mfsr_float3* in, int inRowBytes, const mfsr_float3* count, int countRowBytes, mfsr_float3* outImg,
                      int outImgRowBytes, void* out, int outRowBytes, int w, int h, const mfsr_denoise* denoise,
                      const mfsr_render* render, int applyGamma, mfsr_stream_t stream);
int mfsr_finishDenoised(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                        int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, mfsr_float3* outImg,
                        int outImgRowBytes, void* out, int outRowBytes, const mfsr_render* render, int w, int h, float threshold,
                        int applyGamma, int colOffset, int rowOffset, int fullWidth, int fullHeight, const mfsr_denoise* denoise,
                        int rowsAbove, int rowsBelow, mfsr_stream_t stream);
/* The burst's denoise description (copied; NULL, radius == 0 or strength == 0 = off, the default).  Between bursts only, as
 * mfsr_burst_set_render.  With one set, every finish of the burst goes through mfsr_finishDenoised, by the plumbing of the
 * sharpened finish: mfsr_burst_finish (cfg.fused = 0 too), _finish_rows (rowsAbove = min(R, row0), rowsBelow = min(R, H -
 * row0 - rows)), _finish_host (band i - 1 after band i has been fused), mfsr_burst_process_source, mfsr_burst_process_joint and
 * the outputs of a stream.  A window clamps at its own edges (the Python layer grows it by one 16-pixel ring and crops).
 * alpha and beta are the description's, not cfg's: the caller decides (the Python and CLI layers default them to cfg's).
 * Refused (MFSR_E_INVALID, by whichever setter comes second): a denoise description that is on together with a two-plane format,
 * and together with a sharpen description that is on (one launch would need a halo of both radii and a third LDS stage;
 * finish denoised to the linear float image, then mfsr_sharpenImage with the render description).  The multi-GPU layer
 * (mfsr_dist.h) never sets one. */
int mfsr_burst_set_denoise(mfsr_burst* b, const mfsr_denoise* denoise);
int mfsr_stream_set_denoise(mfsr_stream* s, const mfsr_denoise* denoise);
/* *finishes = the launches of mfsr_finishDenoised this burst has made since mfsr_burst_begin (as mfsr_burst_debug_sharpened) */
int mfsr_burst_debug_denoised(const mfsr_burst* b, int* finishes);
/* *launches = the launches of mfsr_robustnessMaskGroup this burst has made since mfsr_burst_begin: one per aligned group that
 * took the patch-mean path (mfsr_set_robustness_group), 0 with the switch off */
int mfsr_burst_debug_robust_group(const mfsr_burst* b, int* launches);

/* ---- image statistics, auto white balance, auto tone.  The measurement the render description
 * lacks: an exact-integer statistics stage on the device, two small fits on the host, and a burst driver that fills and
 * installs the mfsr_render of the finish.  Nothing here runs unless it is called.
 * THE STATISTIC.  For an HR pixel, p is the value of the rendered output's rule (after ApplyWeighting, with the fallback, before
 * gamma) and q is p after its step 1: the matrix (useMatrix != 0; same clamp, same order of operations), else q = p.
 *   codes    c_k = (int)(clamp(q_k, 0, 1) * 4095.0f + 0.5f), NaN -> 0                         (k = 0, 1, 2; 0 .. 4095)
 *   luma key y = (54 c_0 + 183 c_1 + 19 c_2 + 128) >> 8;   peak key m = max(c_0, c_1, c_2)     (both 0 .. 4095)
 *   neutral  lo <= min(c) and max(c) <= hi and, if chromaTol > 0, 256 |c_0 - c_1| <= chromaTol c_1 and
 *            256 |c_2 - c_1| <= chromaTol c_1
 * One table of MFSR_IMAGE_STATS_WORDS uint64_t: [0] pixels measured, [1] neutral pixels, [2..4] sums of c_0, c_1, c_2 over the
 * neutral set, [5..7] the same sums over all pixels, [8 .. 8+4096) the histogram of y, [8+4096 .. 8+8192) the histogram of m.
 * A launch ADDS to the table (device memory, 8-byte aligned; the caller zeroes it first), so stripes, windows and bands of an
 * image add up to the whole image's table exactly; integers, so nothing depends on the order of arrival or the launch shape.
 * mfsr_imageStats measures an existing float image (q from p = the image's value); mfsr_finishStats measures the accumulators
 * of a burst: its arguments are those of mfsr_finishRendered without the outputs and the render description, and it evaluates
 * the same float expressions (one definition), so what is measured is what the finish renders.  0 <= lo <= hi <= 4095,
 * 0 <= chromaTol <= 65536, a matrix in use finite with |m| <= 256, reserved zero-filled, w, h > 0 with w * h < 2^31, row bytes
 * >= 12 w and a multiple of 4: every argument is checked on the host before any device call (MFSR_E_INVALID).  Asynchronous on
 * `stream`, nothing is allocated: capturable. */
#define MFSR_IMAGE_STATS_BINS 4096
#define MFSR_IMAGE_STATS_WORDS (8 + 2 * MFSR_IMAGE_STATS_BINS)
typedef struct {
    int32_t useMatrix;   /* 0: matrix[] is ignored */
    float matrix[9];     /* row-major 3x3, as mfsr_render.matrix */
    int32_t lo, hi;      /* the neutral set: codes */
    int32_t chromaTol;   /* ... and its chroma bound in 1/256 of the green code; 0 = none */
    int32_t reserved[3]; /* zeros */
} mfsr_image_stats_params;
int mfsr_imageStats(const mfsr_float3* in, int inRowBytes, int w, int h, const mfsr_image_stats_params* params,
                    uint64_t* statsDev, mfsr_stream_t stream);
int mfsr_finishStats(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                     int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, int w, int h, float threshold,
                     int colOffset, int rowOffset, int fullWidth, int fullHeight, const mfsr_image_stats_params* params,
                     uint64_t* statsDev, mfsr_stream_t stream);
/* THE FITS (host only, no device call, double precision; the table as a HOST array).
 * mfsr_awb_gains: grey-world gains over the neutral set, S_k = stats[2 + k]: g_0 = S_1 / S_0, g_1 = 1, g_2 = S_1 / S_2, each
 * rounded to float.  *status: 0 ok; 1 unmeasurable (stats[1] < minCount, or a sum is 0: the gains are 1, 1, 1); 2 a gain was
 * clamped to [1/8, 8].
 * mfsr_tone_fit: black point, white point and a mid-tone gamma from the two histograms, and the tone table of them.  N =
 * stats[0] > 0; tLo = (uint64)(pLo N); tHi = (uint64)((1 - pHi) N); cumY / cumM = the running sums of the two histograms;
 *   kLo = the smallest k with cumY(k) > tLo;  kHi = the smallest k with cumM(k) >= N - tHi;  kMed = the smallest k with
 *   cumY(k) >= (N + 1) / 2 (integer division); each 4095 when the table never gets there;
 *   b = kLo / 4095;  span = max(kHi / 4095 - b, 1 / maxGain) (*status 1 when the floor was taken, else 0);
 *   u(v) = clamp((v - b) / span, 0, 1);  um = u(kMed / 4095);
 *   gamma = 1 if mid <= 0 or um is not inside (0, 1), else clamp(log(mid) / log(um), 0.5, 2);
 *   lut[k] = (float)sRGB(u(k / toneSize)^gamma), k = 0 .. toneSize, with sRGB(v) = v <= 0.0031308 ? 12.92 v :
 *   1.055 v^(1/2.4) - 0.055: toneSize + 1 floats for mfsr_render.toneLut once copied to the device.
 * *black = b, *white = b + span, *gamma; lutHost and the three may be NULL.  0 <= pLo, pHi <= 1, 1 <= maxGain <= 65536,
 * mid < 1, 1 <= toneSize <= 65536 (MFSR_E_INVALID otherwise).
 * mfsr_auto_defaults: awb = tone = 1, lo = 64, hi = 3967, chromaTol = 64, iterations = 2, minCount = pixels / 64, pLo = 0.001,
 * pHi = 0.999, maxGain = 8, mid = 0.18, toneSize = 4096. */
typedef struct {
    double pLo, pHi;  /* the shares of the pixels below the black point and up to the white point */
    double maxGain;   /* the span is at least 1 / maxGain */
    double mid;       /* where the median luma should land after the stretch; <= 0: no gamma */
} mfsr_tone_params;
typedef struct {
    int32_t awb, tone;          /* which of the two measurements run */
    int32_t lo, hi, chromaTol;  /* the neutral set (chromaTol: from the second pass on) */
    int32_t iterations;         /* white-balance passes, 1 .. 4 */
    long long minCount;         /* neutral pixels a pass needs; <= 0: 1/64 of the pixels measured */
    mfsr_tone_params toneParams;
    int32_t toneSize;           /* intervals of the table mfsr_burst_auto_render writes, 1 .. 65536 */
    int32_t reserved[3];        /* zeros */
} mfsr_auto_params;
typedef struct {
    float gains[3];          /* the white-balance gains in the installed matrix (1, 1, 1 without awb or when unmeasurable) */
    int32_t awbStatus;       /* 0 ok (or off); 1 the first pass was unmeasurable; 2 a gain was clamped to [1/8, 8] */
    int32_t awbPasses;       /* passes that changed the gains */
    int32_t toneStatus;      /* as mfsr_tone_fit (0 when off) */
    int32_t reserved;
    double black, white, gamma; /* as mfsr_tone_fit (0, 1, 1 when off) */
    double neutralShare;     /* stats[1] / stats[0] of the last white-balance pass (0 when off) */
} mfsr_auto_result;
int mfsr_awb_gains(const uint64_t* statsHost, long long minCount, float gains[3], int32_t* status);
int mfsr_tone_fit(const uint64_t* statsHost, const mfsr_tone_params* tone, int toneSize, float* lutHost, double* black,
                  double* white, double* gamma, int32_t* status);
int mfsr_auto_defaults(long long pixels, mfsr_auto_params* ap);
/* THE BURST DRIVER.  After the last mfsr_burst_add_frame and before mfsr_burst_finish: measures the burst's accumulators (the
 * output, or the zoom window when one is set; whatever cfg.fused is) with mfsr_finishStats and the arguments the finish itself
 * uses, and fills and installs the render description the finish then consumes.
 *   1. the frames still waiting are fused (as mfsr_burst_flush);
 *   2. ap->awb: pass 1 measures without a matrix and with chromaTol = 0 and takes g = mfsr_awb_gains; every further pass, up
 *      to ap->iterations in all, measures with the matrix diag(g) and ap->chromaTol and multiplies g by its gains,
 *      g_k = (float)((double)g_k * c_k), clamped to [1/8, 8]; a pass of status 1 leaves g as it is.  Else g = 1, 1, 1;
 *   3. M = render->matrix * diag(g) (render->useMatrix != 0), entry (float)((double)matrix[3i+j] * g_j), or diag(g) (awb
 *      without a matrix); |m| > 256 is refused (MFSR_E_INVALID).  Without awb the caller's matrix (or none) stays as given;
 *   4. ap->tone: one measurement with M, mfsr_tone_fit, and the table is copied to lutDev (ap->toneSize + 1 floats of device
 *      memory, 4-byte aligned, the caller's: it must stay valid as mfsr_render.toneLut must).  Else render->toneLut / toneSize
 *      stay as given;
 *   5. *render (in: format, the optional matrix and table, reserved; out: as installed) is installed exactly as
 *      mfsr_burst_set_render would install it (same checks), and *res reports the outcome.
 * statsDev: MFSR_IMAGE_STATS_WORDS uint64_t of device memory, 8-byte aligned.  ap NULL = mfsr_auto_defaults.  The driver waits
 * for the stream after every measurement (the fits run on the host): it is not capturable, like mfsr_burst_calibrate_noise; the
 * host staging is the burst's own.  The description stays installed for the following bursts until mfsr_burst_set_render
 * replaces it or turns it off.  Not for host-memory bursts (mfsr_burst_finish_host, mfsr_burst_process_source: their bands
 * finish before the accumulators are complete), frame streams, the joint mode or the multi-GPU layer. */
int mfsr_burst_auto_render(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights, const mfsr_auto_params* ap,
                           uint64_t* statsDev, float* lutDev, mfsr_render* render, mfsr_auto_result* res, mfsr_stream_t stream);

/* ---- local tone mapping in the finish: a bilateral grid of gains over (x, y, luma).  One global tone
 * curve can only spend the dynamic range of a merged burst by flattening the whole image; a gain that depends on where the pixel
 * is and how bright its surroundings are lifts shadows locally and keeps local contrast.  Three stages: exact integer statistics
 * per grid entry on the device, the gains fitted on the host, and a trilinear lookup of the gain per pixel inside the rendered
 * finish.  Nothing here runs unless it is called; without a description every entry point produces the bits it produced before.
 * THE GRID belongs to the FULL frame, fullWidth x fullHeight: GX = cdiv(fullWidth, C), GY = cdiv(fullHeight, C), GZ = NZ
 * (mfsr_local_tone_grid).  Every launch carries colOffset / rowOffset of its pixel (0, 0) in the full frame, as every finish
 * does, so that stripes and windows add up to (statistics) or are the crop of (slice) the whole-frame launch.
 * mfsr_local_tone_validate: anything out of the ranges below, or not finite, is MFSR_E_INVALID.  mfsr_local_tone_defaults: cell =
 * the smallest power of two >= 16 with cdiv(max(w, h), cell) <= 128, bins 16, smooth 1, shadows 0.5, highlights 0.25, pivot 0
 * (measured), maxGain 4. */
typedef struct {
    int32_t cell;        /* C: HR pixels per grid cell, a power of two, 16..512 */
    int32_t bins;        /* NZ: luma bins, 4, 8, 16 or 32 */
    int32_t smooth;      /* passes of the [1 2 1]/4 blur along x, y and luma, 0..4 */
    float shadows;       /* 0..1: exponent below the pivot; 0 = leave shadows */
    float highlights;    /* 0..1: exponent above the pivot; 0 = leave highlights */
    float pivot;         /* linear luma in (0, 1]; 0 = measured (log-average) */
    float maxGain;       /* 1..64: gains are clamped to [1/maxGain, maxGain] */
    int32_t reserved[4]; /* zeros */
} mfsr_local_tone;
int mfsr_local_tone_validate(const mfsr_local_tone* lt);
int mfsr_local_tone_defaults(int w, int h, mfsr_local_tone* lt);
int mfsr_local_tone_grid(int fullWidth, int fullHeight, const mfsr_local_tone* lt, int* gx, int* gy, int* gz);
/* 1. THE STATISTICS (device, exact).  For a pixel at full-frame position (X, Y), p and q as for mfsr_imageStats (q = the matrix
 * applied to p when `matrix` is not NULL: nine host floats, row-major, finite, |m| <= 256), the codes c_k and the luma key
 *   key = (54 c_0 + 183 c_1 + 19 c_2 + 128) >> 8                                                  (0 .. 4095)
 * of mfsr_imageStats: the pixel adds 1 to count[Y / C][X / C][(key NZ) >> 12] and key to sum[...] of the same entry.  The table
 * has 2 GX GY NZ uint64_t words of device memory (8-byte aligned): entries in the order y, x, luma (luma fastest), the two words
 * of an entry adjacent, count first.  A launch ADDS to the table and the caller zeroes it, so stripes and windows add up to the
 * whole image's table exactly, for any launch shape.  mfsr_toneGridStats measures a float image, mfsr_finishToneGridStats the
 * accumulators of a burst with the arguments of mfsr_finishStats.  w h < 2^31; every argument is checked on the host before any
 * device call.  Asynchronous on `stream`, nothing is allocated: capturable. */
int mfsr_toneGridStats(const mfsr_float3* in, int inRowBytes, int w, int h, int colOffset, int rowOffset, int fullWidth,
                       int fullHeight, const float* matrix, const mfsr_local_tone* lt, uint64_t* statsDev, mfsr_stream_t stream);
int mfsr_finishToneGridStats(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                             int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, int w, int h, float threshold,
                             int colOffset, int rowOffset, int fullWidth, int fullHeight, const float* matrix,
                             const mfsr_local_tone* lt, uint64_t* statsDev, mfsr_stream_t stream);
/* 2. THE FIT (host only, no device call, doubles; the table as a HOST array, the grid as GX GY NZ host floats, luma fastest, then
 * x, then y).  N = counts, S = sums as doubles.
 *   a. `smooth` passes, each [1 2 1] / 4 with replicated borders, ((lo + 2 c) + hi) * 0.25, along x, then y, then luma, on N
 *      and on S;
 *   b. base B = N > 0 ? S / (4095 N) : (k + 0.5) / NZ, floored at 1 / 4095;
 *   c. pivot = lt->pivot if > 0, else exp(sum n ln(max(s / (4095 n), 1 / 4095)) / sum n) over the UNSMOOTHED entries with
 *      n > 0, in the table's order; an empty table: *status = 1 and pivot 0.18 (else *status = 0);
 *   d. r = B / pivot; g = r < 1 ? pow(r, -shadows) : pow(r, -highlights), clamped to [1 / maxGain, maxGain], rounded to float.
 * shadows = highlights = 0 gives exactly 1.0f everywhere.  *pivotUsed (may be NULL) = the pivot. */
int mfsr_local_tone_fit(const uint64_t* statsHost, int fullWidth, int fullHeight, const mfsr_local_tone* lt, float* gridHost,
                        double* pivotUsed, int32_t* status);
/* 3. THE SLICE (device).  mfsr_localToneImage / mfsr_finishLocalTone: mfsr_renderImage / mfsr_finishRendered with the gain of
 * the grid applied to the pixel before step 1 of the rendered output.  For a pixel of value p at full-frame (X, Y), all in
 * float32, one rounding per operation, in the order written:
 *   a. q = matrix applied to p (render->useMatrix), else p; v_k = isnan(q_k) ? 0 : min(max(q_k, 0), 1);
 *      l = ((54 v_0 + 183 v_1) + 19 v_2) * (1 / 256);
 *   b. fx = (X + 0.5f) * (1 / C) - 0.5f clamped to [0, GX - 1]; i0 = (int)fx, i1 = min(i0 + 1, GX - 1), ax = fx - i0; fy, j0,
 *      j1, ay likewise with Y and GY; fz = l NZ - 0.5f clamped to [0, NZ - 1], k0, k1, az;
 *   c. at each of the four (y, x) corners a + (b - a) az with a, b the gains at k0, k1; the same expression along x for the
 *      rows j0 and j1; then along y: the gain g;
 *   d. o_k = p_k g, the same g for the three channels (hue is kept), and o takes the place of p in steps 1-3 of the rendered
 *      output.  A NaN stays a NaN and is quantised to 0 as before.
 * gridDev: GX GY NZ floats of device memory, 4-byte aligned, read only.  The four single-plane formats; the two-plane formats
 * are refused.  The image form may run in place (outImg == in).  The tone table is staged as mfsr_renderImage stages it; the
 * corner columns of the grid a workgroup's tile touches are staged in LDS or read through the cache (MFSR_LOCAL_TONE_GRID = lds |
 * cache forces one; both give the same bits).  Asynchronous on `stream`, nothing is allocated: capturable. */
int mfsr_localToneImage(const mfsr_float3* in, int inRowBytes, mfsr_float3* outImg, int outImgRowBytes, void* out, int outRowBytes,
                        int w, int h, const mfsr_render* render, int applyGamma, const float* gridDev, const mfsr_local_tone* lt,
                        int colOffset, int rowOffset, int fullWidth, int fullHeight, mfsr_stream_t stream);
int mfsr_finishLocalTone(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                         int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, mfsr_float3* outImg,
                         int outImgRowBytes, void* out, int outRowBytes, const mfsr_render* render, int w, int h, float threshold,
                         int applyGamma, int colOffset, int rowOffset, int fullWidth, int fullHeight, const float* gridDev,
                         const mfsr_local_tone* lt, mfsr_stream_t stream);
/* 4. BURSTS.  mfsr_burst_set_local_tone installs a grid (device memory of the caller's, GX GY NZ floats of the FULL HR frame,
 * valid while installed); NULL switches it off.  Between bursts only, as mfsr_burst_set_render.  With one installed every finish
 * of the burst (mfsr_burst_finish, mfsr_burst_finish_rows; a stripe is the crop) goes through mfsr_finishLocalTone, whatever
 * cfg.fused is; without a render description it renders {MFSR_OUT_RGB16, no matrix, no table}.  Refused (MFSR_E_INVALID): a handle
 * with cfg.uploadRing (its bands finish before the accumulators are complete), together with a sharpen or a denoise description
 * that is on, or with a two-plane format -- whichever setter comes second is refused.  Frame streams and the multi-GPU layer never
 * set one.
 * mfsr_burst_local_tone: after the last mfsr_burst_add_frame and before mfsr_burst_finish.  It fuses the frames still waiting,
 * zeroes statsDev (2 GX GY NZ uint64_t, 8-byte aligned), measures the accumulators with mfsr_finishToneGridStats, the finish's
 * own arguments and the burst's current matrix (so after mfsr_burst_auto_render: the matrix it installed), downloads, runs
 * mfsr_local_tone_fit, uploads the grid to gridDev and installs it.  lt NULL = mfsr_local_tone_defaults of the HR frame.  With a
 * zoom window the grid is still the full frame's, filled from the window's pixels only: entries the window does not reach hold
 * the gain of their bin's centre.  Waits for the stream (the fit runs on the host): not capturable. */
typedef struct {
    double pivot;        /* the pivot the fit used */
    int32_t status;      /* as mfsr_local_tone_fit */
    int32_t reserved;
    float minGain, maxGain; /* the smallest and the largest gain of the grid */
} mfsr_local_tone_result;
int mfsr_burst_set_local_tone(mfsr_burst* b, const mfsr_local_tone* lt, const float* gridDev);
int mfsr_burst_local_tone(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights, const mfsr_local_tone* lt,
                          uint64_t* statsDev, float* gridDev, mfsr_local_tone_result* res, mfsr_stream_t stream);

/* ---- the finish chain: denoise, then sharpen, then the local-tone gain, then matrix, tone and the store of ANY output format,
 * the two-plane ones included, in one launch.  Off unless asked for: a separate description; the
 * setters above keep their refusals and every other entry point produces the bits and the launches it always did.  At each
 * pixel of the launch, in this order, each stage only if it is on:
 *   1. p = the value section 2.19 calls p (a stripe or window is the crop of the whole frame)
 *   2. d = steps 1-6 of the denoise above on p (the count is the weight with the + 1 under the threshold); off: d = p
 *   3. s = steps 1-4 of the unsharp mask above on d (NaN cleaning, clamped coordinates, coring); off: s = d
 *   4. t = s * g, g the trilinear gain of section 2.25 looked up with the luma key of s (through the matrix when the render
 *      description has one) at the pixel's place in the full frame; off: t = s
 *   5. t takes the place of p in the rendered output: matrix, tone and store of the four single-plane formats, or the Y'CbCr and
 *      the 2 x 2 chroma mean of MFSR_OUT_NV12 / MFSR_OUT_P010
 * A stage's stencil at a position outside the valid pixels takes that stage's value at the clamped position: the sharpen reads
 * the DENOISED value of the clamped pixel.  So the result equals, bit for bit, mfsr_finishDenoised to a float image ({no
 * matrix, no table}, applyGamma 0), then mfsr_sharpenImage to a float image likewise, then mfsr_localToneImage,
 * mfsr_renderImage or mfsr_renderImageYuv with the real render description.  The cleaning is that of the first stage that is
 * on.  A stage is off with radius 0 or strength / amount 0 (local tone: useLocalTone 0); its description must still be a valid
 * one (mfsr_denoise_defaults, mfsr_local_tone_defaults; a zero-filled mfsr_sharpen is valid).
 * mfsr_finish_chain_validate: the three descriptions' own validators, useLocalTone 0 or 1, reserved zero-filled.
 * mfsr_finish_chain_reach: *rows = R_d + R_s, a stage that is off counting 0 (at most 7): the rows beyond its own that a launch
 * reads.  mfsr_chain_tile: the output tile one workgroup owns. */
typedef struct {
    mfsr_denoise denoise;
    mfsr_sharpen sharpen;
    mfsr_local_tone localTone;
    int32_t useLocalTone;  /* 1: stage 4 is on and a grid is given */
    int32_t reserved[7];   /* zeros */
} mfsr_finish_chain;
int mfsr_finish_chain_validate(const mfsr_finish_chain* chain);
int mfsr_finish_chain_reach(const mfsr_finish_chain* chain, int* rows);
int mfsr_chain_tile(int* tileW, int* tileH);
/* mfsr_chainImage: steps 2-5 on an existing float image (p = in); the valid extent is the image.  count as for
 * mfsr_denoiseImage (NULL: n = 1 everywhere; read only when the denoise stage is on).  The image is the rectangle at (colOffset,
 * rowOffset) of the fullWidth x fullHeight frame the grid belongs to (used by stage 4 only, always checked).
 * mfsr_finishChain: mfsr_finishRendered with steps 2-4 in the same launch.  Columns are valid in [0, w), rows in [-rowsAbove,
 * h + rowsBelow) relative to the launch's first row, as for the two stencil finishes: the accumulator and weight rows in that
 * range must be complete.  The result equals the composition run on exactly those rows, cropped; with rowsAbove / rowsBelow >=
 * min(reach, rows available) it is the crop of the whole frame's.
 * Outputs: outImg (the float image the integers quantise) and / or the integer output.  Single-plane formats: out / outRowBytes,
 * outUV NULL.  Two-plane formats: out is the Y plane, outUV the chroma plane (h / 2 rows uvRowBytes apart), both or neither, w
 * and h even.  render NULL = {MFSR_OUT_RGB16, no matrix, no table}.  gridDev: the grid of gains (GX GY NZ floats of the full
 * frame, 4-byte aligned), non-NULL if and only if useLocalTone.  Refused (MFSR_E_INVALID), on the host and before any device
 * call: a description with every stage off; an output -- the chroma plane included -- that overlaps the rows read (a stencil
 * cannot run in place); rowsAbove / rowsBelow outside the full frame.  A wave whose positions all have lambda == 0 skips the
 * denoise stencil.  Asynchronous on `stream`; nothing is allocated. */
int mfsr_chainImage(const mfsr_float3* in, int inRowBytes, const mfsr_float3* count, int countRowBytes, mfsr_float3* outImg,
                    int outImgRowBytes, void* out, int outRowBytes, void* outUV, int uvRowBytes, int w, int h,
                    const mfsr_render* render, int applyGamma, const mfsr_finish_chain* chain, const float* gridDev, int colOffset,
                    int rowOffset, int fullWidth, int fullHeight, mfsr_stream_t stream);
int mfsr_finishChain(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                     int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, mfsr_float3* outImg,
                     int outImgRowBytes, void* out, int outRowBytes, void* outUV, int uvRowBytes, const mfsr_render* render, int w,
                     int h, float threshold, int applyGamma, int colOffset, int rowOffset, int fullWidth, int fullHeight,
                     const mfsr_finish_chain* chain, const float* gridDev, int rowsAbove, int rowsBelow, mfsr_stream_t stream);
/* The burst's chain (copied; gridDev: the caller's device memory, valid while installed).  NULL, or a chain with every stage
 * off, removes it.  Between bursts only, as mfsr_burst_set_render.  With one installed every finish of the burst goes through
 * mfsr_finishChain; a chain with a stencil stage is a stencil finish of reach R_d + R_s (mfsr_burst_finish_rows, the lagged host
 * bands, streams), and mfsr_burst_set_render accepts the two-plane formats (even extents as ever).  Refused (MFSR_E_INVALID; a
 * refused call changes nothing): while mfsr_burst_set_sharpen, _denoise or _local_tone has a description on, and those three
 * with a description that is on while a chain is installed; useLocalTone on a handle with cfg.uploadRing (its bands finish
 * before the grid can be measured).  The grid is measured as ever (mfsr_finishToneGridStats on p, mfsr_local_tone_fit): before
 * the denoise and the sharpen. */
int mfsr_burst_set_finish_chain(mfsr_burst* b, const mfsr_finish_chain* chain, const float* gridDev);
int mfsr_stream_set_finish_chain(mfsr_stream* s, const mfsr_finish_chain* chain, const float* gridDev);
/* *finishes = the launches of mfsr_finishChain this burst has made since mfsr_burst_begin (as mfsr_burst_debug_denoised) */
int mfsr_burst_debug_chained(const mfsr_burst* b, int* finishes);

/* ---- the geometric finish: any output size, lens distortion and lateral chromatic aberration as ONE resample of the value the
 * finish holds.  Off unless asked for: its own entry points; every other entry point produces the bits
 * and the launches it always did.  All arithmetic is float32 with one rounding per operation and no contraction, in exactly the
 * order written.  For pixel (X, Y) of the FULL outW x outH output (a launch on a sub-rectangle adds its colOffset / rowOffset
 * first, so a crop is the crop bit for bit) of a source of srcW x srcH pixels:
 *   dx  = (((float)X + 0.5f) - ocx) * stepX          dy likewise with ocy, stepY
 *   rho = (dx*dx + dy*dy) * rnorm2
 *   per channel c, with (k0, k1, k2, k3) = k[c]:
 *     m = ((k3*rho + k2)*rho + k1)*rho + k0
 *     u = (scx + dx*m) - 0.5f ;  u = fminf(fmaxf(u, -1.0f), (float)srcW)      v likewise with scy, dy, srcH
 *     ix = (int)floorf(u) ;  fx = u - (float)ix                                iy, fy likewise
 *     s(i, j) = channel c of p at (clamp(i, 0, srcW-1), clamp(j, 0, srcH-1)),  NaN -> 0
 *     bilinear: h_j = s(ix, j) + (s(ix+1, j) - s(ix, j)) * fx,  j = iy, iy+1 ;  o = h_iy + (h_iy+1 - h_iy) * fy
 *     cubic (Catmull-Rom), the weights of f = fx (w) and of f = fy (wy):
 *               w0 = ((-0.5f*f + 1.0f)*f - 0.5f)*f     w1 = ((1.5f*f - 2.5f)*f)*f + 1.0f
 *               w2 = ((-1.5f*f + 2.0f)*f + 0.5f)*f     w3 = ((0.5f*f - 0.5f)*f)*f
 *               h_j = (w0*s(ix-1,j) + w1*s(ix,j)) + (w2*s(ix+1,j) + w3*s(ix+2,j)),  j = iy-1 .. iy+2
 *               o = (wy0*h_(iy-1) + wy1*h_iy) + (wy2*h_(iy+1) + wy3*h_(iy+2))
 * p is the value section 2.19 calls p (after ApplyWeighting with the fallback, before gamma) at the SOURCE pixel's own
 * coordinates in the full HR frame: the fallback resample of a low-weight source pixel is the one every other finish computes.
 * o takes the place of p in steps 1-3 of the rendered output (matrix, tone, quantise); with no render description the steps are
 * those of {MFSR_OUT_RGB16, no matrix, no table}.  The mapping has no square root and no division: the polynomial is in rho =
 * r^2.  The coefficients are those of the usual FORWARD lens model (ideal -> distorted), which is also the direction a correcting
 * resample needs (output -> source): a lens profile's numbers are passed as they are.  Borders replicate.  There is NO
 * anti-alias prefilter: steps above 1 alias as any plain bilinear / bicubic does.  An inf among the taps is not cleaned (a
 * weight of 0 times inf is NaN, as in the sharpen); the quantiser maps NaN to 0 and clamps inf as ever.
 * mfsr_geometry_validate refuses (MFSR_E_INVALID, host only): extents outside 1 .. 32768, an unknown filter, any non-finite
 * float, steps outside [1/8, 8], rnorm2 <= 0 or > 4 (a normalising radius under half a pixel), |k0 - 1| > 0.25, |k1|, |k2|,
 * |k3| > 4, a centre outside [-extent, 2 extent] (ocx against outW, scx against srcW <= 32768: the source extent is known at
 * the launch, which checks scx / scy; validate alone bounds them by [-32768, 65536]), non-zero reserved.
 * With these bounds no NaN and no integer overflow can arise in the mapping: |X + 0.5 - ocx| <= 2^16, so |dx| <= 2^19 and
 * rho <= 2^39 * 4 = 2^41; |m| <= 4 * 2^123 + 4 * 2^82 + 4 * 2^41 + 1.25 < 2^126 is finite, so dx * m is never 0 * inf; it may
 * overflow to +-inf for such extreme values, scx + (+-inf) and the subtraction keep it, and the clamp maps it to srcW or -1 (a
 * border pixel).  After the clamp u lies in [-1, srcW] with srcW <= 32768: ix lies in [-1, srcW], u - (float)ix is exact and
 * lies in [0, 1).
 * mfsr_geometry_lens (host only) fills a description from a lens profile, computing in double and rounding once: centres at
 * the two image centres (dstW/2, dstH/2, srcW/2, srcH/2; outW x outH = dstW x dstH), stepX = stepY = min(srcW/dstW,
 * srcH/dstH) / zoom, rnorm2 = 1 / ((srcW/2)^2 + (srcH/2)^2), k1 .. k3 = k[0 .. 2] for the three channels, k0 = (lateral[0], 1, lateral[1]); the result is
 * validated.  mfsr_geometry_defaults: the identity (outW x outH = srcW x srcH, step 1, k0 = 1, cubic).
 * mfsr_geometry_tile: the output tile one workgroup owns and the capacity of its LDS stage in source pixels (see DESIGN.md
 * section 5: a workgroup whose exact box of source taps fits the stage evaluates p once per source pixel into LDS; one whose box
 * does not reads every tap from memory and produces the same bits; MFSR_GEOMETRY_STAGE=0, read at every call, forces the latter
 * everywhere). */
#define MFSR_GEO_BILINEAR 0
#define MFSR_GEO_CUBIC 1
typedef struct {
    int32_t outW, outH;   /* the full output extent, 1 .. 32768 each */
    int32_t filter;       /* MFSR_GEO_BILINEAR or MFSR_GEO_CUBIC */
    float ocx, ocy;       /* optical centre in output coordinates (pixel X covers [X, X+1)) */
    float scx, scy;       /* optical centre in source (HR accumulator) coordinates */
    float stepX, stepY;   /* source pixels per output pixel at the centre, [1/8, 8] */
    float rnorm2;         /* 1 / (normalising radius in source pixels)^2, (0, 4] */
    float k[3][4];        /* per channel: k0 (lateral magnification; 1 for green), k1, k2, k3 */
    int32_t reserved[10]; /* zeros */
} mfsr_geometry;
int mfsr_geometry_validate(const mfsr_geometry* geometry);
int mfsr_geometry_defaults(int srcW, int srcH, mfsr_geometry* out);
int mfsr_geometry_lens(int srcW, int srcH, int dstW, int dstH, double zoom, const double k[3], const double lateral[2], int filter,
                       mfsr_geometry* out);
int mfsr_geometry_tile(int* tileW, int* tileH, int* stageW, int* stageH);
/* mfsr_finishGeometry: the arguments of mfsr_finishRendered for the accumulator pair, the fallback, u0 .. v1, threshold and
 * applyGamma; finalImg / weight are the FULL HR frame of srcW x srcH pixels.  The launch writes the rectangle (colOffset,
 * rowOffset, w, h) of the outW x outH output to outImg (the float image the integers quantise) and / or out (the format's
 * integers), whose pixel (0, 0) is the rectangle's first.  render may be NULL.  Not in place: no output may overlap the
 * accumulators or the weights.  mfsr_geometryImage: the same on an existing float image (s = NaN-cleaned `in`); no output may
 * overlap `in`.  Both check every argument on the host before any device call (MFSR_E_INVALID), allocate nothing, are
 * asynchronous on `stream` (capturable) and refuse the two-plane formats.  The other stages combine with it at the image level,
 * in this order: mfsr_finishChain (or mfsr_finishDenoised / mfsr_finishSharpened) to a float image with {no matrix, no table},
 * then mfsr_geometryImage with the real render description. */
int mfsr_finishGeometry(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                        int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, int srcW, int srcH,
                        mfsr_float3* outImg, int outImgRowBytes, void* out, int outRowBytes, const mfsr_render* render,
                        const mfsr_geometry* geometry, float threshold, int applyGamma, int colOffset, int rowOffset, int w, int h,
                        mfsr_stream_t stream);
int mfsr_geometryImage(const mfsr_float3* in, int inRowBytes, int srcW, int srcH, mfsr_float3* outImg, int outImgRowBytes, void* out,
                       int outRowBytes, const mfsr_render* render, const mfsr_geometry* geometry, int applyGamma, int colOffset,
                       int rowOffset, int w, int h, mfsr_stream_t stream);
/* The geometric finish of a burst: fuses whatever is waiting, as mfsr_burst_finish does, then runs ONE mfsr_finishGeometry over
 * the whole outW x outH output with the burst's render description (or plainly), cfg.weightThreshold and cfg.applyGamma.  outImg
 * (12 * outW bytes a row at least) and / or out (the format's rows; uint16_t RGB without a render description).  An explicit
 * call, not a mode: the burst's own output extent and every other finish stay as they are (mfsr_burst_finish may follow and
 * gives what it always gave), and the finish inside the burst launch is never taken by it.  Refused (MFSR_E_INVALID, before any
 * work; the burst stays usable): a burst with a window; an installed sharpen, denoise, local-tone or chain description; a
 * two-plane render format.  mfsr_burst_debug_geometry: its launches since mfsr_burst_begin. */
int mfsr_burst_finish_geometry(mfsr_burst* b, const mfsr_float3* imgOut, const mfsr_float3* totalWeights, const mfsr_geometry* geometry,
                               mfsr_float3* outImg, int outImgRowBytes, void* out, int outRowBytes, mfsr_stream_t stream);
int mfsr_burst_debug_geometry(const mfsr_burst* b, int* finishes);

/* HIP-event timing of the warp+fuse (accumulate) launches made by add_frame on
 * the caller's stream: timing(b,1) starts a series, timing_read synchronises with
 * the events and returns the summed kernel milliseconds, the launch count and the
 * number of frames those launches fused (2 per launch with pairFrames).  A burst launch of the
 * burst hold (mfsr_burst_hold_fuse) counts as one launch per group it fused, so that
 * totalMs / launches stays the time per group of mfsr_burst_group_size frames.  Where mfsr_burst_finish takes the finish
 * inside that launch (see there), the events around it include the finish: the tile launch's epilogue and the ring launch. */
int mfsr_burst_timing(mfsr_burst* b, int enable);
int mfsr_burst_timing_read(mfsr_burst* b, double* totalMs, int* launches, int* frames);
/* last per-frame flow field (tracking resolution, raw-pixel units) and mask,
 * for tests: returns device pointers valid until the next add_frame.  With frame-batched alignment a frame is aligned
 * when its group is complete (or on mfsr_burst_flush / finish): while the last frame is still waiting, asking for its
 * flow / mask returns MFSR_E_INVALID (never the previous frame's buffers) -- flush first. */
int mfsr_burst_debug_views(mfsr_burst* b, mfsr_tex2d* flow, mfsr_tex2d* mask, mfsr_tex2d* kernelParam,
                           mfsr_tex2d* tracking);
/* products of the frame aligned `framesBack` frames before the last one (0 = the last: what mfsr_burst_debug_views gives).
 * Valid while framesBack < 2 * MFSR_MAX_FUSE_GROUP (the ring of per-frame slots) and the burst has aligned that many;
 * MFSR_E_INVALID for a frame that is still waiting for its group (see above). */
int mfsr_burst_debug_frame_views(mfsr_burst* b, int framesBack, mfsr_tex2d* flow, mfsr_tex2d* mask);
/* Which of the driver's branches a burst took, for tests: plain host-side counters the burst driver increments where it
 * chooses a kernel (csrc/pipeline.cpp), zeroed by mfsr_burst_create and mfsr_burst_begin.  They count LAUNCHES unless noted
 * (a batched launch over several frames counts once), add no device work and read no environment variable.  A frame-batched
 * group is counted when it is aligned (group complete, flush or finish), so read them after mfsr_burst_flush / finish. */
typedef enum {
    MFSR_PATH_PREPARE_FUSED = 0,   /* A1 + tracking pyramid: mfsr_prepareFrameFused (reference and moved frames) */
    MFSR_PATH_PREPARE_CHAIN,       /* ... the kernel chain (monochrome, more than 17 prefilter taps, cfg.fused = 0) */
    MFSR_PATH_PREPARE_BATCH,       /* ... mfsr_prepareFrameFusedBatch, one launch per aligned group */
    MFSR_PATH_TRACK_FUSED_UP,      /* tile tracker, one per pyramid level: mfsr_trackTilesFusedUp (levels above the coarsest) */
    MFSR_PATH_TRACK_FUSED_BASE,    /* ... mfsr_trackTilesFusedBase (the coarsest level) */
    MFSR_PATH_TRACK_FUSED_BATCH,   /* ... mfsr_trackTilesFusedBatch, one launch per level and aligned group */
    MFSR_PATH_TRACK_CHAIN,         /* ... the reference's kernel chain (cfg.fused = 0) */
    MFSR_PATH_TRACK_FAST_PAIR,     /* tracker launches (any of the four above) whose (tileSize, maxShift) is a pair of the
                                      compile-time kernel, mfsr_trackTilesFastSupported */
    MFSR_PATH_TRACK_GENERIC_PAIR,  /* ... and those whose pair is not: the fused forms then run the generic LDS tracker */
    MFSR_PATH_FLOW_WARPED,         /* flow field: mfsr_CreateFlowFieldWarped (flow + first warp) */
    MFSR_PATH_FLOW_WARPED_BATCH,   /* ... mfsr_CreateFlowFieldWarpedBatch, one launch per aligned group */
    MFSR_PATH_FLOW_BASE,           /* ... mfsr_CreateFlowFieldFromTilesBase (cfg.preAlign off the warped path) */
    MFSR_PATH_FLOW_PLAIN,          /* ... mfsr_CreateFlowFieldFromTiles */
    MFSR_PATH_LK_SWEEP_BATCH,      /* Lucas-Kanade iteration: mfsr_lucasKanadeSweepBatch over an aligned group */
    MFSR_PATH_LK_SWEEP_SINGLE,     /* ... mfsr_lucasKanadeSweepBatch of one frame */
    MFSR_PATH_LK_ITERATION_WARPED, /* ... mfsr_lucasKanadeIterationWarped (half windows the sweep refuses) */
    MFSR_PATH_LK_ITERATION_FUSED,  /* ... mfsr_lucasKanadeIterationFused (off the warped path) */
    MFSR_PATH_LK_CHAIN,            /* ... warp + derivatives + mfsr_lucasKanadeOptim (cfg.fused = 0) */
    MFSR_PATH_SCALE_FLOW,          /* separate mfsr_scaleFlow passes */
    MFSR_PATH_FRAMES_DEFERRED,     /* FRAMES (the reference included) registered for the frame-batched alignment */
    MFSR_PATH_FRAMES_IMMEDIATE,    /* FRAMES aligned by the call that added them */
    MFSR_PATH_ALIGN_BATCHES,       /* groups aligned as one batch */
    MFSR_PATH_STAGE_BATCHES,       /* ... of them, groups whose per-frame stages ran as batched launches too */
    MFSR_PATH_ROBUST_FUSED,        /* robustness mask: mfsr_robustnessMaskFused */
    MFSR_PATH_ROBUST_BATCH,        /* ... mfsr_robustnessMaskFusedBatch, one launch per aligned group */
    MFSR_PATH_ROBUST_CHAIN,        /* ... mfsr_zeroRing_f32x4 + mfsr_ComputeRobustnessMask (cfg.fused = 0) */
    MFSR_PATH_REF_FIELD_FUSED,     /* reference's kernel-shape field: mfsr_kernelParamField (else the five-kernel chain) */
    MFSR_PATH_COUNT
} mfsr_path;
/* copies min(capacity, MFSR_PATH_COUNT) counters into counts[] (indexed by mfsr_path) and stores MFSR_PATH_COUNT in *count;
 * host memory only, no device call, no synchronisation */
int mfsr_burst_debug_paths(const mfsr_burst* b, int32_t* counts, int capacity, int* count);
/* global pre-alignment of the last add_frame (cfg.preAlign), copied to HOST memory; aligns a frame that is still waiting
 * for its group first, then synchronises the stream */
int mfsr_burst_prealign_result(mfsr_burst* b, mfsr_prealign* hostOut, mfsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MFSR_H */
