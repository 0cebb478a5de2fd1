// half_pixel.hpp -- the half-resolution pixel of a raw quad (A1) and the exact small divisions of the 3 x 3 patch means:
// what debayer.hip (prepare kernels) and robustness.hip (mask kernels) must compute with one definition, because the
// patch means of the moved image are made by either and compared bit for bit.
#pragma once

#include "common.hpp"

// x / 9 and x / 3 as reciprocal multiply + one fma correction (3 instructions instead of the ~11 of the
// IEEE division expansion): q = x*r, q' = fma(fma(-d, q, x), r, q) with r = RN(1/d).  For d = 9 and
// d = 3 this equals the correctly rounded quotient for EVERY finite float x, checked exhaustively over
// all bit patterns on the host (it does not for 12 or sqrt(2), which keep the division).
__device__ __forceinline__ float div9(float x)
{
    const float q = x * 0.111111112f;
    return __builtin_fmaf(__builtin_fmaf(-9.0f, q, x), 0.111111112f, q);
}
__device__ __forceinline__ float div3(float x)
{
    const float q = x * 0.333333343f;
    return __builtin_fmaf(__builtin_fmaf(-3.0f, q, x), 0.333333343f, q);
}

// deBayersSubSample3 (DeBayerKernels.cu:244-283) of the quad at half-resolution (x, y): dataIn is the dense raw frame of
// 2 * dimX samples per row, factor = 1 / maxVal
__device__ __forceinline__ pix3 a1_pixel(const uint16_t* __restrict__ dataIn, int dimX, int x, int y, float factor, int cfa)
{
    const size_t rowElems = (size_t)dimX * 2;
    const uint32_t top = *(const uint32_t*)(dataIn + (size_t)(2 * y) * rowElems + 2 * x);
    const uint32_t bot = *(const uint32_t*)(dataIn + (size_t)(2 * y + 1) * rowElems + 2 * x);
    const float raw[2][2] = {{(float)(top & 0xffffu), (float)(top >> 16)}, {(float)(bot & 0xffffu), (float)(bot >> 16)}};
    pix3 pixel = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ix = 0; ix < 2; ix++) {
#pragma unroll
        for (int iy = 0; iy < 2; iy++) {
            const int c = cfa_at(cfa, iy, ix);
            const float v = raw[iy][ix] * factor;
            if (c == MFSR_GREEN)
                pixel.y += v * 0.5f;
            else if (c == MFSR_RED)
                pixel.x = v;
            else if (c == MFSR_BLUE)
                pixel.z = v;
        }
    }
    return pixel;
}
