// yuv_common.hpp -- the two-plane 4:2:0 store of the rendered finish: Y'CbCr, the 2 x 2 chroma mean and
// the NV12 / P010 stores of a lane's 2 x 4 block, and the host's constants and plane checks.  Shared by render_yuv.hip
// (k_renderImageYuv, k_finishRenderedYuv) and finish_chain.hip (k_chainImage, k_finishChain): one definition, so that a chain to
// a two-plane format stores what the rendered finish stores.  Every step is float32 + - * with -ffp-contract=off (the Makefile),
// so the numpy float32 restatement (tests/yuv_ref.py) is bit-exact; the pixel up to the tone curve is render_pixel's.
#pragma once

#include "render_common.hpp"

namespace {

struct YuvArgs {
    float kr, kg, kb, sb, sr;  // Y = (kr c0 + kg c1) + kb c2;  Cb = (c2 - Y) sb;  Cr = (c0 - Y) sr
    float yOff, yScale;        // yq = yOff + yScale * Y
    float cOff, cScale;        // cq = cOff + cScale * C
    float maxCode;             // 2^N - 1
};

__device__ __forceinline__ float unit_clamp(float o) { return isnan(o) ? 0.0f : fminf(fmaxf(o, 0.0f), 1.0f); }

__device__ __forceinline__ uint32_t yuv_code(float v, float maxCode) { return (uint32_t)(int)(fminf(fmaxf(v, 0.0f), maxCode) + 0.5f); }

// `n` (2 or 4) samples of codes q[] at `dst`: one wide store when the lane has all four and `wide` (the row's first sample is
// aligned to the store: uniform per row), else sample by sample.  P010 words carry the code in bits 15..6.
template <int BITS>
__device__ __forceinline__ void store_samples(uint8_t* dst, const uint32_t q[4], int n, bool wide)
{
    if constexpr (BITS == 8) {
        if (n == 4 && wide) {
            *(uint32_t*)dst = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < n) dst[k] = (uint8_t)q[k];
        }
    } else {
        uint16_t* d16 = (uint16_t*)dst;
        if (n == 4 && wide) {
            uint2 v;
            v.x = q[0] << 6 | q[1] << 22;
            v.y = q[2] << 6 | q[3] << 22;
            *(uint2*)dst = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < n) d16[k] = (uint16_t)(q[k] << 6);
        }
    }
}

// The 2 x 4 block with top-left pixel (x0, 2 * yPair) of the launch: src(k, row) is the value before step 1 of section 2.19 at
// column k (0..3) and row (0..1) OF THE BLOCK -- block-relative, so that a caller that holds the block in registers indexes them
// with constants.  width and height are even, so the block holds 2 or 4 whole columns and both rows.  src(k, row) is read
// before outImg's pixel is written and no other lane touches it: in place is fine.
template <int BITS, class Src>
__device__ __forceinline__ void yuv_block(const Src& src, pix3* outImg, int outPitch, uint8_t* outY, int yRowBytes, uint8_t* outUV,
                                          int uvRowBytes, int x0, int yPair, int width, const RenderArgs& r, const YuvArgs& ya,
                                          const float* lut)
{
    constexpr int BPS = BITS == 8 ? 1 : 2;          // bytes per sample
    constexpr uintptr_t WIDE = BITS == 8 ? 3 : 7;   // alignment mask of the wide store
    const int n = width - x0 >= 4 ? 4 : 2;
    float cb[4], cr[4];  // row 0's chroma, then the 2 x 2 sums
#pragma unroll
    for (int row = 0; row < 2; row++) {
        const int y = 2 * yPair + row;
        pix3* imgRow = outImg ? row_ptr(outImg, outPitch, y) : nullptr;
        uint32_t q[4] = {0, 0, 0, 0};
        float rb[4], rr[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            rb[k] = rr[k] = 0.0f;
            if (k < n) {
                const pix3 o = render_pixel(src(k, row), r, lut);
                if (imgRow) imgRow[x0 + k] = o;
                const float c0 = unit_clamp(o.x), c1 = unit_clamp(o.y), c2 = unit_clamp(o.z);
                const float Y = (ya.kr * c0 + ya.kg * c1) + ya.kb * c2;
                rb[k] = (c2 - Y) * ya.sb;
                rr[k] = (c0 - Y) * ya.sr;
                q[k] = yuv_code(ya.yOff + ya.yScale * Y, ya.maxCode);
            }
        }
        if (outY) {
            uint8_t* yRow = outY + (size_t)yRowBytes * (size_t)y;
            store_samples<BITS>(yRow + (size_t)x0 * BPS, q, n, ((uintptr_t)yRow & WIDE) == 0);
        }
        // x first, rows second: ((C(x, y) + C(x+1, y)) + (C(x, y+1) + C(x+1, y+1))) * 0.25
        if (row == 0) {
            cb[0] = rb[0] + rb[1];
            cb[1] = rb[2] + rb[3];
            cr[0] = rr[0] + rr[1];
            cr[1] = rr[2] + rr[3];
        } else {
            cb[0] = (cb[0] + (rb[0] + rb[1])) * 0.25f;
            cb[1] = (cb[1] + (rb[2] + rb[3])) * 0.25f;
            cr[0] = (cr[0] + (rr[0] + rr[1])) * 0.25f;
            cr[1] = (cr[1] + (rr[2] + rr[3])) * 0.25f;
        }
    }
    if (!outUV) return;
    uint32_t q[4];
    q[0] = yuv_code(ya.cOff + ya.cScale * cb[0], ya.maxCode);
    q[1] = yuv_code(ya.cOff + ya.cScale * cr[0], ya.maxCode);
    q[2] = yuv_code(ya.cOff + ya.cScale * cb[1], ya.maxCode);
    q[3] = yuv_code(ya.cOff + ya.cScale * cr[1], ya.maxCode);
    // x0 / 2 (Cb, Cr) pairs = x0 samples into the chroma row
    uint8_t* uvRow = outUV + (size_t)uvRowBytes * (size_t)yPair;
    store_samples<BITS>(uvRow + (size_t)x0 * BPS, q, n, ((uintptr_t)uvRow & WIDE) == 0);
}

// the five constants are the float32 roundings of doubles; the scales are exact in float32.  A single-plane format: zeros (the
// chain passes them to kernels that never read them).
YuvArgs yuv_args(const mfsr_render* r)
{
    static const double K[3][2] = {{0.2126, 0.0722}, {0.299, 0.114}, {0.2627, 0.0593}};  // Kr, Kb: BT.709, BT.601, BT.2020
    YuvArgs a;
    memset(&a, 0, sizeof(a));
    if (!yuv_format(r->format)) return a;
    const int std_ = r->reserved[0] & 3, full = r->reserved[0] & MFSR_YUV_FULL;
    const double kr = K[std_][0], kb = K[std_][1];
    const int bits = r->format == MFSR_OUT_NV12 ? 8 : 10;
    const float m = (float)(1 << (bits - 8)), M = (float)((1 << bits) - 1);
    a.kr = (float)kr;
    a.kg = (float)(1.0 - kr - kb);
    a.kb = (float)kb;
    a.sb = (float)(0.5 / (1.0 - kb));
    a.sr = (float)(0.5 / (1.0 - kr));
    a.yOff = full ? 0.0f : 16.0f * m;
    a.yScale = full ? M : 219.0f * m;
    a.cOff = full ? (float)(1 << (bits - 1)) : 128.0f * m;
    a.cScale = full ? M : 224.0f * m;
    a.maxCode = M;
    return a;
}

// the two planes of a launch: both or neither, and the alignment and length the format's stores need
int check_planes(int format, const void* outY, int yRowBytes, const void* outUV, int uvRowBytes, int width)
{
    MFSR_REQUIRE((outY != nullptr) == (outUV != nullptr));
    if (!outY) return MFSR_OK;
    const long long rowBytes = format == MFSR_OUT_NV12 ? (long long)width : 2LL * width;
    MFSR_REQUIRE((long long)yRowBytes >= rowBytes && (long long)uvRowBytes >= rowBytes);
    if (format == MFSR_OUT_P010)
        MFSR_REQUIRE(((uintptr_t)outY & 1) == 0 && ((uintptr_t)outUV & 1) == 0 && (yRowBytes & 1) == 0 && (uvRowBytes & 1) == 0);
    return MFSR_OK;
}

}  // namespace
