// render_yuv.hip -- two-plane YUV 4:2:0 output of the rendered finish: NV12 (8-bit) and P010 (10-bit
// code in bits 15..6 of a 16-bit word), as the pixel body of its own (mfsr_renderImageYuv) and folded into the burst's finish
// (mfsr_finishRenderedYuv = H1 + fallback resample + matrix + tone + Y'CbCr + 2 x 2 chroma mean + quantise in one launch).
// gfx950, wave64.
//
// A lane owns 2 rows x 4 columns: eight pixels, 24 tone-table reads as an RGB8 lane makes, one 4-byte (NV12) or 8-byte (P010)
// store per Y row and one of chroma.  Every step is float32 + - * with -ffp-contract=off (the Makefile), so the numpy float32
// restatement (tests/yuv_ref.py) is bit-exact; the pixel up to the tone curve is render_pixel of render_common.hpp.
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

// The 2 x 4 block with top-left pixel (x0, 2 * yPair) of the launch: src(x, y) is the value before step 1 of section 2.19.
// width and height are even, so the block holds 2 or 4 whole columns and both rows.  src(x, y) is read before
// outImg's pixel (x, y) is written and no other lane touches it: in place is fine.
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
                const pix3 o = render_pixel(src(x0 + k, y), r, lut);
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

template <int BITS, int LDS>
__global__ void __launch_bounds__(LDS ? 1024 : 256)
    k_renderImageYuv(const pix3* in, int inPitch, pix3* outImg, int outPitch, uint8_t* outY, int yRowBytes, uint8_t* outUV,
                     int uvRowBytes, int width, int height, RenderArgs r, YuvArgs ya)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    const float* lut = stage_lut<LDS>(r, s_lut);
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int yPair = blockIdx.y * blockDim.y + threadIdx.y;
    if (x0 >= width || 2 * yPair >= height) return;
    yuv_block<BITS>([&](int x, int y) { return row_ptr(in, inPitch, y)[x]; }, outImg, outPitch, outY, yRowBytes, outUV, uvRowBytes,
                    x0, yPair, width, r, ya, lut);
}

template <int BITS, int LDS>
__global__ void __launch_bounds__(LDS ? 1024 : 256)
    k_finishRenderedYuv(const pix3* __restrict__ finalImg, const pix3* __restrict__ weight, int imgPitch, FinishSrc f,
                        pix3* __restrict__ outImg, int outPitch, uint8_t* __restrict__ outY, int yRowBytes,
                        uint8_t* __restrict__ outUV, int uvRowBytes, int width, int height, RenderArgs r, YuvArgs ya)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    const float* lut = stage_lut<LDS>(r, s_lut);
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int yPair = blockIdx.y * blockDim.y + threadIdx.y;
    if (x0 >= width || 2 * yPair >= height) return;
    // k_finishRendered's value up to its tone curve (finish_value: one definition; a stripe or window is the crop of the whole)
    auto src = [&](int x, int y) { return finish_value(row_ptr(finalImg, imgPitch, y)[x], row_ptr(weight, imgPitch, y)[x], x, y, f); };
    yuv_block<BITS>(src, outImg, outPitch, outY, yRowBytes, outUV, uvRowBytes, x0, yPair, width, r, ya, lut);
}

// the five constants are the float32 roundings of doubles; the scales are exact in float32
YuvArgs yuv_args(const mfsr_render* r)
{
    static const double K[3][2] = {{0.2126, 0.0722}, {0.299, 0.114}, {0.2627, 0.0593}};  // Kr, Kb: BT.709, BT.601, BT.2020
    const int std_ = r->reserved[0] & 3, full = r->reserved[0] & MFSR_YUV_FULL;
    const double kr = K[std_][0], kb = K[std_][1];
    const int bits = r->format == MFSR_OUT_NV12 ? 8 : 10;
    const float m = (float)(1 << (bits - 8)), M = (float)((1 << bits) - 1);
    YuvArgs a;
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

#define YUV_DISPATCH(KERNEL, format, lds, ...)                                                                     \
    do {                                                                                                           \
        const dim3 block(64, (lds) ? 16 : 4);                                                                      \
        const dim3 grid(mfsr_cdiv(mfsr_cdiv(w, 4), 64), mfsr_cdiv(h / 2, block.y));                                \
        if ((format) == MFSR_OUT_NV12) {                                                                           \
            if (lds)                                                                                               \
                hipLaunchKernelGGL((KERNEL<8, 1>), grid, block, 0, mfsr_s(stream), __VA_ARGS__);                   \
            else                                                                                                   \
                hipLaunchKernelGGL((KERNEL<8, 0>), grid, block, 0, mfsr_s(stream), __VA_ARGS__);                   \
        } else {                                                                                                   \
            if (lds)                                                                                               \
                hipLaunchKernelGGL((KERNEL<10, 1>), grid, block, 0, mfsr_s(stream), __VA_ARGS__);                  \
            else                                                                                                   \
                hipLaunchKernelGGL((KERNEL<10, 0>), grid, block, 0, mfsr_s(stream), __VA_ARGS__);                  \
        }                                                                                                          \
    } while (0)

extern "C" int mfsr_renderImageYuv(const mfsr_float3* in, int inRowBytes, mfsr_float3* outImg, int outImgRowBytes, void* outY,
                                   int yRowBytes, void* outUV, int uvRowBytes, int w, int h, const mfsr_render* render,
                                   int applyGamma, mfsr_stream_t stream)
{
    MFSR_REQUIRE(in && (outImg || outY || outUV) && w > 0 && h > 0 && (w & 1) == 0 && (h & 1) == 0);
    MFSR_REQUIRE((long long)inRowBytes >= 12LL * w && (inRowBytes & 3) == 0 && ((uintptr_t)in & 3) == 0);
    if (outImg) MFSR_REQUIRE((long long)outImgRowBytes >= 12LL * w && (outImgRowBytes & 3) == 0 && ((uintptr_t)outImg & 3) == 0);
    if (int rc = mfsr_render_validate(render)) return rc;
    MFSR_REQUIRE(yuv_format(render->format));
    if (int rc = check_planes(render->format, outY, yRowBytes, outUV, uvRowBytes, w)) return rc;
    const RenderArgs a = render_args(render, applyGamma);
    const YuvArgs ya = yuv_args(render);
    const bool lds = lut_in_lds(render);
    YUV_DISPATCH(k_renderImageYuv, render->format, lds, (const pix3*)in, inRowBytes, (pix3*)outImg, outImgRowBytes, (uint8_t*)outY,
                 yRowBytes, (uint8_t*)outUV, uvRowBytes, w, h, a, ya);
    return mfsr_launch_status("renderImageYuv");
}

extern "C" int mfsr_finishRenderedYuv(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes,
                                      const mfsr_float3* fallback, int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0,
                                      float v1, mfsr_float3* outImg, int outImgRowBytes, void* outY, int yRowBytes, void* outUV,
                                      int uvRowBytes, const mfsr_render* render, int w, int h, float threshold, int applyGamma,
                                      int colOffset, int rowOffset, int fullWidth, int fullHeight, mfsr_stream_t stream)
{
    if (int rc = finish_check(finalImg, weight, imgRowBytes, fallback, fbRowBytes, fbW, fbH, outImg, outImgRowBytes, outY ? outY : outUV,
                              w, h, colOffset, rowOffset, fullWidth, fullHeight))
        return rc;
    MFSR_REQUIRE((w & 1) == 0 && (h & 1) == 0);
    if (int rc = mfsr_render_validate(render)) return rc;
    MFSR_REQUIRE(yuv_format(render->format));
    if (int rc = check_planes(render->format, outY, yRowBytes, outUV, uvRowBytes, w)) return rc;
    const RenderArgs a = render_args(render, applyGamma);
    const YuvArgs ya = yuv_args(render);
    const FinishSrc f = finish_src(fallback, fbRowBytes, fbW, fbH, u0, u1, v0, v1, threshold, colOffset, rowOffset, fullWidth, fullHeight);
    const bool lds = lut_in_lds(render);
    YUV_DISPATCH(k_finishRenderedYuv, render->format, lds, (const pix3*)finalImg, (const pix3*)weight, imgRowBytes, f, (pix3*)outImg,
                 outImgRowBytes, (uint8_t*)outY, yRowBytes, (uint8_t*)outUV, uvRowBytes, w, h, a, ya);
    return mfsr_launch_status("finishRenderedYuv");
}
