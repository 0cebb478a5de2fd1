// render_yuv.hip -- two-plane YUV 4:2:0 output of the rendered finish: NV12 (8-bit) and P010 (10-bit
// code in bits 15..6 of a 16-bit word), as the pixel body of its own (mfsr_renderImageYuv) and folded into the burst's finish
// (mfsr_finishRenderedYuv = H1 + fallback resample + matrix + tone + Y'CbCr + 2 x 2 chroma mean + quantise in one launch).
// gfx950, wave64.
//
// A lane owns 2 rows x 4 columns: eight pixels, 24 tone-table reads as an RGB8 lane makes, one 4-byte (NV12) or 8-byte (P010)
// store per Y row and one of chroma.  Every step is float32 + - * with -ffp-contract=off (the Makefile), so the numpy float32
// restatement (tests/yuv_ref.py) is bit-exact; the pixel up to the tone curve is render_pixel of render_common.hpp.  The block's
// body (yuv_block) and the constants are yuv_common.hpp's, which finish_chain.hip shares.
#include "yuv_common.hpp"

namespace {

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
    auto src = [&](int k, int row) { return row_ptr(in, inPitch, 2 * yPair + row)[x0 + k]; };
    yuv_block<BITS>(src, outImg, outPitch, outY, yRowBytes, outUV, uvRowBytes, x0, yPair, width, r, ya, lut);
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
    auto src = [&](int k, int row) {
        const int x = x0 + k, y = 2 * yPair + row;
        return finish_value(row_ptr(finalImg, imgPitch, y)[x], row_ptr(weight, imgPitch, y)[x], x, y, f);
    };
    yuv_block<BITS>(src, outImg, outPitch, outY, yRowBytes, outUV, uvRowBytes, x0, yPair, width, r, ya, lut);
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
