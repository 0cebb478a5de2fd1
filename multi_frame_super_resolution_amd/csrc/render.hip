// render.hip -- the rendered finish: colour matrix, tone curve and a display-format store, as the
// pixel body of its own (mfsr_renderImage) and folded into the burst's finish (mfsr_finishRendered = H1 + fallback resample +
// matrix + tone + quantise in one launch).  gfx950, wave64.
//
// Every step is float32 + - * with -ffp-contract=off (the Makefile), so a numpy float32 restatement is bit-exact
// (tests/render_ref.py); the only inexact operation is the powf of the built-in gamma.
#include "render_common.hpp"

namespace {

template <int FORMAT, int LDS>
__global__ void __launch_bounds__(LDS ? 1024 : 256)
    k_renderImage(const pix3* in, int inPitch, pix3* outImg, int outPitch, uint8_t* out, int outRowBytes, int width, int height,
                  RenderArgs r)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    const float* lut = stage_lut<LDS>(r, s_lut);
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * Fmt<FORMAT>::ppl;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x0 >= width || y >= height) return;
    const pix3* inRow = row_ptr(in, inPitch, y);
    render_span<FORMAT>([&](int x) { return inRow[x]; }, outImg ? row_ptr(outImg, outPitch, y) : nullptr,
                        out ? out + (size_t)outRowBytes * (size_t)y : nullptr, x0, width, r, lut);
}

template <int FORMAT, int LDS>
__global__ void __launch_bounds__(LDS ? 1024 : 256)
    k_finishRendered(const pix3* __restrict__ finalImg, const pix3* __restrict__ weight, int imgPitch, FinishSrc f,
                     pix3* __restrict__ outImg, int outPitch, uint8_t* __restrict__ out, int outRowBytes, int width, int height,
                     RenderArgs r)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    const float* lut = stage_lut<LDS>(r, s_lut);
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * Fmt<FORMAT>::ppl;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x0 >= width || y >= height) return;
    const pix3* valRow = row_ptr(finalImg, imgPitch, y);
    const pix3* wRow = row_ptr(weight, imgPitch, y);
    // the body of k_finishFused up to its gamma (finish_value, finish_common.hpp: shared with the statistics of section 2.23)
    auto src = [&](int x) { return finish_value(valRow[x], wRow[x], x, y, f); };
    render_span<FORMAT>(src, outImg ? row_ptr(outImg, outPitch, y) : nullptr, out ? out + (size_t)outRowBytes * (size_t)y : nullptr,
                        x0, width, r, lut);
}

}  // namespace

extern "C" int mfsr_render_row_bytes(int format, int widthPx)
{
    if (yuv_format(format)) {  // a Y row; a chroma row of widthPx / 2 (Cb, Cr) pairs has the same bytes
        const int bps = format == MFSR_OUT_NV12 ? 1 : 2;
        if (widthPx <= 0 || (widthPx & 1) || (long long)bps * widthPx > 2147483647LL) return MFSR_E_INVALID;
        return bps * widthPx;
    }
    const int bpp = bytes_per_pixel(format);
    if (bpp < 0 || widthPx <= 0 || (long long)bpp * widthPx > 2147483647LL) return MFSR_E_INVALID;
    return bpp * widthPx;
}

extern "C" long long mfsr_render_image_bytes(int format, int w, int h)
{
    const int rowBytes = mfsr_render_row_bytes(format, w);
    if (rowBytes < 0 || h <= 0) return MFSR_E_INVALID;
    if (!yuv_format(format)) return (long long)rowBytes * h;
    if (h & 1) return MFSR_E_INVALID;
    return (long long)rowBytes * h * 3 / 2;
}

int mfsr_render_validate(const mfsr_render* r)
{
    MFSR_REQUIRE(r != nullptr);
    if (yuv_format(r->format)) {  // reserved[0]: the colour description (MFSR_YUV_*)
        MFSR_REQUIRE((r->reserved[0] & ~7) == 0 && (r->reserved[0] & 3) != 3 && r->reserved[1] == 0 && r->reserved[2] == 0);
    } else {
        MFSR_REQUIRE(bytes_per_pixel(r->format) > 0);
    }
    if (r->useMatrix)
        for (int i = 0; i < 9; i++) MFSR_REQUIRE(std::isfinite(r->matrix[i]) && fabsf(r->matrix[i]) <= 256.0f);
    if (r->toneLut) MFSR_REQUIRE(r->toneSize >= 1 && r->toneSize <= 65536 && ((uintptr_t)r->toneLut & 3) == 0);
    return MFSR_OK;
}

// 64 x 4 lanes (64 x 16 where the workgroup stages the table), one or (RGB8) four pixels of a row per lane; w, h, stream: the caller's
#define RENDER_DISPATCH(KERNEL, format, lds, ...)                                                                                    \
    FORMAT_LUT_DISPATCH(KERNEL, dim3(mfsr_cdiv(mfsr_cdiv(w, (format) == MFSR_OUT_RGB8 ? 4 : 1), 64), mfsr_cdiv(h, (lds) ? 16 : 4)), \
                        dim3(64, (lds) ? 16 : 4), format, lds, __VA_ARGS__)

extern "C" int mfsr_renderImage(const mfsr_float3* in, int inRowBytes, mfsr_float3* outImg, int outImgRowBytes, void* out,
                                int outRowBytes, int w, int h, const mfsr_render* render, int applyGamma, mfsr_stream_t stream)
{
    MFSR_REQUIRE(in && (outImg || out) && w > 0 && h > 0);
    MFSR_REQUIRE((long long)inRowBytes >= 12LL * w && (inRowBytes & 3) == 0 && ((uintptr_t)in & 3) == 0);
    if (outImg) MFSR_REQUIRE((long long)outImgRowBytes >= 12LL * w && (outImgRowBytes & 3) == 0 && ((uintptr_t)outImg & 3) == 0);
    if (int rc = mfsr_render_validate(render)) return rc;
    MFSR_REQUIRE(!yuv_format(render->format));  // two planes: mfsr_renderImageYuv / mfsr_finishRenderedYuv
    if (out)
        if (int rc = check_out(render->format, out, outRowBytes, w)) return rc;
    const RenderArgs a = render_args(render, applyGamma);
    const bool lds = lut_in_lds(render);
    RENDER_DISPATCH(k_renderImage, render->format, lds, (const pix3*)in, inRowBytes, (pix3*)outImg, outImgRowBytes, (uint8_t*)out,
                    outRowBytes, w, h, a);
    return mfsr_launch_status("renderImage");
}

extern "C" int mfsr_finishRendered(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes,
                                   const mfsr_float3* fallback, int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0,
                                   float v1, mfsr_float3* outImg, int outImgRowBytes, void* out, int outRowBytes,
                                   const mfsr_render* render, int w, int h, float threshold, int applyGamma, int colOffset,
                                   int rowOffset, int fullWidth, int fullHeight, mfsr_stream_t stream)
{
    if (int rc = finish_check(finalImg, weight, imgRowBytes, fallback, fbRowBytes, fbW, fbH, outImg, outImgRowBytes, out, w, h, colOffset,
                              rowOffset, fullWidth, fullHeight))
        return rc;
    if (int rc = mfsr_render_validate(render)) return rc;
    MFSR_REQUIRE(!yuv_format(render->format));  // two planes: mfsr_renderImageYuv / mfsr_finishRenderedYuv
    if (out)
        if (int rc = check_out(render->format, out, outRowBytes, w)) return rc;
    const RenderArgs a = render_args(render, applyGamma);
    const FinishSrc f = finish_src(fallback, fbRowBytes, fbW, fbH, u0, u1, v0, v1, threshold, colOffset, rowOffset, fullWidth, fullHeight);
    const bool lds = lut_in_lds(render);
    RENDER_DISPATCH(k_finishRendered, render->format, lds, (const pix3*)finalImg, (const pix3*)weight, imgRowBytes, f, (pix3*)outImg,
                    outImgRowBytes, (uint8_t*)out, outRowBytes, w, h, a);
    return mfsr_launch_status("finishRendered");
}
