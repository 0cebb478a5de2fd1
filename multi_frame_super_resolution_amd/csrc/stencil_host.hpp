// stencil_host.hpp -- the host side that the two stencil finishes share: sharpen.hip and denoise.hip
// (section 2.24).  Both run a tile kernel with a halo on the value the finish holds and hand its pixels to render_span, so
// their entry points take the same arguments and refuse the same things: one definition of the argument checks, of the
// "no output may overlap what the stencil reads" rule, of the tone-table decision and of the format dispatch; the finish chain
// (finish_chain.hip, section 2.26) takes the same, and pipeline.cpp the two "is the stage on" tests.  Host code only: no kernel
// is defined or changed here (the stages' device steps are finish_stages.hpp's).
#pragma once

#include "render_common.hpp"

namespace {

// Whether a description's stage does anything (a radius or a strength / amount of 0: the plain finish).  The stand-alone entry
// points refuse a description that is off, the chain (finish_chain.hip) skips the stage, and the burst's setters (pipeline.cpp)
// keep the plain finish.
bool denoise_on(const mfsr_denoise* d) { return d->radius != 0 && d->strength != 0.0f; }
bool sharpen_on(const mfsr_sharpen* s) { return s->radius != 0 && s->amount != 0.0f; }

bool ranges_overlap(const void* a, long long aBytes, const void* b, long long bBytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bBytes && b0 < a0 + (uintptr_t)aBytes;
}

// How the tone table is read by the stencil kernels.  Measured at 7680 x 4320 with a 4096-interval table (DESIGN.md section 5,
// "Sharpened finish"): with the tile's 39 KB of LDS a staged table (32 KB more) halves the workgroups per CU, and RGB8 -- the
// one format render.hip stages it for -- takes 621 / 904 us (R = 1 / 4) staged against 412 / 538 us through the cache.  So
// every format reads the table through the cache; MFSR_RENDER_LUT=lds still forces the staged form (A/B, and the tests run
// both).
bool stencil_lut_in_lds(const mfsr_render* r)
{
    return render_lut_forced() == LUT_LDS && lut_in_lds(r);
}

// bytes from the first byte of row 0 to the last byte of row h - 1 of an image of w pixels of bpp bytes
inline long long image_span(int rowBytes, int h, int bpp, int w) { return (long long)rowBytes * (h - 1) + (long long)bpp * w; }

// *use = the render description of the launch (NULL: *plain); validated, single-plane
int stencil_render(const mfsr_render* render, const mfsr_render* plain, const mfsr_render** use)
{
    if (!render) render = plain;
    if (int rc = mfsr_render_validate(render)) return rc;
    MFSR_REQUIRE(!yuv_format(render->format));  // the tile kernels render single rows: no two-plane 4:2:0 output
    *use = render;
    return MFSR_OK;
}

// the integer output's alignment and length (when given), and: neither output overlaps the `readBytes` bytes at `read` (a
// stencil cannot run in place)
int stencil_outputs_apart(const void* read, long long readBytes, const void* outImg, int outImgRowBytes, const void* out,
                          int outRowBytes, int format, int w, int h)
{
    if (outImg) MFSR_REQUIRE(!ranges_overlap(read, readBytes, outImg, image_span(outImgRowBytes, h, 12, w)));
    if (out) {
        if (int rc = check_out(format, out, outRowBytes, w)) return rc;
        MFSR_REQUIRE(!ranges_overlap(read, readBytes, out, image_span(outRowBytes, h, bytes_per_pixel(format), w)));
    }
    return MFSR_OK;
}

// the arguments of mfsr_sharpenImage / mfsr_denoiseImage before their descriptions
int stencil_image_args(const void* in, int inRowBytes, const void* outImg, int outImgRowBytes, const void* out, int w, int h)
{
    MFSR_REQUIRE(in && (outImg || out) && w > 0 && h > 0);
    MFSR_REQUIRE((long long)inRowBytes >= 12LL * w && (inRowBytes & 3) == 0 && ((uintptr_t)in & 3) == 0);
    if (outImg) MFSR_REQUIRE((long long)outImgRowBytes >= 12LL * w && (outImgRowBytes & 3) == 0 && ((uintptr_t)outImg & 3) == 0);
    return MFSR_OK;
}

// the arguments of mfsr_finishSharpened / mfsr_finishDenoised before their descriptions: every finish's (finish_check), and
// the reach lies inside the full frame
int stencil_finish_args(const void* finalImg, const void* weight, int imgRowBytes, const void* fallback, int fbRowBytes, int fbW,
                        int fbH, const void* outImg, int outImgRowBytes, const void* out, int w, int h, int colOffset,
                        int rowOffset, int fullWidth, int fullHeight, int rowsAbove, int rowsBelow)
{
    if (int rc = finish_check(finalImg, weight, imgRowBytes, fallback, fbRowBytes, fbW, fbH, outImg, outImgRowBytes, out, w, h, colOffset,
                              rowOffset, fullWidth, fullHeight))
        return rc;
    MFSR_REQUIRE(rowsAbove >= 0 && rowsAbove <= rowOffset && rowsBelow >= 0 && rowsBelow <= fullHeight - rowOffset - h);
    return MFSR_OK;
}

// no output of a finish launch may overlap the accumulator or weight rows it reads (its own and the reach's)
int stencil_finish_apart(const void* finalImg, const void* weight, int imgRowBytes, int rowsAbove, int rowsBelow, const void* outImg,
                         int outImgRowBytes, const void* out, int outRowBytes, int format, int w, int h)
{
    const long long readBytes = (long long)imgRowBytes * (h - 1 + rowsAbove + rowsBelow) + 12LL * w;
    const char* fin0 = (const char*)finalImg - (long long)imgRowBytes * rowsAbove;
    const char* wt0 = (const char*)weight - (long long)imgRowBytes * rowsAbove;
    if (int rc = stencil_outputs_apart(fin0, readBytes, outImg, outImgRowBytes, out, outRowBytes, format, w, h)) return rc;
    return stencil_outputs_apart(wt0, readBytes, outImg, outImgRowBytes, out, outRowBytes, format, w, h);
}

}  // namespace

// one launch of KERNEL<format, lds> over tiles of tileW x tileH output pixels, `lanes` lanes per workgroup; w, h and stream
// are the caller's
#define STENCIL_DISPATCH(KERNEL, tileW, tileH, lanes, format, lds, ...) \
    FORMAT_LUT_DISPATCH(KERNEL, dim3(mfsr_cdiv(w, tileW), mfsr_cdiv(h, tileH)), dim3(lanes), format, lds, __VA_ARGS__)
