// finish_common.hpp -- the pixel arithmetic of the burst's finish (stage H), shared by glue.hip (k_finishFused, k_quantize,
// k_resampleFloat3), render.hip (k_finishRendered, k_renderImage), render_yuv.hip (k_finishRenderedYuv), sharpen.hip
// (k_finishSharpened), denoise.hip (k_finishDenoised), local_tone.hip (k_finishLocalTone, k_toneGridStats), image_stats.hip
// (k_imageStats) and accumulate_fast.hip (the finishing burst tile kernel and k_finishRing, which write what k_finishFused
// writes): one definition, so that every finish holds the same value as the plain one before its own step, quantises by the
// same rule, and is measured as it is rendered.  The host side of those launches is here as well: one check of the arguments
// they share and one fill of FinishSrc.
#pragma once

#include "common.hpp"

// bilinear fetch of a float3 image (clamp) -- shared with finishFused
__device__ __forceinline__ pix3 sample_pix3(const pix3* __restrict__ in, int inPitch, int inW, int inH, float u, float v)
{
    const TexCoord c = tex_coord<ADDR_CLAMP>(inW, inH, u, v);
    const pix3* r0 = row_ptr(in, inPitch, c.j0);
    const pix3* r1 = row_ptr(in, inPitch, c.j1);
    const pix3 t00 = r0[c.i0], t10 = r0[c.i1], t01 = r1[c.i0], t11 = r1[c.i1];
    pix3 o;
    o.x = lerp4(t00.x, t10.x, t01.x, t11.x, c.a, c.b);
    o.y = lerp4(t00.y, t10.y, t01.y, t11.y, c.a, c.b);
    o.z = lerp4(t00.z, t10.z, t01.z, t11.z, c.a, c.b);
    return o;
}

__device__ __forceinline__ int quantize1(float f, float maxOut)
{
    if (isnan(f)) f = 0;
    f = fmaxf(fminf(f, 1.0f), 0.0f);
    return (int)(f * maxOut + 0.5f);
}

__device__ __forceinline__ float apply_weight_f(float inout, float val, float w, float threshold)
{
    // kernel.cu:447-456
    if (w < threshold) {
        val += inout;
        w += 1;
    }
    inout = 0;
    if (w != 0) inout = val / w;
    return inout;
}

// Where the fallback of a finish launch lies and which pixel of the whole image the launch's pixel (0, 0) is: the arguments of
// mfsr_finishRendered that its pixel value depends on.
struct FinishSrc {
    const pix3* fallback;  // or null
    int fbPitch, fbW, fbH;
    float u0, u1, v0, v1;
    float threshold;
    int rowOffset, fullHeight, colOffset, fullWidth;
};

// The three pieces of finish_value (below), for the launches that take them apart (the finishing burst tile kernel,
// accumulate_fast.hip, asks a whole wave whether any pixel needs the fallback before it resamples):
// ApplyWeighting reads the fallback only where a weight is under the threshold (kernel.cu:444-462): the resample (12 loads, two
// divisions, the bilinear mix: 40 % of the plain finish's instructions) is skipped by the waves that need none
__device__ __forceinline__ bool finish_needs_fallback(pix3 w, const FinishSrc& f)
{
    return f.fallback && (w.x < f.threshold || w.y < f.threshold || w.z < f.threshold);
}

// Row y of a launch is row y + rowOffset of a fullHeight-row image (column x + colOffset of a fullWidth-column image likewise:
// a window's finish): the same float expression as the whole-image launch evaluates for that pixel, so a stripe-wise or
// window-wise finish is bit-identical to the whole one
__device__ __forceinline__ pix3 finish_fallback(int x, int y, const FinishSrc& f)
{
    const float u = f.u0 + (f.u1 - f.u0) * (((float)(x + f.colOffset) + 0.5f) / (float)f.fullWidth);
    const float v = f.v0 + (f.v1 - f.v0) * (((float)(y + f.rowOffset) + 0.5f) / (float)f.fullHeight);
    return sample_pix3(f.fallback, f.fbPitch, f.fbW, f.fbH, u, v);
}

__device__ __forceinline__ pix3 finish_weighted(pix3 inout, pix3 val, pix3 w, const FinishSrc& f)
{
    inout.x = apply_weight_f(inout.x, val.x, w.x, f.threshold);
    inout.y = apply_weight_f(inout.y, val.y, w.y, f.threshold);
    inout.z = apply_weight_f(inout.z, val.z, w.z, f.threshold);
    return inout;
}

// The value section 2.19 calls p at pixel (x, y) of the launch: the body of k_finishFused up to its gamma (a stripe or window is
// the crop of the whole).  val / w: the accumulator and the weight of the pixel.  One definition for every finish kernel and
// both statistics passes (the list at the head of this file): what is measured is what is rendered.  (The test is
// finish_needs_fallback's, spelled out: through the call k_finishFused came out as other code.)
__device__ __forceinline__ pix3 finish_value(pix3 val, pix3 w, int x, int y, const FinishSrc& f)
{
    pix3 inout = {0.0f, 0.0f, 0.0f};
    if (f.fallback && (w.x < f.threshold || w.y < f.threshold || w.z < f.threshold)) inout = finish_fallback(x, y, f);
    return finish_weighted(inout, val, w, f);
}

// finish_value at pixel (x, y) of a launch whose accumulator and weight rows are imgPitch bytes apart.  The stencil finishes
// (sharpen.hip, denoise.hip) fetch through this: their reach puts y below 0 (rowsAbove), so the address is signed 64-bit.
__device__ __forceinline__ pix3 finish_value_at(const pix3* finalImg, const pix3* weight, int imgPitch, int x, int y,
                                                const FinishSrc& f)
{
    const pix3 val = *(const pix3*)((const char*)finalImg + (long long)imgPitch * y + 12LL * x);
    const pix3 w = *(const pix3*)((const char*)weight + (long long)imgPitch * y + 12LL * x);
    return finish_value(val, w, x, y, f);
}

// ---- host: what every finish entry point checks and fills before its own arguments --------------------------------------
// the FinishSrc of an entry point's arguments
static inline FinishSrc finish_src(const void* fallback, int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1,
                                   float threshold, int colOffset, int rowOffset, int fullWidth, int fullHeight)
{
    return FinishSrc{(const pix3*)fallback, fbRowBytes, fbW, fbH, u0, u1, v0, v1, threshold, rowOffset, fullHeight, colOffset, fullWidth};
}

// what a finish launch of w x h pixels reads: the accumulator pair, the fallback's extent and pitch, the launch's place in the
// full frame.  (The statistics passes stop here: they have no image output.)
static inline int finish_check_src(const void* finalImg, const void* weight, int imgRowBytes, const void* fallback, int fbRowBytes,
                                   int fbW, int fbH, int w, int h, int colOffset, int rowOffset, int fullWidth, int fullHeight)
{
    MFSR_REQUIRE(finalImg && weight && w > 0 && h > 0);
    MFSR_REQUIRE((long long)imgRowBytes >= 12LL * w && (imgRowBytes & 3) == 0);
    if (fallback) MFSR_REQUIRE(fbW > 0 && fbH > 0 && (long long)fbRowBytes >= 12LL * fbW && (fbRowBytes & 3) == 0);
    MFSR_REQUIRE(rowOffset >= 0 && fullHeight >= rowOffset + h);
    MFSR_REQUIRE(colOffset >= 0 && fullWidth >= colOffset + w);
    return MFSR_OK;
}

// ... and writes: the float image and / or an integer output (`out`: any plane of it), one of them at least
static inline int finish_check(const void* finalImg, const void* weight, int imgRowBytes, const void* fallback, int fbRowBytes, int fbW,
                               int fbH, const void* outImg, int outImgRowBytes, const void* out, int w, int h, int colOffset,
                               int rowOffset, int fullWidth, int fullHeight)
{
    MFSR_REQUIRE(outImg || out);
    if (int rc = finish_check_src(finalImg, weight, imgRowBytes, fallback, fbRowBytes, fbW, fbH, w, h, colOffset, rowOffset, fullWidth,
                                  fullHeight))
        return rc;
    if (outImg) MFSR_REQUIRE((long long)outImgRowBytes >= 12LL * w && (outImgRowBytes & 3) == 0);
    return MFSR_OK;
}

// the plain uint16_t RGB of p: three samples of maxOut levels
__device__ __forceinline__ void finish_quantize3(pix3 p, float maxOut, uint16_t* __restrict__ o)
{
    o[0] = (uint16_t)quantize1(p.x, maxOut);
    o[1] = (uint16_t)quantize1(p.y, maxOut);
    o[2] = (uint16_t)quantize1(p.z, maxOut);
}

__device__ __forceinline__ float gamma_f(float v)
{
    // kernel.cu:380-390, :407-420
    if (isnan(v)) v = 0;
    v = fmaxf(fminf(v, 1.0f), 0.0f);
    if (v <= 0.0031308f) return 12.92f * v;
    return (1.0f + 0.055f) * powf(v, 1.0f / 2.4f) - 0.055f;
}
