// render_common.hpp -- the pixel body of the rendered finish and the host checks of its output, shared
// by render.hip (k_renderImage, k_finishRendered), sharpen.hip, denoise.hip and local_tone.hip (their image and finish kernels):
// one definition, so that a sharpened finish renders and stores exactly as the rendered one does, and one (format, table form)
// launch switch (FORMAT_LUT_DISPATCH, at the end).  All of them compile with -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.hpp"
#include "finish_common.hpp"

namespace {

struct RenderArgs {
    float m[9];
    const float* lut;  // toneSize + 1 floats of device memory, or null
    int n;             // toneSize
    int useMatrix;
    int applyGamma;
};

// tables up to this many intervals can be staged in LDS (MFSR_RENDER_LUT=lds): 8193 floats = 32 KiB + 4 B per workgroup
constexpr int kLdsLutMax = 8192;

__device__ __forceinline__ float tone1(float q, const RenderArgs& r, const float* lut)
{
    if (lut) {  // uniform
        float v = isnan(q) ? 0.0f : fmaxf(fminf(q, 1.0f), 0.0f);
        const float t = v * (float)r.n;
        const int i = min((int)t, r.n - 1);
        const float f = t - (float)i;
        const float a = lut[i], b = lut[i + 1];
        return a + (b - a) * f;
    }
    return r.applyGamma ? gamma_f(q) : q;
}

__device__ __forceinline__ float matrix_in(float p) { return isnan(p) ? 0.0f : fminf(fmaxf(p, 0.0f), 65536.0f); }

// step 1 of section 2.19 with a matrix (also what the statistics of section 2.23 measure: image_stats.hip)
__device__ __forceinline__ pix3 matrix_pixel(pix3 p, const float* m)
{
    const float c0 = matrix_in(p.x), c1 = matrix_in(p.y), c2 = matrix_in(p.z);
    pix3 q;
    q.x = (m[0] * c0 + m[1] * c1) + m[2] * c2;
    q.y = (m[3] * c0 + m[4] * c1) + m[5] * c2;
    q.z = (m[6] * c0 + m[7] * c1) + m[8] * c2;
    return q;
}

// steps 1 and 2 of section 2.19: the float value the image holds and the integer output quantises
__device__ __forceinline__ pix3 render_pixel(pix3 p, const RenderArgs& r, const float* lut)
{
    pix3 q = p;
    if (r.useMatrix) q = matrix_pixel(p, r.m);  // uniform
    pix3 o;
    o.x = tone1(q.x, r, lut);
    o.y = tone1(q.y, r, lut);
    o.z = tone1(q.z, r, lut);
    return o;
}

template <int FORMAT>
struct Fmt {
    static constexpr int ppl = FORMAT == MFSR_OUT_RGB8 ? 4 : 1;  // consecutive pixels of a row one lane owns
    static constexpr float maxOut = FORMAT == MFSR_OUT_RGB16 ? 65535.0f : (FORMAT == MFSR_OUT_RGB10A2 ? 1023.0f : 255.0f);
};

struct __attribute__((packed, aligned(4))) dword3 {
    uint32_t a, b, c;
};

// Pixels [x0, x0 + ppl) of one row, clipped to `width`: src(x) is the value before step 1.  outImgRow / outRow: the row's
// first pixel / byte, or null.  src(x) is read before outImgRow[x] is written and no other lane touches pixel x: in place is
// fine.
template <int FORMAT, class Src>
__device__ __forceinline__ void render_span(const Src& src, pix3* outImgRow, uint8_t* outRow, int x0, int width,
                                            const RenderArgs& r, const float* lut)
{
    constexpr int PPL = Fmt<FORMAT>::ppl;
    constexpr float maxOut = Fmt<FORMAT>::maxOut;
    uint32_t q[PPL][3];
#pragma unroll
    for (int k = 0; k < PPL; k++) {
        q[k][0] = q[k][1] = q[k][2] = 0;
        if (x0 + k < width) {
            const pix3 o = render_pixel(src(x0 + k), r, lut);
            if (outImgRow) outImgRow[x0 + k] = o;
            q[k][0] = (uint32_t)quantize1(o.x, maxOut);
            q[k][1] = (uint32_t)quantize1(o.y, maxOut);
            q[k][2] = (uint32_t)quantize1(o.z, maxOut);
        }
    }
    if (!outRow) return;
    if constexpr (FORMAT == MFSR_OUT_RGB16) {
        uint16_t* o16 = (uint16_t*)outRow + (size_t)x0 * 3;
        o16[0] = (uint16_t)q[0][0];
        o16[1] = (uint16_t)q[0][1];
        o16[2] = (uint16_t)q[0][2];
    } else if constexpr (FORMAT == MFSR_OUT_RGBA8) {
        ((uint32_t*)outRow)[x0] = q[0][0] | q[0][1] << 8 | q[0][2] << 16 | 255u << 24;
    } else if constexpr (FORMAT == MFSR_OUT_RGB10A2) {
        ((uint32_t*)outRow)[x0] = q[0][0] | q[0][1] << 10 | q[0][2] << 20 | 3u << 30;
    } else {
        // RGB8: the lane's 12 bytes start at byte 3 * x0 = 12 * (lane index) of the row, so they are dword-aligned exactly
        // where the row's first byte is (uniform per row); a partial quad at the row's end goes out byte by byte
        uint8_t* o8 = outRow + (size_t)x0 * 3;
        if (x0 + PPL <= width && ((uintptr_t)outRow & 3) == 0) {
            dword3 d;
            d.a = q[0][0] | q[0][1] << 8 | q[0][2] << 16 | q[1][0] << 24;
            d.b = q[1][1] | q[1][2] << 8 | q[2][0] << 16 | q[2][1] << 24;
            d.c = q[2][2] | q[3][0] << 8 | q[3][1] << 16 | q[3][2] << 24;
            *(dword3*)o8 = d;
        } else {
#pragma unroll
            for (int k = 0; k < PPL; k++)
                if (x0 + k < width) {
                    o8[3 * k] = (uint8_t)q[k][0];
                    o8[3 * k + 1] = (uint8_t)q[k][1];
                    o8[3 * k + 2] = (uint8_t)q[k][2];
                }
        }
    }
}

// LDS = 1: the workgroup copies the table into LDS first (64 x 16 lanes, so that one copy serves 4 x as many pixels as the
// 64 x 4 workgroup of the cached form).  Returns the table the pixels read.
template <int LDS>
__device__ __forceinline__ const float* stage_lut(const RenderArgs& r, float* s_lut)
{
    if (!LDS || !r.lut) return r.lut;
    const int tid = threadIdx.y * blockDim.x + threadIdx.x, nt = blockDim.x * blockDim.y;
    for (int i = tid; i <= r.n; i += nt) s_lut[i] = r.lut[i];
    __syncthreads();
    return s_lut;
}

int bytes_per_pixel(int format)
{
    switch (format) {
        case MFSR_OUT_RGB16: return 6;
        case MFSR_OUT_RGB8: return 3;
        case MFSR_OUT_RGBA8:
        case MFSR_OUT_RGB10A2: return 4;
    }
    return -1;
}

// the two-plane 4:2:0 formats: their kernels and entry points are render_yuv.hip's
inline bool yuv_format(int format) { return format == MFSR_OUT_NV12 || format == MFSR_OUT_P010; }

// How the tone table is read.  Measured at 7680 x 4320 with a 4096-interval table ("Rendered finish"):
// the one-pixel-per-lane formats are faster reading it through the cache (235 against 272 us), RGB8 -- four pixels, 24 table
// reads per lane -- is faster with the table staged in LDS by 1024-lane workgroups (237 against 346 us).  So RGB8 stages
// tables that fit (up to kLdsLutMax intervals) and the other formats do not.  MFSR_RENDER_LUT=lds | cache forces one form for
// every format (A/B); read at every call: host only, and a test can switch it.  The two-plane formats (eight pixels, 24 table
// reads per lane) follow RGB8.
enum { LUT_BY_FORMAT = 0, LUT_LDS = 1, LUT_CACHE = 2 };
int render_lut_forced()
{
    const char* e = getenv("MFSR_RENDER_LUT");
    return !e ? LUT_BY_FORMAT : (strcmp(e, "lds") == 0 ? LUT_LDS : (strcmp(e, "cache") == 0 ? LUT_CACHE : LUT_BY_FORMAT));
}
bool lut_in_lds(const mfsr_render* r)
{
    if (!r->toneLut || r->toneSize > kLdsLutMax) return false;
    const int forced = render_lut_forced();
    if (forced != LUT_BY_FORMAT) return forced == LUT_LDS;
    return r->format == MFSR_OUT_RGB8 || yuv_format(r->format);
}

RenderArgs render_args(const mfsr_render* r, int applyGamma)
{
    RenderArgs a;
    for (int i = 0; i < 9; i++) a.m[i] = r->matrix[i];
    a.lut = r->toneLut;
    a.n = r->toneLut ? r->toneSize : 0;
    a.useMatrix = r->useMatrix != 0;
    a.applyGamma = applyGamma != 0;
    return a;
}

// the output rows of a launch: alignment and length the format's stores need
int check_out(int format, const void* out, int outRowBytes, int width)
{
    const int bpp = bytes_per_pixel(format);
    MFSR_REQUIRE(bpp > 0);
    MFSR_REQUIRE((long long)outRowBytes >= (long long)bpp * width);
    if (format == MFSR_OUT_RGB16) MFSR_REQUIRE(((uintptr_t)out & 1) == 0 && (outRowBytes & 1) == 0);
    if (format == MFSR_OUT_RGBA8 || format == MFSR_OUT_RGB10A2) MFSR_REQUIRE(((uintptr_t)out & 3) == 0 && (outRowBytes & 3) == 0);
    return MFSR_OK;
}

}  // namespace

// one launch of KERNEL<format, lds> over `grid` workgroups of `block` lanes on the caller's `stream`: the (format, table form)
// switch of every single-plane rendering kernel (render.hip, sharpen.hip, denoise.hip)
#define FORMAT_LUT_DISPATCH(KERNEL, grid, block, format, lds, ...)                                                              \
    do {                                                                                                                        \
        switch (((format) << 1) | ((lds) ? 1 : 0)) {                                                                            \
            case 0: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGB16, 0>), (grid), (block), 0, mfsr_s(stream), __VA_ARGS__); break;    \
            case 1: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGB16, 1>), (grid), (block), 0, mfsr_s(stream), __VA_ARGS__); break;    \
            case 2: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGB8, 0>), (grid), (block), 0, mfsr_s(stream), __VA_ARGS__); break;     \
            case 3: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGB8, 1>), (grid), (block), 0, mfsr_s(stream), __VA_ARGS__); break;     \
            case 4: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGBA8, 0>), (grid), (block), 0, mfsr_s(stream), __VA_ARGS__); break;    \
            case 5: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGBA8, 1>), (grid), (block), 0, mfsr_s(stream), __VA_ARGS__); break;    \
            case 6: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGB10A2, 0>), (grid), (block), 0, mfsr_s(stream), __VA_ARGS__); break;  \
            default: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGB10A2, 1>), (grid), (block), 0, mfsr_s(stream), __VA_ARGS__); break; \
        }                                                                                                                       \
    } while (0)
