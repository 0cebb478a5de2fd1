// render.hip -- the rendered finish: colour matrix, tone curve and a display-format store, as the
// pixel body of its own (mfsr_renderImage) and folded into the burst's finish (mfsr_finishRendered = H1 + fallback resample +
// matrix + tone + quantise in one launch).  gfx950, wave64.
//
// Every step is float32 + - * with -ffp-contract=off (the Makefile), so a numpy float32 restatement is bit-exact
// (tests/render_ref.py); the only inexact operation is the powf of the built-in gamma.
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

// steps 1 and 2 of section 2.19: the float value the image holds and the integer output quantises
__device__ __forceinline__ pix3 render_pixel(pix3 p, const RenderArgs& r, const float* lut)
{
    pix3 q = p;
    if (r.useMatrix) {  // uniform
        const float c0 = matrix_in(p.x), c1 = matrix_in(p.y), c2 = matrix_in(p.z);
        q.x = (r.m[0] * c0 + r.m[1] * c1) + r.m[2] * c2;
        q.y = (r.m[3] * c0 + r.m[4] * c1) + r.m[5] * c2;
        q.z = (r.m[6] * c0 + r.m[7] * c1) + r.m[8] * c2;
    }
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
    k_finishRendered(const pix3* __restrict__ finalImg, const pix3* __restrict__ weight, int imgPitch,
                     const pix3* __restrict__ fallback, int fbPitch, int fbW, int fbH, float u0, float u1, float v0, float v1,
                     pix3* __restrict__ outImg, int outPitch, uint8_t* __restrict__ out, int outRowBytes, int width, int height,
                     float threshold, int rowOffset, int fullHeight, int colOffset, int fullWidth, RenderArgs r)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    const float* lut = stage_lut<LDS>(r, s_lut);
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * Fmt<FORMAT>::ppl;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x0 >= width || y >= height) return;
    const pix3* valRow = row_ptr(finalImg, imgPitch, y);
    const pix3* wRow = row_ptr(weight, imgPitch, y);
    // the body of k_finishFused up to its gamma, expression for expression (a stripe or window is the crop of the whole)
    auto src = [&](int x) {
        const pix3 val = valRow[x];
        const pix3 w = wRow[x];
        pix3 inout = {0.0f, 0.0f, 0.0f};
        if (fallback && (w.x < threshold || w.y < threshold || w.z < threshold)) {
            const float u = u0 + (u1 - u0) * (((float)(x + colOffset) + 0.5f) / (float)fullWidth);
            const float v = v0 + (v1 - v0) * (((float)(y + rowOffset) + 0.5f) / (float)fullHeight);
            inout = sample_pix3(fallback, fbPitch, fbW, fbH, u, v);
        }
        inout.x = apply_weight_f(inout.x, val.x, w.x, threshold);
        inout.y = apply_weight_f(inout.y, val.y, w.y, threshold);
        inout.z = apply_weight_f(inout.z, val.z, w.z, threshold);
        return inout;
    };
    render_span<FORMAT>(src, outImg ? row_ptr(outImg, outPitch, y) : nullptr, out ? out + (size_t)outRowBytes * (size_t)y : nullptr,
                        x0, width, r, lut);
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

// How the tone table is read.  Measured at 7680 x 4320 with a 4096-interval table ("Rendered finish"):
// the one-pixel-per-lane formats are faster reading it through the cache (235 against 272 us), RGB8 -- four pixels, 24 table
// reads per lane -- is faster with the table staged in LDS by 1024-lane workgroups (237 against 346 us).  So RGB8 stages
// tables that fit (up to kLdsLutMax intervals) and the other formats do not.  MFSR_RENDER_LUT=lds | cache forces one form for
// every format (A/B); read at every call: host only, and a test can switch it.
bool lut_in_lds(const mfsr_render* r)
{
    if (!r->toneLut || r->toneSize > kLdsLutMax) return false;
    if (const char* e = getenv("MFSR_RENDER_LUT")) {
        if (strcmp(e, "lds") == 0) return true;
        if (strcmp(e, "cache") == 0) return false;
    }
    return r->format == MFSR_OUT_RGB8;
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

extern "C" int mfsr_render_row_bytes(int format, int widthPx)
{
    const int bpp = bytes_per_pixel(format);
    if (bpp < 0 || widthPx <= 0 || (long long)bpp * widthPx > 2147483647LL) return MFSR_E_INVALID;
    return bpp * widthPx;
}

int mfsr_render_validate(const mfsr_render* r)
{
    MFSR_REQUIRE(r != nullptr);
    MFSR_REQUIRE(bytes_per_pixel(r->format) > 0);
    if (r->useMatrix)
        for (int i = 0; i < 9; i++) MFSR_REQUIRE(std::isfinite(r->matrix[i]) && fabsf(r->matrix[i]) <= 256.0f);
    if (r->toneLut) MFSR_REQUIRE(r->toneSize >= 1 && r->toneSize <= 65536 && ((uintptr_t)r->toneLut & 3) == 0);
    return MFSR_OK;
}

#define RENDER_DISPATCH(KERNEL, format, lds, ...)                                                                   \
    do {                                                                                                            \
        const dim3 block(64, (lds) ? 16 : 4);                                                                       \
        const dim3 grid(mfsr_cdiv(mfsr_cdiv(w, (format) == MFSR_OUT_RGB8 ? 4 : 1), 64), mfsr_cdiv(h, block.y));     \
        switch (((format) << 1) | ((lds) ? 1 : 0)) {                                                                \
            case 0: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGB16, 0>), grid, block, 0, mfsr_s(stream), __VA_ARGS__); break;   \
            case 1: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGB16, 1>), grid, block, 0, mfsr_s(stream), __VA_ARGS__); break;   \
            case 2: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGB8, 0>), grid, block, 0, mfsr_s(stream), __VA_ARGS__); break;    \
            case 3: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGB8, 1>), grid, block, 0, mfsr_s(stream), __VA_ARGS__); break;    \
            case 4: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGBA8, 0>), grid, block, 0, mfsr_s(stream), __VA_ARGS__); break;   \
            case 5: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGBA8, 1>), grid, block, 0, mfsr_s(stream), __VA_ARGS__); break;   \
            case 6: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGB10A2, 0>), grid, block, 0, mfsr_s(stream), __VA_ARGS__); break; \
            default: hipLaunchKernelGGL((KERNEL<MFSR_OUT_RGB10A2, 1>), grid, block, 0, mfsr_s(stream), __VA_ARGS__); break; \
        }                                                                                                           \
    } while (0)

extern "C" int mfsr_renderImage(const mfsr_float3* in, int inRowBytes, mfsr_float3* outImg, int outImgRowBytes, void* out,
                                int outRowBytes, int w, int h, const mfsr_render* render, int applyGamma, mfsr_stream_t stream)
{
    MFSR_REQUIRE(in && (outImg || out) && w > 0 && h > 0);
    MFSR_REQUIRE((long long)inRowBytes >= 12LL * w && (inRowBytes & 3) == 0 && ((uintptr_t)in & 3) == 0);
    if (outImg) MFSR_REQUIRE((long long)outImgRowBytes >= 12LL * w && (outImgRowBytes & 3) == 0 && ((uintptr_t)outImg & 3) == 0);
    if (int rc = mfsr_render_validate(render)) return rc;
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
    MFSR_REQUIRE(finalImg && weight && (outImg || out) && w > 0 && h > 0);
    MFSR_REQUIRE((long long)imgRowBytes >= 12LL * w && (imgRowBytes & 3) == 0);
    if (outImg) MFSR_REQUIRE((long long)outImgRowBytes >= 12LL * w && (outImgRowBytes & 3) == 0);
    if (fallback) MFSR_REQUIRE(fbW > 0 && fbH > 0 && (long long)fbRowBytes >= 12LL * fbW && (fbRowBytes & 3) == 0);
    MFSR_REQUIRE(rowOffset >= 0 && fullHeight >= rowOffset + h);
    MFSR_REQUIRE(colOffset >= 0 && fullWidth >= colOffset + w);
    if (int rc = mfsr_render_validate(render)) return rc;
    if (out)
        if (int rc = check_out(render->format, out, outRowBytes, w)) return rc;
    const RenderArgs a = render_args(render, applyGamma);
    const bool lds = lut_in_lds(render);
    RENDER_DISPATCH(k_finishRendered, render->format, lds, (const pix3*)finalImg, (const pix3*)weight, imgRowBytes,
                    (const pix3*)fallback, fbRowBytes, fbW, fbH, u0, u1, v0, v1, (pix3*)outImg, outImgRowBytes, (uint8_t*)out,
                    outRowBytes, w, h, threshold, rowOffset, fullHeight, colOffset, fullWidth, a);
    return mfsr_launch_status("finishRendered");
}
