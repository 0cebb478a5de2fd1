// sharpen.hip -- sharpening inside the finish: a separable unsharp mask on the linear float value the
// finish holds, before the colour matrix and the tone curve, in the same launch as the finish and the display-format store
// (mfsr_finishSharpened), and the same tile body on an existing float image (mfsr_sharpenImage).  gfx950, wave64.
//
// Every step is float32 + - * with -ffp-contract=off (the Makefile), so a numpy float32 restatement is bit-exact
// (tests/sharpen_ref.py).
//
// A workgroup of 256 lanes owns a kTW x kTH tile of output pixels.  It stages s (the NaN-cleaned finish value) of the tile plus
// a halo of R at clamped coordinates in LDS, runs the horizontal pass into a second LDS array (tile columns, tile + halo rows),
// takes the vertical pass and the coring for the lane's pixels, and hands them to render_span as its src, so the store is that
// of the rendered finish.
// LDS is planar (one plane per channel) with rows of kTW + 2 * kMaxR = 72 (s) and kTW = 64 (h) floats; the tile's first column
// sits at float kMaxR of an s row whatever R is, so that column 4 * k of the tile is 16-byte aligned in both arrays.  A wave of
// a one-pixel-per-lane format reads 64 consecutive dwords of one row (no bank conflict in either 32-lane half).  An RGB8 lane
// owns four consecutive columns: it reads them as one float4 per row, channel and tap (ds_read_b128; four dword reads would
// put the 32 lanes of a half on 8 banks, a 4-way conflict), computes its four pixels, and then hands them to render_span.
// R is a runtime argument: one set of kernels.  The arithmetic of the steps (sharpen_clean, sharpen_tap, sharpen_core) and
// load_span are finish_stages.hpp's, which the finish chain (finish_chain.hip) calls too; the chain restates the loops of the
// two passes around them (its stage 3 and sharpened_span): change both together.
#include "finish_stages.hpp"
#include "stencil_host.hpp"

namespace {

constexpr int kMaxR = kMaxRs;
constexpr int kSW = kTW + 2 * kMaxR, kSH = kTH + 2 * kMaxR;  // the staged extent at R = 4

// The tile of the workgroup at (tileX0, tileY0): fetch(x, y) is p of section 2.20 at a valid pixel of the launch.
template <int FORMAT, class Fetch>
__device__ __forceinline__ void sharpen_tile(const Fetch& fetch, float (*s_s)[kSH][kSW], float (*s_h)[kSH][kTW], pix3* outImg,
                                             int outPitch, uint8_t* out, int outRowBytes, int width, int height,
                                             const SharpenArgs& a, const RenderArgs& r, const float* lut)
{
    const int tid = threadIdx.x, R = a.R;
    const int tileX0 = blockIdx.x * kTW, tileY0 = blockIdx.y * kTH;
    const int sw = kTW + 2 * R, sh = kTH + 2 * R;
    // 1. s of tile + halo at clamped coordinates (what lies beyond the image's last tile is staged too: clamped, never stored)
    for (int i = tid; i < sw * sh; i += kLanes) {
        const int ly = i / sw, lx = i - ly * sw;
        const int gx = min(max(tileX0 + lx - R, 0), width - 1);
        const int gy = min(max(tileY0 + ly - R, a.yLo), a.yHi);
        const pix3 p = fetch(gx, gy);
        const int c0 = lx + (kMaxR - R);  // (the tile's column 0 at float kMaxR of the row)
        s_s[0][ly][c0] = sharpen_clean(p.x);
        s_s[1][ly][c0] = sharpen_clean(p.y);
        s_s[2][ly][c0] = sharpen_clean(p.z);
    }
    __syncthreads();
    // 2. the horizontal pass on every staged row
    for (int i = tid; i < kTW * sh; i += kLanes) {
        const int ly = i / kTW, lx = i - ly * kTW;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float* row = &s_s[c][ly][lx + kMaxR];
            float h = a.k[0] * row[0];
            for (int d = 1; d <= R; d++) h = sharpen_tap(h, a.k[d], row[-d], row[d]);
            s_h[c][ly][lx] = h;
        }
    }
    __syncthreads();
    // 3. + 4. the lane's PPL pixels of one row, then the rendered finish's span with them as its src
    constexpr int PPL = Fmt<FORMAT>::ppl, lanesX = kTW / PPL, rowsPerPass = kLanes / lanesX;
    const int lx0 = (tid % lanesX) * PPL, x0 = tileX0 + lx0;
    for (int ly = tid / lanesX; ly < kTH; ly += rowsPerPass) {
        const int y = tileY0 + ly;
        if (x0 >= width || y >= height) continue;
        float o[PPL][3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float s[PPL], b[PPL];
            load_span<PPL>(&s_s[c][ly + R][lx0 + kMaxR], s);
            load_span<PPL>(&s_h[c][ly + R][lx0], b);
#pragma unroll
            for (int k = 0; k < PPL; k++) b[k] = a.k[0] * b[k];
            for (int d = 1; d <= R; d++) {
                float up[PPL], dn[PPL];
                load_span<PPL>(&s_h[c][ly + R - d][lx0], up);
                load_span<PPL>(&s_h[c][ly + R + d][lx0], dn);
#pragma unroll
                for (int k = 0; k < PPL; k++) b[k] = sharpen_tap(b[k], a.k[d], up[k], dn[k]);
            }
#pragma unroll
            for (int k = 0; k < PPL; k++) o[k][c] = sharpen_core(s[k], b[k], a);
        }
        auto src = [&](int x) {
            pix3 q = {o[0][0], o[0][1], o[0][2]};
#pragma unroll
            for (int k = 1; k < PPL; k++)
                if (x - x0 == k) q = {o[k][0], o[k][1], o[k][2]};
            return q;
        };
        render_span<FORMAT>(src, outImg ? row_ptr(outImg, outPitch, y) : nullptr, out ? out + (size_t)outRowBytes * (size_t)y : nullptr,
                            x0, width, r, lut);
    }
}

template <int FORMAT, int LDS>
__global__ void __launch_bounds__(kLanes)
    k_sharpenImage(const pix3* __restrict__ in, int inPitch, pix3* __restrict__ outImg, int outPitch, uint8_t* __restrict__ out,
                   int outRowBytes, int width, int height, SharpenArgs a, RenderArgs r)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    __shared__ __attribute__((aligned(16))) float s_s[3][kSH][kSW];
    __shared__ __attribute__((aligned(16))) float s_h[3][kSH][kTW];
    const float* lut = stage_lut<LDS>(r, s_lut);
    sharpen_tile<FORMAT>([&](int x, int y) { return row_ptr(in, inPitch, y)[x]; }, s_s, s_h, outImg, outPitch, out, outRowBytes,
                         width, height, a, r, lut);
}

template <int FORMAT, int LDS>
__global__ void __launch_bounds__(kLanes)
    k_finishSharpened(const pix3* __restrict__ finalImg, const pix3* __restrict__ weight, int imgPitch, FinishSrc f,
                      pix3* __restrict__ outImg, int outPitch, uint8_t* __restrict__ out, int outRowBytes, int width, int height,
                      SharpenArgs a, RenderArgs r)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    __shared__ __attribute__((aligned(16))) float s_s[3][kSH][kSW];
    __shared__ __attribute__((aligned(16))) float s_h[3][kSH][kTW];
    const float* lut = stage_lut<LDS>(r, s_lut);
    // k_finishRendered's value (finish_value_at: one definition); y may be negative (rowsAbove)
    auto fetch = [&](int x, int y) { return finish_value_at(finalImg, weight, imgPitch, x, y, f); };
    sharpen_tile<FORMAT>(fetch, s_s, s_h, outImg, outPitch, out, outRowBytes, width, height, a, r, lut);
}

}  // namespace

#define SHARPEN_DISPATCH(KERNEL, format, lds, ...) STENCIL_DISPATCH(KERNEL, kTW, kTH, kLanes, format, lds, __VA_ARGS__)

extern "C" int mfsr_sharpen_tile(int* tileW, int* tileH)
{
    MFSR_REQUIRE(tileW && tileH);
    *tileW = kTW;
    *tileH = kTH;
    return MFSR_OK;
}

extern "C" int mfsr_sharpen_validate(const mfsr_sharpen* s)
{
    MFSR_REQUIRE(s != nullptr);
    MFSR_REQUIRE(s->radius >= 0 && s->radius <= kMaxR);
    for (int d = 0; d <= kMaxR; d++) MFSR_REQUIRE(std::isfinite(s->taps[d]) && fabsf(s->taps[d]) <= 4.0f);
    MFSR_REQUIRE(std::isfinite(s->amount) && s->amount >= 0.0f && s->amount <= 16.0f);
    MFSR_REQUIRE(std::isfinite(s->threshold) && s->threshold >= 0.0f);
    for (int i = 0; i < 4; i++) MFSR_REQUIRE(s->reserved[i] == 0);
    return MFSR_OK;
}

extern "C" int mfsr_sharpen_gaussian(float sigma, int radius, float amount, float threshold, mfsr_sharpen* out)
{
    MFSR_REQUIRE(out != nullptr);
    MFSR_REQUIRE(std::isfinite(sigma) && sigma > 0.0f);
    MFSR_REQUIRE(radius >= 0 && radius <= kMaxR);
    if (radius == 0) {
        const int r = (int)ceilf(2.5f * sigma);
        radius = r < 1 ? 1 : (r > kMaxR ? kMaxR : r);
    }
    mfsr_sharpen s;
    memset(&s, 0, sizeof(s));
    double w[kMaxR + 1], sum = 0.0;
    for (int d = 0; d <= radius; d++) {
        w[d] = exp(-(double)(d * d) / (2.0 * (double)sigma * (double)sigma));
        sum += d ? 2.0 * w[d] : w[d];
    }
    for (int d = 0; d <= radius; d++) s.taps[d] = (float)(w[d] / sum);
    s.radius = radius;
    s.amount = amount;
    s.threshold = threshold;
    if (int rc = mfsr_sharpen_validate(&s)) return rc;
    *out = s;
    return MFSR_OK;
}

extern "C" int mfsr_sharpenImage(const mfsr_float3* in, int inRowBytes, mfsr_float3* outImg, int outImgRowBytes, void* out,
                                 int outRowBytes, int w, int h, const mfsr_sharpen* sharpen, const mfsr_render* render,
                                 int applyGamma, mfsr_stream_t stream)
{
    if (int rc = stencil_image_args(in, inRowBytes, outImg, outImgRowBytes, out, w, h)) return rc;
    if (int rc = mfsr_sharpen_validate(sharpen)) return rc;
    MFSR_REQUIRE(sharpen_on(sharpen));
    const mfsr_render plain = mfsr_plain_render();
    if (int rc = stencil_render(render, &plain, &render)) return rc;
    if (int rc = stencil_outputs_apart(in, image_span(inRowBytes, h, 12, w), outImg, outImgRowBytes, out, outRowBytes, render->format, w, h))
        return rc;
    const RenderArgs ra = render_args(render, applyGamma);
    const SharpenArgs sa = sharpen_args(sharpen, 0, h - 1);
    const bool lds = stencil_lut_in_lds(render);
    SHARPEN_DISPATCH(k_sharpenImage, render->format, lds, (const pix3*)in, inRowBytes, (pix3*)outImg, outImgRowBytes, (uint8_t*)out,
                     outRowBytes, w, h, sa, ra);
    return mfsr_launch_status("sharpenImage");
}

extern "C" int mfsr_finishSharpened(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes,
                                    const mfsr_float3* fallback, int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0,
                                    float v1, mfsr_float3* outImg, int outImgRowBytes, void* out, int outRowBytes,
                                    const mfsr_render* render, int w, int h, float threshold, int applyGamma, int colOffset,
                                    int rowOffset, int fullWidth, int fullHeight, const mfsr_sharpen* sharpen, int rowsAbove,
                                    int rowsBelow, mfsr_stream_t stream)
{
    if (int rc = stencil_finish_args(finalImg, weight, imgRowBytes, fallback, fbRowBytes, fbW, fbH, outImg, outImgRowBytes, out, w, h,
                                     colOffset, rowOffset, fullWidth, fullHeight, rowsAbove, rowsBelow))
        return rc;
    if (int rc = mfsr_sharpen_validate(sharpen)) return rc;
    MFSR_REQUIRE(sharpen_on(sharpen));
    const mfsr_render plain = mfsr_plain_render();
    if (int rc = stencil_render(render, &plain, &render)) return rc;
    if (int rc = stencil_finish_apart(finalImg, weight, imgRowBytes, rowsAbove, rowsBelow, outImg, outImgRowBytes, out, outRowBytes,
                                      render->format, w, h))
        return rc;
    const RenderArgs ra = render_args(render, applyGamma);
    const SharpenArgs sa = sharpen_args(sharpen, -rowsAbove, h - 1 + rowsBelow);
    const FinishSrc f = finish_src(fallback, fbRowBytes, fbW, fbH, u0, u1, v0, v1, threshold, colOffset, rowOffset, fullWidth, fullHeight);
    const bool lds = stencil_lut_in_lds(render);
    SHARPEN_DISPATCH(k_finishSharpened, render->format, lds, (const pix3*)finalImg, (const pix3*)weight, imgRowBytes, f, (pix3*)outImg,
                     outImgRowBytes, (uint8_t*)out, outRowBytes, w, h, sa, ra);
    return mfsr_launch_status("finishSharpened");
}
