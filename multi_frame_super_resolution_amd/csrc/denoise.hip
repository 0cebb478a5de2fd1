// denoise.hip -- merge-aware denoise inside the finish: a range filter on the linear float value the
// finish holds whose tolerance is the variance the merge left at the pixel, (alpha p + beta) / n, before the colour matrix and
// the tone curve, in the same launch as the finish and the display-format store (mfsr_finishDenoised), and the same tile body
// on an existing float image with an optional count image (mfsr_denoiseImage).  gfx950, wave64.
//
// Every step is float32 + - * / fmaxf fminf with -ffp-contract=off (the Makefile) in the order include/mfsr.h writes it, and the
// range kernel is a polynomial, so a numpy float32 restatement is bit-exact (tests/denoise_ref.py).
//
// A workgroup of 256 lanes owns a kTW x kTH tile of output pixels.  It stages s (the cleaned finish value) of the tile plus a
// halo of R at clamped coordinates in planar LDS (one plane per channel, rows of kTW + 2 * kPad = 72 floats); the tile's first
// column sits at float kPad = 4 of a row whatever R is, so that column 4 * k of the tile is 16-byte aligned.  A wave of a
// one-pixel-per-lane format reads 64 consecutive dwords of one row per tap (no bank conflict in either 32-lane half).  An RGB8
// lane owns four consecutive columns: per row and channel it reads the twelve floats around them as three 16-byte loads
// (ds_read_b128: the 16 lanes of a group read 256 consecutive bytes, every bank once; dword reads at a stride of four would
// put the 32 lanes of a half on 8 banks, a 4-way conflict) and slides its four windows over them in registers.  Those loads go
// through lds_load16, whose volatile access is what keeps them 16 bytes wide in the compiled kernel: the first elements and
// the last of a window are never used and fewer are at R < 3, and the optimiser narrowed plain float4 loads to dword and
// 8-byte reads at the conflicting stride.  Compiled, each RGB8 kernel has 66 ds_read_b128 (3 + 7 rows x 3 channels x 3)
// and no other LDS read of the tile.
// The count n and the fade are needed at the lane's own pixels only: they are read from global memory there, not staged.
// R is a runtime argument: one set of kernels.  The dy and dx loops are unrolled over -kMaxR .. kMaxR with a uniform test
// against R, so every window index is a constant (no scratch) and the row sums of different dy are independent chains.
// The steps clean_value, clean_count, fade_of and denoise_inv_tolerance are finish_stages.hpp's, which the finish chain
// (finish_chain.hip) calls too; its denoise_at restates the one-pixel form of the window loop below, tap weight and blend
// included: change both together.
#include "finish_stages.hpp"
#include "stencil_host.hpp"

namespace {

constexpr int kMaxR = kMaxRd, kPad = 4;
constexpr int kSW = kTW + 2 * kPad, kSH = kTH + 2 * kMaxR;  // the staged extent at R = 3 (columns: padded to the alignment)

// 16 bytes of LDS at a 16-byte aligned address as ONE ds_read_b128.  The load is volatile: a plain float4 load is narrowed by
// the optimiser to the elements a given R uses and sunk into the uniform branches on R (dword and 8-byte reads at a lane
// stride of 16 bytes: the bank conflict this layout exists to avoid).  The assembly is the check: DESIGN.md section 5.
typedef float lds_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void lds_load16(const float* p, float* v)
{
    // (the LDS address space is named: address-space inference leaves a volatile access on a generic pointer a flat load)
    const lds_f32x4 f = *(const volatile __attribute__((address_space(3))) lds_f32x4*)p;
    v[0] = f.x;
    v[1] = f.y;
    v[2] = f.z;
    v[3] = f.w;
}

// The tile of the workgroup at (tileX0, tileY0): fetch(x, y) is p of section 2.24 at a valid pixel of the launch, count(x, y)
// is n before its NaN cleaning at a pixel of the launch's own rows.
template <int FORMAT, class Fetch, class Count>
__device__ __forceinline__ void denoise_tile(const Fetch& fetch, const Count& count, float (*s_s)[kSH][kSW], pix3* outImg,
                                             int outPitch, uint8_t* out, int outRowBytes, int width, int height,
                                             const DenoiseArgs& a, const RenderArgs& r, const float* lut)
{
    const int tid = threadIdx.x, R = a.R;
    const int tileX0 = blockIdx.x * kTW, tileY0 = blockIdx.y * kTH;
    const int sw = kTW + 2 * R, sh = kTH + 2 * R;
    // s of tile + halo at clamped coordinates (what lies beyond the image's last tile is staged too: clamped, never stored)
    for (int i = tid; i < sw * sh; i += kLanes) {
        const int ly = i / sw, lx = i - ly * sw;
        const int gx = min(max(tileX0 + lx - R, 0), width - 1);
        const int gy = min(max(tileY0 + ly - R, a.yLo), a.yHi);
        const pix3 p = fetch(gx, gy);
        const int c0 = lx + (kPad - R);  // (the tile's column 0 at float kPad of the row)
        s_s[0][ly][c0] = clean_value(p.x);
        s_s[1][ly][c0] = clean_value(p.y);
        s_s[2][ly][c0] = clean_value(p.z);
    }
    __syncthreads();
    constexpr int PPL = Fmt<FORMAT>::ppl, lanesX = kTW / PPL, rowsPerPass = kLanes / lanesX;
    // the window of one row a lane holds: columns [lx0 - lead, lx0 + PPL + lead)
    constexpr int lead = PPL == 4 ? 4 : kMaxR, WN = PPL + 2 * lead;
    const int lx0 = (tid % lanesX) * PPL, x0 = tileX0 + lx0;
    for (int ly = tid / lanesX; ly < kTH; ly += rowsPerPass) {  // (the same trip count for every lane of the workgroup)
        const int y = tileY0 + ly;
        const bool active = x0 < width && y < height;
        // the lane's own pixels: s, the cleaned count n and whether any channel has lambda != 0
        float s[PPL][3], n[PPL][3];
        bool need = false;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float* own = &s_s[c][ly + R][lx0 + kPad];
            if constexpr (PPL == 4) {  // (one 16-byte read, as the windows below)
                float f[4];
                lds_load16(own, f);
#pragma unroll
                for (int k = 0; k < PPL; k++) s[k][c] = f[k];
            } else {
                s[0][c] = own[0];
            }
        }
#pragma unroll
        for (int k = 0; k < PPL; k++) {
            const bool valid = active && x0 + k < width;
            pix3 nv = {1.0f, 1.0f, 1.0f};
            if (valid) nv = count(x0 + k, y);
            const float n3[3] = {nv.x, nv.y, nv.z};
#pragma unroll
            for (int c = 0; c < 3; c++) {
                n[k][c] = clean_count(n3[c]);
                need = need || (valid && fade_of(n[k][c], a) != 0.0f);
            }
        }
        float o[PPL][3];
#pragma unroll
        for (int k = 0; k < PPL; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) o[k][c] = s[k][c];
        if (__any(need)) {  // a wave whose every pixel has lambda == 0 in every channel skips the stencil: o = s
            float rr[PPL][3], G[PPL], S[PPL][3];  // (the tolerance's two divisions per channel: only where a wave filters)
#pragma unroll
            for (int k = 0; k < PPL; k++) {
#pragma unroll
                for (int c = 0; c < 3; c++) rr[k][c] = denoise_inv_tolerance(s[k][c], n[k][c], a);
                G[k] = S[k][0] = S[k][1] = S[k][2] = 0.0f;
            }
#pragma unroll
            for (int dy = -kMaxR; dy <= kMaxR; dy++) {
                if (dy < -R || dy > R) continue;  // uniform
                float win[3][WN];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float* row = &s_s[c][ly + R + dy][lx0 + kPad - lead];
                    if constexpr (PPL == 4) {
#pragma unroll
                        for (int q = 0; q < WN; q += 4) lds_load16(row + q, &win[c][q]);
                    } else {
#pragma unroll
                        for (int q = 0; q < WN; q++) win[c][q] = (q - lead >= -R && q - lead <= R) ? row[q] : 0.0f;
                    }
                }
                float Gr[PPL], Sr[PPL][3];
#pragma unroll
                for (int k = 0; k < PPL; k++) Gr[k] = Sr[k][0] = Sr[k][1] = Sr[k][2] = 0.0f;
#pragma unroll
                for (int dx = -kMaxR; dx <= kMaxR; dx++) {
                    if (dx < -R || dx > R) continue;  // uniform
#pragma unroll
                    for (int k = 0; k < PPL; k++) {
                        const float j0 = win[0][lead + k + dx], j1 = win[1][lead + k + dx], j2 = win[2][lead + k + dx];
                        const float d0 = j0 - s[k][0], d1 = j1 - s[k][1], d2 = j2 - s[k][2];
                        const float t = ((d0 * d0) * rr[k][0] + (d1 * d1) * rr[k][1]) + (d2 * d2) * rr[k][2];
                        const float u = fmaxf(1.0f - t, 0.0f);
                        const float g = u * u;
                        Gr[k] = Gr[k] + g;
                        Sr[k][0] = Sr[k][0] + g * j0;
                        Sr[k][1] = Sr[k][1] + g * j1;
                        Sr[k][2] = Sr[k][2] + g * j2;
                    }
                }
#pragma unroll
                for (int k = 0; k < PPL; k++) {
                    G[k] = G[k] + Gr[k];
                    S[k][0] = S[k][0] + Sr[k][0];
                    S[k][1] = S[k][1] + Sr[k][1];
                    S[k][2] = S[k][2] + Sr[k][2];
                }
            }
#pragma unroll
            for (int k = 0; k < PPL; k++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float f = S[k][c] / G[k], l = fade_of(n[k][c], a);
                    o[k][c] = l == 0.0f ? s[k][c] : s[k][c] + l * (f - s[k][c]);
                }
        }
        if (!active) continue;
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
    k_denoiseImage(const pix3* __restrict__ in, int inPitch, const pix3* __restrict__ cnt, int cntPitch, pix3* __restrict__ outImg,
                   int outPitch, uint8_t* __restrict__ out, int outRowBytes, int width, int height, DenoiseArgs a, RenderArgs r)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    __shared__ __attribute__((aligned(16))) float s_s[3][kSH][kSW];
    const float* lut = stage_lut<LDS>(r, s_lut);
    auto fetch = [&](int x, int y) { return row_ptr(in, inPitch, y)[x]; };
    auto count = [&](int x, int y) {
        pix3 n = {1.0f, 1.0f, 1.0f};
        if (cnt) n = row_ptr(cnt, cntPitch, y)[x];  // uniform
        return n;
    };
    denoise_tile<FORMAT>(fetch, count, s_s, outImg, outPitch, out, outRowBytes, width, height, a, r, lut);
}

template <int FORMAT, int LDS>
__global__ void __launch_bounds__(kLanes)
    k_finishDenoised(const pix3* __restrict__ finalImg, const pix3* __restrict__ weight, int imgPitch, FinishSrc f,
                     pix3* __restrict__ outImg, int outPitch, uint8_t* __restrict__ out, int outRowBytes, int width, int height,
                     DenoiseArgs a, RenderArgs r)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    __shared__ __attribute__((aligned(16))) float s_s[3][kSH][kSW];
    const float* lut = stage_lut<LDS>(r, s_lut);
    // k_finishRendered's value (finish_value_at: one definition); y may be negative (rowsAbove)
    auto fetch = [&](int x, int y) { return finish_value_at(finalImg, weight, imgPitch, x, y, f); };
    // step 2: the count apply_weight_f divided by
    auto count = [&](int x, int y) {
        pix3 n = row_ptr(weight, imgPitch, y)[x];
        if (n.x < f.threshold) n.x += 1;
        if (n.y < f.threshold) n.y += 1;
        if (n.z < f.threshold) n.z += 1;
        return n;
    };
    denoise_tile<FORMAT>(fetch, count, s_s, outImg, outPitch, out, outRowBytes, width, height, a, r, lut);
}

}  // namespace

// (the tone table follows the sharpened kernels' decision: stencil_lut_in_lds)
#define DENOISE_DISPATCH(KERNEL, format, lds, ...) STENCIL_DISPATCH(KERNEL, kTW, kTH, kLanes, format, lds, __VA_ARGS__)

extern "C" int mfsr_denoise_tile(int* tileW, int* tileH)
{
    MFSR_REQUIRE(tileW && tileH);
    *tileW = kTW;
    *tileH = kTH;
    return MFSR_OK;
}

extern "C" int mfsr_denoise_validate(const mfsr_denoise* d)
{
    MFSR_REQUIRE(d != nullptr);
    MFSR_REQUIRE(d->radius >= 0 && d->radius <= kMaxR);
    MFSR_REQUIRE(std::isfinite(d->strength) && (d->strength == 0.0f || (d->strength >= 0.0625f && d->strength <= 16.0f)));
    MFSR_REQUIRE(std::isfinite(d->gain) && d->gain > 0.0f && d->gain <= 1024.0f);
    MFSR_REQUIRE(std::isfinite(d->alpha) && d->alpha >= 0.0f && d->alpha <= 1.0f);
    MFSR_REQUIRE(std::isfinite(d->beta) && d->beta >= 0.0f && d->beta <= 1.0f);
    MFSR_REQUIRE(std::isfinite(d->wLo) && std::isfinite(d->wHi) && d->wLo >= 0.0f);
    MFSR_REQUIRE(d->wHi <= d->wLo || d->wHi - d->wLo >= 0.0009765625f);
    for (int i = 0; i < 5; i++) MFSR_REQUIRE(d->reserved[i] == 0);
    return MFSR_OK;
}

extern "C" int mfsr_denoise_defaults(float alpha, float beta, mfsr_denoise* out)
{
    MFSR_REQUIRE(out != nullptr);
    mfsr_denoise d;
    memset(&d, 0, sizeof(d));
    d.radius = 2;
    d.strength = 3.0f;
    d.gain = 2.0f;
    d.alpha = alpha;
    d.beta = beta;
    if (int rc = mfsr_denoise_validate(&d)) return rc;
    *out = d;
    return MFSR_OK;
}

extern "C" int mfsr_denoiseImage(const mfsr_float3* in, int inRowBytes, const mfsr_float3* count, int countRowBytes,
                                 mfsr_float3* outImg, int outImgRowBytes, void* out, int outRowBytes, int w, int h,
                                 const mfsr_denoise* denoise, const mfsr_render* render, int applyGamma, mfsr_stream_t stream)
{
    if (int rc = stencil_image_args(in, inRowBytes, outImg, outImgRowBytes, out, w, h)) return rc;
    if (count) MFSR_REQUIRE((long long)countRowBytes >= 12LL * w && (countRowBytes & 3) == 0 && ((uintptr_t)count & 3) == 0);
    if (int rc = mfsr_denoise_validate(denoise)) return rc;
    MFSR_REQUIRE(denoise_on(denoise));
    const mfsr_render plain = mfsr_plain_render();
    if (int rc = stencil_render(render, &plain, &render)) return rc;
    if (int rc = stencil_outputs_apart(in, image_span(inRowBytes, h, 12, w), outImg, outImgRowBytes, out, outRowBytes, render->format, w, h))
        return rc;
    if (count)
        if (int rc = stencil_outputs_apart(count, image_span(countRowBytes, h, 12, w), outImg, outImgRowBytes, out, outRowBytes,
                                           render->format, w, h))
            return rc;
    const RenderArgs ra = render_args(render, applyGamma);
    const DenoiseArgs da = denoise_args(denoise, 0, h - 1);
    const bool lds = stencil_lut_in_lds(render);
    DENOISE_DISPATCH(k_denoiseImage, render->format, lds, (const pix3*)in, inRowBytes, (const pix3*)count, countRowBytes, (pix3*)outImg,
                     outImgRowBytes, (uint8_t*)out, outRowBytes, w, h, da, ra);
    return mfsr_launch_status("denoiseImage");
}

extern "C" int mfsr_finishDenoised(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes,
                                   const mfsr_float3* fallback, int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0,
                                   float v1, mfsr_float3* outImg, int outImgRowBytes, void* out, int outRowBytes,
                                   const mfsr_render* render, int w, int h, float threshold, int applyGamma, int colOffset,
                                   int rowOffset, int fullWidth, int fullHeight, const mfsr_denoise* denoise, int rowsAbove,
                                   int rowsBelow, mfsr_stream_t stream)
{
    if (int rc = stencil_finish_args(finalImg, weight, imgRowBytes, fallback, fbRowBytes, fbW, fbH, outImg, outImgRowBytes, out, w, h,
                                     colOffset, rowOffset, fullWidth, fullHeight, rowsAbove, rowsBelow))
        return rc;
    if (int rc = mfsr_denoise_validate(denoise)) return rc;
    MFSR_REQUIRE(denoise_on(denoise));
    const mfsr_render plain = mfsr_plain_render();
    if (int rc = stencil_render(render, &plain, &render)) return rc;
    if (int rc = stencil_finish_apart(finalImg, weight, imgRowBytes, rowsAbove, rowsBelow, outImg, outImgRowBytes, out, outRowBytes,
                                      render->format, w, h))
        return rc;
    const RenderArgs ra = render_args(render, applyGamma);
    const DenoiseArgs da = denoise_args(denoise, -rowsAbove, h - 1 + rowsBelow);
    const bool lds = stencil_lut_in_lds(render);
    const FinishSrc f = finish_src(fallback, fbRowBytes, fbW, fbH, u0, u1, v0, v1, threshold, colOffset, rowOffset, fullWidth, fullHeight);
    DENOISE_DISPATCH(k_finishDenoised, render->format, lds, (const pix3*)finalImg, (const pix3*)weight, imgRowBytes, f, (pix3*)outImg,
                     outImgRowBytes, (uint8_t*)out, outRowBytes, w, h, da, ra);
    return mfsr_launch_status("finishDenoised");
}
