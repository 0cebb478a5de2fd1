// accumulate_common.hpp -- tap arithmetic shared by the accumulate kernels
// (reference test_opencv/DeBayerKernels.cu:288-468).
#pragma once
#include <type_traits>
#include <utility>
#include "common.hpp"
#include "margin_sites.hpp"

struct Levels3 {
    float white[3], black[3];
};

static inline Levels3 make_levels(mfsr_float3 white, mfsr_float3 black)
{
    Levels3 l;
    l.white[0] = white.x;
    l.white[1] = white.y;
    l.white[2] = white.z;
    l.black[0] = black.x;
    l.black[1] = black.y;
    l.black[2] = black.z;
    return l;
}

template <bool FAST>
__device__ __forceinline__ float tap_weight(int px, int py, float kx, float ky, float kz)
{
    // DeBayerKernels.cu:335-338 / :427-430
    float w = (float)(px * px) * kx + (float)(2 * px * py) * kz + (float)(py * py) * ky;
    if (FAST) {
        const float t = w * -0.72134752044448170368f;  // -0.5 * log2(e)
        w = __builtin_amdgcn_exp2f(t);
    } else {
        w = expf(-0.5f * w);
    }
    if (!finitef(w)) w = (px * py == 0) ? 1.0f : 0.0f;
    return w;
}

__device__ __forceinline__ void tap_accumulate(float raw, float w, int color, const float4& cert4, const Levels3& lv,
                                               pix3& pixel, pix3& totalWeight)
{
    // DeBayerKernels.cu:342-370 / :434-462
    if (color == MFSR_GREEN) {
        raw = (raw - lv.black[1]) / lv.white[1];
        float certainty = cert4.y;
        if (!finitef(certainty)) certainty = 0.0f;
        pixel.y += raw * w * certainty;
        totalWeight.y += w * certainty;
    } else if (color == MFSR_RED) {
        raw = (raw - lv.black[0]) / lv.white[0];
        float certainty = cert4.x;
        if (!finitef(certainty)) certainty = 0.0f;
        pixel.x += raw * w * certainty;
        totalWeight.x += w * certainty;
    } else if (color == MFSR_BLUE) {
        raw = (raw - lv.black[2]) / lv.white[2];
        float certainty = cert4.z;
        if (!finitef(certainty)) certainty = 0.0f;
        pixel.z += raw * w * certainty;
        totalWeight.z += w * certainty;
    }
}


// tap_accumulate for the FAST kernels: the white level enters as a reciprocal (one v_rcp per channel and
// pixel instead of an IEEE division per tap); inside the FAST kernels' tolerance, not bit-identical to
// tap_accumulate.  (A branch-free variant -- operands picked with selects, masked adds to all three
// channels -- was measured slower: 36 instead of 28 us for the margin kernel.)
__device__ __forceinline__ void tap_accumulate_fast(float raw, float w, int color, const float4& cert4, const Levels3& lv,
                                                    const float (&invWhite)[3], pix3& pixel, pix3& totalWeight)
{
    if (color == MFSR_GREEN) {
        raw = (raw - lv.black[1]) * invWhite[1];
        float certainty = cert4.y;
        if (!finitef(certainty)) certainty = 0.0f;
        pixel.y += raw * w * certainty;
        totalWeight.y += w * certainty;
    } else if (color == MFSR_RED) {
        raw = (raw - lv.black[0]) * invWhite[0];
        float certainty = cert4.x;
        if (!finitef(certainty)) certainty = 0.0f;
        pixel.x += raw * w * certainty;
        totalWeight.x += w * certainty;
    } else if (color == MFSR_BLUE) {
        raw = (raw - lv.black[2]) * invWhite[2];
        float certainty = cert4.z;
        if (!finitef(certainty)) certainty = 0.0f;
        pixel.z += raw * w * certainty;
        totalWeight.z += w * certainty;
    }
}

// Branch-free tap for the kernels that run the straight arithmetic on whole wavefronts (frame margin): the three colour
// branches of tap_accumulate_fast all execute when the lanes of a wave sit on different colours (they always do on a
// Bayer row).  Here the tap adds (raw / wm) * w * c and w * c to per-COLOUR sums with lane masks (wm = the largest white
// level: a colour-independent scale that keeps the terms <= w * c -- kernel parameters that are not positive
// semi-definite give weights up to 1e38, and sums of un-scaled raw * w * c would overflow where the reference's do not);
// black and white level enter once per pixel: sum((raw - b) / wl * w c) = sum(raw / wm * w c) * (wm / wl) - (b / wl) * sum(w c).
__device__ __forceinline__ void tap_accumulate_sums(float raw, float w, int color, const float4& cert4, float invWm, float (&S)[3],
                                                    float (&W)[3])
{
    float certainty = color == MFSR_GREEN ? cert4.y : (color == MFSR_RED ? cert4.x : cert4.z);
    if (!finitef(certainty)) certainty = 0.0f;
    const float t = w * certainty;
    const float v = (raw * invWm) * t;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint32_t m = 0u - (uint32_t)(color == c);  // MFSR_RED = 0, MFSR_GREEN = 1, MFSR_BLUE = 2
        S[c] += __uint_as_float(m & __float_as_uint(v));
        W[c] += __uint_as_float(m & __float_as_uint(t));
    }
}

// GEOM_CROP: the reference geometry (x2, output grid dimX x dimY over the central
//            half of the frame).
// GEOM_FULL: scale s, output grid (s*dimX) x (s*dimY) over the whole frame.
enum { GEOM_CROP = 0, GEOM_FULL = 1 };

__device__ __forceinline__ int floordiv_pos(int a, int s)
{
    // floor(a / s) for s > 0 and any a
    int q = a / s;
    return (a % s < 0) ? q - 1 : q;
}

// One output pixel of accumulateImagesSuperRes (:379-468) / its full-frame
// generalisation, straight from the reference: read-modify-write of imgOut and
// totalWeights at (x, y).  Caller guarantees 1 <= x < outW-1, 1 <= y < outH-1.
// core: accumulates the 25 taps of output pixel (x, y) into the register values pixel / totalWeight
template <int GEOM, bool FAST, bool SUMS = false>
__device__ __forceinline__ void accumulate_pixel_core(int x, int y, const uint16_t* __restrict__ dataIn,
                                                      const float4* __restrict__ certaintyMask,
                                                      const mfsr_tex2d& kernelParam, const mfsr_tex2d& shifts,
                                                      const Levels3& lv, int dimX, int dimY, int scale, int strideMask,
                                                      int cfa, pix3& pixel, pix3& totalWeight)
{
    const int outW = (GEOM == GEOM_CROP) ? dimX : dimX * scale;
    const int outH = (GEOM == GEOM_CROP) ? dimY : dimY * scale;

    float posX, posY, fscale;
    if (GEOM == GEOM_CROP) {
        posX = ((float)x + 0.5f + (float)(dimX / 2)) / 2.0f / (float)dimX;  // :398
        posY = ((float)y + 0.5f + (float)(dimY / 2)) / 2.0f / (float)dimY;
        fscale = 2.0f;
    } else {
        posX = ((float)x + 0.5f) / (float)outW;
        posY = ((float)y + 0.5f) / (float)outH;
        fscale = (float)scale;
    }
    const float4 kernel = tex4<ADDR_CLAMP>(kernelParam, posX, posY);
    const float2 shift = tex2<ADDR_CLAMP>(shifts, posX, posY);
    const int sx = round2i(shift.x * fscale);  // :403-406
    const int sy = round2i(shift.y * fscale);

    // FAST: the 13 distinct weights (w(px,py) == w(-px,-py), and so is the non-finite rule) and the
    // reciprocal white levels, once per pixel
    float wSym[13];
    float invWhite[3] = {0.0f, 0.0f, 0.0f};
    if (FAST) {
#pragma unroll
        for (int n = 0; n < 13; n++) wSym[n] = tap_weight<true>(n % 5 - 2, n / 5 - 2, kernel.x, kernel.y, kernel.z);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) invWhite[ch] = __builtin_amdgcn_rcpf(lv.white[ch]);
    }
    float sumS[3] = {0.0f, 0.0f, 0.0f}, sumW[3] = {0.0f, 0.0f, 0.0f};  // SUMS: per-colour sums of this call
    const float wm = fmaxf(fmaxf(lv.white[0], lv.white[1]), lv.white[2]);
    const float invWm = __builtin_amdgcn_rcpf(wm);
    int ppsxA[5], ppxA[5];
#pragma unroll
    for (int px = -2; px <= 2; px++) {
        if (GEOM == GEOM_CROP) {
            ppsxA[px + 2] = clampi((x + px + sx + dimX / 2) / 2, dimX / 4, dimX / 2 - 1 + dimX / 4);  // :419
            ppxA[px + 2] = clampi((x + px + dimX / 2) / 2, dimX / 4, dimX / 2 - 1 + dimX / 4);        // :422
        } else {
            ppsxA[px + 2] = clampi(floordiv_pos(x + px + sx, scale), 0, dimX - 1);
            ppxA[px + 2] = clampi(floordiv_pos(x + px, scale), 0, dimX - 1);
        }
    }
    auto taps = [&](auto useSums) {
#pragma unroll
        for (int py = -2; py <= 2; py++) {
            int ppsy, ppy;
            if (GEOM == GEOM_CROP) {
                ppsy = clampi((y + py + sy + dimY / 2) / 2, dimY / 4, dimY / 2 - 1 + dimY / 4);
                ppy = clampi((y + py + dimY / 2) / 2, dimY / 4, dimY / 2 - 1 + dimY / 4);
            } else {
                ppsy = clampi(floordiv_pos(y + py + sy, scale), 0, dimY - 1);
                ppy = clampi(floordiv_pos(y + py, scale), 0, dimY - 1);
            }
            const uint16_t* rawRow = dataIn + (size_t)ppsy * dimX;
            const float4* maskRow = row_ptr(certaintyMask, strideMask, ppy / 2);
#pragma unroll
            for (int px = -2; px <= 2; px++) {
                const int ppsx = ppsxA[px + 2];
                const int color = cfa_at(cfa, ppsy, ppsx);
                const float raw = (float)rawRow[ppsx];
                const float4 cert4 = maskRow[ppxA[px + 2] / 2];
                if constexpr (decltype(useSums)::value) {
                    const int n = (py + 2) * 5 + (px + 2);
                    tap_accumulate_sums(raw, wSym[n <= 12 ? n : 24 - n], color, cert4, invWm, sumS, sumW);
                } else if (FAST) {
                    const int n = (py + 2) * 5 + (px + 2);
                    tap_accumulate_fast(raw, wSym[n <= 12 ? n : 24 - n], color, cert4, lv, invWhite, pixel, totalWeight);
                } else {
                    const float w = tap_weight<false>(px, py, kernel.x, kernel.y, kernel.z);
                    tap_accumulate(raw, w, color, cert4, lv, pixel, totalWeight);
                }
            }
        }
    };
    // per-colour sums with deferred levels only where every weight is in [0, 1] (positive semi-definite kernel parameters):
    // other pixels (weights up to 1e38 -- hostile input, rare) keep the per-tap normalisation, whose overflow behaviour is
    // the reference's
    const bool sums = FAST && SUMS && kernel.x >= 0.0f && kernel.y >= 0.0f && kernel.z * kernel.z <= kernel.x * kernel.y &&
                      kernel.x < 1e30f && kernel.y < 1e30f;
    if (sums)
        taps(std::true_type{});
    else
        taps(std::false_type{});
    if (sums) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float v = __builtin_fmaf(sumS[ch], wm * invWhite[ch], -(lv.black[ch] * invWhite[ch]) * sumW[ch]);
            if (ch == 0) pixel.x += v;
            if (ch == 1) pixel.y += v;
            if (ch == 2) pixel.z += v;
        }
        totalWeight.x += sumW[0];
        totalWeight.y += sumW[1];
        totalWeight.z += sumW[2];
    }
    (void)outW;
    (void)outH;
}

template <int GEOM, bool FAST, bool SUMS = false>
__device__ __forceinline__ void accumulate_pixel_generic(int x, int y, const uint16_t* __restrict__ dataIn,
                                                         pix3* __restrict__ imgOut, pix3* __restrict__ totalWeights,
                                                         const float4* __restrict__ certaintyMask,
                                                         const mfsr_tex2d& kernelParam, const mfsr_tex2d& shifts,
                                                         const Levels3& lv, int dimX, int dimY, int scale, int strideOut,
                                                         int strideMask, int cfa, int accX0 = 0, int accY0 = 0)
{
    // (accX0, accY0): HR pixel the accumulators' first element stands for (a window's origin; 0, 0 for whole-frame planes)
    pix3 pixel = row_ptr(imgOut, strideOut, y - accY0)[x - accX0];
    pix3 totalWeight = row_ptr(totalWeights, strideOut, y - accY0)[x - accX0];
    accumulate_pixel_core<GEOM, FAST, SUMS>(x, y, dataIn, certaintyMask, kernelParam, shifts, lv, dimX, dimY, scale, strideMask,
                                      cfa, pixel, totalWeight);
    row_ptr(imgOut, strideOut, y - accY0)[x - accX0] = pixel;
    row_ptr(totalWeights, strideOut, y - accY0)[x - accX0] = totalWeight;
}

// ---- the site-wise straight body of the margin kernels (GEOM_FULL, FAST, SUMS) ----------------------------------------------
// accumulate_pixel_core<GEOM_FULL, true, true> visits 25 taps and for each loads, converts, scales and colour-classifies a raw
// sample and loads and checks a certainty texel -- of 3 x 3 (x2) or 2 x 2 (x4) distinct raw sites and at most 2 x 2 distinct
// certainty texels.  accumulate_pixel_sites does that work once per site and per texel (margin_sites.hpp: the mapping) and
// leaves the tap only what is the tap's: per colour c the products t_c = w * certainty_c and v_c = (raw * invWm) * t_c, with
// certainty_c masked to +0.0 where the tap's site is not of colour c, added to W[c] and S[c] in the tap order of
// accumulate_pixel_core.  For the site's colour these are t and v of tap_accumulate_sums; for the other two the addend is a
// zero where tap_accumulate_sums adds a masked +0.0, and the sums start at +0.0, so they are never -0.0 and x + (+-0.0) == x
// (the argument is at the tap).  Every S[c] and W[c] therefore goes through the same values in the same order: the same
// bits.  No add is dropped: which of a tap's adds is the zero depends on the lane.
// What depends on the pixel alone comes from the caller: the 13 distinct tap weights (wsym(n), n = 0..12: tap_weight<true>
// of tap n) and the `sums` predicate of the pixel's kernel parameters, margin_pixel_sums().

// normalised position of HR pixel (x, y): where accumulate_pixel_core<GEOM_FULL> reads the kernel parameters and the flow
template <int SCALE>
__device__ __forceinline__ float2 margin_pixel_pos(int x, int y, int dimX, int dimY)
{
    return make_float2(((float)x + 0.5f) / (float)(dimX * SCALE), ((float)y + 0.5f) / (float)(dimY * SCALE));
}

// the 13 weights' predicate of accumulate_pixel_core: every weight in [0, 1] (positive semi-definite kernel parameters)
__device__ __forceinline__ bool margin_pixel_sums(const float4& kernel)
{
    return kernel.x >= 0.0f && kernel.y >= 0.0f && kernel.z * kernel.z <= kernel.x * kernel.y && kernel.x < 1e30f && kernel.y < 1e30f;
}

// the per-tap loops of accumulate_pixel_core<GEOM_FULL, true, SUMS> with the flow and the weights given: the pixels the
// site-wise body does not take
template <int SCALE, bool USE_SUMS, class WF>
__device__ __forceinline__ void margin_pixel_taps(int x, int y, int sx, int sy, const uint16_t* __restrict__ dataIn,
                                                  const float4* __restrict__ certaintyMask, const Levels3& lv,
                                                  const float (&invWhite)[3], float invWm, int dimX, int dimY, int strideMask, int cfa,
                                                  WF wsym, float (&sumS)[3], float (&sumW)[3], pix3& pixel, pix3& totalWeight)
{
    int ppsxA[5], ppxA[5];
#pragma unroll
    for (int px = -2; px <= 2; px++) {
        ppsxA[px + 2] = clampi(floordiv_pos(x + px + sx, SCALE), 0, dimX - 1);
        ppxA[px + 2] = clampi(floordiv_pos(x + px, SCALE), 0, dimX - 1);
    }
#pragma unroll
    for (int py = -2; py <= 2; py++) {
        const int ppsy = clampi(floordiv_pos(y + py + sy, SCALE), 0, dimY - 1);
        const int ppy = clampi(floordiv_pos(y + py, SCALE), 0, dimY - 1);
        const uint16_t* rawRow = dataIn + (size_t)ppsy * dimX;
        const float4* maskRow = row_ptr(certaintyMask, strideMask, ppy / 2);
#pragma unroll
        for (int px = -2; px <= 2; px++) {
            const int ppsx = ppsxA[px + 2];
            const int color = cfa_at(cfa, ppsy, ppsx);
            const float raw = (float)rawRow[ppsx];
            const float4 cert4 = maskRow[ppxA[px + 2] / 2];
            const int n = (py + 2) * 5 + (px + 2);
            const float w = wsym(n <= 12 ? n : 24 - n);
            if (USE_SUMS)
                tap_accumulate_sums(raw, w, color, cert4, invWm, sumS, sumW);
            else
                tap_accumulate_fast(raw, w, color, cert4, lv, invWhite, pixel, totalWeight);
        }
    }
}

template <class F, int... I>
__device__ __forceinline__ void margin_static_for_impl(F&& f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void margin_static_for(F&& f)
{
    margin_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// the taps of a pixel whose flow keeps x + px + sx far from the ends of int, site-wise
template <int SCALE, class WF>
__device__ __forceinline__ void margin_pixel_sites(int x, int y, int sx, int sy, const uint16_t* __restrict__ dataIn,
                                                   const float4* __restrict__ certaintyMask, float invWm, int dimX, int dimY,
                                                   int strideMask, int cfa, WF wsym, float (&S)[3], float (&W)[3])
{
    constexpr int NS = MarginSites<SCALE>::count;
    int bx, phx, by, phy;
    margin_axis<SCALE>(x + sx - 2, bx, phx);
    margin_axis<SCALE>(y + sy - 2, by, phy);
    int cellX[2], cellY[2], qx, qy;
    margin_cert_axis<SCALE>(x - 2, dimX, cellX, qx);
    margin_cert_axis<SCALE>(y - 2, dimY, cellY, qy);
    // the certainty texels, non-finite components replaced once.  Addresses: one base per frame and a 32-bit offset (the
    // launchers take this body for planes below 2 GiB only)
    float cert[2][2][3];
#pragma unroll
    for (int cj = 0; cj < 2; cj++)
#pragma unroll
        for (int ci = 0; ci < 2; ci++) {
            const uint32_t off = (uint32_t)(cellY[cj] * strideMask) + (uint32_t)cellX[ci] * 16u;
            const float4 c = *(const float4*)((const char*)certaintyMask + off);
            cert[cj][ci][0] = finitef(c.x) ? c.x : 0.0f;
            cert[cj][ci][1] = finitef(c.y) ? c.y : 0.0f;
            cert[cj][ci][2] = finitef(c.z) ? c.z : 0.0f;
        }
    // the raw sites: sample * invWm and colour.  The colour of a site is the CFA word's byte at (row parity, column parity) of
    // the CLAMPED site (clamped sites repeat a coordinate, so site columns 0 and 2 need not share a colour at the border).
    // It is kept one-hot (bit c: colour c; the CFA word holds colours 0..3, mfsr_set_cfa_pattern): a tap's lane mask of
    // colour c is bit c of it spread over the word, and masking a value is one v_and.
    uint32_t hotWord = 0;  // the CFA word with 1 << colour in each byte (launch-uniform: scalar code)
#pragma unroll
    for (int k = 0; k < 4; k++) hotWord |= (1u << (((uint32_t)cfa >> (8 * k)) & 31u)) << (8 * k);
    int cxA[NS], xsh[NS];
#pragma unroll
    for (int i = 0; i < NS; i++) {
        cxA[i] = margin_site_coord(bx, i, dimX);
        xsh[i] = (margin_site_cfa_pos(0, cxA[i])) << 3;
    }
    float r[NS][NS];
    uint32_t hot[NS][NS];
#pragma unroll
    for (int j = 0; j < NS; j++) {
        const int ry = margin_site_coord(by, j, dimY);
        const uint32_t rowOff = (uint32_t)(ry * dimX);
        const uint32_t rowWord = hotWord >> (margin_site_cfa_pos(ry, 0) << 3);
#pragma unroll
        for (int i = 0; i < NS; i++) {
            r[j][i] = (float)dataIn[rowOff + (uint32_t)cxA[i]] * invWm;
            hot[j][i] = (rowWord >> xsh[i]) & 0xffu;
        }
    }
    // (tap indices as compile-time constants: with loop counters the site arrays end up indexed at run time)
    margin_static_for<5>([&](auto jtTag) {
        // the site row and the certainty cell row of this tap row
        constexpr int jt = decltype(jtTag)::value;
        constexpr int jlo = margin_tap_site_lo<SCALE>(jt), jhi = jlo + 1 < NS ? jlo + 1 : jlo;
        const bool cy = margin_tap_carry_varies<SCALE>(jt) && margin_tap_carry<SCALE>(phy, jt) != 0;
        float rRow[NS];
        uint32_t hotRow[NS];
#pragma unroll
        for (int i = 0; i < NS; i++) {
            rRow[i] = cy ? r[jhi][i] : r[jlo][i];
            hotRow[i] = cy ? hot[jhi][i] : hot[jlo][i];
        }
        const bool my = margin_tap_cell_varies<SCALE>(jt) ? margin_tap_cell<SCALE>(qy, jt) != 0 : jt != 0;
        float certRow[2][3];
#pragma unroll
        for (int ci = 0; ci < 2; ci++)
#pragma unroll
            for (int k = 0; k < 3; k++) certRow[ci][k] = my ? cert[1][ci][k] : cert[0][ci][k];
        margin_static_for<5>([&](auto itTag) {
            constexpr int it = decltype(itTag)::value;
            constexpr int ilo = margin_tap_site_lo<SCALE>(it), ihi = ilo + 1 < NS ? ilo + 1 : ilo;
            const bool cx = margin_tap_carry_varies<SCALE>(it) && margin_tap_carry<SCALE>(phx, it) != 0;
            const float raw = cx ? rRow[ihi] : rRow[ilo];
            const uint32_t h = cx ? hotRow[ihi] : hotRow[ilo];
            uint32_t m[3];  // MFSR_RED = 0, MFSR_GREEN = 1, MFSR_BLUE = 2
#pragma unroll
            for (int c = 0; c < 3; c++) m[c] = (uint32_t)__builtin_amdgcn_sbfe((int)h, c, 1);
            const bool mx = margin_tap_cell_varies<SCALE>(it) ? margin_tap_cell<SCALE>(qx, it) != 0 : it != 0;
            const float cR = mx ? certRow[1][0] : certRow[0][0];
            const float cG = mx ? certRow[1][1] : certRow[0][1];
            const float cB = mx ? certRow[1][2] : certRow[0][2];
            // per colour c the tap adds t_c = w * (m_c & certainty_c) and v_c = raw * t_c: t and v of tap_accumulate_sums for the
            // site's colour, and +-0.0 for the other two -- w is finite and >= 0 under the sums predicate and raw is finite
            // (the caller checks invWm), so w * (+0.0) and raw * (+0.0) are zeros, and a sum that started at +0.0 is never
            // -0.0: x + (+-0.0) == x, the bits of the masked adds.  No colour pick of the certainty, no t and v besides.
            const float cc[3] = {cR, cG, cB};
            const float w = wsym(jt * 5 + it <= 12 ? jt * 5 + it : 24 - (jt * 5 + it));
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float tc = w * __uint_as_float(m[c] & __float_as_uint(cc[c]));
                W[c] += tc;
                S[c] += raw * tc;
            }
        });
    });
}

// One margin pixel of one frame: accumulate_pixel_core<GEOM_FULL, true, true> with the pixel's weights and predicate given.
// Pixels whose kernel parameters fail the predicate keep the per-tap normalisation, and so do pixels with a flow beyond
// +-2^30 HR pixels (an infinite flow rounds to INT_MAX): there x + px + sx wraps around for some taps of a pixel and not for
// others, and taps that share a site no longer share the coordinate the per-tap expression gives them.
template <int SCALE, class WF>
__device__ __forceinline__ void accumulate_pixel_sites(int x, int y, const uint16_t* __restrict__ dataIn,
                                                       const float4* __restrict__ certaintyMask, const mfsr_tex2d& shifts,
                                                       const Levels3& lv, int dimX, int dimY, int strideMask, int cfa, float posX,
                                                       float posY, bool sums, WF wsym, pix3& pixel, pix3& totalWeight)
{
    // (posX, posY): margin_pixel_pos(x, y) -- the pixel's, the same for every frame
    const float2 shift = tex2<ADDR_CLAMP>(shifts, posX, posY);
    const int sx = round2i(shift.x * (float)SCALE);
    const int sy = round2i(shift.y * (float)SCALE);
    float invWhite[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) invWhite[ch] = __builtin_amdgcn_rcpf(lv.white[ch]);
    const float wm = fmaxf(fmaxf(lv.white[0], lv.white[1]), lv.white[2]);
    const float invWm = __builtin_amdgcn_rcpf(wm);
    float sumS[3] = {0.0f, 0.0f, 0.0f}, sumW[3] = {0.0f, 0.0f, 0.0f};
    const bool inRange = (uint32_t)sx + (1u << 30) <= (2u << 30) && (uint32_t)sy + (1u << 30) <= (2u << 30) && finitef(invWm);
    // (the per-tap paths work on opaque copies: their clamps and addresses are otherwise hoisted above the branch, into
    // every pixel's way)
    int xo = x, yo = y, sxo = sx, syo = sy;
    if (sums && inRange) {
        margin_pixel_sites<SCALE>(x, y, sx, sy, dataIn, certaintyMask, invWm, dimX, dimY, strideMask, cfa, wsym, sumS, sumW);
    } else if (sums) {
        asm volatile("" : "+v"(xo), "+v"(yo), "+v"(sxo), "+v"(syo));
        margin_pixel_taps<SCALE, true>(xo, yo, sxo, syo, dataIn, certaintyMask, lv, invWhite, invWm, dimX, dimY, strideMask, cfa, wsym, sumS,
                                       sumW, pixel, totalWeight);
    } else {
        asm volatile("" : "+v"(xo), "+v"(yo), "+v"(sxo), "+v"(syo));
        margin_pixel_taps<SCALE, false>(xo, yo, sxo, syo, dataIn, certaintyMask, lv, invWhite, invWm, dimX, dimY, strideMask, cfa, wsym, sumS,
                                        sumW, pixel, totalWeight);
    }
    if (sums) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float v = __builtin_fmaf(sumS[ch], wm * invWhite[ch], -(lv.black[ch] * invWhite[ch]) * sumW[ch]);
            if (ch == 0) pixel.x += v;
            if (ch == 1) pixel.y += v;
            if (ch == 2) pixel.z += v;
        }
        totalWeight.x += sumW[0];
        totalWeight.y += sumW[1];
        totalWeight.z += sumW[2];
    }
}

// HR output window of a warp+fuse launch: pixels [x0, x1) x [y0, y1) of the whole-frame grid.  rel = 0: the accumulators are
// the whole frame's (pointer = pixel (0, 0)); rel = 1: they hold the window only (pointer = pixel (x0, y0)).
struct HrWindow {
    int x0, y0, x1, y1;
    int rel;
};

// the frame-border margin ring of the fast kernels (x in [1, M) or [hrW-M, hrW-1), y in [1, M) or [hrH-M, hrH-1)) cut to a
// window: four rectangles enumerated back to back (start[r] = first thread index of rectangle r, start[4] = their total)
struct MarginRects {
    int x0[4], y0[4], w[4];
    int start[5];
    int accX0, accY0;  // origin of the window-relative accumulators
};

inline MarginRects margin_rects(int hrW, int hrH, int M, const HrWindow& w)
{
    const int r[4][4] = {{1, 1, hrW - 1, M}, {1, hrH - M, hrW - 1, hrH - 1}, {1, M, M, hrH - M}, {hrW - M, M, hrW - 1, hrH - M}};
    MarginRects m{};
    m.start[0] = 0;
    for (int i = 0; i < 4; i++) {
        const int x0 = r[i][0] > w.x0 ? r[i][0] : w.x0, x1 = r[i][2] < w.x1 ? r[i][2] : w.x1;
        const int y0 = r[i][1] > w.y0 ? r[i][1] : w.y0, y1 = r[i][3] < w.y1 ? r[i][3] : w.y1;
        const int cw = x1 > x0 ? x1 - x0 : 0, ch = y1 > y0 ? y1 - y0 : 0;
        m.x0[i] = x0;
        m.y0[i] = y0;
        m.w[i] = cw > 0 ? cw : 1;
        m.start[i + 1] = m.start[i] + cw * ch;
    }
    m.accX0 = w.x0;
    m.accY0 = w.y0;
    return m;
}

// thread index -> pixel of the window's margin rectangles; false past their end
__device__ __forceinline__ bool margin_rect_pixel(const MarginRects& m, int idx, int& x, int& y)
{
    if (idx >= m.start[4]) return false;
    const int i = idx < m.start[1] ? 0 : (idx < m.start[2] ? 1 : (idx < m.start[3] ? 2 : 3));
    const int r = idx - m.start[i];
    y = m.y0[i] + r / m.w[i];
    x = m.x0[i] + r % m.w[i];
    return true;
}
