// field_math.hpp -- the arithmetic of the kernel-shape field, shared by the one-launch-per-
// reference-kernel chain (optical_flow.hip, tile_tracker.hip, glue.hip) and by the single-launch field kernel
// (kernel_field.hip).  Both take every float operation from here, in the same order, so that they agree bit for bit: E3's
// eigen-decomposition turns a last-bit difference of the tensor into a visible difference of the kernel orientation.
#pragma once

#include "common.hpp"

// ---- D3/E1: 5-point derivative (opticalFlow.cu:97-185) ------------------------
// normalised coordinate of stencil tap k = 0..3 (+2, +1, -1, -2 steps of d from x)
__device__ __forceinline__ float deriv5_tap(float x, float d, int k)
{
    return k == 0 ? x + 2.0f * d : k == 1 ? x + 1.0f * d : k == 2 ? x - 1.0f * d : x - 2.0f * d;
}

// the stencil over the four taps' values, fetch(k) = the image at tap k
template <typename Fetch>
__device__ __forceinline__ float deriv5_of(Fetch fetch)
{
    float t0 = fetch(0);
    t0 -= fetch(1) * 8.0f;
    t0 += fetch(2) * 8.0f;
    t0 -= fetch(3);
    t0 /= 12.0f;
    return t0;
}

__device__ __forceinline__ float deriv5(const mfsr_tex2d& t, float x, float y, float dx, float dy)
{
    return deriv5_of([&](int k) { return tex1<ADDR_MIRROR>(t, deriv5_tap(x, dx, k), deriv5_tap(y, dy, k)); });
}

// ---- E2: structure tensor of one pixel (kernel.cu:691-715) ---------------------
__device__ __forceinline__ pix3 tensor_products(float dx, float dy)
{
    pix3 val = {dx * dx, dy * dy, dx * dy};
    return val;
}

// ---- one tap of the separable filter: ascending taps from s = 0 ----------------
__device__ __forceinline__ float filter_step(float s, float tap, float v)
{
    s += tap * v;
    return s;
}

// ---- E3: ComputeKernelParam (kernel.cu:718-790) --------------------------------
__device__ __forceinline__ pix3 kernel_param(pix3 grad, float Dth, float Dtr, float kDetail, float kDenoise,
                                             float kStretch, float kShrink)
{
    const float a11 = grad.x, a22 = grad.y, a12 = grad.z;
    const float help = sqrtf((a22 - a11) * (a22 - a11) + 4.0f * a12 * a12);
    float c = 2.0f * a12;
    float s = a22 - a11 + help;
    const float norm = sqrtf(c * c + s * s);
    if (norm > 0) {
        c /= norm;
        s /= norm;
    } else {
        c = 1;
        s = 0;
    }
    const float lam1 = (a11 + a22 + help) / 2.0f;
    const float lam2 = (a11 + a22 - help) / 2.0f;
    const float A = 1 + sqrtf((lam1 - lam2) * (lam1 - lam2) / ((lam1 + lam2) * (lam1 + lam2)));
    float D = 1 - sqrtf(lam1) / Dtr + Dth;
    D = fmaxf(fminf(1.0f, D), 0.0f);
    const float k1h = kDetail * kStretch * A;
    const float k2h = kDetail / kShrink * A;
    float k1 = ((1.0f - D) * k1h + D * kDetail * kDenoise);
    float k2 = ((1.0f - D) * k2h + D * kDetail * kDenoise);
    k1 *= k1;
    k2 *= k2;
    const float x2 = c, y2 = s, x1 = s, y1 = -c;
    const float b11 = k1 * x1 * x1 + x2 * x2 * k2;
    const float b12 = k1 * x1 * y1 + x2 * y2 * k2;
    const float b22 = k1 * y1 * y1 + y2 * y2 * k2;
    const float det = b11 * b22 - b12 * b12 + 0.0000000001f;
    pix3 kernel = {b22 / det, b11 / det, -b12 / det};
    return kernel;
}
