// stats_common.hpp -- what the two statistics stages of the merged image share: image_stats.hip and
// local_tone.hip (section 2.25).  The 12-bit codes, the four-pixel load of a lane and the 64-bit wave sum: one definition, so
// that both stages measure the same codes of the same pixels.
#pragma once

#include "render_common.hpp"

namespace {

constexpr int kStatsThreads = 1024;
constexpr int kStatsPpl = 4;                   // consecutive pixels of a row one lane owns
constexpr float kMaxCode = 4095.0f;            // codes 0 .. 4095

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_sum64(u64 v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// pixels [x0, x0 + 4) of a row, clipped to `width` (pixels beyond it: zeros, never loaded)
__device__ __forceinline__ void load_quad(const pix3* row, int x0, int width, pix3 (&p)[kStatsPpl])
{
    const pix3* a = row + x0;
    if (x0 + kStatsPpl <= width && ((uintptr_t)a & 15) == 0) {
        const float4* v = (const float4*)a;
        const float4 A = v[0], B = v[1], C = v[2];
        p[0] = {A.x, A.y, A.z};
        p[1] = {A.w, B.x, B.y};
        p[2] = {B.z, B.w, C.x};
        p[3] = {C.y, C.z, C.w};
    } else {
#pragma unroll
        for (int k = 0; k < kStatsPpl; k++) {
            p[k] = {0.0f, 0.0f, 0.0f};
            if (x0 + k < width) p[k] = a[k];
        }
    }
}

// the luma key of sections 2.23 and 2.25: the 12-bit codes of q and their integer luma, 0 .. 4095
__device__ __forceinline__ int luma_key(pix3 q)
{
    const int c0 = quantize1(q.x, kMaxCode), c1 = quantize1(q.y, kMaxCode), c2 = quantize1(q.z, kMaxCode);
    return (54 * c0 + 183 * c1 + 19 * c2 + 128) >> 8;
}

}  // namespace
