// finish_stages.hpp -- the per-pixel arithmetic of the three finish stages that run before the matrix and the tone curve: the
// merge-aware denoise, the unsharp mask (section 2.20) and the local-tone gain (section 2.25).  A
// step is ONE definition here, called by the stage's own file (denoise.hip, sharpen.hip, local_tone.hip) and by finish_chain.hip
// (section 2.26), so the chain cannot drift from the stand-alone entry points it promises to compose.  Every step is float32
// + - * / fmaxf fminf with -ffp-contract=off (the Makefile) in the order include/mfsr.h writes it.
//
// What is here is what could move without changing one instruction of any kernel (tools/isa_table.py, profiles/
// isa_finish_stage_bodies.txt): the straight-line steps and slice_gain, which was a function before.  The loops around them --
// the denoise's window, its tap weight and blend, the sharpen's two passes -- stay written out in both callers: as functions of
// their own the compiler simplifies them before it inlines them, and the stand-alone kernels came out as other code.  The
// argument structs, their host fills and the tile's constants are here so that both callers see one of each.
#pragma once

#include "render_common.hpp"

namespace {

// the tile of the stencil kernels (denoise, sharpen, chain): a workgroup of kLanes lanes owns kTW x kTH output pixels
constexpr int kTW = 64, kTH = 16, kLanes = 256;
constexpr int kMaxRd = 3, kMaxRs = 4;  // the largest radius of the denoise / of the sharpen

// ---- denoise (section 2.24) ---------------------------------------------------------------------------------------------
// The step functions take the stage's constants as `const A& a`: DenoiseArgs, or the chain's ChainArgs, which holds members of
// the same names (one struct embedded in both moved twelve of the chain's kernels: profiles/isa_finish_stage_bodies.txt).
struct DenoiseArgs {
    float gain, alpha, beta, hh;  // hh = strength * strength
    float wHi, rSpan;             // the fade; used when fade != 0
    int fade;
    int R;
    int yLo, yHi;  // valid rows [yLo, yHi] relative to the launch's first row
};

// step 1: the cleaned value s
__device__ __forceinline__ float clean_value(float p) { return isnan(p) ? 0.0f : fminf(fmaxf(p, -65536.0f), 65536.0f); }

// step 2: the cleaned count n
__device__ __forceinline__ float clean_count(float n) { return isnan(n) ? 0.0f : n; }

// step 3: the fade lambda of the cleaned count
template <class A>
__device__ __forceinline__ float fade_of(float n, const A& a)
{
    return a.fade ? fminf(fmaxf((a.wHi - n) * a.rSpan, 0.0f), 1.0f) : 1.0f;
}

// step 4: 1 / (h^2 v) of one channel, v the variance the merge left at the pixel (two divisions: only where a wave filters)
template <class A>
__device__ __forceinline__ float denoise_inv_tolerance(float s, float n, const A& a)
{
    const float v = fmaxf((a.gain * (a.alpha * fmaxf(s, 0.0f) + a.beta)) / fmaxf(n, 1e-6f), 1e-20f);
    return 1.0f / (a.hh * v);
}

DenoiseArgs denoise_args(const mfsr_denoise* d, int yLo, int yHi)
{
    DenoiseArgs a;
    a.gain = d->gain;
    a.alpha = d->alpha;
    a.beta = d->beta;
    a.hh = d->strength * d->strength;
    a.fade = d->wHi > d->wLo;
    a.wHi = d->wHi;
    a.rSpan = a.fade ? 1.0f / (d->wHi - d->wLo) : 0.0f;
    a.R = d->radius;
    a.yLo = yLo;
    a.yHi = yHi;
    return a;
}

// ---- sharpen (section 2.20) ---------------------------------------------------------------------------------------------
struct SharpenArgs {
    float k[kMaxRs + 1];
    float amount, threshold;
    int R;
    int yLo, yHi;  // valid rows [yLo, yHi] relative to the launch's first row
};

// step 1: the cleaned value s
__device__ __forceinline__ float sharpen_clean(float p) { return isnan(p) ? 0.0f : p; }

// N consecutive floats of an LDS row; N = 4: one 16-byte read (the address is 16-byte aligned: the callers' layouts)
template <int N>
__device__ __forceinline__ void load_span(const float* p, float (&v)[N])
{
    if constexpr (N == 4) {
        const float4 q = *(const float4*)p;
        v[0] = q.x;
        v[1] = q.y;
        v[2] = q.z;
        v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = p[k];
    }
}

// steps 2 and 3: one symmetric pair of taps of either pass, added to the sum so far
__device__ __forceinline__ float sharpen_tap(float sum, float k, float lo, float hi) { return sum + k * (lo + hi); }

// step 4: the coring of the difference between s and its blur b, and the result
template <class A>
__device__ __forceinline__ float sharpen_core(float s, float b, const A& a)
{
    const float e = s - b;
    const float t = fabsf(e) - a.threshold;
    const float g = t > 0.0f ? copysignf(t, e) : 0.0f;
    return s + a.amount * g;
}

SharpenArgs sharpen_args(const mfsr_sharpen* s, int yLo, int yHi)
{
    SharpenArgs a;
    for (int d = 0; d <= kMaxRs; d++) a.k[d] = d <= s->radius ? s->taps[d] : 0.0f;
    a.amount = s->amount;
    a.threshold = s->threshold;
    a.R = s->radius;
    a.yLo = yLo;
    a.yHi = yHi;
    return a;
}

// ---- the local-tone gain (section 2.25): the slice ----------------------------------------------------------------------
struct GridGeom {
    int cellShift;                             // log2 C
    int nz, nzShift;                           // luma bins and log2 of them
    int gx, gy;                                // cells of the full frame
    int colOffset, rowOffset;                  // the launch's pixel (0, 0) in the full frame
};

struct SliceArgs {
    const float* grid;                         // GX GY NZ floats: luma fastest, then x, then y
    GridGeom g;
    float invCell;                             // 1 / C (a power of two: exact)
    float fnz;                                 // (float)NZ
};

struct Axis {
    int i0, i1;
    float a;
};

// fx = (X + 0.5f) (1 / C) - 0.5f clamped to [0, n - 1]; monotone in X
__device__ __forceinline__ Axis grid_axis(int X, float invCell, int n)
{
    float fx = ((float)X + 0.5f) * invCell - 0.5f;
    fx = fminf(fmaxf(fx, 0.0f), (float)(n - 1));
    Axis r;
    r.i0 = (int)fx;
    r.i1 = min(r.i0 + 1, n - 1);
    r.a = fx - (float)r.i0;
    return r;
}

// a pair of gains as one 64-bit word: the LDS read of a corner is then one 8-byte access (a float2 is read as two dwords, at
// twice the LDS cycles)
__device__ __forceinline__ unsigned long long pack_pair(float a, float b)
{
    return (unsigned long long)__float_as_uint(a) | ((unsigned long long)__float_as_uint(b) << 32);
}
__device__ __forceinline__ float2 unpack_pair(unsigned long long v)
{
    return make_float2(__uint_as_float((uint32_t)v), __uint_as_float((uint32_t)(v >> 32)));
}

// The corner columns of the workgroup's tile, staged as pairs (local_tone.hip's stage_grid):
// sPair[(row - j0) * cols + (col - i0)][k] = (g[k], g[min(k+1, NZ-1)])
struct Tile {
    int i0, j0, cols;                          // cols = 0: not staged, read the grid through the cache
};

// steps 1-3 of section 2.25: the gain of the pixel p at (x, y) of the launch.  GL = 0: through the cache, whatever tl and sPair.
template <int GL>
__device__ __forceinline__ float slice_gain(pix3 p, int x, int y, const RenderArgs& r, const SliceArgs& t, const Tile& tl,
                                            const unsigned long long* sPair)
{
    const pix3 q = r.useMatrix ? matrix_pixel(p, r.m) : p;          // uniform
    const float v0 = isnan(q.x) ? 0.0f : fminf(fmaxf(q.x, 0.0f), 1.0f);
    const float v1 = isnan(q.y) ? 0.0f : fminf(fmaxf(q.y, 0.0f), 1.0f);
    const float v2 = isnan(q.z) ? 0.0f : fminf(fmaxf(q.z, 0.0f), 1.0f);
    const float l = ((54.0f * v0 + 183.0f * v1) + 19.0f * v2) * (1.0f / 256.0f);
    const Axis ax = grid_axis(x + t.g.colOffset, t.invCell, t.g.gx);
    const Axis ay = grid_axis(y + t.g.rowOffset, t.invCell, t.g.gy);
    float fz = l * t.fnz - 0.5f;
    fz = fminf(fmaxf(fz, 0.0f), (float)(t.g.nz - 1));
    const int k0 = (int)fz;
    const float az = fz - (float)k0;
    float2 c00, c01, c10, c11;                                      // (y, x) corners: the pair (g[k0], g[k1]) of each
    if (GL && tl.cols) {                                            // uniform
        const int r0 = (ay.i0 - tl.j0) * tl.cols - tl.i0, r1 = (ay.i1 - tl.j0) * tl.cols - tl.i0;
        c00 = unpack_pair(sPair[((r0 + ax.i0) << t.g.nzShift) + k0]);
        c01 = unpack_pair(sPair[((r0 + ax.i1) << t.g.nzShift) + k0]);
        c10 = unpack_pair(sPair[((r1 + ax.i0) << t.g.nzShift) + k0]);
        c11 = unpack_pair(sPair[((r1 + ax.i1) << t.g.nzShift) + k0]);
    } else {
        const int k1 = min(k0 + 1, t.g.nz - 1);
        const float* g0 = t.grid + (((size_t)ay.i0 * t.g.gx) << t.g.nzShift);
        const float* g1 = t.grid + (((size_t)ay.i1 * t.g.gx) << t.g.nzShift);
        const int o0 = ax.i0 << t.g.nzShift, o1 = ax.i1 << t.g.nzShift;
        c00 = make_float2(g0[o0 + k0], g0[o0 + k1]);
        c01 = make_float2(g0[o1 + k0], g0[o1 + k1]);
        c10 = make_float2(g1[o0 + k0], g1[o0 + k1]);
        c11 = make_float2(g1[o1 + k0], g1[o1 + k1]);
    }
    const float z00 = c00.x + (c00.y - c00.x) * az, z01 = c01.x + (c01.y - c01.x) * az;
    const float z10 = c10.x + (c10.y - c10.x) * az, z11 = c11.x + (c11.y - c11.x) * az;
    const float x0 = z00 + (z01 - z00) * ax.a, x1 = z10 + (z11 - z10) * ax.a;
    return x0 + (x1 - x0) * ay.a;
}

}  // namespace
