// erode.hip -- ghost suppression: erosion of the certainty mask.
//
// The robustness model (stage F) decides every cell on its own.  At the rim of a moving object, and inside low-contrast
// parts of it, single cells pass although their neighbours fail, and the merge takes a frame there that shows something
// else.  The hand-held multi-frame super-resolution method closes those holes with the minimum of the robustness over a
// 5x5 neighbourhood before the merge; the reference repository ships the robustness kernel without that step.
//
// Semantics (radius r = 1 or 2, mask w x h float4 cells, the one-cell ring all zero), for interior cells
// 1 <= x <= w-2, 1 <= y <= h-2:
//   out.c(x, y) = min over |i| <= r, |j| <= r of in.c(clamp(x+i, 1, w-2), clamp(y+j, 1, h-2))   c = x, y, z, each alone
//   out.w(x, y) = in.w(x, y)                                                                     (the motion measure M)
// Ring cells of the output are zero in all four components; the input's ring is never part of a window (it would reject the
// frame's outer r cells for good).  Stage F never writes a NaN or a negative zero into .x .y .z (fmaxf(fminf(.., 1), 0)), so
// plain fminf is enough and the result is defined bit for bit, whatever the launch shape.
//
// k_maskErode<R>: one workgroup per 64 x 16 tile of cells.  The tile and its R-cell halo go through LDS as whole 16-byte
// cells (window clamp applied to the load address), a row pass replaces every tile row (halo rows included) by its horizontal
// minima, a column pass takes the vertical minimum of those and stores the cell with the input's .w.
// A minimum is separable and has no rounding, so the two passes equal the 2-D window.  Not in place: a workgroup's halo
// would read cells a neighbour has already eroded.
#include "common.hpp"

#define ER_TX 64
#define ER_TY 16
#define ER_ROWS 4  // block = ER_TX x ER_ROWS threads; each takes ER_TY / ER_ROWS cells of a column

struct ErodeFrames {
    const float4* in[MFSR_MAX_FUSE_GROUP];
    float4* out[MFSR_MAX_FUSE_GROUP];
};

__device__ __forceinline__ float4 min3(const float4& a, const float4& b)
{
    return make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), 0.0f);
}

template <int R>
__global__ void __launch_bounds__(ER_TX* ER_ROWS)
    k_maskErode(ErodeFrames fr, int width, int height, int inPitch, int outPitch)
{
    constexpr int LW = ER_TX + 2 * R, LH = ER_TY + 2 * R;
    constexpr int NT = ER_TX * ER_ROWS, PER = (LH * ER_TX + NT - 1) / NT;
    __shared__ float4 sT[LH][LW];
    const float4* __restrict__ in = fr.in[blockIdx.z];
    float4* __restrict__ out = fr.out[blockIdx.z];
    const int lx = threadIdx.x, ly = threadIdx.y;
    const int tid = ly * ER_TX + lx;
    const int x0 = blockIdx.x * ER_TX, y0 = blockIdx.y * ER_TY;
    // tile + halo; the window is clamped to the interior [1, w-2] x [1, h-2] (every address is inside the image)
    for (int t = tid; t < LH * LW; t += NT) {
        const int r = t / LW, c = t - r * LW;
        const int gy = clampi(y0 - R + r, 1, height - 2), gx = clampi(x0 - R + c, 1, width - 2);
        sT[r][c] = row_ptr(in, inPitch, gy)[gx];
    }
    __syncthreads();
    // rows: horizontal minimum of every tile row (halo rows included), .w of the centre cell; taken into registers and
    // written back over the tile's first ER_TX columns after a barrier -- one LDS plane instead of two
    float4 m[PER];
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int t = tid + k * NT;
        if (t < LH * ER_TX) {
            const int r = t / ER_TX, c = t - r * ER_TX;
            float4 v = sT[r][c];
#pragma unroll
            for (int i = 1; i <= 2 * R; i++) v = min3(v, sT[r][c + i]);
            v.w = sT[r][c + R].w;
            m[k] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int t = tid + k * NT;
        if (t < LH * ER_TX) sT[t / ER_TX][t % ER_TX] = m[k];
    }
    __syncthreads();
    // columns: vertical minimum, .w from the centre row, ring cells zero
    const int x = x0 + lx;
    if (x >= width) return;
#pragma unroll
    for (int k = 0; k < ER_TY / ER_ROWS; k++) {
        const int r = ly + k * ER_ROWS, y = y0 + r;
        if (y >= height) break;
        float4 v = sT[r][lx];
#pragma unroll
        for (int j = 1; j <= 2 * R; j++) v = min3(v, sT[r + j][lx]);
        v.w = sT[r + R][lx].w;
        if (x < 1 || y < 1 || x >= width - 1 || y >= height - 1) v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        row_ptr(out, outPitch, y)[x] = v;
    }
}

// every argument is checked on the host before any device call
extern "C" int mfsr_erodeMaskBatch(int nFrames, const mfsr_float4* const* in, mfsr_float4* const* out, int width, int height,
                                   int inPitch, int outPitch, int radius, mfsr_stream_t stream)
{
    MFSR_REQUIRE(nFrames >= 1 && nFrames <= MFSR_MAX_FUSE_GROUP && in != nullptr && out != nullptr);
    MFSR_REQUIRE(radius >= 1 && radius <= 2);
    MFSR_REQUIRE(width >= 3 && height >= 3);
    MFSR_REQUIRE((long long)inPitch >= 16LL * width && (inPitch & 15) == 0);
    MFSR_REQUIRE((long long)outPitch >= 16LL * width && (outPitch & 15) == 0);
    ErodeFrames fr;
    for (int k = 0; k < MFSR_MAX_FUSE_GROUP; k++) {
        fr.in[k] = nullptr;
        fr.out[k] = nullptr;
    }
    const unsigned long long inSpan = (unsigned long long)inPitch * (height - 1) + 16ULL * width;
    const unsigned long long outSpan = (unsigned long long)outPitch * (height - 1) + 16ULL * width;
    for (int k = 0; k < nFrames; k++) {
        MFSR_REQUIRE(in[k] != nullptr && out[k] != nullptr);
        MFSR_REQUIRE(((uintptr_t)in[k] & 15) == 0 && ((uintptr_t)out[k] & 15) == 0);
        fr.in[k] = (const float4*)in[k];
        fr.out[k] = (float4*)out[k];
    }
    // no output may overlap any input, or another output
    for (int k = 0; k < nFrames; k++) {
        const unsigned long long o0 = (unsigned long long)(uintptr_t)out[k], o1 = o0 + outSpan;
        for (int j = 0; j < nFrames; j++) {
            const unsigned long long i0 = (unsigned long long)(uintptr_t)in[j];
            MFSR_REQUIRE(o1 <= i0 || i0 + inSpan <= o0);
            if (j != k) {
                const unsigned long long p0 = (unsigned long long)(uintptr_t)out[j];
                MFSR_REQUIRE(o1 <= p0 || p0 + outSpan <= o0);
            }
        }
    }
    dim3 block(ER_TX, ER_ROWS), grid(mfsr_cdiv(width, ER_TX), mfsr_cdiv(height, ER_TY), nFrames);
    if (radius == 1)
        hipLaunchKernelGGL(k_maskErode<1>, grid, block, 0, mfsr_s(stream), fr, width, height, inPitch, outPitch);
    else
        hipLaunchKernelGGL(k_maskErode<2>, grid, block, 0, mfsr_s(stream), fr, width, height, inPitch, outPitch);
    return mfsr_launch_status("erodeMaskBatch");
}
