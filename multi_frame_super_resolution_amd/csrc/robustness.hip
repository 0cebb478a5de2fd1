// robustness.hip -- per-pixel robustness weight.
// Behavioural spec: reference test_opencv/RobustnessModell.cu:29-158.
//
// The reference keeps a 3x3 float3 patch per thread in dynamic shared memory
// purely as private scratch (:45-46, no barrier); here the 9 reference pixels
// stay in VGPRs.  Quirk kept: of the 25 flow fetches only the last one
// (x=2,y=2) can influence min/max (:62-72), so only that one is issued -- the
// other 24 are dead in the reference too.
//
// Kernels of this file: k_ComputeRobustnessMask (the straight port), k_robustnessFused (one frame per grid layer: a table of
// frames, the flow fetched before the reference patch is staged) and k_robustnessGroup (all frames of a group in one pass over
// the reference: the burst's kernel).  The last two end in the same per-frame tail (maxShift / minShift to the four stored
// floats), written out in both: as a shared function it moved k_robustnessGroup's instructions
// (profiles/isa_alignment_forks.txt).
#include <cstdlib>
#include <cstring>
#include "common.hpp"
#include "half_pixel.hpp"

__global__ void __launch_bounds__(256)
    k_ComputeRobustnessMask(const pix3* __restrict__ rawImgRef, const pix3* __restrict__ rawImgMoved,
                            float4* __restrict__ robustnessMask, mfsr_tex2d texUV, int imgWidth, int imgHeight,
                            int imgPitch, int maskPitch, float alpha, float beta, float thresholdM)
{
    const int pxX = blockIdx.x * blockDim.x + threadIdx.x;
    const int pxY = blockIdx.y * blockDim.y + threadIdx.y;
    if (pxX >= imgWidth - 1 || pxY >= imgHeight - 1 || pxX < 1 || pxY < 1) return;

    const float2 shiftf =
        tex2<ADDR_CLAMP>(texUV, ((float)pxX + 0.5f) / (float)imgWidth, ((float)pxY + 0.5f) / (float)imgHeight);
    // last sample of the 5x5 loop (:66 with x = y = 2)
    const float2 s = tex2<ADDR_CLAMP>(texUV, ((float)pxX + (float)2 + 0.5f) / (float)imgWidth,
                                      ((float)pxY + (float)2 + 0.5f) / (float)imgHeight);
    float2 maxShift, minShift;
    maxShift.x = fmaxf(s.x, shiftf.x);
    maxShift.y = fmaxf(s.y, shiftf.y);
    minShift.x = fminf(s.x, shiftf.x);
    minShift.y = fminf(s.y, shiftf.y);

    const int shx = round2i(shiftf.x * 0.5f);
    const int shy = round2i(shiftf.y * 0.5f);

    pix3 pixelsRef[9];
    float mrx = 0, mry = 0, mrz = 0, mmx = 0, mmy = 0, mmz = 0;
#pragma unroll
    for (int y = -1; y <= 1; y++) {
        const pix3* rr = row_ptr(rawImgRef, imgPitch, pxY + y);
        const int ppy = clampi(pxY + shy + y, 0, imgHeight - 1);
        const pix3* rm = row_ptr(rawImgMoved, imgPitch, ppy);
#pragma unroll
        for (int x = -1; x <= 1; x++) {
            pix3 p = rr[pxX + x];
            pixelsRef[(y + 1) * 3 + (x + 1)] = p;
            mrx += p.x;
            mry += p.y;
            mrz += p.z;
            const int ppx = clampi(pxX + shx + x, 0, imgWidth - 1);
            p = rm[ppx];
            mmx += p.x;
            mmy += p.y;
            mmz += p.z;
        }
    }
    mrx = div9(mrx);
    mry = div9(mry);
    mrz = div9(mrz);
    mmx = div9(mmx);
    mmy = div9(mmy);
    mmz = div9(mmz);

    float meandist = fabsf(mrx - mmx) + fabsf(mry - mmy) + fabsf(mrz - mmz);
    meandist = div3(meandist);
    maxShift.x *= 0.5f * meandist;
    maxShift.y *= 0.5f * meandist;
    minShift.x *= 0.5f * meandist;
    minShift.y *= 0.5f * meandist;
    const float M = sqrtf((maxShift.x - minShift.x) * (maxShift.x - minShift.x) +
                          (maxShift.y - minShift.y) * (maxShift.y - minShift.y));

    float sdx = 0, sdy = 0, sdz = 0;
#pragma unroll
    for (int p = 0; p < 9; p++) {
        sdx += (pixelsRef[p].x - mrx) * (pixelsRef[p].x - mrx);
        sdy += (pixelsRef[p].y - mry) * (pixelsRef[p].y - mry);
        sdz += (pixelsRef[p].z - mrz) * (pixelsRef[p].z - mrz);
    }
    sdx = sqrtf(div9(sdx));
    sdy = sqrtf(div9(sdy));
    sdz = sqrtf(div9(sdz));

    const float smx = sqrtf(alpha * mrx + beta);
    const float smy = sqrtf(alpha * mry + beta) / sqrtf(2.0f);
    const float smz = sqrtf(alpha * mrz + beta);

    float dx = fabsf(mrx - mmx), dy = fabsf(mry - mmy), dz = fabsf(mrz - mmz);
    const float sgx = fmaxf(smx, sdx), sgy = fmaxf(smy, sdy), sgz = fmaxf(smz, sdz);
    dx = dx * (sdx * sdx / (sdx * sdx + smx * smx));
    dy = dy * (sdy * sdy / (sdy * sdy + smy * smy));
    dz = dz * (sdz * sdz / (sdz * sdz + smz * smz));

    float sc = 1.5f;
    if (M > thresholdM) sc = 0;
    const float t = 0.12f;
    float4 mask;
    mask.x = fmaxf(fminf(sc * expf(-dx * dx / (sgx * sgx)) - t, 1.0f), 0.0f);
    mask.y = fmaxf(fminf(sc * expf(-dy * dy / (sgy * sgy)) - t, 1.0f), 0.0f);
    mask.z = fmaxf(fminf(sc * expf(-dz * dz / (sgz * sgz)) - t, 1.0f), 0.0f);
    mask.w = M;
    row_ptr(robustnessMask, maskPitch, pxY)[pxX] = mask;
}

// ---- MI355X kernel ---------------------------------------------------------------------------------------------------
// The straight kernel above is VALU-bound, not memory-bound (706 VALU instructions per pixel: IEEE sqrt / division
// expansions, three ocml expf, two full bilinear fetches, 18 address computations; 38.9 us per 4K frame for 99.5 MB of
// algorithmic traffic, 164 MB counted).  This one
//  * stages the reference patch rows of a 64 x 8 tile (+1 halo) in LDS as three planes: the 27 reads of a pixel are
//    LDS reads at compile-time offsets instead of nine 12-byte global gathers with their address arithmetic
//    (HBM/L2 traffic of the reference image: once per tile instead of ~1.65x);
//  * takes every square root, reciprocal and exponential on the hardware units (v_sqrt_f32, v_rcp_f32, v_exp_f32: 1 ulp)
//    -- the mask is a continuous function of them, so the result moves by a few 1e-7 (test tolerance 2e-6); the two
//    discontinuities (round(0.5 * flow), M > thresholdM) keep their exact arithmetic: the flow fetch is the bit-exact
//    bilinear of the straight kernel and the means are summed in the reference's order and divided exactly;
//  * reads the one live sample of the 5 x 5 flow loop (x = y = 2, :66) as a plain texel when the flow field has the
//    image's resolution (the Bayer pipeline): the bilinear fetch lands on a texel centre up to 1 ulp of the coordinate;
//  * writes the zero ring the reference leaves to its caller (:48-49): no separate ring launch;
//  * (round 3) fetches the pixel's flow BEFORE the reference patch is staged and gathers the moved patch
//    before the barrier: of the three dependent round trips (stage, flow, gather) two overlap -- the kernel waits twice as
//    long as it issues (SQ_WAIT_INST_ANY 1.05e8 vs SQ_ACTIVE_INST_VALU 5.2e7 per 4-frame launch); 115.5 -> 106 us against
//    fetching the flow after the barrier.
#define RB_TX 64
#define RB_TY 8

struct RobustFusedFrame {
    const pix3* moved;
    float4* mask;
    const float2* flow;
};
struct RobustFusedFrames {
    RobustFusedFrame f[MFSR_BATCH_MAX];
};
// texUV: the flow fields' pitch and size; its pointer is the frame's flow
template <bool ALIGNED>
__global__ void __launch_bounds__(RB_TX* RB_TY)
    k_robustnessFused(const pix3* __restrict__ rawImgRef, RobustFusedFrames frames, mfsr_tex2d texUV, int imgWidth, int imgHeight,
                      int imgPitch, int maskPitch, float alpha, float beta, float thresholdM, MfsrExactDiv dW, MfsrExactDiv dH)
{
    const pix3* __restrict__ rawImgMoved = frames.f[blockIdx.z].moved;
    float4* __restrict__ robustnessMask = frames.f[blockIdx.z].mask;
    texUV.ptr = frames.f[blockIdx.z].flow;
    __shared__ float sR[3][RB_TY + 2][RB_TX + 2];
    const int lx = threadIdx.x, ly = threadIdx.y;
    const int x0 = blockIdx.x * RB_TX, y0 = blockIdx.y * RB_TY;
    // this pixel's flow first: its fetch and the moved-image gather that depends on it are then in flight while the
    // reference patch is staged (three dependent round trips become two)
    const int pxXe = min(x0 + lx, imgWidth - 1), pxYe = min(y0 + ly, imgHeight - 1);
    // (/ imgWidth, / imgHeight: mfsr_div, common.hpp)
    const float2 shiftfE = tex2<ADDR_CLAMP>(texUV, mfsr_div((float)pxXe + 0.5f, dW), mfsr_div((float)pxYe + 0.5f, dH));
    float2 sE;
    if (ALIGNED) {
        sE = row_ptr((const float2*)texUV.ptr, texUV.pitch, min(pxYe + 2, imgHeight - 1))[min(pxXe + 2, imgWidth - 1)];
    } else {
        sE = tex2<ADDR_CLAMP>(texUV, mfsr_div((float)pxXe + (float)2 + 0.5f, dW), mfsr_div((float)pxYe + (float)2 + 0.5f, dH));
    }
    for (int t = ly * RB_TX + lx; t < (RB_TY + 2) * (RB_TX + 2); t += RB_TX * RB_TY) {
        const int r = t / (RB_TX + 2), c = t - r * (RB_TX + 2);
        const int gy = clampi(y0 - 1 + r, 0, imgHeight - 1), gx = clampi(x0 - 1 + c, 0, imgWidth - 1);
        const pix3 p = row_ptr(rawImgRef, imgPitch, gy)[gx];
        sR[0][r][c] = p.x;
        sR[1][r][c] = p.y;
        sR[2][r][c] = p.z;
    }
    // the moved patch under the rounded flow: gathered before the barrier, summed after it
    const int shxE = round2i(shiftfE.x * 0.5f), shyE = round2i(shiftfE.y * 0.5f);
    pix3 pmv[9];
#pragma unroll
    for (int y = 0; y < 3; y++) {
        const pix3* rm = row_ptr(rawImgMoved, imgPitch, clampi(pxYe + shyE + y - 1, 0, imgHeight - 1));
#pragma unroll
        for (int x = 0; x < 3; x++) pmv[y * 3 + x] = rm[clampi(pxXe + shxE + x - 1, 0, imgWidth - 1)];
    }
    __syncthreads();
    const int pxX = x0 + lx, pxY = y0 + ly;
    if (pxX >= imgWidth || pxY >= imgHeight) return;
    float4* out = row_ptr(robustnessMask, maskPitch, pxY) + pxX;
    if (pxX < 1 || pxY < 1 || pxX >= imgWidth - 1 || pxY >= imgHeight - 1) {
        *out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float2 shiftf = shiftfE, s = sE;   // (pxX == pxXe, pxY == pxYe for every pixel that gets here)
    float2 maxShift, minShift;
    maxShift.x = fmaxf(s.x, shiftf.x);
    maxShift.y = fmaxf(s.y, shiftf.y);
    minShift.x = fminf(s.x, shiftf.x);
    minShift.y = fminf(s.y, shiftf.y);

    // means in the reference's summation order (row-major from 0), exact division by 9
    float pr[3][9];
    float mr[3] = {0.0f, 0.0f, 0.0f}, mm[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int y = 0; y < 3; y++) {
#pragma unroll
        for (int x = 0; x < 3; x++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                pr[c][y * 3 + x] = sR[c][ly + y][lx + x];
                mr[c] += pr[c][y * 3 + x];
            }
            const pix3 p = pmv[y * 3 + x];
            mm[0] += p.x;
            mm[1] += p.y;
            mm[2] += p.z;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        mr[c] = div9(mr[c]);
        mm[c] = div9(mm[c]);
    }
    float meandist = fabsf(mr[0] - mm[0]) + fabsf(mr[1] - mm[1]) + fabsf(mr[2] - mm[2]);
    meandist = div3(meandist);
    const float hm = 0.5f * meandist;
    const float ddx = maxShift.x * hm - minShift.x * hm, ddy = maxShift.y * hm - minShift.y * hm;
    const float M = __builtin_amdgcn_sqrtf(ddx * ddx + ddy * ddy);
    const float sc = (M > thresholdM) ? 0.0f : 1.5f;
    float m3[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float sd2 = 0.0f;
#pragma unroll
        for (int p = 0; p < 9; p++) {
            const float d = pr[c][p] - mr[c];
            sd2 = __builtin_fmaf(d, d, sd2);
        }
        sd2 = div9(sd2);                                            // variance of the reference patch
        float smd2 = __builtin_fmaf(alpha, mr[c], beta);            // noise model variance (green: / 2, :131)
        if (c == 1) smd2 *= 0.5f;
        const float sg2 = fmaxf(smd2, sd2);                         // max(sigma_md, std)^2
        float d = fabsf(mr[c] - mm[c]);
        d = d * (sd2 * __builtin_amdgcn_rcpf(sd2 + smd2));          // Wiener shrink (:142-144); 0 * inf = NaN as in the reference
        const float e = __builtin_amdgcn_exp2f(-(d * d) * __builtin_amdgcn_rcpf(sg2) * 1.44269504088896340736f);
        m3[c] = fmaxf(fminf(__builtin_fmaf(sc, e, -0.12f), 1.0f), 0.0f);
    }
    *out = make_float4(m3[0], m3[1], m3[2], M);
}

// ---- the masks of a whole group in one pass --------------------------------------------------------------------------
// k_robustnessFused<true> for the 1 .. 4 moved frames of a group in ONE pass over the reference (gridDim.z = 1), same bits:
//  * everything that depends on the reference alone -- the patch means mr, the Wiener factor A = sd2 * rcp(sd2 + smd2) and
//    Rg = rcp(max(smd2, sd2)) -- is computed once per pixel from the LDS tile and kept in nine registers across the frames
//    (the fused kernel recomputes it per frame; 403 -> 166 VALU instructions per pixel and frame at four frames);
//  * the moved side is ONE gather: the frame's image holds the 3 x 3 patch MEANS (k_prepareFrameFused<true>, debayer.hip:
//    the very sum and division of k_robustnessFused), and mm at pixel p is the mean at q = p + round(0.5 * flow).  That holds
//    for q inside the image.  For q outside, the fused kernel clamps each of the nine coordinates on its own (q = -1 reads
//    column 0 three times), which is not the mean at clamp(q): under a wave-uniform ballot those lanes rebuild the nine
//    pixels from the frame's raw samples (a1_pixel, half_pixel.hpp) and sum them as the fused kernel does;
//  * the flow fetches of all frames are issued first, the gathers of all frames before the barrier: the two dependent
//    round trips per frame overlap across the frames and with the staging of the reference.
// Coordinates are formed modulo 2^32 (an infinite flow saturates round2i), as the fused kernel's adds behave on the hardware.
struct RobustGroupFrame {
    const pix3* means;
    const uint16_t* raw;
    float4* mask;
    const float2* flow;
};
struct RobustGroupArgs {
    RobustGroupFrame f[MFSR_BATCH_MAX];
};
__device__ __forceinline__ int rb_wrap_add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }

constexpr int RB_GROUP_WAVES = 8;  // waves per SIMD the group kernel is compiled for
template <int NF>
__global__ void __launch_bounds__(RB_TX* RB_TY) __attribute__((amdgpu_waves_per_eu(RB_GROUP_WAVES, RB_GROUP_WAVES)))
    k_robustnessGroup(const pix3* __restrict__ rawImgRef, RobustGroupArgs ga, int imgWidth, int imgHeight, int imgPitch, int flowPitch,
                      int meansPitch, int maskPitch, float maxVal, int cfa, float alpha, float beta, float thresholdM, MfsrExactDiv dW,
                      MfsrExactDiv dH)
{
    __shared__ float sR[3][RB_TY + 2][RB_TX + 2];
    const int lx = threadIdx.x, ly = threadIdx.y;
    const int x0 = blockIdx.x * RB_TX, y0 = blockIdx.y * RB_TY;
    const int pxXe = min(x0 + lx, imgWidth - 1), pxYe = min(y0 + ly, imgHeight - 1);
    // a frame's flow at this pixel (the bit-exact bilinear fetch) and the one live sample of the 5 x 5 loop; its patch mean
    // under the rounded flow.  Two frames are in flight at a time (ten flow registers each while their loads are): the first
    // two are fetched before the reference tile is staged and gathered before the barrier, the others are fetched before
    // the barrier and gathered after it, ahead of the reference side.
    // Every address is a frame's base pointer (uniform) plus a 32-bit byte offset that all frames share (the host checks
    // that the images are below 2 GiB): no 64-bit address arithmetic per frame and texel.
    float2 shiftf[NF], s[NF];
    pix3 mm[NF];
    const TexCoord tc = tex_coord<ADDR_CLAMP>(imgWidth, imgHeight, mfsr_div((float)pxXe + 0.5f, dW), mfsr_div((float)pxYe + 0.5f, dH));
    const unsigned fr0 = (unsigned)tc.j0 * (unsigned)flowPitch, fr1 = (unsigned)tc.j1 * (unsigned)flowPitch;
    const unsigned o00 = fr0 + 8u * (unsigned)tc.i0, o10 = fr0 + 8u * (unsigned)tc.i1, o01 = fr1 + 8u * (unsigned)tc.i0,
                   o11 = fr1 + 8u * (unsigned)tc.i1;
    const unsigned oS = (unsigned)min(pxYe + 2, imgHeight - 1) * (unsigned)flowPitch + 8u * (unsigned)min(pxXe + 2, imgWidth - 1);
    auto fetch_flow = [&](int f) {
        const char* base = (const char*)ga.f[f].flow;
        const float2 t00 = *(const float2*)(base + o00), t10 = *(const float2*)(base + o10), t01 = *(const float2*)(base + o01),
                     t11 = *(const float2*)(base + o11);
        shiftf[f] = make_float2(lerp4(t00.x, t10.x, t01.x, t11.x, tc.a, tc.b), lerp4(t00.y, t10.y, t01.y, t11.y, tc.a, tc.b));  // tex2
        s[f] = *(const float2*)(base + oS);
    };
    auto gather_mean = [&](int f) {
        const int qx = rb_wrap_add(pxXe, round2i(shiftf[f].x * 0.5f)), qy = rb_wrap_add(pxYe, round2i(shiftf[f].y * 0.5f));
        const unsigned o = (unsigned)clampi(qy, 0, imgHeight - 1) * (unsigned)meansPitch + 12u * (unsigned)clampi(qx, 0, imgWidth - 1);
        mm[f] = *(const pix3*)((const char*)ga.f[f].means + o);
    };
#pragma unroll
    for (int f = 0; f < NF && f < 2; f++) fetch_flow(f);
    for (int t = ly * RB_TX + lx; t < (RB_TY + 2) * (RB_TX + 2); t += RB_TX * RB_TY) {
        const int r = t / (RB_TX + 2), c = t - r * (RB_TX + 2);
        const int gy = clampi(y0 - 1 + r, 0, imgHeight - 1), gx = clampi(x0 - 1 + c, 0, imgWidth - 1);
        const pix3 p = row_ptr(rawImgRef, imgPitch, gy)[gx];
        sR[0][r][c] = p.x;
        sR[1][r][c] = p.y;
        sR[2][r][c] = p.z;
    }
#pragma unroll
    for (int f = 0; f < NF && f < 2; f++) gather_mean(f);
#pragma unroll
    for (int f = 2; f < NF; f++) fetch_flow(f);
    __syncthreads();
    const int pxX = x0 + lx, pxY = y0 + ly;
    if (pxX >= imgWidth || pxY >= imgHeight) return;
    const unsigned oM = (unsigned)pxY * (unsigned)maskPitch + 16u * (unsigned)pxX;
    if (pxX < 1 || pxY < 1 || pxX >= imgWidth - 1 || pxY >= imgHeight - 1) {
#pragma unroll
        for (int f = 0; f < NF; f++) *(float4*)((char*)ga.f[f].mask + oM) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
#pragma unroll
    for (int f = 2; f < NF; f++) gather_mean(f);
    // the reference side, once: means in the reference's summation order (row-major from 0), exact division by 9
    float mr[3], A[3], Rg[3];
    int patch = ly * (RB_TX + 2) + lx;  // the patch's first element in a plane of sR
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float pr[9];
        float m = 0.0f;
#pragma unroll
        for (int p = 0; p < 9; p++) {
            pr[p] = (&sR[c][0][0])[patch + (p / 3) * (RB_TX + 2) + p % 3];
            m += pr[p];
        }
        m = div9(m);
        float sd2 = 0.0f;
#pragma unroll
        for (int p = 0; p < 9; p++) {
            const float d = pr[p] - m;
            sd2 = __builtin_fmaf(d, d, sd2);
        }
        sd2 = div9(sd2);                                  // variance of the reference patch
        float smd2 = __builtin_fmaf(alpha, m, beta);      // noise model variance (green: / 2, :131)
        if (c == 1) smd2 *= 0.5f;
        mr[c] = m;
        A[c] = sd2 * __builtin_amdgcn_rcpf(sd2 + smd2);   // Wiener shrink (:142-144)
        Rg[c] = __builtin_amdgcn_rcpf(fmaxf(smd2, sd2));  // 1 / max(sigma_md, std)^2
        // channel after channel -- nine patch registers live, not 27: the next channel's reads wait for this one's results
        asm volatile("" : "+v"(patch) : "v"(mr[c]), "v"(A[c]), "v"(Rg[c]));
    }
#pragma unroll
    for (int f = 0; f < NF; f++) {
        const int shx = round2i(shiftf[f].x * 0.5f), shy = round2i(shiftf[f].y * 0.5f);
        const int qx = rb_wrap_add(pxX, shx), qy = rb_wrap_add(pxY, shy);
        const bool outside = (unsigned)qx >= (unsigned)imgWidth || (unsigned)qy >= (unsigned)imgHeight;
        if (__ballot(outside) != 0) {
            if (outside) {
                // the nine individually clamped pixels, summed and divided as k_robustnessFused does
                const float factor = 1.0f / maxVal;
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
                // (a rare path: rolled, so that its eighteen loads do not set the kernel's register count)
#pragma unroll 1
                for (int k = 0; k < 9; k++) {
                    const int y = k / 3, x = k - 3 * y;
                    const pix3 p = a1_pixel(ga.f[f].raw, imgWidth, clampi(rb_wrap_add(qx, x - 1), 0, imgWidth - 1),
                                            clampi(rb_wrap_add(qy, y - 1), 0, imgHeight - 1), factor, cfa);
                    a0 += p.x;
                    a1 += p.y;
                    a2 += p.z;
                }
                mm[f].x = div9(a0);
                mm[f].y = div9(a1);
                mm[f].z = div9(a2);
            }
        }
        float2 maxShift, minShift;
        maxShift.x = fmaxf(s[f].x, shiftf[f].x);
        maxShift.y = fmaxf(s[f].y, shiftf[f].y);
        minShift.x = fminf(s[f].x, shiftf[f].x);
        minShift.y = fminf(s[f].y, shiftf[f].y);
        const float mmc[3] = {mm[f].x, mm[f].y, mm[f].z};
        float meandist = fabsf(mr[0] - mmc[0]) + fabsf(mr[1] - mmc[1]) + fabsf(mr[2] - mmc[2]);
        meandist = div3(meandist);
        const float hm = 0.5f * meandist;
        const float ddx = maxShift.x * hm - minShift.x * hm, ddy = maxShift.y * hm - minShift.y * hm;
        const float M = __builtin_amdgcn_sqrtf(ddx * ddx + ddy * ddy);
        const float sc = (M > thresholdM) ? 0.0f : 1.5f;
        float m3[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float d = fabsf(mr[c] - mmc[c]);
            d = d * A[c];                                 // (0 * inf = NaN as in the reference)
            const float e = __builtin_amdgcn_exp2f(-(d * d) * Rg[c] * 1.44269504088896340736f);
            m3[c] = fmaxf(fminf(__builtin_fmaf(sc, e, -0.12f), 1.0f), 0.0f);
        }
        *(float4*)((char*)ga.f[f].mask + oM) = make_float4(m3[0], m3[1], m3[2], M);
    }
}

// 0: the straight kernel (IEEE sqrt / division, ocml expf: tight parity tests); 1 (default): k_robustnessFused
static std::atomic<int> g_robustness_fast{1};
extern "C" int mfsr_set_robustness_fast(int enable)
{
    g_robustness_fast = enable ? 1 : 0;
    return MFSR_OK;
}

// k_robustnessFused for 1 .. 4 moved frames against one reference in one launch: the frame table's checks and the launch
static int robustness_fused_launch(int nFrames, const mfsr_robustness_frame* frames, const mfsr_float3* rawImgRef, int flowPitch,
                                   int flowWidth, int flowHeight, int imgWidth, int imgHeight, int imgPitch, int maskPitch, float alpha,
                                   float beta, float thresholdM, mfsr_stream_t stream, const char* what)
{
    mfsr_tex2d texUV;
    texUV.ptr = frames[0].flow;
    texUV.pitch = flowPitch;
    texUV.width = flowWidth;
    texUV.height = flowHeight;
    MFSR_REQUIRE(mfsr_tex_ok(texUV, 8) && (flowPitch & 7) == 0);
    RobustFusedFrames fr;
    memset(&fr, 0, sizeof(fr));
    for (int i = 0; i < nFrames; i++) {
        MFSR_REQUIRE(frames[i].movedHalf && frames[i].mask && frames[i].flow);
        MFSR_REQUIRE(((uintptr_t)frames[i].mask & 15) == 0 && ((uintptr_t)frames[i].flow & 7) == 0);
        fr.f[i] = RobustFusedFrame{(const pix3*)frames[i].movedHalf, (float4*)frames[i].mask, (const float2*)frames[i].flow};
    }
    dim3 block(RB_TX, RB_TY), grid(mfsr_cdiv(imgWidth, RB_TX), mfsr_cdiv(imgHeight, RB_TY), nFrames);
    const MfsrExactDiv dW = mfsr_exact_div((float)imgWidth), dH = mfsr_exact_div((float)imgHeight);
    if (flowWidth == imgWidth && flowHeight == imgHeight)
        hipLaunchKernelGGL(k_robustnessFused<true>, grid, block, 0, mfsr_s(stream), (const pix3*)rawImgRef, fr, texUV, imgWidth, imgHeight,
                           imgPitch, maskPitch, alpha, beta, thresholdM, dW, dH);
    else
        hipLaunchKernelGGL(k_robustnessFused<false>, grid, block, 0, mfsr_s(stream), (const pix3*)rawImgRef, fr, texUV, imgWidth, imgHeight,
                           imgPitch, maskPitch, alpha, beta, thresholdM, dW, dH);
    return mfsr_launch_status(what);
}

// F1 + the zero ring in one launch (what the burst pipeline calls); falls back to ring + straight kernel when the fast
// kernel is switched off
extern "C" int mfsr_robustnessMaskFused(const mfsr_float3* rawImgRef, const mfsr_float3* rawImgMoved, mfsr_float4* robustnessMask,
                                        mfsr_tex2d texUV, int imgWidth, int imgHeight, int imgPitch, int maskPitch, float alpha,
                                        float beta, float thresholdM, mfsr_stream_t stream)
{
    MFSR_REQUIRE(rawImgRef && rawImgMoved && robustnessMask && imgWidth > 2 && imgHeight > 2);
    MFSR_REQUIRE((long long)imgPitch >= 12LL * imgWidth && (imgPitch & 3) == 0);
    MFSR_REQUIRE((long long)maskPitch >= 16LL * imgWidth && (maskPitch & 15) == 0 && ((uintptr_t)robustnessMask & 15) == 0);
    MFSR_REQUIRE(mfsr_tex_ok(texUV, 8) && ((uintptr_t)texUV.ptr & 7) == 0 && (texUV.pitch & 7) == 0);
    if (!g_robustness_fast) {
        int rc = mfsr_zeroRing_f32x4(robustnessMask, maskPitch, imgWidth, imgHeight, stream);
        if (rc) return rc;
        return mfsr_ComputeRobustnessMask(rawImgRef, rawImgMoved, robustnessMask, texUV, imgWidth, imgHeight, imgPitch, maskPitch,
                                          alpha, beta, thresholdM, stream);
    }
    const mfsr_robustness_frame one = {rawImgMoved, robustnessMask, (const mfsr_float2*)texUV.ptr};
    return robustness_fused_launch(1, &one, rawImgRef, texUV.pitch, texUV.width, texUV.height, imgWidth, imgHeight, imgPitch, maskPitch,
                                   alpha, beta, thresholdM, stream, "robustnessMaskFused");
}

// mfsr_robustnessMaskFused for 1 .. 4 moved frames against one reference in one launch (the fused kernel only)
extern "C" int mfsr_robustnessMaskFusedBatch(int nFrames, const mfsr_robustness_frame* frames, const mfsr_float3* rawImgRef, int flowPitch,
                                             int flowWidth, int flowHeight, int imgWidth, int imgHeight, int imgPitch, int maskPitch,
                                             float alpha, float beta, float thresholdM, mfsr_stream_t stream)
{
    MFSR_REQUIRE(frames && nFrames >= 1 && nFrames <= MFSR_BATCH_MAX && rawImgRef && imgWidth > 2 && imgHeight > 2);
    MFSR_REQUIRE((long long)imgPitch >= 12LL * imgWidth && (imgPitch & 3) == 0);
    MFSR_REQUIRE((long long)maskPitch >= 16LL * imgWidth && (maskPitch & 15) == 0);
    if (!g_robustness_fast) return MFSR_E_UNSUPPORTED;
    return robustness_fused_launch(nFrames, frames, rawImgRef, flowPitch, flowWidth, flowHeight, imgWidth, imgHeight, imgPitch, maskPitch,
                                   alpha, beta, thresholdM, stream, "robustnessMaskFusedBatch");
}

// 1 (default): the burst driver makes the masks of an aligned group with mfsr_prepareFrameMeansBatch + mfsr_robustnessMaskGroup;
// 0 (mfsr_set_robustness_group / MFSR_ROBUST_GROUP=0): with mfsr_prepareFrameFusedBatch + mfsr_robustnessMaskFusedBatch (A/B)
static MfsrKnob g_robustness_group;
extern "C" int mfsr_set_robustness_group(int enable)
{
    g_robustness_group.set(enable ? 1 : 0);
    return MFSR_OK;
}
int mfsr_robustness_group()
{
    return g_robustness_group.get([] { return mfsr_env_is0("MFSR_ROBUST_GROUP") ? 0 : 1; }) && g_robustness_fast;
}

// the kernel addresses a frame's flow, patch-mean and mask images with 32-bit byte offsets
int mfsr_robustness_group_fits(int h, int flowRowBytes, int meansRowBytes, int maskRowBytes)
{
    const long long lim = 1LL << 31;
    return (long long)flowRowBytes * h < lim && (long long)meansRowBytes * h < lim && (long long)maskRowBytes * h < lim;
}

template <int NF>
static void launch_robustness_group(int cfa, dim3 grid, dim3 block, hipStream_t st, const pix3* ref, const RobustGroupArgs& ga, int w, int h,
                                    int refRowBytes, int flowRowBytes, int meansRowBytes, int maskRowBytes, float maxVal, float alpha,
                                    float beta, float thresholdM)
{
    hipLaunchKernelGGL(k_robustnessGroup<NF>, grid, block, 0, st, ref, ga, w, h, refRowBytes, flowRowBytes, meansRowBytes, maskRowBytes,
                       maxVal, cfa, alpha, beta, thresholdM, mfsr_exact_div((float)w), mfsr_exact_div((float)h));
}

// The masks of 1 .. 4 moved frames against one reference in one pass (k_robustnessGroup): bit-identical to
// mfsr_robustnessMaskFusedBatch with a flow field of the image's resolution
int mfsr_cfa::robustnessMaskGroup(int cfa, int nFrames, const mfsr_robustness_group_frame* frames, const mfsr_float3* refHalf,
                                  int refRowBytes, int flowRowBytes, int meansRowBytes, int maskRowBytes, int w, int h, float maxVal,
                                  float alpha, float beta, float thresholdM, mfsr_stream_t stream)
{
    MFSR_REQUIRE(frames && nFrames >= 1 && nFrames <= MFSR_BATCH_MAX && refHalf && w > 2 && h > 2);
    MFSR_REQUIRE((long long)refRowBytes >= 12LL * w && (refRowBytes & 3) == 0);
    MFSR_REQUIRE((long long)meansRowBytes >= 12LL * w && (meansRowBytes & 3) == 0);
    MFSR_REQUIRE((long long)maskRowBytes >= 16LL * w && (maskRowBytes & 15) == 0);
    MFSR_REQUIRE((long long)flowRowBytes >= 8LL * w && (flowRowBytes & 7) == 0);
    MFSR_REQUIRE(((uintptr_t)refHalf & 3) == 0);
    RobustGroupArgs ga;
    memset(&ga, 0, sizeof(ga));
    for (int i = 0; i < nFrames; i++) {
        MFSR_REQUIRE(frames[i].movedMeans && frames[i].movedRaw && frames[i].mask && frames[i].flow);
        MFSR_REQUIRE(((uintptr_t)frames[i].mask & 15) == 0 && ((uintptr_t)frames[i].flow & 7) == 0);
        MFSR_REQUIRE(((uintptr_t)frames[i].movedMeans & 3) == 0 && ((uintptr_t)frames[i].movedRaw & 3) == 0);
        ga.f[i].means = (const pix3*)frames[i].movedMeans;
        ga.f[i].raw = frames[i].movedRaw;
        ga.f[i].mask = (float4*)frames[i].mask;
        ga.f[i].flow = (const float2*)frames[i].flow;
    }
    if (!g_robustness_fast || !mfsr_robustness_group_fits(h, flowRowBytes, meansRowBytes, maskRowBytes)) return MFSR_E_UNSUPPORTED;
    dim3 block(RB_TX, RB_TY), grid(mfsr_cdiv(w, RB_TX), mfsr_cdiv(h, RB_TY));
    const pix3* ref = (const pix3*)refHalf;
    hipStream_t st = mfsr_s(stream);
#define RB_GROUP_ARGS cfa, grid, block, st, ref, ga, w, h, refRowBytes, flowRowBytes, meansRowBytes, maskRowBytes, maxVal, alpha, beta, thresholdM
    switch (nFrames) {
        case 1: launch_robustness_group<1>(RB_GROUP_ARGS); break;
        case 2: launch_robustness_group<2>(RB_GROUP_ARGS); break;
        case 3: launch_robustness_group<3>(RB_GROUP_ARGS); break;
        default: launch_robustness_group<4>(RB_GROUP_ARGS); break;
    }
#undef RB_GROUP_ARGS
    return mfsr_launch_status("robustnessMaskGroup");
}
extern "C" int mfsr_robustnessMaskGroup(int nFrames, const mfsr_robustness_group_frame* frames, const mfsr_float3* refHalf, int refRowBytes,
                                        int flowRowBytes, int meansRowBytes, int maskRowBytes, int w, int h, float maxVal, float alpha,
                                        float beta, float thresholdM, mfsr_stream_t stream)
{
    return mfsr_cfa::robustnessMaskGroup(mfsr_cfa_packed(), nFrames, frames, refHalf, refRowBytes, flowRowBytes, meansRowBytes, maskRowBytes, w,
                                         h, maxVal, alpha, beta, thresholdM, stream);
}

extern "C" int mfsr_ComputeRobustnessMask(const mfsr_float3* rawImgRef, const mfsr_float3* rawImgMoved,
                                          mfsr_float4* robustnessMask, mfsr_tex2d texUV, int imgWidth, int imgHeight,
                                          int imgPitch, int maskPitch, float alpha, float beta, float thresholdM,
                                          mfsr_stream_t stream)
{
    MFSR_REQUIRE(rawImgRef && rawImgMoved && robustnessMask && imgWidth > 2 && imgHeight > 2);
    MFSR_REQUIRE((long long)imgPitch >= 12LL * imgWidth && (imgPitch & 3) == 0);
    MFSR_REQUIRE((long long)maskPitch >= 16LL * imgWidth && (maskPitch & 15) == 0 && ((uintptr_t)robustnessMask & 15) == 0);
    MFSR_REQUIRE(mfsr_tex_ok(texUV, 8) && ((uintptr_t)texUV.ptr & 7) == 0 && (texUV.pitch & 7) == 0);
    dim3 block(64, 4), grid(mfsr_cdiv(imgWidth, 64), mfsr_cdiv(imgHeight, 4));
    hipLaunchKernelGGL(k_ComputeRobustnessMask, grid, block, 0, mfsr_s(stream), (const pix3*)rawImgRef,
                       (const pix3*)rawImgMoved, (float4*)robustnessMask, texUV, imgWidth, imgHeight, imgPitch, maskPitch,
                       alpha, beta, thresholdM);
    return mfsr_launch_status("ComputeRobustnessMask");
}
