// common.hpp -- shared device/host helpers of the MI355X (gfx950) MFSR kernels.
//
// Canonical arithmetic: compiled with -ffp-contract=off so that the
// straight ports of +,-,*,/ kernels are bit-identical to the no-contraction
// CPU oracle; fused multiply-adds appear only where written explicitly.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/mfsr.h"

#define MFSR_WAVE 64

// ---- error handling: int codes, never throw (kernel.cu:36-114 convention) ----
#define MFSR_HIP_TRY(expr)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "mfsr: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, \
                    __LINE__);                                                                      \
            return (int)e_;                                                                         \
        }                                                                                           \
    } while (0)

#define MFSR_REQUIRE(cond)                                                                  \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            fprintf(stderr, "mfsr: invalid argument: %s (%s:%d)\n", #cond, __FILE__, __LINE__); \
            return MFSR_E_INVALID;                                                          \
        }                                                                                   \
    } while (0)

static inline int mfsr_launch_status(const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fprintf(stderr, "mfsr: launch of %s failed: %s\n", what, hipGetErrorString(e));
        return (int)e;
    }
    return MFSR_OK;
}

static inline hipStream_t mfsr_s(mfsr_stream_t s) { return (hipStream_t)s; }

// an HR output window [x0, x0+w) x [y0, y0+h) of an hrW x hrH grid the fuse kernels take (host only): origin on the 16-pixel
// grid, sides multiples of 16 unless they reach the frame's right / bottom edge, inside the frame, not empty
static inline bool mfsr_window_ok(int hrW, int hrH, int x0, int y0, int w, int h)
{
    if (hrW <= 0 || hrH <= 0 || x0 < 0 || y0 < 0 || w <= 0 || h <= 0) return false;
    if ((x0 % 16) != 0 || (y0 % 16) != 0) return false;
    if ((long long)x0 + w > hrW || (long long)y0 + h > hrH) return false;
    if ((w % 16) != 0 && x0 + w != hrW) return false;
    if ((h % 16) != 0 && y0 + h != hrH) return false;
    return true;
}
static inline unsigned mfsr_cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }
// ceil(log2 v) for v >= 1; the callers pass powers of two (pyramid factors, the local-tone grid's cell and bins)
static inline int ilog2(int v)
{
    int s = 0;
    while ((1 << s) < v) s++;
    return s;
}
// the host checks of a render description (format, matrix coefficients, tone table size): MFSR_OK or MFSR_E_INVALID; render.hip
int mfsr_render_validate(const mfsr_render* r);
// without a render description: the plain finish's steps (no matrix, no table, uint16_t RGB)
static inline mfsr_render mfsr_plain_render()
{
    mfsr_render r = {};
    r.format = MFSR_OUT_RGB16;
    return r;
}

// Frame batches: a batched kernel takes a table of up to MFSR_BATCH_MAX entries of its own typed per-frame pointers by value and
// reads entry blockIdx.z (a scalar load); a single-frame entry point launches it with a table of one.
#define MFSR_BATCH_MAX 4

// internal C++ functions shared between the library's translation units: not part of its exported symbols
#define MFSR_INTERNAL __attribute__((visibility("hidden")))

// ---- environment knobs (A/B switches) --------------------
// The three parses the knobs use.  A knob without a setter keeps its value in a function-local `static const`.
static inline bool mfsr_env_is0(const char* name)  // set and begins with '0'
{
    const char* e = getenv(name);
    return e && e[0] == '0';
}
static inline bool mfsr_env_is1(const char* name)  // set and begins with '1'
{
    const char* e = getenv(name);
    return e && e[0] == '1';
}
static inline int mfsr_env_int(const char* name, int dflt)  // atoi of the value, dflt when unset
{
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
// A knob that also has a setter (mfsr_set_*): the first get() takes the environment's value (fromEnv), unless set() came first;
// set() overrides it for good.  Values are >= 0.  Rank threads read and set it concurrently, hence the atomic.
class MfsrKnob {
public:
    template <class FromEnv>
    int get(FromEnv fromEnv)
    {
        int v = v_.load(std::memory_order_relaxed);
        if (v < 0) {
            const int e = fromEnv();
            if (v_.compare_exchange_strong(v, e, std::memory_order_relaxed)) v = e;  // (lost to a set(): v holds its value)
        }
        return v;
    }
    void set(int v) { v_.store(v, std::memory_order_relaxed); }

private:
    std::atomic<int> v_{-1};
};

// compute units of the current device, cached per device (256 where the query fails)
static inline int mfsr_device_cus()
{
    constexpr int kDevs = 64;
    static std::atomic<int> cache[kDevs];
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kDevs) return 256;
    if ((cus = cache[dev].load(std::memory_order_relaxed)) > 0) return cus;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 256;
    cache[dev].store(cus, std::memory_order_relaxed);
    return cus;
}

// ---- CFA pattern: packed 4 x 8 bit, [y%2][x%2] -> bits ((y&1)*2+(x&1))*8 -----
// Every kernel takes the pattern as a packed launch argument.  A burst or frame stream packs cfg.cfa once at create and
// passes it down (the mfsr_cfa:: forms below); the process-wide pattern of mfsr_set_cfa_pattern, the port of the reference's
// module constant, serves the reference-shaped extern "C" entry points only, which forward mfsr_cfa_packed().
// *packed = the launch word of `pattern`; MFSR_E_INVALID (mfsr_set_cfa_pattern's refusal) for an entry outside 0..MFSR_WHITE
static inline int mfsr_pack_cfa(const int32_t pattern[4], int* packed)
{
    MFSR_REQUIRE(pattern != nullptr);
    for (int i = 0; i < 4; i++) MFSR_REQUIRE(pattern[i] >= 0 && pattern[i] <= MFSR_WHITE);
    *packed = pattern[0] | (pattern[1] << 8) | (pattern[2] << 16) | (pattern[3] << 24);
    return MFSR_OK;
}
MFSR_INTERNAL int mfsr_cfa_packed();  // the process-wide pattern, packed; debayer.hip
// The launchers with the packed pattern as their first argument; everything else as the extern "C" entry point of the same name
// (include/mfsr.h), which forwards here.  prepareFrames serves mfsr_prepareFrameFused / FusedBatch / MeansBatch (means).
namespace mfsr_cfa {
MFSR_INTERNAL int deBayersSubSample3(int cfa, const uint16_t* dataIn, mfsr_float3* imgOut, float maxVal, int dimX, int dimY, int strideOut,
                                     mfsr_stream_t stream);
MFSR_INTERNAL int prepareFrames(int cfa, int n, const mfsr_prepare_frame* f, int halfPitch, float maxVal, int dimX, int dimY, int pyr0Pitch,
                                int pyr1Pitch, const float* taps, int ntaps, mfsr_stream_t stream, bool means);
MFSR_INTERNAL int deBayerGreenKernel(int cfa, int width, int height, const float* imgIn, int strideIn, mfsr_float3* outImage, int strideOut,
                                     mfsr_float3 blackPoint, mfsr_float3 scale, mfsr_stream_t stream);
MFSR_INTERNAL int deBayerRedBlueKernel(int cfa, int width, int height, const float* imgIn, int strideIn, mfsr_float3* outImage,
                                       int strideOut, mfsr_float3 blackPoint, mfsr_float3 scale, mfsr_stream_t stream);
MFSR_INTERNAL int deBayerFused(int cfa, const uint16_t* raw, mfsr_float3* outImage, int strideOut, int width, int height,
                               mfsr_float3 blackPoint, mfsr_float3 scale, mfsr_stream_t stream);
MFSR_INTERNAL int deBayerFusedRing(int cfa, const uint16_t* raw, mfsr_tex2d outImage, mfsr_float3 blackPoint, mfsr_float3 scale,
                                   mfsr_stream_t stream);
MFSR_INTERNAL int accumulateSuperResFullRows(int cfa, int nFrames, const uint16_t* const* dataIn, mfsr_float3* imgOut,
                                             mfsr_float3* totalWeights, const mfsr_float4* const* certaintyMask, mfsr_tex2d kernelParam,
                                             const mfsr_tex2d* shifts, mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int dimX, int dimY,
                                             int scale, int strideOut, int strideMask, int accumulatorsUndefined, int rowBegin, int rowEnd,
                                             mfsr_stream_t stream);
MFSR_INTERNAL int accumulateSuperResFullWindow(int cfa, int nFrames, const uint16_t* const* dataIn, mfsr_float3* imgOut,
                                               mfsr_float3* totalWeights, const mfsr_float4* const* certaintyMask, mfsr_tex2d kernelParam,
                                               const mfsr_tex2d* shifts, mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int dimX, int dimY,
                                               int scale, int strideOut, int strideMask, int accumulatorsUndefined, int x0, int y0, int w,
                                               int h, mfsr_stream_t stream);
MFSR_INTERNAL int accumulateSuperResBurst(int cfa, int nFrames, const uint16_t* const* dataIn, mfsr_tex2d imgOut, mfsr_tex2d totalWeights,
                                          const mfsr_tex2d* certaintyMasks, mfsr_tex2d kernelParam, const mfsr_tex2d* shifts,
                                          mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int scale, int accumulatorsUndefined,
                                          mfsr_stream_t stream);
MFSR_INTERNAL int accumulateSuperResBurstFinish(int cfa, int nFrames, const uint16_t* const* dataIn, mfsr_tex2d imgOut,
                                                mfsr_tex2d totalWeights, const mfsr_tex2d* certaintyMasks, mfsr_tex2d kernelParam,
                                                const mfsr_tex2d* shifts, mfsr_float3 whiteLevel, mfsr_float3 blackLevel, int scale,
                                                int accumulatorsUndefined, mfsr_tex2d fallback, float u0, float u1, float v0, float v1,
                                                float threshold, uint16_t* out16, int out16Width, int out16Height, int applyGamma,
                                                float maxOut, int colOffset, int rowOffset, int fullWidth, int fullHeight,
                                                mfsr_stream_t stream);
MFSR_INTERNAL int robustnessMaskGroup(int cfa, int nFrames, const mfsr_robustness_group_frame* frames, const mfsr_float3* refHalf,
                                      int refRowBytes, int flowRowBytes, int meansRowBytes, int maskRowBytes, int w, int h, float maxVal,
                                      float alpha, float beta, float thresholdM, mfsr_stream_t stream);
}  // namespace mfsr_cfa
int mfsr_reference_fused();  // the switch of mfsr_set_reference_fused, kernel_field.hip (process-wide state)
int mfsr_robustness_group();  // mfsr_set_robustness_group and the fast robustness kernel both on, robustness.hip (process-wide state)
int mfsr_robustness_group_fits(int h, int flowRowBytes, int meansRowBytes, int maskRowBytes);  // images below 2 GiB (k_robustnessGroup's offsets)
// what mfsr_lucasKanadeSweepBatch takes: MFSR_OK, or the status it returns (lk_fused.hip)
MFSR_INTERNAL int mfsr_lk_sweep_accepts(int nFrames, int width, int height, int halfWindowSize, int pitchShift, int pitchImg, int pitchSD);
// x / d for a divisor that is the same for a whole launch (an image dimension): q = x r, q' = fma(fma(-d, q, x), r, q) with
// r = RN(1 / d) -- two multiply-adds after the product instead of the ~10 instructions of the IEEE division expansion.  For a
// given d the sequence either is the correctly rounded quotient for EVERY x or it is not (scaling x by a power of two
// commutes with every rounding involved), so the host checks it once per divisor over all 2^23 significands of one binade
// (mfsr_exact_div in glue.hip: ~15 ms, cached) and the kernels take the sequence only when that check passed (ok), else the
// division: bit-identical to `x / d` by construction.  (Every image dimension tried passes; the check is the proof, not the
// assumption.)  Infinite and NaN quotients (an infinite flow) are passed through as the division gives them.
// MFSR_EXACT_DIV=0: always the division (A/B).
struct MfsrExactDiv {
    float d, r;
    int ok;
};
MfsrExactDiv mfsr_exact_div(float d);  // host; glue.hip
__device__ __forceinline__ float mfsr_div(float x, const MfsrExactDiv& e)
{
    if (e.ok) {  // uniform
        const float q = x * e.r;
        const float q2 = __builtin_fmaf(__builtin_fmaf(-e.d, q, x), e.r, q);
        return fabsf(q) < __builtin_inff() ? q2 : q;
    }
    return x / e.d;
}

__device__ __forceinline__ int cfa_at(int packed, int y, int x) { return (packed >> ((((y & 1) << 1) | (x & 1)) << 3)) & 0xff; }

// ---- row addressing with byte pitches ----------------------------------------
template <typename T>
__device__ __forceinline__ T* row_ptr(T* base, int pitch, int y)
{
    return (T*)((char*)base + (size_t)pitch * (size_t)y);
}
template <typename T>
__device__ __forceinline__ const T* row_ptr(const T* base, int pitch, int y)
{
    return (const T*)((const char*)base + (size_t)pitch * (size_t)y);
}

// packed 12-byte pixel (the reference's float3); float3 in HIP is also 12 B
struct __attribute__((packed, aligned(4))) pix3 {
    float x, y, z;
};

// float -> int: v_cvt_i32_f32 (NaN -> 0, saturating), the CPU oracle converts the same way
__device__ __forceinline__ int f2i(float f) { return __float2int_rz(f); }

// f2i(roundf(f)) in three instructions: adding the largest float below 0.5 (with f's sign) and
// truncating is roundf for EVERY float (half away from zero; checked exhaustively over all 2^32
// bit patterns on the host), and v_cvt_i32_f32 is the truncation.
__device__ __forceinline__ int round2i(float f) { return __float2int_rz(f + copysignf(0.49999997f, f)); }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < __builtin_inff(); }

// ---- texture stand-in: exact-float bilinear, normalised coordinates ----------
// unnormalised coord = u*W - 0.5, texel indices clamped; MIRROR reflects the
// normalised coordinate first (CUDA cudaAddressModeMirror).
enum { ADDR_CLAMP = 0, ADDR_MIRROR = 1 };

__device__ __forceinline__ float mirror_coord(float x)
{
    float f = floorf(x);
    float fr = x - f;
    return (f2i(f) & 1) ? 1.0f - fr : fr;
}

struct TexCoord {
    int i0, i1, j0, j1;
    float a, b;
};

template <int MODE>
__device__ __forceinline__ TexCoord tex_coord(int w, int h, float u, float v)
{
    if (MODE == ADDR_MIRROR) {
        u = mirror_coord(u);
        v = mirror_coord(v);
    }
    float xB = u * (float)w - 0.5f;
    float yB = v * (float)h - 0.5f;
    if (!finitef(xB)) xB = 0.0f;
    if (!finitef(yB)) yB = 0.0f;
    float fx = floorf(xB), fy = floorf(yB);
    TexCoord c;
    c.a = xB - fx;
    c.b = yB - fy;
    int ix = f2i(fx), iy = f2i(fy);
    c.i0 = clampi(ix, 0, w - 1);
    c.i1 = (ix >= 2147483647) ? w - 1 : clampi(ix + 1, 0, w - 1);
    c.j0 = clampi(iy, 0, h - 1);
    c.j1 = (iy >= 2147483647) ? h - 1 : clampi(iy + 1, 0, h - 1);
    return c;
}

__device__ __forceinline__ float lerp4(float t00, float t10, float t01, float t11, float a, float b)
{
    return (((1.0f - a) * (1.0f - b) * t00 + a * (1.0f - b) * t10) + (1.0f - a) * b * t01) + a * b * t11;
}

template <int MODE>
__device__ __forceinline__ float tex1(const mfsr_tex2d& t, float u, float v)
{
    TexCoord c = tex_coord<MODE>(t.width, t.height, u, v);
    const float* r0 = row_ptr((const float*)t.ptr, t.pitch, c.j0);
    const float* r1 = row_ptr((const float*)t.ptr, t.pitch, c.j1);
    return lerp4(r0[c.i0], r0[c.i1], r1[c.i0], r1[c.i1], c.a, c.b);
}

template <int MODE>
__device__ __forceinline__ float2 tex2(const mfsr_tex2d& t, float u, float v)
{
    TexCoord c = tex_coord<MODE>(t.width, t.height, u, v);
    const float2* r0 = row_ptr((const float2*)t.ptr, t.pitch, c.j0);
    const float2* r1 = row_ptr((const float2*)t.ptr, t.pitch, c.j1);
    float2 t00 = r0[c.i0], t10 = r0[c.i1], t01 = r1[c.i0], t11 = r1[c.i1];
    return make_float2(lerp4(t00.x, t10.x, t01.x, t11.x, c.a, c.b), lerp4(t00.y, t10.y, t01.y, t11.y, c.a, c.b));
}

template <int MODE>
__device__ __forceinline__ float4 tex4(const mfsr_tex2d& t, float u, float v)
{
    TexCoord c = tex_coord<MODE>(t.width, t.height, u, v);
    const float4* r0 = row_ptr((const float4*)t.ptr, t.pitch, c.j0);
    const float4* r1 = row_ptr((const float4*)t.ptr, t.pitch, c.j1);
    float4 t00 = r0[c.i0], t10 = r0[c.i1], t01 = r1[c.i0], t11 = r1[c.i1];
    return make_float4(lerp4(t00.x, t10.x, t01.x, t11.x, c.a, c.b), lerp4(t00.y, t10.y, t01.y, t11.y, c.a, c.b),
                       lerp4(t00.z, t10.z, t01.z, t11.z, c.a, c.b), lerp4(t00.w, t10.w, t01.w, t11.w, c.a, c.b));
}

// ---- argument checks shared by the entry points -------------------------------
static inline bool mfsr_tex_ok(const mfsr_tex2d& t, int texel_bytes)
{
    return t.ptr != nullptr && t.width > 0 && t.height > 0 && (long long)t.pitch >= (long long)t.width * texel_bytes;
}
