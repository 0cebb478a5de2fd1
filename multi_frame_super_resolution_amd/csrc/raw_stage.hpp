// raw_stage.hpp -- what the raw-domain stages share (select.hip, exposure.hip, noise.hip, defect.hip, shading.hip, unpack.hip):
// the frame table of a launch, the host checks of their entry points, the whole-wave exchanges, and for the two stages that
// stream quad rows down strips and bands (k_frameSharpness, k_frameLevels) the loader and the band planner.  Internal: every
// rule an entry point states in include/mfsr.h is composed from the checks here, and a check is shared only where the rule
// is the same.
#pragma once

#include "common.hpp"

#include <climits>

constexpr int kRawMaxFrames = 64;              // frame pointers in one launch's argument table
constexpr int kRawLanes = 64;
constexpr int kRawChunk = 4;                   // quad rows loaded per step of a walk down a band (two steps in flight)
constexpr long long kRawMaxArea = 1LL << 23;   // quads of a half-resolution rectangle: the 64-bit sums over it cannot overflow

template <typename T>
struct RawFramesT {
    T* p[kRawMaxFrames];
};
typedef RawFramesT<const uint16_t> RawFrames;
typedef RawFramesT<uint16_t> RawFramesMut;     // the in-place kernels (k_applyGains, k_defectRepair)

// ---- host checks --------------------------------------------------------------------------------------------------------
// 1 .. maxFrames frames, each 2-byte aligned, rows of `width` samples within an even pitch
static inline bool raw_frames_ok(int nFrames, int maxFrames, const uint16_t* const* frames, int pitch, int width)
{
    if (nFrames < 1 || nFrames > maxFrames || frames == nullptr) return false;
    if ((long long)pitch < 2LL * width || (pitch % 2) != 0) return false;
    for (int k = 0; k < nFrames; k++)
        if (frames[k] == nullptr || ((uintptr_t)frames[k] & 1) != 0) return false;
    return true;
}

// whole quads
static inline bool raw_even_ok(int width, int height) { return width > 0 && height > 0 && (width % 2) == 0 && (height % 2) == 0; }

// a half-resolution rectangle (x0, y0, x1, y1): not empty, inside the frame less its one-quad ring, at most kRawMaxArea quads
static inline bool raw_half_rect_ok(const int32_t rect[4], int width, int height)
{
    if (rect == nullptr) return false;
    const int hw = width / 2, hh = height / 2;
    const int x0 = rect[0], y0 = rect[1], x1 = rect[2], y1 = rect[3];
    if (!(x0 >= 1 && x0 < x1 && x1 <= hw - 1 && y0 >= 1 && y0 < y1 && y1 <= hh - 1)) return false;
    return (long long)(x1 - x0) * (y1 - y0) <= kRawMaxArea;
}

// every frame pointer and the pitch are multiples of `bytes`: the kernels' VEC decision
template <typename T>
static inline bool raw_aligned(int nFrames, T* const* frames, int pitch, int bytes)
{
    bool ok = (pitch % bytes) == 0;
    for (int k = 0; k < nFrames; k++) ok = ok && ((uintptr_t)frames[k] % (uintptr_t)bytes) == 0;
    return ok;
}

// the bounds of exposure matching (mfsr_exposure_gains, mfsr_burst_match_exposure)
static inline bool exposure_bounds_ok(int deadband, int minGain, int maxGain)
{
    return deadband >= 0 && deadband < 65536 && minGain >= 4096 && minGain <= 65536 && maxGain >= 65536 && maxGain <= 1048576;
}

template <typename T>
static inline RawFramesT<T> raw_table(int nFrames, T* const* frames)
{
    RawFramesT<T> t = {};
    for (int k = 0; k < nFrames; k++) t.p[k] = frames[k];
    return t;
}

// ---- launch planning ----------------------------------------------------------------------------------------------------
// workgroups of Kernel the current device holds at once (CUs x occupancy), cached per device
template <auto Kernel>
static int resident_blocks(int threads)
{
    constexpr int kDevs = 64;
    static std::atomic<int> cache[kDevs];
    int dev = 0, perCU = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kDevs) dev = -1;
    if (dev >= 0 && cache[dev] > 0) return cache[dev];
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, Kernel, threads, 0) != hipSuccess || perCU <= 0) perCU = 4;
    const int r = mfsr_device_cus() * perCU;
    if (dev >= 0) cache[dev] = r;
    return r;
}

// One wave owns a strip of columns and a band of rows of one frame.  Bands as short as keeps the launch within one round of
// resident workgroups (every wave then streams from the start to the end of the launch, no tail), within [minRows, maxRows].
struct RawBands {
    int rows, n;  // rows of a band, bands
};
static inline RawBands plan_bands(int rows, int nStrips, int framesInLaunch, int resident, int wavesPerBlock, int minRows, int maxRows)
{
    const int wavesPerFrame = wavesPerBlock * (resident / framesInLaunch > 1 ? resident / framesInLaunch : 1);
    const int bands = wavesPerFrame / nStrips > 1 ? wavesPerFrame / nStrips : 1;
    RawBands b;
    b.rows = (int)mfsr_cdiv(rows, bands);
    b.rows = b.rows < minRows ? minRows : b.rows;
    b.rows = b.rows > maxRows ? maxRows : b.rows;
    b.n = (int)mfsr_cdiv(rows, b.rows);
    return b;
}

// ---- whole-wave exchange ------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_shr1(T v)  // lane l <- lane l-1 (lane 0 <- 0)
{
    static_assert(sizeof(T) == 4, "one register");
    return (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true);
}
template <typename T>
__device__ __forceinline__ T wave_shl1(T v)  // lane l <- lane l+1 (lane 63 <- 0)
{
    static_assert(sizeof(T) == 4, "one register");
    return (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, true);
}

// the sum over the 64 lanes, in every lane (32-bit and 64-bit integers)
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = kRawLanes / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the sum over each aligned group of `lanes` lanes (a power of two, 1 .. 64; the same in the whole wave), in every lane of the group
template <typename T>
__device__ __forceinline__ T wave_group_sum(T v, int lanes)
{
#pragma unroll
    for (int o = kRawLanes / 2; o > 0; o >>= 1)
        if (o < lanes) v += __shfl_xor(v, o);
    return v;
}

// ---- a Q16 gain about the black level (k_applyGains, k_applyShading) -------------------------------------------------------------
// v (at quad position q's black level b, gain g = gh * 65536 + gl): (d * g + 32768) >> 16 = d * gh + ((d * gl + 32768) >> 16)
// for d = v - b < 2^16 -- d * gl + 32768 < 2^32, so 32-bit arithmetic is exact where the product d * g is not
__device__ __forceinline__ uint32_t gain_sample(uint32_t v, int b, int g, int sat, int maxValue)
{
    if ((int)v <= b || (int)v >= sat) return v;  // at or below black, or clipped: unchanged
    const uint32_t d = v - (uint32_t)b;
    const uint32_t r = (uint32_t)b + d * ((uint32_t)g >> 16) + ((d * ((uint32_t)g & 0xffffu) + 32768u) >> 16);
    return min(r, (uint32_t)maxValue);
}

// ---- quad rows ----------------------------------------------------------------------------------------------------------
// quad rows 2r (a) and 2r+1 (b) of half-resolution columns col .. col+3: one 32-bit word per column, x = 0 in the low half.
// Branch-free, so that the loads of a chunk issue back to back and the wait before a row's use counts only older loads: a
// column outside the frame reads a clamped in-frame address instead (no output depends on such a column: the caller masks
// it).  VEC: one 16-byte load per row at col clamped to [0, hw - 4] -- exact for every column inside the frame when
// hw % 4 == 0 (col is a multiple of 4, so a lane lies entirely inside or entirely outside the frame).
template <bool VEC>
__device__ __forceinline__ void quad_rows_load(const char* rowA, int pitch, int col, int hw, uint4& a, uint4& b)
{
    const char* rowB = rowA + pitch;
    if (VEC) {
        const size_t o = 4 * (size_t)clampi(col, 0, hw - 4);
        a = *(const uint4*)(rowA + o);
        b = *(const uint4*)(rowB + o);
        return;
    }
    uint32_t wa[4], wb[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const size_t o = 4 * (size_t)clampi(col + j, 0, hw - 1);
        const uint16_t* pa = (const uint16_t*)(rowA + o);
        const uint16_t* pb = (const uint16_t*)(rowB + o);
        wa[j] = (uint32_t)pa[0] | ((uint32_t)pa[1] << 16);
        wb[j] = (uint32_t)pb[0] | ((uint32_t)pb[1] << 16);
    }
    a = make_uint4(wa[0], wa[1], wa[2], wa[3]);
    b = make_uint4(wb[0], wb[1], wb[2], wb[3]);
}
