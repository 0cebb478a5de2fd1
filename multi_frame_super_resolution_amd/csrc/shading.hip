// shading.hip -- lens-shading correction of raw frames: a flat-field gain map applied in place, and the box statistics and the
// host fit that measure such a map from flat-field frames.
//
// The rule is stated in include/mfsr.h (mfsr_applyShading / mfsr_shadingStats / mfsr_shading_fit): exact integer arithmetic, the
// results equal the numpy restatement of the tests bit for bit, for any launch shape.
//
// k_applyShading: a workgroup works on one row, so the map rows j, j+1, the vertical weight and the two quad positions are the
// same for all its lanes.  Its first lanes blend the map columns under the workgroup's samples vertically, A = (cell - fy) *
// G[j] + fy * G[j+1] for both quad positions, and leave them in LDS split as A = Ah * cell + Al; then one lane per 16-byte
// aligned piece of the row (8 samples: one load, one store) as in k_applyGains, the pieces a row's ends cut and the samples
// before the first aligned address sample by sample.  With N = (cell - fx) * A0 + fx * A1 = P * cell + Q, P and Q from the
// high and the low parts, (N + cell^2/2) >> 2k = (P + ((Q + cell^2/2) >> k)) >> k: every factor is below 2^24 and every sum
// below 2^32, so the 64-bit rule is four 24-bit multiply-adds, two adds and two shifts in 32-bit registers.
//
// k_shadingStats: the shape of k_frameLevels (one wavefront per strip of 4 * 64 half-resolution columns and band of quad
// rows, 16-byte loads, the next 4 rows in flight while 4 are reduced) with the strips shifted left by half a cell and the
// bands cut at multiples of half a cell: a band then lies in one row of boxes and every aligned group of cell/4 lanes in one
// box, so the five sums are reduced over the group with shuffles and its first lane adds them with one 64-bit atomic each.
#include "raw_stage.hpp"

namespace {

// ---- apply ----------------------------------------------------------------------------------------------------------------
constexpr int kShadeThreads = 256;
// map columns under one workgroup's samples: 8 * 256 + 7 samples are at most 1028 quads, which touch at most 1028 / 8 + 1 = 129
// cells at the smallest cell, and the right-hand column of the last one
constexpr int kShadeMaxCols = 132;

struct ShadeGeom {
    int pitch, width, height;
    int lanesPerRow;   // 1 (the samples before the first 16-byte boundary) + the 8-sample pieces after it
    int blocksPerRow;
    int k, gw, gh;     // cell = 1 << k quads; the map is [4][gh][gw]
    int black[4];
    int maxValue;
};

// the gain of quad column X at the position whose blended map columns are (h, l) of c0 (left) and c1 (right)
__device__ __forceinline__ int shade_gain(uint32_t h0, uint32_t l0, uint32_t h1, uint32_t l1, uint32_t fx, int k)
{
    const uint32_t wx = (1u << k) - fx;
    const uint32_t P = __umul24(wx, h0) + __umul24(fx, h1);
    const uint32_t Q = __umul24(wx, l0) + __umul24(fx, l1);
    return (int)((P + ((Q + ((1u << (2 * k)) >> 1)) >> k)) >> k);
}

__global__ __launch_bounds__(kShadeThreads) void k_applyShading(RawFramesMut frames, ShadeGeom g, const int32_t* __restrict__ map)
{
    __shared__ uint4 cols[kShadeMaxCols];  // (Ah, Al) of the even-x position, (Ah, Al) of the odd-x position
    const int y = (int)(blockIdx.x / (unsigned)g.blocksPerRow), c0 = (int)(blockIdx.x % (unsigned)g.blocksPerRow) * kShadeThreads;
    char* row = (char*)frames.p[blockIdx.y] + (size_t)y * (size_t)g.pitch;
    const int head = (int)((16 - ((uintptr_t)row & 15)) & 15) >> 1;  // samples before the row's first 16-byte boundary (0 .. 7)
    const int k = g.k, cm = (1 << k) - 1;
    // the workgroup's samples [xs, xe) and the map columns i0 .. i1 under them (the right-hand column of the last cell included)
    const int xs = min(c0 == 0 ? 0 : head + 8 * (c0 - 1), g.width - 1);
    const int xe = min(head + 8 * (c0 + kShadeThreads - 1), g.width);
    const int i0 = (xs >> 1) >> k;
    const int i1 = min(((max(xe - 1, xs) >> 1) >> k) + 1, i0 + kShadeMaxCols - 1);
    const int Y = y >> 1, j = min(Y >> k, g.gh - 1), j1 = min(j + 1, g.gh - 1), fy = Y & cm;  // (fy = 0 where j + 1 is clamped)
    const int q0 = 2 * (y & 1);
    for (int t = threadIdx.x; t <= i1 - i0; t += kShadeThreads) {
        const int i = min(i0 + t, g.gw - 1);  // (a clamped column has weight 0: fx = 0 at the last grid point)
        uint32_t a[2];
#pragma unroll
        for (int o = 0; o < 2; o++) {
            const int32_t* m = map + (size_t)(q0 + o) * g.gh * g.gw + i;
            a[o] = (uint32_t)(cm + 1 - fy) * (uint32_t)m[(size_t)j * g.gw] + (uint32_t)fy * (uint32_t)m[(size_t)j1 * g.gw];
        }
        cols[t] = make_uint4(a[0] >> k, a[0] & (uint32_t)cm, a[1] >> k, a[1] & (uint32_t)cm);
    }
    __syncthreads();

    const int c = c0 + (int)threadIdx.x;
    if (c >= g.lanesPerRow) return;
    const int xa = c == 0 ? 0 : head + 8 * (c - 1);
    const int xb = min(c == 0 ? head : xa + 8, g.width);
    if (xa >= xb) return;
    // the gain of sample x (any x of this lane)
    auto gain_at = [&](int x) {
        const int X = x >> 1, t = (X >> k) - i0;
        const uint4 l = cols[t], r = cols[min(t + 1, kShadeMaxCols - 1)];
        return (x & 1) ? shade_gain(l.z, l.w, r.z, r.w, (uint32_t)(X & cm), k) : shade_gain(l.x, l.y, r.x, r.y, (uint32_t)(X & cm), k);
    };
    if (xb - xa == 8 && c >= 1) {  // (16-byte aligned)
        uint4* p = (uint4*)(row + 2 * (size_t)xa);
        const uint4 v = *p;
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const int qe = q0 + (xa & 1), qo = q0 + ((xa & 1) ^ 1);  // quad positions of the low / high half of a word
        const int be = g.black[qe], bo = g.black[qo];
        if ((xa & 1) == 0) {  // a word is a quad: its two samples share the columns and fx
#pragma unroll
            for (int n = 0; n < 4; n++) {
                const int X = (xa >> 1) + n, t = (X >> k) - i0;
                const uint32_t fx = (uint32_t)(X & cm);
                const uint4 l = cols[t], r = cols[min(t + 1, kShadeMaxCols - 1)];
                const int ge = shade_gain(l.x, l.y, r.x, r.y, fx, k), go = shade_gain(l.z, l.w, r.z, r.w, fx, k);
                w[n] = gain_sample(w[n] & 0xffffu, be, ge, 65536, g.maxValue) | (gain_sample(w[n] >> 16, bo, go, 65536, g.maxValue) << 16);
            }
        } else {
#pragma unroll
            for (int n = 0; n < 4; n++)
                w[n] = gain_sample(w[n] & 0xffffu, be, gain_at(xa + 2 * n), 65536, g.maxValue) |
                       (gain_sample(w[n] >> 16, bo, gain_at(xa + 2 * n + 1), 65536, g.maxValue) << 16);
        }
        *p = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    uint16_t* p = (uint16_t*)row;
    for (int x = xa; x < xb; x++) p[x] = (uint16_t)gain_sample(p[x], g.black[q0 + (x & 1)], gain_at(x), 65536, g.maxValue);
}

// ---- statistics -----------------------------------------------------------------------------------------------------------
constexpr int kStatStripCols = 4 * kRawLanes;  // half-resolution columns of one wave's strip
constexpr int kStatMaxBandRows = 32;           // quad rows of one wave's band: half a cell, at most this many
constexpr int kStatWavesPerBlock = 4;

struct StatGeom {
    int pitch;
    int hw, hh;  // half-resolution size
    int k, gw;
    int bandRows, nStrips, nBands;
    int black[4];
    int sat;
};

// VEC: every frame pointer and the pitch are 16-byte aligned and hw % 4 == 0 (16-byte loads); otherwise 16-bit loads
template <bool VEC>
__global__ __launch_bounds__(kStatWavesPerBlock * kRawLanes) void k_shadingStats(RawFrames frames, StatGeom g, unsigned long long* sums,
                                                                                 unsigned long long* counts, size_t plane)
{
    const int lane = threadIdx.x & (kRawLanes - 1);
    const int wave = blockIdx.x * kStatWavesPerBlock + (threadIdx.x >> 6);
    if (wave >= g.nStrips * g.nBands) return;  // (whole waves)
    const int strip = wave % g.nStrips, band = wave / g.nStrips;
    const int half = (1 << g.k) >> 1;
    const int col = strip * kStatStripCols - half + 4 * lane;  // a multiple of 4; box = (col + half) >> k for all four columns
    const int rb0 = band * g.bandRows;
    const int rb1 = min(rb0 + g.bandRows, g.hh);
    const char* base = (const char*)frames.p[blockIdx.y];

    bool m[4];  // this lane's column j lies in the frame
#pragma unroll
    for (int j = 0; j < 4; j++) m[j] = col + j >= 0 && col + j < g.hw;

    uint32_t s[4] = {0, 0, 0, 0}, cnt = 0;  // (a band has at most 32 rows: 4 * 32 * 65535 < 2^32)
    const int n = rb1 - rb0;                // >= 1
    const char* row = base + (size_t)2 * rb0 * g.pitch;
    const size_t step = (size_t)2 * g.pitch;  // one quad row = two raw rows
    // double-buffered chunks, as in k_frameLevels: every load is unconditional, rows past the band re-read its last row
    uint4 a[kRawChunk], b[kRawChunk];
#pragma unroll
    for (int c = 0; c < kRawChunk; c++) quad_rows_load<VEC>(row + (size_t)min(c, n - 1) * step, g.pitch, col, g.hw, a[c], b[c]);
    for (int t0 = 0; t0 < n; t0 += kRawChunk) {
        uint4 na[kRawChunk], nb[kRawChunk];
#pragma unroll
        for (int c = 0; c < kRawChunk; c++)
            quad_rows_load<VEC>(row + (size_t)min(t0 + kRawChunk + c, n - 1) * step, g.pitch, col, g.hw, na[c], nb[c]);
#pragma unroll
        for (int c = 0; c < kRawChunk; c++) {
            if (t0 + c >= n) break;
            const uint32_t wa[4] = {a[c].x, a[c].y, a[c].z, a[c].w}, wb[4] = {b[c].x, b[c].y, b[c].z, b[c].w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int v0 = (int)(wa[j] & 0xffffu), v1 = (int)(wa[j] >> 16), v2 = (int)(wb[j] & 0xffffu), v3 = (int)(wb[j] >> 16);
                const bool ok = m[j] && max(max(v0, v1), max(v2, v3)) < g.sat;  // a usable quad: all four samples below sat
                s[0] += ok ? (uint32_t)max(v0 - g.black[0], 0) : 0u;
                s[1] += ok ? (uint32_t)max(v1 - g.black[1], 0) : 0u;
                s[2] += ok ? (uint32_t)max(v2 - g.black[2], 0) : 0u;
                s[3] += ok ? (uint32_t)max(v3 - g.black[3], 0) : 0u;
                cnt += ok ? 1u : 0u;
            }
        }
#pragma unroll
        for (int c = 0; c < kRawChunk; c++) {
            a[c] = na[c];
            b[c] = nb[c];
        }
    }
    // the strip starts half a cell left of a grid point and 256 is a multiple of the cell: aligned groups of cell/4 lanes
    const int groupLanes = 1 << (g.k - 2);
    const int bi = (strip << (8 - g.k)) + (lane >> (g.k - 2));
    const int bj = (rb0 + half) >> g.k;
    const bool leader = (lane & (groupLanes - 1)) == 0 && bi < g.gw;  // (a box beyond the grid holds no column of the frame)
    const size_t at = (size_t)bj * g.gw + (size_t)min(bi, g.gw - 1);
#pragma unroll
    for (int q = 0; q < 5; q++) {
        const unsigned long long t = wave_group_sum<unsigned long long>(q < 4 ? s[q] : cnt, groupLanes);
        if (leader && t != 0) atomicAdd(q < 4 ? &sums[q * plane + at] : &counts[at], t);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// cell = 1 << k quads with 3 <= k <= 8: k, or -1
int shade_log2(int cell)
{
    for (int k = 3; k <= 8; k++)
        if (cell == (1 << k)) return k;
    return -1;
}

int shade_grid(int half, int cell) { return (half - 2 + cell) / cell + 1; }

bool shade_black_ok(const int32_t black[4])
{
    if (black == nullptr) return false;
    for (int q = 0; q < 4; q++)
        if (black[q] < 0 || black[q] > 65535) return false;
    return true;
}

}  // namespace

extern "C" int mfsr_applyShading(int nFrames, uint16_t* const* frames, int pitch, int width, int height, const int32_t* mapDev, int cell,
                                 const int32_t black[4], int maxValue, mfsr_stream_t stream)
{
    // host validation first: nothing below touches the device before every argument has passed
    MFSR_REQUIRE(raw_even_ok(width, height) && raw_frames_ok(nFrames, kRawMaxFrames, frames, pitch, width));
    const int k = shade_log2(cell);
    MFSR_REQUIRE(k >= 0 && mapDev != nullptr && ((uintptr_t)mapDev & 3) == 0);
    MFSR_REQUIRE(shade_black_ok(black) && 0 < maxValue && maxValue <= 65535);
    ShadeGeom g;
    g.pitch = pitch;
    g.width = width;
    g.height = height;
    g.lanesPerRow = 1 + (int)mfsr_cdiv(width, 8);
    g.blocksPerRow = (int)mfsr_cdiv(g.lanesPerRow, kShadeThreads);
    MFSR_REQUIRE((long long)g.blocksPerRow * height <= INT_MAX);
    g.k = k;
    g.gw = shade_grid(width / 2, cell);
    g.gh = shade_grid(height / 2, cell);
    for (int q = 0; q < 4; q++) g.black[q] = black[q];
    g.maxValue = maxValue;
    const RawFramesMut t = raw_table(nFrames, frames);
    const dim3 block(kShadeThreads), grid((unsigned)(g.blocksPerRow * height), (unsigned)nFrames);
    hipLaunchKernelGGL(k_applyShading, grid, block, 0, mfsr_s(stream), t, g, mapDev);
    return mfsr_launch_status("k_applyShading");
}

extern "C" int mfsr_shadingStats(int nFrames, const uint16_t* const* frames, int pitch, int width, int height, int cell,
                                 const int32_t black[4], int sat, long long* sumsDev, long long* countsDev, mfsr_stream_t stream)
{
    MFSR_REQUIRE(raw_even_ok(width, height) && raw_frames_ok(nFrames, kRawMaxFrames, frames, pitch, width));
    const int k = shade_log2(cell);
    MFSR_REQUIRE(k >= 0 && shade_black_ok(black) && 0 < sat && sat <= 65535);
    MFSR_REQUIRE(sumsDev != nullptr && ((uintptr_t)sumsDev & 7) == 0 && countsDev != nullptr && ((uintptr_t)countsDev & 7) == 0);
    const int hw = width / 2, hh = height / 2;
    const bool aligned16 = raw_aligned(nFrames, frames, pitch, 16) && hw % 4 == 0;
    const RawFrames t = raw_table(nFrames, frames);

    StatGeom g;
    g.pitch = pitch;
    g.hw = hw;
    g.hh = hh;
    g.k = k;
    g.gw = shade_grid(hw, cell);
    const int gh = shade_grid(hh, cell);
    g.bandRows = cell / 2 < kStatMaxBandRows ? cell / 2 : kStatMaxBandRows;  // divides half a cell: a band lies in one row of boxes
    g.nStrips = (int)mfsr_cdiv(hw + cell / 2, kStatStripCols);
    g.nBands = (int)mfsr_cdiv(hh, g.bandRows);
    MFSR_REQUIRE((long long)g.nStrips * g.nBands <= INT_MAX);
    for (int q = 0; q < 4; q++) g.black[q] = black[q];
    g.sat = sat;
    const size_t plane = (size_t)gh * g.gw;

    MFSR_HIP_TRY(hipMemsetAsync(sumsDev, 0, 4 * plane * sizeof(long long), mfsr_s(stream)));
    MFSR_HIP_TRY(hipMemsetAsync(countsDev, 0, plane * sizeof(long long), mfsr_s(stream)));
    const int threads = kStatWavesPerBlock * kRawLanes;
    const dim3 grid(mfsr_cdiv((long long)g.nStrips * g.nBands, kStatWavesPerBlock), (unsigned)nFrames), block(threads);
    if (aligned16)
        hipLaunchKernelGGL(k_shadingStats<true>, grid, block, 0, mfsr_s(stream), t, g, (unsigned long long*)sumsDev,
                           (unsigned long long*)countsDev, plane);
    else
        hipLaunchKernelGGL(k_shadingStats<false>, grid, block, 0, mfsr_s(stream), t, g, (unsigned long long*)sumsDev,
                           (unsigned long long*)countsDev, plane);
    return mfsr_launch_status("k_shadingStats");
}

extern "C" int mfsr_shading_fit(const long long* sums, const long long* counts, int gw, int gh, int minQuads, int maxGain,
                                int32_t* map, int32_t* status)
{
    MFSR_REQUIRE(sums != nullptr && counts != nullptr && map != nullptr && status != nullptr);
    MFSR_REQUIRE(gw >= 1 && gh >= 1 && (long long)gw * gh <= (1LL << 24));
    MFSR_REQUIRE(minQuads >= 1 && maxGain >= 65536 && maxGain <= 1048576);
    const size_t np = (size_t)gw * gh;
    for (size_t i = 0; i < 4 * np; i++) MFSR_REQUIRE(sums[i] >= 0 && sums[i] < (1LL << 48));  // (products < 2^114)
    for (size_t i = 0; i < np; i++) MFSR_REQUIRE(counts[i] >= 0 && counts[i] < (1LL << 48));
    typedef unsigned __int128 u128;
    for (size_t i = 0; i < 4 * np; i++) map[i] = 65536;
    bool measurable = true;
    for (size_t p = 0; p < np; p++) {
        measurable = measurable && counts[p] >= (long long)minQuads;
        for (int q = 0; q < 4; q++) measurable = measurable && sums[q * np + p] != 0;
    }
    if (!measurable) {
        *status = 2;
        return MFSR_OK;
    }
    // the anchor: the largest mean level T / C, compared as T[p] * C[a] > T[a] * C[p]; ties go to the lowest index
    auto total = [&](size_t p) { return (u128)sums[p] + (u128)sums[np + p] + (u128)sums[2 * np + p] + (u128)sums[3 * np + p]; };
    size_t a = 0;
    for (size_t p = 1; p < np; p++)
        if (total(p) * (u128)counts[a] > total(a) * (u128)counts[p]) a = p;
    bool clamped = false;
    for (int q = 0; q < 4; q++)
        for (size_t p = 0; p < np; p++) {
            const u128 den = (u128)sums[q * np + p] * (u128)counts[a];
            u128 v = ((u128)sums[q * np + a] * (u128)counts[p] * 65536u + den / 2) / den;
            if (v > (u128)maxGain) {
                v = (u128)maxGain;
                clamped = true;
            }
            map[q * np + p] = v < 65536u ? 65536 : (int32_t)v;
        }
    *status = clamped ? 3 : 0;
    return MFSR_OK;
}
