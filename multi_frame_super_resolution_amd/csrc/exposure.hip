// exposure.hip -- exposure matching of raw frames: per-frame level sums, and a per-colour gain applied in place.
//
// The rule is stated in include/mfsr.h (mfsr_frameLevels / mfsr_exposure_gains / mfsr_applyGains): exact integer arithmetic,
// the results equal the numpy restatement of the tests bit for bit, for any launch shape.
//
// Shape (k_frameLevels): one wavefront owns a strip of 4 * 64 half-resolution columns and a band of quad rows of one frame, as
// short as keeps the whole launch within one round of resident workgroups (no tail).  Lane l loads the quad row pair of its 4
// columns (two 16-byte loads per quad row; the next 4 rows are in flight while 4 are reduced).  Per-lane partial sums in 32-bit
// integers (a band is short enough for them), widened for the whole-wave reduction, then one 64-bit integer atomic add per
// wave and quantity into the frame's five slots.  No LDS, no floating point.
//
// k_applyGains: one lane per 16-byte aligned piece of a row (8 samples: one load, one store); the pieces a row's ends cut, and
// the samples before the first aligned address, go sample by sample.  Only the status-0 frames are in the launch's table.
#include "raw_stage.hpp"

namespace {

constexpr int kLevStripCols = 4 * kRawLanes;      // half-resolution columns of one wave's strip
constexpr int kLevMinBandRows = 8;                // quad rows of one wave's band: at least this many,
constexpr int kLevMaxBandRows = 8192;             // at most this many: 4 * 8192 * 65535 < 2^32 per lane and quantity
constexpr int kLevWavesPerBlock = 4;

struct LevGeom {
    int pitch;           // bytes
    int hw;              // half-resolution width
    int x0, y0, x1, y1;  // half-resolution rectangle (within kRawMaxArea: S < 2^39, C <= 2^23)
    int cs0;             // first column of strip 0 (a multiple of 4, <= x0)
    int bandRows;
    int nStrips, nBands;
    int black[4];
    int sat;
};

// VEC: every frame pointer and the pitch are 16-byte aligned and hw % 4 == 0 (16-byte loads); otherwise 16-bit loads
template <bool VEC>
__global__ __launch_bounds__(kLevWavesPerBlock * kRawLanes) void k_frameLevels(RawFrames frames, LevGeom g, unsigned long long* levels)
{
    const int lane = threadIdx.x & (kRawLanes - 1);
    const int wave = blockIdx.x * kLevWavesPerBlock + (threadIdx.x >> 6);
    if (wave >= g.nStrips * g.nBands) return;  // (whole waves)
    const int strip = wave % g.nStrips, band = wave / g.nStrips;
    const int col = g.cs0 + strip * kLevStripCols + 4 * lane;
    const int rb0 = g.y0 + band * g.bandRows;
    const int rb1 = min(rb0 + g.bandRows, g.y1);
    const char* base = (const char*)frames.p[blockIdx.y];

    bool m[4];  // this lane's column j lies in the rectangle
#pragma unroll
    for (int j = 0; j < 4; j++) m[j] = col + j >= g.x0 && col + j < g.x1;

    uint32_t s[4] = {0, 0, 0, 0}, cnt = 0;
    const int n = rb1 - rb0;  // >= 1
    const char* row = base + (size_t)2 * rb0 * g.pitch;
    const size_t step = (size_t)2 * g.pitch;  // one quad row = two raw rows
    // double-buffered chunks: the loads of chunk c+1 are in flight while chunk c is reduced (rows past the band re-read its
    // last row: every load is unconditional)
    uint4 a[kRawChunk], b[kRawChunk];
#pragma unroll
    for (int k = 0; k < kRawChunk; k++) quad_rows_load<VEC>(row + (size_t)min(k, n - 1) * step, g.pitch, col, g.hw, a[k], b[k]);
    for (int t0 = 0; t0 < n; t0 += kRawChunk) {
        uint4 na[kRawChunk], nb[kRawChunk];
#pragma unroll
        for (int k = 0; k < kRawChunk; k++)
            quad_rows_load<VEC>(row + (size_t)min(t0 + kRawChunk + k, n - 1) * step, g.pitch, col, g.hw, na[k], nb[k]);
#pragma unroll
        for (int k = 0; k < kRawChunk; k++) {
            if (t0 + k >= n) break;
            const uint32_t wa[4] = {a[k].x, a[k].y, a[k].z, a[k].w}, wb[4] = {b[k].x, b[k].y, b[k].z, b[k].w};
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
        for (int k = 0; k < kRawChunk; k++) {
            a[k] = na[k];
            b[k] = nb[k];
        }
    }
    unsigned long long* out = levels + 5 * (size_t)blockIdx.y;
#pragma unroll
    for (int q = 0; q < 5; q++) {
        const unsigned long long t = wave_sum<unsigned long long>(q < 4 ? s[q] : cnt);
        if (lane == 0 && t != 0) atomicAdd(&out[q], t);
    }
}

// ---- apply ----------------------------------------------------------------------------------------------------------------
struct GainFrames : RawFramesMut {
    int gain[kRawMaxFrames][4];  // Q16 gain of quad position q
};

struct GainGeom {
    int pitch, width, height;
    int lanesPerRow;  // 1 (the samples before the first 16-byte boundary) + the 8-sample pieces after it
    int black[4];
    int sat, maxValue;
};

__global__ __launch_bounds__(256) void k_applyGains(GainFrames frames, GainGeom g)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)g.lanesPerRow * g.height) return;
    const int y = (int)(idx / g.lanesPerRow), c = (int)(idx % g.lanesPerRow);
    char* row = (char*)frames.p[blockIdx.y] + (size_t)y * (size_t)g.pitch;
    const int head = (int)((16 - ((uintptr_t)row & 15)) & 15) >> 1;  // samples before the row's first 16-byte boundary (0 .. 7)
    const int xa = c == 0 ? 0 : head + 8 * (c - 1);
    const int xb = min(c == 0 ? head : xa + 8, g.width);
    if (xa >= xb) return;
    const int q0 = 2 * (y & 1);
    const int* gq = frames.gain[blockIdx.y];
    if (xb - xa == 8) {  // (c >= 1: 16-byte aligned)
        uint4* p = (uint4*)(row + 2 * (size_t)xa);
        const uint4 v = *p;
        const int qe = q0 + (xa & 1), qo = q0 + ((xa & 1) ^ 1);  // quad positions of the low / high half of a word
        const int be = g.black[qe], bo = g.black[qo], ge = gq[qe], go = gq[qo];
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++)
            w[j] = gain_sample(w[j] & 0xffffu, be, ge, g.sat, g.maxValue) | (gain_sample(w[j] >> 16, bo, go, g.sat, g.maxValue) << 16);
        *p = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    uint16_t* p = (uint16_t*)row;
    for (int x = xa; x < xb; x++) {
        const int q = q0 + (x & 1);
        p[x] = (uint16_t)gain_sample(p[x], g.black[q], gq[q], g.sat, g.maxValue);
    }
}

bool exp_levels_ok(const int32_t black[4], int sat, int maxValue)
{
    if (black == nullptr) return false;
    for (int q = 0; q < 4; q++)
        if (black[q] < 0 || black[q] > 65535) return false;
    return 0 < sat && sat <= maxValue && maxValue <= 65535;
}

// colour class of quad position q: cfa[q] (red, green or blue), one class for mono
bool exp_classes(const int32_t cfa[4], int mono, int cls[4])
{
    for (int q = 0; q < 4; q++) {
        if (mono)
            cls[q] = 0;
        else {
            if (cfa == nullptr || cfa[q] < MFSR_RED || cfa[q] > MFSR_BLUE) return false;
            cls[q] = cfa[q];
        }
    }
    return true;
}

}  // namespace

extern "C" int mfsr_frameLevels(int nFrames, const uint16_t* const* frames, int pitch, int width, int height, const int32_t black[4],
                                int sat, const int32_t rect[4], long long* levelsDev, mfsr_stream_t stream)
{
    // host validation first: nothing below touches the device before every argument has passed
    MFSR_REQUIRE(raw_even_ok(width, height) && raw_frames_ok(nFrames, kRawMaxFrames, frames, pitch, width));
    MFSR_REQUIRE(exp_levels_ok(black, sat, 65535));
    MFSR_REQUIRE(raw_half_rect_ok(rect, width, height) && levelsDev != nullptr && ((uintptr_t)levelsDev & 7) == 0);
    const int hw = width / 2;
    const int x0 = rect[0], y0 = rect[1], x1 = rect[2], y1 = rect[3];
    const bool aligned16 = raw_aligned(nFrames, frames, pitch, 16) && hw % 4 == 0;
    const RawFrames t = raw_table(nFrames, frames);

    LevGeom g;
    g.pitch = pitch;
    g.hw = hw;
    g.x0 = x0;
    g.y0 = y0;
    g.x1 = x1;
    g.y1 = y1;
    g.cs0 = x0 & ~3;
    g.nStrips = (int)mfsr_cdiv(x1 - g.cs0, kLevStripCols);
    for (int q = 0; q < 4; q++) g.black[q] = black[q];
    g.sat = sat;
    const int threads = kLevWavesPerBlock * kRawLanes;
    const int resident = aligned16 ? resident_blocks<k_frameLevels<true>>(threads) : resident_blocks<k_frameLevels<false>>(threads);
    const RawBands bands = plan_bands(y1 - y0, g.nStrips, nFrames, resident, kLevWavesPerBlock, kLevMinBandRows, kLevMaxBandRows);
    g.bandRows = bands.rows;
    g.nBands = bands.n;

    MFSR_HIP_TRY(hipMemsetAsync(levelsDev, 0, 5 * sizeof(long long) * (size_t)nFrames, mfsr_s(stream)));
    const unsigned blocks = mfsr_cdiv((long long)g.nStrips * g.nBands, kLevWavesPerBlock);
    const dim3 grid(blocks, (unsigned)nFrames), block(threads);
    if (aligned16)
        hipLaunchKernelGGL(k_frameLevels<true>, grid, block, 0, mfsr_s(stream), t, g, (unsigned long long*)levelsDev);
    else
        hipLaunchKernelGGL(k_frameLevels<false>, grid, block, 0, mfsr_s(stream), t, g, (unsigned long long*)levelsDev);
    return mfsr_launch_status("k_frameLevels");
}

extern "C" int mfsr_exposure_gains(int n, const long long* levels, int reference, const int32_t cfa[4], int mono, int perColour,
                                   int deadband, int minGain, int maxGain, int32_t* gains, int32_t* status)
{
    MFSR_REQUIRE(n >= 1 && levels != nullptr && gains != nullptr && status != nullptr);
    MFSR_REQUIRE(reference >= 0 && reference < n);
    MFSR_REQUIRE(exposure_bounds_ok(deadband, minGain, maxGain));
    int cls[4];
    MFSR_REQUIRE(exp_classes(cfa, mono, cls));
    for (long long i = 0; i < 5LL * n; i++) MFSR_REQUIRE(levels[i] >= 0 && levels[i] < (1LL << 48));  // (products < 2^99)
    const bool split = perColour != 0 && !mono;
    typedef unsigned __int128 u128;
    // T[c] of frame k: the sums of the positions of class c (common mode: one class, all four positions, copied to all three)
    auto totals = [&](int k, unsigned long long T[3], bool used[3]) {
        for (int c = 0; c < 3; c++) {
            T[c] = 0;
            used[c] = false;
        }
        for (int q = 0; q < 4; q++) {
            const int c = split ? cls[q] : 0;
            T[c] += (unsigned long long)levels[5 * (size_t)k + q];
            used[c] = true;
        }
        if (!split) {
            T[1] = T[2] = T[0];
            used[1] = used[2] = true;
        }
    };
    unsigned long long Tr[3];
    bool used[3];
    totals(reference, Tr, used);
    const unsigned long long Cr = (unsigned long long)levels[5 * (size_t)reference + 4];
    for (int k = 0; k < n; k++) {
        int32_t* gk = gains + 3 * (size_t)k;
        gk[0] = gk[1] = gk[2] = 65536;
        if (k == reference) {
            status[k] = 1;
            continue;
        }
        unsigned long long Tk[3];
        bool u[3];
        totals(k, Tk, u);
        const unsigned long long Ck = (unsigned long long)levels[5 * (size_t)k + 4];
        bool measurable = Ck != 0 && Cr != 0;
        for (int c = 0; c < 3; c++)
            if (used[c] && (Tk[c] == 0 || Tr[c] == 0)) measurable = false;
        if (!measurable) {
            status[k] = 2;
            continue;
        }
        int32_t gq[3] = {65536, 65536, 65536};
        bool inBand = true, inRange = true;
        for (int c = 0; c < 3; c++) {
            if (!used[c]) continue;  // a colour the CFA does not have: 65536, takes no part
            const u128 den = (u128)Tk[c] * Cr;
            const u128 v = ((u128)Tr[c] * Ck * 65536u + den / 2) / den;
            gq[c] = v > (u128)INT32_MAX ? INT32_MAX : (int32_t)v;
            const long long off = (long long)gq[c] - 65536;
            inBand = inBand && off >= -(long long)deadband && off <= (long long)deadband;
            inRange = inRange && gq[c] >= minGain && gq[c] <= maxGain;
        }
        if (inBand) {
            status[k] = 1;
            continue;
        }
        for (int c = 0; c < 3; c++) gk[c] = gq[c];
        status[k] = inRange ? 0 : 3;
    }
    return MFSR_OK;
}

extern "C" int mfsr_applyGains(int nFrames, uint16_t* const* frames, int pitch, int width, int height, const int32_t cfa[4], int mono,
                               const int32_t black[4], int sat, int maxValue, const int32_t* gains, const int32_t* status,
                               mfsr_stream_t stream)
{
    MFSR_REQUIRE(raw_even_ok(width, height) && raw_frames_ok(nFrames, kRawMaxFrames, frames, pitch, width));
    MFSR_REQUIRE(exp_levels_ok(black, sat, maxValue));
    MFSR_REQUIRE(gains != nullptr && status != nullptr);
    int cls[4];
    MFSR_REQUIRE(exp_classes(cfa, mono, cls));
    GainFrames t = {};
    int nf = 0;
    for (int k = 0; k < nFrames; k++) {
        MFSR_REQUIRE(status[k] >= 0 && status[k] <= 3);
        if (status[k] != 0) continue;  // never written: not in the launch's table at all
        for (int q = 0; q < 4; q++) {
            const int32_t gq = gains[3 * (size_t)k + cls[q]];
            MFSR_REQUIRE(gq >= 4096 && gq <= 1048576);
            t.gain[nf][q] = gq;
        }
        t.p[nf++] = frames[k];
    }
    if (nf == 0) return MFSR_OK;
    GainGeom g;
    g.pitch = pitch;
    g.width = width;
    g.height = height;
    g.lanesPerRow = 1 + (int)mfsr_cdiv(width, 8);
    for (int q = 0; q < 4; q++) g.black[q] = black[q];
    g.sat = sat;
    g.maxValue = maxValue;
    const dim3 block(256), grid(mfsr_cdiv((long long)g.lanesPerRow * height, 256), (unsigned)nf);
    hipLaunchKernelGGL(k_applyGains, grid, block, 0, mfsr_s(stream), t, g);
    return mfsr_launch_status("k_applyGains");
}
