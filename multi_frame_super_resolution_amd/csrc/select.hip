// select.hip -- sharpness score of raw frames, the input of a burst's reference / frame selection.
//
// S = sum over a half-resolution rectangle of gx^2 + gy^2, the 3x3 Sobel gradients of the integer green plane
// G(i, j) = raw(2i+ay, 2j+ax) + raw(2i+by, 2j+bx) (the two green quad positions of the CFA; mono: (0,1) and (1,0)).
// Everything is integer arithmetic: the sum is exact, independent of the reduction order and of the launch shape.
//
// Shape (k_frameSharpness): one wavefront owns a strip of 4 * 64 half-resolution columns and a band of rows of one frame, as
// short as keeps the whole launch within one round of resident workgroups (no tail) and at least 8 rows.  Lane l loads the
// quad row pair of its 4 columns (two 16-byte loads per half-resolution row; the next 4 rows are in flight while 4 are
// reduced), the wave walks down the band with the horizontal Sobel terms of three rows in registers; the column left / right
// of a lane's four come from its neighbours through whole-wave DPP shifts, so lanes 0 and 63 are halo lanes and a strip
// yields 4 * 62 output columns.  Re-reads: the two halo lanes of a strip and the two halo rows of a band.  Per-lane sums in
// 64-bit integers, one 64-bit integer atomic add per wave into the frame's slot.  No LDS.
#include "common.hpp"

namespace {

constexpr int kSelMaxFrames = 64;                    // frame pointers in one launch's argument table
constexpr int kSelLanes = 64;
constexpr int kSelStripCols = 4 * (kSelLanes - 2);  // output columns of one wave's strip
constexpr int kSelMinBandRows = 8;                  // output rows of one wave's band: at least this many
constexpr int kSelChunk = 4;                        // rows loaded per step (two steps in flight)
constexpr int kSelWavesPerBlock = 4;
constexpr long long kSelMaxArea = 1LL << 23;        // S < 2^62 below this area (each term < 2^39)

struct SelFrames {
    const uint16_t* p[kSelMaxFrames];
};

struct SelGeom {
    int pitch;               // bytes
    int hw;                  // half-resolution width
    int x0, y0, x1, y1;      // half-resolution rectangle
    int cs0;                 // first G column of strip 0 (a multiple of 4; lane 0 of strip 0 may lie left of the frame)
    int bandRows;            // output rows of one wave's band
    int nStrips, nBands;
    int ay, sa, by, sb;      // raw row (0/1) and bit shift (0/16, the column within the quad) of the two green samples
};

__device__ __forceinline__ int sel_wshr1(int v)  // lane l <- lane l-1 (lane 0 <- 0)
{
    return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, true);
}
__device__ __forceinline__ int sel_wshl1(int v)  // lane l <- lane l+1 (lane 63 <- 0)
{
    return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, true);
}

// quad rows 2r (a) and 2r+1 (b) of half-resolution columns col .. col+3: one 32-bit word per column, x = 0 in the low half.
// Branch-free, so that the loads of a chunk issue back to back and the wait before a row's use counts only older loads: a
// column outside the frame reads a clamped in-frame address instead (only halo lanes hold such columns, and no output
// depends on them).  VEC: one 16-byte load per row at col clamped to [0, hw - 4] -- exact for every column a lane needs when
// hw % 4 == 0 (col is a multiple of 4, so a lane lies entirely inside or entirely outside the frame).
template <bool VEC>
__device__ __forceinline__ void sel_load(const char* rowA, int pitch, int col, int hw, uint4& a, uint4& b)
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

// VEC: every frame pointer and the pitch are 16-byte aligned and hw % 4 == 0 (16-byte loads); otherwise 16-bit loads
template <bool VEC>
__global__ __launch_bounds__(kSelWavesPerBlock * kSelLanes) void k_frameSharpness(SelFrames frames, SelGeom g, long long* sums)
{
    const int lane = threadIdx.x & (kSelLanes - 1);
    const int wave = blockIdx.x * kSelWavesPerBlock + (threadIdx.x >> 6);
    if (wave >= g.nStrips * g.nBands) return;  // (whole waves)
    const int strip = wave % g.nStrips, band = wave / g.nStrips;
    const int col = g.cs0 + strip * kSelStripCols + 4 * lane;
    const int rb0 = g.y0 + band * g.bandRows;
    const int rb1 = min(rb0 + g.bandRows, g.y1);
    const char* base = (const char*)frames.p[blockIdx.y];

    bool m[4];  // this lane's column j is an output column
#pragma unroll
    for (int j = 0; j < 4; j++) m[j] = lane >= 1 && lane <= kSelLanes - 2 && col + j >= g.x0 && col + j < g.x1;

    // horizontal Sobel terms of the rows above (m) and at (c) the next output row: D = G(j+1) - G(j-1), H = G(j-1) + 2G(j) + G(j+1)
    int Dm[4] = {0, 0, 0, 0}, Hm[4] = {0, 0, 0, 0}, Dc[4] = {0, 0, 0, 0}, Hc[4] = {0, 0, 0, 0};
    long long acc = 0;
    const int n = rb1 - rb0 + 2;  // G rows rb0-1 .. rb1 (inside [0, hh): 1 <= y0, y1 <= hh - 1)
    const char* row = base + (size_t)2 * (rb0 - 1) * g.pitch;
    const size_t step = (size_t)2 * g.pitch;  // one G row = two raw rows
    // double-buffered chunks: the loads of chunk c+1 are in flight while chunk c is reduced (rows past the band re-read its
    // last row: every load is unconditional)
    uint4 a[kSelChunk], b[kSelChunk];
#pragma unroll
    for (int k = 0; k < kSelChunk; k++) sel_load<VEC>(row + (size_t)min(k, n - 1) * step, g.pitch, col, g.hw, a[k], b[k]);
    for (int t0 = 0; t0 < n; t0 += kSelChunk) {
        uint4 na[kSelChunk], nb[kSelChunk];
#pragma unroll
        for (int k = 0; k < kSelChunk; k++)
            sel_load<VEC>(row + (size_t)min(t0 + kSelChunk + k, n - 1) * step, g.pitch, col, g.hw, na[k], nb[k]);
#pragma unroll
        for (int k = 0; k < kSelChunk; k++) {
            if (t0 + k >= n) break;
            const uint32_t wa[4] = {a[k].x, a[k].y, a[k].z, a[k].w}, wb[4] = {b[k].x, b[k].y, b[k].z, b[k].w};
            int G[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                G[j] = (int)(((g.ay ? wb[j] : wa[j]) >> g.sa) & 0xffffu) + (int)(((g.by ? wb[j] : wa[j]) >> g.sb) & 0xffffu);
            const int left = sel_wshr1(G[3]), right = sel_wshl1(G[0]);
            const int Dn[4] = {G[1] - left, G[2] - G[0], G[3] - G[1], right - G[2]};
            const int Hn[4] = {left + 2 * G[0] + G[1], G[0] + 2 * G[1] + G[2], G[1] + 2 * G[2] + G[3], G[2] + 2 * G[3] + right};
            if (t0 + k >= 2) {  // output row rb0 - 1 + t0 + k - 1
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int gx = Dm[j] + 2 * Dc[j] + Dn[j], gy = Hn[j] - Hm[j];  // |gx|, |gy| <= 4 * 131070 < 2^20
                    if (m[j]) acc += (long long)gx * gx + (long long)gy * gy;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                Dm[j] = Dc[j];
                Hm[j] = Hc[j];
                Dc[j] = Dn[j];
                Hc[j] = Hn[j];
            }
        }
#pragma unroll
        for (int k = 0; k < kSelChunk; k++) {
            a[k] = na[k];
            b[k] = nb[k];
        }
    }
#pragma unroll
    for (int o = kSelLanes / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0 && acc != 0) atomicAdd((unsigned long long*)&sums[blockIdx.y], (unsigned long long)acc);
}

// workgroups of k_frameSharpness the current device holds at once (CUs x occupancy), cached per device
int sel_resident_blocks(bool vec)
{
    constexpr int kDevs = 64;
    static int cache[2][kDevs];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kDevs) dev = -1;
    if (dev >= 0 && cache[vec][dev] > 0) return cache[vec][dev];
    int cus = 0, perCU = 0;
    if (dev < 0 || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const hipError_t e = vec ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, k_frameSharpness<true>, kSelWavesPerBlock * kSelLanes, 0)
                             : hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, k_frameSharpness<false>, kSelWavesPerBlock * kSelLanes, 0);
    if (e != hipSuccess || perCU <= 0) perCU = 4;
    const int r = cus * perCU;
    if (dev >= 0) cache[vec][dev] = r;
    return r;
}

}  // namespace

extern "C" int mfsr_frameSharpness(int nFrames, const uint16_t* const* frames, int pitch, int width, int height, const int32_t cfa[4],
                                   int mono, const int32_t rect[4], long long* sumsDev, mfsr_stream_t stream)
{
    // host validation first: nothing below touches the device before every argument has passed
    MFSR_REQUIRE(nFrames >= 1 && frames != nullptr && rect != nullptr && sumsDev != nullptr);
    MFSR_REQUIRE(width > 0 && height > 0 && (width % 2) == 0 && (height % 2) == 0);
    MFSR_REQUIRE((long long)pitch >= 2LL * width && (pitch % 2) == 0);
    bool aligned16 = (pitch % 16) == 0 && (width / 2) % 4 == 0;
    for (int k = 0; k < nFrames; k++) {
        MFSR_REQUIRE(frames[k] != nullptr && ((uintptr_t)frames[k] & 1) == 0);
        aligned16 = aligned16 && ((uintptr_t)frames[k] & 15) == 0;
    }
    int gy[2] = {0, 1}, gxp[2] = {1, 0};  // mono: (0,1) and (1,0)
    if (!mono) {
        MFSR_REQUIRE(cfa != nullptr);
        int n = 0;
        for (int i = 0; i < 4; i++)
            if (cfa[i] == MFSR_GREEN) {
                if (n < 2) {
                    gy[n] = i >> 1;
                    gxp[n] = i & 1;
                }
                n++;
            }
        MFSR_REQUIRE(n == 2);
    }
    const int hw = width / 2, hh = height / 2;
    const int x0 = rect[0], y0 = rect[1], x1 = rect[2], y1 = rect[3];
    MFSR_REQUIRE(x0 >= 1 && x0 < x1 && x1 <= hw - 1 && y0 >= 1 && y0 < y1 && y1 <= hh - 1);
    MFSR_REQUIRE((long long)(x1 - x0) * (y1 - y0) <= kSelMaxArea);

    SelGeom g;
    g.pitch = pitch;
    g.hw = hw;
    g.x0 = x0;
    g.y0 = y0;
    g.x1 = x1;
    g.y1 = y1;
    g.cs0 = (x0 & ~3) - 4;
    g.nStrips = (int)mfsr_cdiv(x1 - (g.cs0 + 4), kSelStripCols);
    g.ay = gy[0];
    g.sa = 16 * gxp[0];
    g.by = gy[1];
    g.sb = 16 * gxp[1];

    MFSR_HIP_TRY(hipMemsetAsync(sumsDev, 0, sizeof(long long) * (size_t)nFrames, mfsr_s(stream)));
    const int resident = sel_resident_blocks(aligned16);
    for (int f0 = 0; f0 < nFrames; f0 += kSelMaxFrames) {
        const int nf = nFrames - f0 < kSelMaxFrames ? nFrames - f0 : kSelMaxFrames;
        SelFrames t = {};
        for (int k = 0; k < nf; k++) t.p[k] = frames[f0 + k];
        // bands as short as keeps the launch within one round of resident workgroups (every wave then streams from the
        // start to the end of the launch, no tail), at least kSelMinBandRows rows (the two halo rows are the re-read)
        const int rows = y1 - y0;
        const int wavesPerFrame = kSelWavesPerBlock * (resident / nf > 1 ? resident / nf : 1);
        const int bands = wavesPerFrame / g.nStrips > 1 ? wavesPerFrame / g.nStrips : 1;
        g.bandRows = (int)mfsr_cdiv(rows, bands);
        g.bandRows = g.bandRows < kSelMinBandRows ? kSelMinBandRows : g.bandRows;
        g.nBands = (int)mfsr_cdiv(rows, g.bandRows);
        const unsigned blocks = mfsr_cdiv((long long)g.nStrips * g.nBands, kSelWavesPerBlock);
        const dim3 grid(blocks, (unsigned)nf), block(kSelWavesPerBlock * kSelLanes);
        if (aligned16)
            hipLaunchKernelGGL(k_frameSharpness<true>, grid, block, 0, mfsr_s(stream), t, g, sumsDev + f0);
        else
            hipLaunchKernelGGL(k_frameSharpness<false>, grid, block, 0, mfsr_s(stream), t, g, sumsDev + f0);
        const int rc = mfsr_launch_status("k_frameSharpness");
        if (rc != MFSR_OK) return rc;
    }
    return MFSR_OK;
}
