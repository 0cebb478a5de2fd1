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
#include "raw_stage.hpp"

namespace {

constexpr int kSelStripCols = 4 * (kRawLanes - 2);  // output columns of one wave's strip
constexpr int kSelMinBandRows = 8;                  // output rows of one wave's band: at least this many
constexpr int kSelWavesPerBlock = 4;

struct SelGeom {
    int pitch;               // bytes
    int hw;                  // half-resolution width
    int x0, y0, x1, y1;      // half-resolution rectangle (S < 2^62 within kRawMaxArea: each term < 2^39)
    int cs0;                 // first G column of strip 0 (a multiple of 4; lane 0 of strip 0 may lie left of the frame)
    int bandRows;            // output rows of one wave's band
    int nStrips, nBands;
    int ay, sa, by, sb;      // raw row (0/1) and bit shift (0/16, the column within the quad) of the two green samples
};

// VEC: every frame pointer and the pitch are 16-byte aligned and hw % 4 == 0 (16-byte loads); otherwise 16-bit loads
template <bool VEC>
__global__ __launch_bounds__(kSelWavesPerBlock * kRawLanes) void k_frameSharpness(RawFrames frames, SelGeom g, long long* sums)
{
    const int lane = threadIdx.x & (kRawLanes - 1);
    const int wave = blockIdx.x * kSelWavesPerBlock + (threadIdx.x >> 6);
    if (wave >= g.nStrips * g.nBands) return;  // (whole waves)
    const int strip = wave % g.nStrips, band = wave / g.nStrips;
    const int col = g.cs0 + strip * kSelStripCols + 4 * lane;
    const int rb0 = g.y0 + band * g.bandRows;
    const int rb1 = min(rb0 + g.bandRows, g.y1);
    const char* base = (const char*)frames.p[blockIdx.y];

    bool m[4];  // this lane's column j is an output column (only halo lanes hold columns outside the frame)
#pragma unroll
    for (int j = 0; j < 4; j++) m[j] = lane >= 1 && lane <= kRawLanes - 2 && col + j >= g.x0 && col + j < g.x1;

    // horizontal Sobel terms of the rows above (m) and at (c) the next output row: D = G(j+1) - G(j-1), H = G(j-1) + 2G(j) + G(j+1)
    int Dm[4] = {0, 0, 0, 0}, Hm[4] = {0, 0, 0, 0}, Dc[4] = {0, 0, 0, 0}, Hc[4] = {0, 0, 0, 0};
    long long acc = 0;
    const int n = rb1 - rb0 + 2;  // G rows rb0-1 .. rb1 (inside [0, hh): 1 <= y0, y1 <= hh - 1)
    const char* row = base + (size_t)2 * (rb0 - 1) * g.pitch;
    const size_t step = (size_t)2 * g.pitch;  // one G row = two raw rows
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
            int G[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                G[j] = (int)(((g.ay ? wb[j] : wa[j]) >> g.sa) & 0xffffu) + (int)(((g.by ? wb[j] : wa[j]) >> g.sb) & 0xffffu);
            const int left = wave_shr1(G[3]), right = wave_shl1(G[0]);
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
        for (int k = 0; k < kRawChunk; k++) {
            a[k] = na[k];
            b[k] = nb[k];
        }
    }
    acc = wave_sum(acc);
    if (lane == 0 && acc != 0) atomicAdd((unsigned long long*)&sums[blockIdx.y], (unsigned long long)acc);
}

}  // namespace

extern "C" int mfsr_frameSharpness(int nFrames, const uint16_t* const* frames, int pitch, int width, int height, const int32_t cfa[4],
                                   int mono, const int32_t rect[4], long long* sumsDev, mfsr_stream_t stream)
{
    // host validation first: nothing below touches the device before every argument has passed
    MFSR_REQUIRE(raw_even_ok(width, height) && raw_frames_ok(nFrames, INT_MAX, frames, pitch, width) && sumsDev != nullptr);
    const bool aligned16 = raw_aligned(nFrames, frames, pitch, 16) && (width / 2) % 4 == 0;
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
    MFSR_REQUIRE(raw_half_rect_ok(rect, width, height));
    const int hw = width / 2;
    const int x0 = rect[0], y0 = rect[1], x1 = rect[2], y1 = rect[3];

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
    const int threads = kSelWavesPerBlock * kRawLanes;
    const int resident = aligned16 ? resident_blocks<k_frameSharpness<true>>(threads) : resident_blocks<k_frameSharpness<false>>(threads);
    for (int f0 = 0; f0 < nFrames; f0 += kRawMaxFrames) {
        const int nf = nFrames - f0 < kRawMaxFrames ? nFrames - f0 : kRawMaxFrames;
        const RawFrames t = raw_table(nf, frames + f0);
        // at least kSelMinBandRows rows to a band: the two halo rows are the re-read
        const RawBands bands = plan_bands(y1 - y0, g.nStrips, nf, resident, kSelWavesPerBlock, kSelMinBandRows, INT_MAX);
        g.bandRows = bands.rows;
        g.nBands = bands.n;
        const unsigned blocks = mfsr_cdiv((long long)g.nStrips * g.nBands, kSelWavesPerBlock);
        const dim3 grid(blocks, (unsigned)nf), block(threads);
        if (aligned16)
            hipLaunchKernelGGL(k_frameSharpness<true>, grid, block, 0, mfsr_s(stream), t, g, sumsDev + f0);
        else
            hipLaunchKernelGGL(k_frameSharpness<false>, grid, block, 0, mfsr_s(stream), t, g, sumsDev + f0);
        const int rc = mfsr_launch_status("k_frameSharpness");
        if (rc != MFSR_OK) return rc;
    }
    return MFSR_OK;
}
