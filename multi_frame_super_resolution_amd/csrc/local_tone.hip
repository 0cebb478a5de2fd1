// local_tone.hip -- local tone mapping in the finish: a bilateral grid of gains over (x, y, luma) of the
// FULL frame.  Three stages: exact integer statistics of the merged image per grid entry (k_toneGridStats, the device), the fit
// of the gains (mfsr_local_tone_fit, the host, doubles), and the slice: a trilinear lookup of the gain per pixel, folded into the
// rendered finish (k_localToneImage, k_finishLocalTone).  The rule is stated in include/mfsr.h.  The statistics are integers and
// the slice is float32 + - * with -ffp-contract=off (the Makefile) in the order written, so both equal the numpy restatement of
// the tests (tests/local_tone_ref.py) word for word and bit for bit, for any launch shape; stripes and windows of an image add up
// to the whole image's table, and a stripe or a window of the slice is the crop of the whole.  gfx950, wave64.
//
// k_toneGridStats (the structure of k_imageStats): a read-only stream of 12 B or 24 B per pixel.  The work is cut on the grid of
// the full frame: an item is a block of R rows inside one row of cells (R a power of two <= C) times a chunk of K = 4096 / NZ
// cells, so its count and sum per (cell, bin) fit 2 x 4096 32-bit LDS counters (32 KiB; at most C x C pixels of codes <= 4095 per
// entry: C^2 4095 < 2^32).  Persistent 1024-lane workgroups walk the items.  A lane owns four consecutive pixels and merges
// those that fall on one entry; the lanes of a wave then merge runs of neighbours on one entry with a prefix sum over the wave
// (twelve shuffles), and only the last lane of a run touches LDS: a flat image costs a wave one add per cell it covers, where
// one add per pixel would put sixteen or more lanes on one address.  A lane whose four pixels straddle entries adds its own.
// After an item the workgroup sweeps its counters once: 64-bit vector atomic adds of the non-zero entries.
//
// The slice reads eight gains per pixel: four (y, x) corners times an adjacent pair along luma.  Two forms (MFSR_LOCAL_TONE_GRID =
// lds | cache, as MFSR_RENDER_LUT): the workgroup stages the few corner columns its tile touches as (g[k], g[k + 1]) pairs in
// LDS, so that a corner is one aligned 8-byte read whatever the parity of k; or every lane reads the grid through the cache.
// The lookup itself (slice_gain, with SliceArgs and the staged Tile it reads) is finish_stages.hpp's, which the finish chain
// (finish_chain.hip) calls in the through-the-cache form.
#include <thread>
#include <vector>

#include "finish_stages.hpp"
#include "stats_common.hpp"

namespace {

constexpr int kGridEntries = 4096;             // (cell, bin) entries of one item in LDS
constexpr int kTileCols = 18, kTileRows = 3;   // corner columns / rows a 256 x 16 pixel tile can touch at C >= 16
constexpr int kTilePairs = kTileCols * kTileRows * 32;

struct ToneStatsArgs {
    float m[9];
    int useMatrix;
    int width, height, pitch;                  // of the launch (its place in the full frame: FinishSrc's offsets, both forms)
    int cellShift, nzShift, gx;                // log2 C, log2 NZ, cells of a full-frame row
    int rowShift;                              // log2 R: rows of an item
    int chunkCells;                            // K
    int block0;                                // first row block (full-frame rows >> rowShift) the launch meets
    int chunk0, chunks;                        // first chunk of cells and how many
    int items;                                 // row blocks x chunks
};

// inclusive prefix sum over the wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// One (entry, count, sum) per lane: runs of neighbouring lanes on one entry are summed and the run's last lane adds to LDS.
// `entry` < 0: the lane has nothing (its run is its own).  Called by all lanes of the wave.
__device__ __forceinline__ void grid_add(uint32_t* sCount, uint32_t* sSum, int entry, uint32_t cnt, uint32_t sum)
{
    const int lane = threadIdx.x & 63;
    const int key = entry >= 0 ? entry : -1 - lane;                 // unique where there is nothing to merge
    const int prev = __shfl_up(key, 1);
    const bool head = lane == 0 || prev != key;
    const u64 heads = __ballot(head);                               // (bit 0 is always set)
    const uint32_t pc = wave_scan(cnt), ps = wave_scan(sum);
    const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1);
    const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));  // the run's first lane
    const int before = start > 0 ? start - 1 : 0;
    const uint32_t bc = __shfl(pc, before), bs = __shfl(ps, before);
    if (tail && entry >= 0) {
        const uint32_t c = pc - (start > 0 ? bc : 0u), s = ps - (start > 0 ? bs : 0u);
        atomicAdd(&sCount[entry], c);
        if (s) atomicAdd(&sSum[entry], s);
    }
}

// FINISH = 0: `a` is the image.  FINISH = 1: `a` is the accumulator, `b` the weight image, and the pixel is finish_value's.
template <int FINISH>
__global__ void __launch_bounds__(kStatsThreads)
    k_toneGridStats(const pix3* __restrict__ a, const pix3* __restrict__ b, FinishSrc f, ToneStatsArgs s, u64* __restrict__ stats)
{
    __shared__ uint32_t sCount[kGridEntries];
    __shared__ uint32_t sSum[kGridEntries];
    for (int k = threadIdx.x; k < kGridEntries; k += kStatsThreads) sCount[k] = sSum[k] = 0;
    __syncthreads();
    const ToneStatsArgs& g = s;
    const int colOffset = f.colOffset, rowOffset = f.rowOffset;
    const int used = s.chunkCells << g.nzShift;                     // entries of a chunk, <= kGridEntries
    for (int item = blockIdx.x; item < s.items; item += gridDim.x) {  // (uniform over the workgroup)
        const int rb = s.block0 + item / s.chunks, ck = s.chunk0 + item % s.chunks;
        // the item's rectangle in the launch's coordinates
        const int ya = max((rb << s.rowShift) - rowOffset, 0), yb = min(((rb + 1) << s.rowShift) - rowOffset, s.height);
        const int cell0 = ck * s.chunkCells;
        const long long xl = ((long long)cell0 << g.cellShift) - colOffset, xr = ((long long)(cell0 + s.chunkCells) << g.cellShift) - colOffset;
        const int xa = (int)(xl > 0 ? xl : 0), xb = (int)(xr < s.width ? xr : s.width);
        const int cellY = (ya + rowOffset) >> g.cellShift;        // one row of cells: R <= C and the blocks are aligned
        if (ya < yb && xa < xb) {
            const unsigned qpr = (unsigned)(xb - xa + kStatsPpl - 1) / kStatsPpl, q1 = qpr * (unsigned)(yb - ya);
            for (unsigned base = 0; base < q1; base += kStatsThreads) {
                const unsigned u = base + threadIdx.x;
                const bool live = u < q1;
                int ent[kStatsPpl], key[kStatsPpl];
#pragma unroll
                for (int k = 0; k < kStatsPpl; k++) ent[k] = -1, key[k] = 0;
                if (live) {
                    const int y = ya + (int)(u / qpr), x0 = xa + (int)(u % qpr) * kStatsPpl;
                    pix3 p[kStatsPpl];
                    load_quad(row_ptr(a, s.pitch, y), x0, xb, p);
                    if (FINISH) {
                        pix3 w[kStatsPpl];
                        load_quad(row_ptr(b, s.pitch, y), x0, xb, w);
#pragma unroll
                        for (int k = 0; k < kStatsPpl; k++) p[k] = finish_value(p[k], w[k], x0 + k, y, f);
                    }
#pragma unroll
                    for (int k = 0; k < kStatsPpl; k++) {
                        if (x0 + k >= xb) continue;
                        key[k] = luma_key(s.useMatrix ? matrix_pixel(p[k], s.m) : p[k]);
                        const int cx = ((x0 + k + colOffset) >> g.cellShift) - cell0;    // 0 .. K - 1
                        ent[k] = (cx << g.nzShift) + ((key[k] << g.nzShift) >> 12);
                    }
                }
                // within the lane: pixels k >= 1 on pixel 0's entry join it; the others are the lane's own adds
                uint32_t cnt = ent[0] >= 0 ? 1u : 0u, sum = (uint32_t)key[0];
                bool single = true;
#pragma unroll
                for (int k = 1; k < kStatsPpl; k++) {
                    if (ent[k] < 0) continue;
                    if (ent[k] == ent[0]) {
                        cnt += 1;
                        sum += (uint32_t)key[k];
                    } else
                        single = false;
                }
                if (__ballot(live) == 0) continue;                  // (uniform over the wave)
                grid_add(sCount, sSum, ent[0], cnt, sum);
                if (!single) {
#pragma unroll
                    for (int k = 1; k < kStatsPpl; k++)
                        if (ent[k] >= 0 && ent[k] != ent[0]) {
                            atomicAdd(&sCount[ent[k]], 1u);
                            if (key[k]) atomicAdd(&sSum[ent[k]], (uint32_t)key[k]);
                        }
                }
            }
        }
        __syncthreads();
        // one sweep: contiguous lanes, contiguous words; the counters are left zeroed for the next item
        for (int e = threadIdx.x; e < used; e += kStatsThreads) {
            const uint32_t c = sCount[e];
            if (c) {
                const uint32_t sm = sSum[e];
                const int cx = cell0 + (e >> g.nzShift), bin = e & ((1 << g.nzShift) - 1);  // cx < GX: only cells with pixels count
                u64* t = stats + 2 * ((((size_t)cellY * g.gx + cx) << g.nzShift) + bin);
                atomicAdd(t, (u64)c);
                if (sm) atomicAdd(t + 1, (u64)sm);
                sCount[e] = sSum[e] = 0;
            }
        }
        __syncthreads();
    }
}

// ---- the slice ----------------------------------------------------------------------------------------------------------
// the corner columns of the workgroup's tile as pairs in sPair (Tile, finish_stages.hpp)
template <int GL>
__device__ __forceinline__ Tile stage_grid(const SliceArgs& t, u64* sPair, int tileX0, int tileX1, int tileY0, int tileY1)
{
    Tile tl = {0, 0, 0};
    if (!GL) return tl;
    // (all uniform over the workgroup; the axis is monotone, so every pixel's corners lie between the tile's first and last)
    const Axis xa = grid_axis(tileX0 + t.g.colOffset, t.invCell, t.g.gx), xb = grid_axis(tileX1 + t.g.colOffset, t.invCell, t.g.gx);
    const Axis ya = grid_axis(tileY0 + t.g.rowOffset, t.invCell, t.g.gy), yb = grid_axis(tileY1 + t.g.rowOffset, t.invCell, t.g.gy);
    const int cols = xb.i1 - xa.i0 + 1, rows = yb.i1 - ya.i0 + 1;
    if (cols > kTileCols || rows > kTileRows) return tl;            // (never at C >= 16: the guard of the LDS array)
    tl.i0 = xa.i0;
    tl.j0 = ya.i0;
    tl.cols = cols;
    const int tid = threadIdx.y * blockDim.x + threadIdx.x, nt = blockDim.x * blockDim.y;
    const int n = (rows * cols) << t.g.nzShift;
    for (int e = tid; e < n; e += nt) {
        const int k = e & (t.g.nz - 1), c = e >> t.g.nzShift;
        const int col = tl.i0 + c % cols, row = tl.j0 + c / cols;
        const float* gp = t.grid + (((size_t)row * t.g.gx + col) << t.g.nzShift);
        sPair[e] = pack_pair(gp[k], gp[min(k + 1, t.g.nz - 1)]);
    }
    __syncthreads();
    return tl;
}

__device__ __forceinline__ pix3 scale3(pix3 p, float g)
{
    pix3 o;
    o.x = p.x * g;
    o.y = p.y * g;
    o.z = p.z * g;
    return o;
}

#define TILE_OF_WORKGROUP(FORMAT)                                                                    \
    const int tileX0 = blockIdx.x * blockDim.x * Fmt<FORMAT>::ppl, tileY0 = blockIdx.y * blockDim.y; \
    const int tileX1 = min(tileX0 + (int)blockDim.x * Fmt<FORMAT>::ppl, width) - 1;                  \
    const int tileY1 = min(tileY0 + (int)blockDim.y, height) - 1

template <int FORMAT, int LDS, int GL>
__global__ void __launch_bounds__(LDS ? 1024 : 256)
    k_localToneImage(const pix3* in, int inPitch, pix3* outImg, int outPitch, uint8_t* out, int outRowBytes, int width, int height,
                     RenderArgs r, SliceArgs t)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    __shared__ u64 s_pair[GL ? kTilePairs : 1];
    const float* lut = stage_lut<LDS>(r, s_lut);
    TILE_OF_WORKGROUP(FORMAT);                                      // (the grid covers the image: the tile is not empty)
    const Tile tl = stage_grid<GL>(t, s_pair, tileX0, tileX1, tileY0, tileY1);
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * Fmt<FORMAT>::ppl;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x0 >= width || y >= height) return;
    const pix3* inRow = row_ptr(in, inPitch, y);
    auto src = [&](int x) {
        const pix3 p = inRow[x];
        return scale3(p, slice_gain<GL>(p, x, y, r, t, tl, s_pair));
    };
    render_span<FORMAT>(src, outImg ? row_ptr(outImg, outPitch, y) : nullptr, out ? out + (size_t)outRowBytes * (size_t)y : nullptr,
                        x0, width, r, lut);
}

template <int FORMAT, int LDS, int GL>
__global__ void __launch_bounds__(LDS ? 1024 : 256)
    k_finishLocalTone(const pix3* __restrict__ finalImg, const pix3* __restrict__ weight, int imgPitch, FinishSrc f,
                      pix3* __restrict__ outImg, int outPitch, uint8_t* __restrict__ out, int outRowBytes, int width, int height,
                      RenderArgs r, SliceArgs t)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    __shared__ u64 s_pair[GL ? kTilePairs : 1];
    const float* lut = stage_lut<LDS>(r, s_lut);
    TILE_OF_WORKGROUP(FORMAT);
    const Tile tl = stage_grid<GL>(t, s_pair, tileX0, tileX1, tileY0, tileY1);
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * Fmt<FORMAT>::ppl;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x0 >= width || y >= height) return;
    const pix3* valRow = row_ptr(finalImg, imgPitch, y);
    const pix3* wRow = row_ptr(weight, imgPitch, y);
    auto src = [&](int x) {
        const pix3 p = finish_value(valRow[x], wRow[x], x, y, f);
        return scale3(p, slice_gain<GL>(p, x, y, r, t, tl, s_pair));
    };
    render_span<FORMAT>(src, outImg ? row_ptr(outImg, outPitch, y) : nullptr, out ? out + (size_t)outRowBytes * (size_t)y : nullptr,
                        x0, width, r, lut);
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

GridGeom grid_geom(const mfsr_local_tone* lt, int colOffset, int rowOffset, int fullWidth, int fullHeight)
{
    GridGeom g;
    g.cellShift = ilog2(lt->cell);
    g.nz = lt->bins;
    g.nzShift = ilog2(lt->bins);
    g.gx = (int)mfsr_cdiv(fullWidth, lt->cell);
    g.gy = (int)mfsr_cdiv(fullHeight, lt->cell);
    g.colOffset = colOffset;
    g.rowOffset = rowOffset;
    return g;
}

// How the gain grid is read.  Measured at 7680 x 4320 with a colour matrix and a 4096-interval table (DESIGN.md section 5,
// "Local tone"; profiles/local_tone_bench_4k16.txt).  MFSR_LOCAL_TONE_GRID=lds | cache forces one form for every format (A/B);
// read at every call: host only, and a test can switch it.
bool grid_in_lds(int format)
{
    if (const char* e = getenv("MFSR_LOCAL_TONE_GRID")) {
        if (strcmp(e, "lds") == 0) return true;
        if (strcmp(e, "cache") == 0) return false;
    }
    return format == MFSR_OUT_RGB8;
}

// what the two slice entry points share: the description, the grid pointer and the window of the full frame
int slice_validate(const float* gridDev, const mfsr_local_tone* lt, int w, int h, int colOffset, int rowOffset, int fullWidth,
                   int fullHeight)
{
    MFSR_REQUIRE(gridDev != nullptr && ((uintptr_t)gridDev & 3) == 0);
    if (int rc = mfsr_local_tone_validate(lt)) return rc;
    MFSR_REQUIRE(rowOffset >= 0 && fullHeight >= rowOffset + h);
    MFSR_REQUIRE(colOffset >= 0 && fullWidth >= colOffset + w);
    return MFSR_OK;
}

SliceArgs slice_args(const float* gridDev, const mfsr_local_tone* lt, int colOffset, int rowOffset, int fullWidth, int fullHeight)
{
    SliceArgs t;
    t.grid = gridDev;
    t.g = grid_geom(lt, colOffset, rowOffset, fullWidth, fullHeight);
    t.invCell = 1.0f / (float)lt->cell;
    t.fnz = (float)lt->bins;
    return t;
}

#define LOCAL_TONE_DISPATCH(KERNEL, format, lds, gl, ...)                                                           \
    do {                                                                                                            \
        const dim3 block(64, (lds) ? 16 : 4);                                                                       \
        const dim3 grid(mfsr_cdiv(mfsr_cdiv(w, (format) == MFSR_OUT_RGB8 ? 4 : 1), 64), mfsr_cdiv(h, block.y));     \
        switch (((format) << 2) | ((lds) ? 2 : 0) | ((gl) ? 1 : 0)) {                                               \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGB16, 0, 0, __VA_ARGS__);                                             \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGB16, 0, 1, __VA_ARGS__);                                             \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGB16, 1, 0, __VA_ARGS__);                                             \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGB16, 1, 1, __VA_ARGS__);                                             \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGB8, 0, 0, __VA_ARGS__);                                              \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGB8, 0, 1, __VA_ARGS__);                                              \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGB8, 1, 0, __VA_ARGS__);                                              \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGB8, 1, 1, __VA_ARGS__);                                              \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGBA8, 0, 0, __VA_ARGS__);                                             \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGBA8, 0, 1, __VA_ARGS__);                                             \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGBA8, 1, 0, __VA_ARGS__);                                             \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGBA8, 1, 1, __VA_ARGS__);                                             \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGB10A2, 0, 0, __VA_ARGS__);                                           \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGB10A2, 0, 1, __VA_ARGS__);                                           \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGB10A2, 1, 0, __VA_ARGS__);                                           \
            LOCAL_TONE_CASE(KERNEL, MFSR_OUT_RGB10A2, 1, 1, __VA_ARGS__);                                           \
        }                                                                                                           \
    } while (0)
#define LOCAL_TONE_CASE(KERNEL, F, L, G, ...) \
    case ((F) << 2) | ((L) << 1) | (G): hipLaunchKernelGGL((KERNEL<F, L, G>), grid, block, 0, mfsr_s(stream), __VA_ARGS__); break

int tone_stats_validate(const float* matrix, const mfsr_local_tone* lt, int w, int h, int rowBytes, int colOffset, int rowOffset,
                        int fullWidth, int fullHeight, const uint64_t* statsDev)
{
    MFSR_REQUIRE(statsDev != nullptr && ((uintptr_t)statsDev & 7) == 0);
    if (int rc = mfsr_local_tone_validate(lt)) return rc;
    MFSR_REQUIRE(w > 0 && h > 0 && (long long)w * h < (1LL << 31));
    MFSR_REQUIRE((long long)rowBytes >= 12LL * w && (rowBytes & 3) == 0);
    MFSR_REQUIRE(rowOffset >= 0 && fullHeight >= rowOffset + h);
    MFSR_REQUIRE(colOffset >= 0 && fullWidth >= colOffset + w);
    if (matrix)
        for (int i = 0; i < 9; i++) MFSR_REQUIRE(std::isfinite(matrix[i]) && fabsf(matrix[i]) <= 256.0f);
    return MFSR_OK;
}

// The items of a launch: row blocks of R rows times chunks of K cells, both on the full frame's grid.  R starts at C and is
// halved while there are fewer items than two per CU and an item still keeps every lane busy for two rounds.
ToneStatsArgs tone_stats_args(const float* matrix, const mfsr_local_tone* lt, int w, int h, int rowBytes, int colOffset, int rowOffset,
                              int fullWidth, int fullHeight, unsigned* groups)
{
    ToneStatsArgs s;
    for (int i = 0; i < 9; i++) s.m[i] = matrix ? matrix[i] : 0.0f;
    s.useMatrix = matrix != nullptr;
    s.width = w;
    s.height = h;
    s.pitch = rowBytes;
    s.cellShift = ilog2(lt->cell);
    s.nzShift = ilog2(lt->bins);
    s.gx = (int)mfsr_cdiv(fullWidth, lt->cell);
    s.chunkCells = kGridEntries / lt->bins;
    s.chunk0 = (colOffset / lt->cell) / s.chunkCells;
    s.chunks = ((colOffset + w - 1) / lt->cell) / s.chunkCells - s.chunk0 + 1;
    const long long chunkPx = (long long)s.chunkCells * lt->cell;
    const long long itemW = chunkPx < w ? chunkPx : w;
    const int want = 2 * mfsr_device_cus();
    int shift = s.cellShift;
    for (;;) {
        const int R = 1 << shift;
        const long long items = (long long)((rowOffset + h - 1) / R - rowOffset / R + 1) * s.chunks;
        if (items >= want || shift == 0 || (long long)(R / 2) * itemW < 2LL * kStatsThreads * kStatsPpl) break;
        shift--;
    }
    s.rowShift = shift;
    s.block0 = rowOffset >> shift;
    const long long items = (long long)(((rowOffset + h - 1) >> shift) - s.block0 + 1) * s.chunks;  // < 2^31: w h < 2^31
    s.items = (int)items;
    *groups = (unsigned)(items < want ? items : want);
    return s;
}

}  // namespace

extern "C" int mfsr_local_tone_validate(const mfsr_local_tone* lt)
{
    MFSR_REQUIRE(lt != nullptr);
    MFSR_REQUIRE(pow2(lt->cell) && lt->cell >= 16 && lt->cell <= 512);
    MFSR_REQUIRE(lt->bins == 4 || lt->bins == 8 || lt->bins == 16 || lt->bins == 32);
    MFSR_REQUIRE(lt->smooth >= 0 && lt->smooth <= 4);
    MFSR_REQUIRE(lt->shadows >= 0.0f && lt->shadows <= 1.0f && lt->highlights >= 0.0f && lt->highlights <= 1.0f);  // (false for NaN)
    MFSR_REQUIRE(lt->pivot >= 0.0f && lt->pivot <= 1.0f);
    MFSR_REQUIRE(lt->maxGain >= 1.0f && lt->maxGain <= 64.0f);
    for (int i = 0; i < 4; i++) MFSR_REQUIRE(lt->reserved[i] == 0);
    return MFSR_OK;
}

extern "C" int mfsr_local_tone_defaults(int w, int h, mfsr_local_tone* lt)
{
    MFSR_REQUIRE(lt != nullptr && w > 0 && h > 0);
    memset(lt, 0, sizeof(*lt));
    const int m = w > h ? w : h;
    int cell = 16;
    while (cell < 512 && mfsr_cdiv(m, cell) > 128) cell *= 2;
    MFSR_REQUIRE(mfsr_cdiv(m, cell) <= 128);  // (an image of more than 65536 pixels a side: choose the cell yourself)
    lt->cell = cell;
    lt->bins = 16;
    lt->smooth = 1;
    lt->shadows = 0.5f;
    lt->highlights = 0.25f;
    lt->pivot = 0.0f;
    lt->maxGain = 4.0f;
    return MFSR_OK;
}

extern "C" int mfsr_local_tone_grid(int fullWidth, int fullHeight, const mfsr_local_tone* lt, int* gx, int* gy, int* gz)
{
    MFSR_REQUIRE(fullWidth > 0 && fullHeight > 0 && gx && gy && gz);
    if (int rc = mfsr_local_tone_validate(lt)) return rc;
    *gx = (int)mfsr_cdiv(fullWidth, lt->cell);
    *gy = (int)mfsr_cdiv(fullHeight, lt->cell);
    *gz = lt->bins;
    return MFSR_OK;
}

extern "C" int mfsr_toneGridStats(const mfsr_float3* in, int inRowBytes, int w, int h, int colOffset, int rowOffset, int fullWidth,
                                  int fullHeight, const float* matrix, const mfsr_local_tone* lt, uint64_t* statsDev,
                                  mfsr_stream_t stream)
{
    // host validation first: nothing below touches the device before every argument has passed
    MFSR_REQUIRE(in != nullptr && ((uintptr_t)in & 3) == 0);
    if (int rc = tone_stats_validate(matrix, lt, w, h, inRowBytes, colOffset, rowOffset, fullWidth, fullHeight, statsDev)) return rc;
    unsigned groups = 0;
    const ToneStatsArgs s = tone_stats_args(matrix, lt, w, h, inRowBytes, colOffset, rowOffset, fullWidth, fullHeight, &groups);
    const FinishSrc none = finish_src(nullptr, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, colOffset, rowOffset, fullWidth, fullHeight);
    hipLaunchKernelGGL(k_toneGridStats<0>, dim3(groups), dim3(kStatsThreads), 0, mfsr_s(stream), (const pix3*)in, (const pix3*)nullptr,
                       none, s, (u64*)statsDev);
    return mfsr_launch_status("k_toneGridStats");
}

extern "C" int mfsr_finishToneGridStats(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes,
                                        const mfsr_float3* fallback, int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0,
                                        float v1, int w, int h, float threshold, int colOffset, int rowOffset, int fullWidth,
                                        int fullHeight, const float* matrix, const mfsr_local_tone* lt, uint64_t* statsDev,
                                        mfsr_stream_t stream)
{
    if (int rc = finish_check_src(finalImg, weight, imgRowBytes, fallback, fbRowBytes, fbW, fbH, w, h, colOffset, rowOffset, fullWidth,
                                  fullHeight))
        return rc;
    // (its own: the quad loads want the three images dword-aligned)
    MFSR_REQUIRE(((uintptr_t)finalImg & 3) == 0 && ((uintptr_t)weight & 3) == 0 && ((uintptr_t)fallback & 3) == 0);
    if (int rc = tone_stats_validate(matrix, lt, w, h, imgRowBytes, colOffset, rowOffset, fullWidth, fullHeight, statsDev)) return rc;
    unsigned groups = 0;
    const ToneStatsArgs s = tone_stats_args(matrix, lt, w, h, imgRowBytes, colOffset, rowOffset, fullWidth, fullHeight, &groups);
    const FinishSrc f = finish_src(fallback, fbRowBytes, fbW, fbH, u0, u1, v0, v1, threshold, colOffset, rowOffset, fullWidth, fullHeight);
    hipLaunchKernelGGL(k_toneGridStats<1>, dim3(groups), dim3(kStatsThreads), 0, mfsr_s(stream), (const pix3*)finalImg,
                       (const pix3*)weight, f, s, (u64*)statsDev);
    return mfsr_launch_status("k_toneGridStats");
}

// ---- the fit (host only, double precision; no contraction, so a float64 numpy restatement differs only through pow and log)
namespace {
// one pass of [1 2 1] / 4 with replicated borders along the axis of `stride` and length `n`: ((lo + 2 c) + hi) * 0.25.  The array
// is `outer` blocks of n * stride values.
void blur_axis(std::vector<double>& v, std::vector<double>& tmp, size_t outer, size_t stride, int n)
{
    tmp.swap(v);
    const double* src = tmp.data();
    double* dst = v.data();
    for (size_t o = 0; o < outer; o++) {
        const size_t base = o * (size_t)n * stride;
        for (int k = 0; k < n; k++) {
            const double* c = src + base + (size_t)k * stride;
            const double* lo = k > 0 ? c - stride : c;
            const double* hi = k < n - 1 ? c + stride : c;
            double* d = dst + base + (size_t)k * stride;
            for (size_t i = 0; i < stride; i++) d[i] = ((lo[i] + 2.0 * c[i]) + hi[i]) * 0.25;
        }
    }
}

// fn(begin, end) over [0, n) on up to eight threads (one where n is small): every index is computed by exactly one thread from
// inputs no thread writes, so the result does not depend on the split
template <class Fn>
void parallel_ranges(size_t n, size_t grain, const Fn& fn)
{
    const unsigned hw = std::thread::hardware_concurrency();
    size_t parts = n / grain;
    parts = parts > 8 ? 8 : parts;
    parts = hw && parts > hw ? hw : parts;
    if (parts < 2) {
        fn((size_t)0, n);
        return;
    }
    std::vector<std::thread> pool;
    const size_t step = (n + parts - 1) / parts;
    for (size_t p = 1; p < parts; p++) pool.emplace_back([&fn, p, step, n] { fn(p * step, (p + 1) * step < n ? (p + 1) * step : n); });
    fn((size_t)0, step);
    for (std::thread& t : pool) t.join();
}
}  // namespace

extern "C" int mfsr_local_tone_fit(const uint64_t* statsHost, int fullWidth, int fullHeight, const mfsr_local_tone* lt, float* gridHost,
                                   double* pivotUsed, int32_t* status)
{
    MFSR_REQUIRE(statsHost != nullptr && gridHost != nullptr && status != nullptr && fullWidth > 0 && fullHeight > 0);
    if (int rc = mfsr_local_tone_validate(lt)) return rc;
    const int gx = (int)mfsr_cdiv(fullWidth, lt->cell), gy = (int)mfsr_cdiv(fullHeight, lt->cell), nz = lt->bins;
    const size_t total = (size_t)gx * gy * nz;
    // (kept between calls: a burst driver fits a grid of the same size for every burst, and fresh pages cost more than the fit)
    static thread_local std::vector<double> N, S, tmp;
    N.resize(total);
    S.resize(total);
    tmp.resize(total);
    double *pN = N.data(), *pS = S.data(), *pT = tmp.data();  // (the worker threads have thread-local vectors of their own)
    const bool measured = !(lt->pivot > 0.0f);
    // the terms n ln(max(s / (4095 n), 1 / 4095)) of the pivot's log-average (the unsmoothed entries), then summed in the table's order
    parallel_ranges(total, 8192, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            pN[i] = (double)statsHost[2 * i];
            pS[i] = (double)statsHost[2 * i + 1];
            pT[i] = 0.0;
            if (measured && statsHost[2 * i]) {
                const double m = pS[i] / (4095.0 * pN[i]);
                pT[i] = pN[i] * log(m > 1.0 / 4095.0 ? m : 1.0 / 4095.0);
            }
        }
    });
    double sumN = 0.0, sumL = 0.0;
    if (measured)
        for (size_t i = 0; i < total; i++)
            if (statsHost[2 * i]) {
                sumN += N[i];
                sumL += tmp[i];
            }
    for (int pass = 0; pass < lt->smooth; pass++)
        for (std::vector<double>* v : {&N, &S}) {
            blur_axis(*v, tmp, (size_t)gy, (size_t)nz, gx);
            blur_axis(*v, tmp, 1, (size_t)nz * gx, gy);
            blur_axis(*v, tmp, (size_t)gx * gy, 1, nz);
        }
    *status = 0;
    double pivot = (double)lt->pivot;
    if (!(pivot > 0.0)) {
        if (sumN > 0.0)
            pivot = exp(sumL / sumN);
        else {
            pivot = 0.18;
            *status = 1;
        }
    }
    const double maxGain = (double)lt->maxGain, minGain = 1.0 / maxGain;
    const double shadows = (double)lt->shadows, highlights = (double)lt->highlights;
    auto gain = [&](double B) {
        if (B < 1.0 / 4095.0) B = 1.0 / 4095.0;
        const double r = B / pivot;
        const double g = r < 1.0 ? pow(r, -shadows) : pow(r, -highlights);
        return (float)(g < minGain ? minGain : (g > maxGain ? maxGain : g));
    };
    float empty[32];  // an entry without pixels (also after the blur) holds the gain of its bin's centre: once per bin
    for (int k = 0; k < nz; k++) empty[k] = gain(((double)k + 0.5) / (double)nz);
    pN = N.data();  // (the blur swaps the vectors)
    pS = S.data();
    parallel_ranges(total / (size_t)nz, 512, [&](size_t c0, size_t c1) {
        for (size_t i = c0 * (size_t)nz; i < c1 * (size_t)nz; i += (size_t)nz)
            for (int k = 0; k < nz; k++) gridHost[i + k] = pN[i + k] > 0.0 ? gain(pS[i + k] / (4095.0 * pN[i + k])) : empty[k];
    });
    if (pivotUsed) *pivotUsed = pivot;
    return MFSR_OK;
}

// ---- the slice's entry points
extern "C" int mfsr_localToneImage(const mfsr_float3* in, int inRowBytes, mfsr_float3* outImg, int outImgRowBytes, void* out,
                                   int outRowBytes, int w, int h, const mfsr_render* render, int applyGamma, const float* gridDev,
                                   const mfsr_local_tone* lt, int colOffset, int rowOffset, int fullWidth, int fullHeight,
                                   mfsr_stream_t stream)
{
    MFSR_REQUIRE(in && (outImg || out) && w > 0 && h > 0);
    MFSR_REQUIRE((long long)inRowBytes >= 12LL * w && (inRowBytes & 3) == 0 && ((uintptr_t)in & 3) == 0);
    if (outImg) MFSR_REQUIRE((long long)outImgRowBytes >= 12LL * w && (outImgRowBytes & 3) == 0 && ((uintptr_t)outImg & 3) == 0);
    if (int rc = mfsr_render_validate(render)) return rc;
    MFSR_REQUIRE(!yuv_format(render->format));  // single-plane formats only
    if (out)
        if (int rc = check_out(render->format, out, outRowBytes, w)) return rc;
    if (int rc = slice_validate(gridDev, lt, w, h, colOffset, rowOffset, fullWidth, fullHeight)) return rc;
    const RenderArgs a = render_args(render, applyGamma);
    const SliceArgs t = slice_args(gridDev, lt, colOffset, rowOffset, fullWidth, fullHeight);
    const bool lds = lut_in_lds(render), gl = grid_in_lds(render->format);
    LOCAL_TONE_DISPATCH(k_localToneImage, render->format, lds, gl, (const pix3*)in, inRowBytes, (pix3*)outImg, outImgRowBytes,
                        (uint8_t*)out, outRowBytes, w, h, a, t);
    return mfsr_launch_status("localToneImage");
}

extern "C" int mfsr_finishLocalTone(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                                    int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, mfsr_float3* outImg,
                                    int outImgRowBytes, void* out, int outRowBytes, const mfsr_render* render, int w, int h,
                                    float threshold, int applyGamma, int colOffset, int rowOffset, int fullWidth, int fullHeight,
                                    const float* gridDev, const mfsr_local_tone* lt, mfsr_stream_t stream)
{
    if (int rc = finish_check(finalImg, weight, imgRowBytes, fallback, fbRowBytes, fbW, fbH, outImg, outImgRowBytes, out, w, h, colOffset,
                              rowOffset, fullWidth, fullHeight))
        return rc;
    if (int rc = mfsr_render_validate(render)) return rc;
    MFSR_REQUIRE(!yuv_format(render->format));
    if (out)
        if (int rc = check_out(render->format, out, outRowBytes, w)) return rc;
    if (int rc = slice_validate(gridDev, lt, w, h, colOffset, rowOffset, fullWidth, fullHeight)) return rc;
    const RenderArgs a = render_args(render, applyGamma);
    const SliceArgs t = slice_args(gridDev, lt, colOffset, rowOffset, fullWidth, fullHeight);
    const FinishSrc f = finish_src(fallback, fbRowBytes, fbW, fbH, u0, u1, v0, v1, threshold, colOffset, rowOffset, fullWidth, fullHeight);
    const bool lds = lut_in_lds(render), gl = grid_in_lds(render->format);
    LOCAL_TONE_DISPATCH(k_finishLocalTone, render->format, lds, gl, (const pix3*)finalImg, (const pix3*)weight, imgRowBytes, f,
                        (pix3*)outImg, outImgRowBytes, (uint8_t*)out, outRowBytes, w, h, a, t);
    return mfsr_launch_status("finishLocalTone");
}
