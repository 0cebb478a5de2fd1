// defect.hip -- defective-pixel detection by a vote over the frames of a burst, and repair under a map.
//
// The rule is stated in include/mfsr.h (mfsr_detectDefects / mfsr_repairDefects): exact integer arithmetic, the results equal
// a numpy restatement bit for bit.  d = 1 (mono) or 2 (Bayer: the same-colour lattice of every quad position).
//
// Shape (k_defectVotes): one wavefront owns a strip of 64 * 4 columns and a band of kDefBand rows of EVERY frame.  Lane l
// holds 4 columns as two packed 2 x u16 words (one 8-byte load per row); per frame it loads the band's kDefBand + 2d rows
// (the next frame's rows are in flight while this frame's are reduced), builds the column-wise max / min of each row triple
// (y-d, y, y+d) with packed 16-bit max / min, takes the +-d columns from the neighbouring words -- across lanes through
// whole-wave DPP shifts, so lanes 0 and 63 are halo lanes and a strip yields 62 * 4 output columns -- and adds the hot / cold
// votes into per-pixel counters that stay in registers over the frame loop: one 32-bit register per word and row, each 16-bit
// half holding the hot count in its low byte and the cold count in its high byte (counts <= 64).  The map is written once
// with plain vector stores (no atomics on the map); the numbers of hot / cold pixels go to two device counters by one vector
// atomic add per wave.  Frame borders: a neighbour outside the frame is replaced by its mirror image about the centre
// (x - d -> x + d), an in-frame duplicate of another neighbour, which for max / min equals leaving it out.  No LDS.
//
// k_defectRepair: a lane reads 16 map bytes; only lanes that see a flagged pixel do anything (per frame: the <= 8 unflagged
// same-colour neighbours, a sorting network in registers, one 2-byte store).  Its cost is the read of the map.
#include "raw_stage.hpp"

namespace {

constexpr int kDefLanes = 64;
constexpr int kDefWords = 2;                                      // packed words of one lane and row
constexpr int kDefLaneCols = 2 * kDefWords;                       // columns of one lane: one 8-byte load per row
constexpr int kDefStripCols = kDefLaneCols * (kDefLanes - 2);     // output columns of one wave's strip
constexpr int kDefBand = 8;                                       // output rows of one wave's band
constexpr int kDefWavesPerBlock = 4;

struct DefGeom {
    int pitch;      // bytes
    int width, height;
    int nFrames;
    int nStrips, nBands;
    int threshold4;  // 4 * threshold
    int spread;
    int minVotes;
    int mapPitch;
    int mapVec;     // the map takes 4-byte stores (pointer and pitch 4-byte aligned, width % 4 == 0)
};

typedef unsigned short def_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ def_u16x2 def_v(uint32_t w) { return __builtin_bit_cast(def_u16x2, w); }
__device__ __forceinline__ uint32_t def_w(def_u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
// packed 2 x u16 max / min / saturating difference (v_pk_max_u16, v_pk_min_u16, v_pk_sub_u16 clamp)
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) { return def_w(__builtin_elementwise_max(def_v(a), def_v(b))); }
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) { return def_w(__builtin_elementwise_min(def_v(a), def_v(b))); }
__device__ __forceinline__ uint32_t pk_subsat(uint32_t a, uint32_t b) { return def_w(__builtin_elementwise_sub_sat(def_v(a), def_v(b))); }

// row slot t of a band (t may lie d rows outside the frame): the mirror image about the centre row that uses it, clamped
// (slots further out serve only rows that are not output)
__device__ __forceinline__ int def_row(int t, int d, int height)
{
    t = t < 0 ? t + 2 * d : (t >= height ? t - 2 * d : t);
    return clampi(t, 0, height - 1);
}

// columns col .. col+3 of one row as two packed words, column col in the low half of word 0.  Branch-free (every load is
// unconditional): VEC is one 8-byte load at col clamped to [0, width - 4] -- a lane lies entirely inside or entirely outside
// the frame then (width % 4 == 0, col a multiple of 4); otherwise 16-bit loads at columns clamped into the row.  A clamped
// column is never a neighbour of an output pixel (the border masks replace it) nor an output pixel itself.
struct DefRow {
    uint32_t w[kDefWords];
};
// off[]: the lane's byte offsets within a row (def_offsets): row is uniform, so a load is scalar base + 32-bit lane offset
template <bool VEC>
__device__ __forceinline__ DefRow def_load(const char* row, const uint32_t off[kDefLaneCols])
{
    DefRow r;
    if (VEC) {
        const uint2 v = *(const uint2*)(row + off[0]);
        r.w[0] = v.x;
        r.w[1] = v.y;
        return r;
    }
#pragma unroll
    for (int j = 0; j < kDefWords; j++) {
        const uint32_t a = *(const uint16_t*)(row + off[2 * j]);
        const uint32_t b = *(const uint16_t*)(row + off[2 * j + 1]);
        r.w[j] = a | (b << 16);
    }
    return r;
}
template <bool VEC>
__device__ __forceinline__ void def_offsets(int col, int width, uint32_t off[kDefLaneCols])
{
#pragma unroll
    for (int k = 0; k < kDefLaneCols; k++) off[k] = 2u * (uint32_t)clampi(col + k, 0, width - (VEC ? kDefLaneCols : 1));
}
static_assert(kDefWords == 2, "def_load and the map store move one lane's row as 8 / 4 bytes");

// D: lattice step (1 mono, 2 Bayer).  VEC: every frame pointer and the pitch are 8-byte aligned and width % 4 == 0.
template <int D, bool VEC>
__global__ __launch_bounds__(kDefWavesPerBlock * kDefLanes) __attribute__((amdgpu_waves_per_eu(3))) void k_defectVotes(RawFrames frames, DefGeom g, uint8_t* map,
                                                                                uint32_t* counts)
{
    constexpr int kRows = kDefBand + 2 * D;  // row slots of a band: rows y0 - D .. y0 + kDefBand - 1 + D
    const int lane = threadIdx.x & (kDefLanes - 1);
    // (readfirstlane: the wave's index is uniform, so that everything derived from it stays in scalar registers)
    const int wave = blockIdx.x * kDefWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave >= g.nStrips * g.nBands) return;  // (whole waves)
    const int strip = wave % g.nStrips, band = wave / g.nStrips;
    const int col = strip * kDefStripCols + kDefLaneCols * (lane - 1);  // lane 0 of strip 0 lies left of the frame
    const int y0 = band * kDefBand;

    size_t rowOff[kRows];  // (uniform)
#pragma unroll
    for (int k = 0; k < kRows; k++) rowOff[k] = (size_t)def_row(y0 - D + k, D, g.height) * (size_t)g.pitch;

    // border masks per word: which halves have their left (x - D) / right (x + D) neighbour inside the frame; the other
    // halves take the mirror image.  Only strips whose output columns reach within D of a frame edge hold such columns: the
    // first one, and every strip whose last output column (strip + 1) * kDefStripCols - 1 has x + D >= width -- for a width just
    // above a multiple of the strip that is the last but one as well as the last.
    const bool edge = strip == 0 || (strip + 1) * kDefStripCols + D > g.width;  // (uniform)
    uint32_t lmask[kDefWords], rmask[kDefWords];
#pragma unroll
    for (int j = 0; j < kDefWords; j++) {
        const int x = col + 2 * j;
        lmask[j] = (x - D >= 0 ? 0xffffu : 0u) | (x + 1 - D >= 0 ? 0xffff0000u : 0u);
        rmask[j] = (x + D < g.width ? 0xffffu : 0u) | (x + 1 + D < g.width ? 0xffff0000u : 0u);
    }

    uint32_t cnt[kDefBand][kDefWords];
#pragma unroll
    for (int i = 0; i < kDefBand; i++)
#pragma unroll
        for (int j = 0; j < kDefWords; j++) cnt[i][j] = 0;

    uint32_t off[kDefLaneCols];
    def_offsets<VEC>(col, g.width, off);
    DefRow cur[kRows];
    {
        const char* base = (const char*)frames.p[0];
#pragma unroll
        for (int k = 0; k < kRows; k++) cur[k] = def_load<VEC>(base + rowOff[k], off);
    }
    for (int f = 0; f < g.nFrames; f++) {
        // the next frame's rows are in flight while this frame's are reduced (the last frame is loaded twice)
        DefRow nxt[kRows];
        const char* base = (const char*)frames.p[min(f + 1, g.nFrames - 1)];
#pragma unroll
        for (int k = 0; k < kRows; k++) nxt[k] = def_load<VEC>(base + rowOff[k], off);
#pragma unroll
        for (int i = 0; i < kDefBand; i++) {
            const uint32_t *up = cur[i].w, *ce = cur[i + D].w, *dn = cur[i + 2 * D].w;
            // vertical neighbours; column max / min of the row triple, words -1 .. kDefWords
            uint32_t vmax[kDefWords], vmin[kDefWords], cmax[kDefWords + 2], cmin[kDefWords + 2];
#pragma unroll
            for (int j = 0; j < kDefWords; j++) {
                vmax[j] = pk_max(up[j], dn[j]);
                vmin[j] = pk_min(up[j], dn[j]);
                cmax[j + 1] = pk_max(vmax[j], ce[j]);
                cmin[j + 1] = pk_min(vmin[j], ce[j]);
            }
            cmax[0] = wave_shr1(cmax[kDefWords]);
            cmin[0] = wave_shr1(cmin[kDefWords]);
            cmax[kDefWords + 1] = wave_shl1(cmax[1]);
            cmin[kDefWords + 1] = wave_shl1(cmin[1]);
#pragma unroll
            for (int j = 0; j < kDefWords; j++) {
                uint32_t lmax, rmax, lmin, rmin;  // column max / min at x - D and x + D of both halves
                if (D == 2) {
                    lmax = cmax[j];
                    rmax = cmax[j + 2];
                    lmin = cmin[j];
                    rmin = cmin[j + 2];
                } else {
                    lmax = __builtin_amdgcn_alignbyte(cmax[j + 1], cmax[j], 2);
                    rmax = __builtin_amdgcn_alignbyte(cmax[j + 2], cmax[j + 1], 2);
                    lmin = __builtin_amdgcn_alignbyte(cmin[j + 1], cmin[j], 2);
                    rmin = __builtin_amdgcn_alignbyte(cmin[j + 2], cmin[j + 1], 2);
                }
                if (edge) {
                    const uint32_t a = lmax, b = lmin;
                    lmax = (lmax & lmask[j]) | (rmax & ~lmask[j]);
                    lmin = (lmin & lmask[j]) | (rmin & ~lmask[j]);
                    rmax = (rmax & rmask[j]) | (a & ~rmask[j]);
                    rmin = (rmin & rmask[j]) | (b & ~rmask[j]);
                }
                const uint32_t hi = pk_max(pk_max(lmax, rmax), vmax[j]);
                const uint32_t lo = pk_min(pk_min(lmin, rmin), vmin[j]);
                // margin = threshold + (((hi - lo) * spread) >> 2) = ((hi - lo) * spread + 4 * threshold) >> 2 per half (< 2^21),
                // saturated to 16 bits: v - hi and lo - v are at most 65535, so the comparison does not change
                const uint32_t r = hi - lo;  // hi >= lo in both halves: no borrow
                const uint32_t m0 = min(((r & 0xffffu) * (uint32_t)g.spread + (uint32_t)g.threshold4) >> 2, 0xffffu);
                const uint32_t m1 = min(((r >> 16) * (uint32_t)g.spread + (uint32_t)g.threshold4) >> 2, 0xffffu);
                const uint32_t m = m0 | (m1 << 16);
                // hot: v > hi + margin <=> sat(v - hi) > margin; cold: v + margin < lo <=> sat(lo - v) > margin
                const uint32_t hot = pk_min(pk_subsat(pk_subsat(ce[j], hi), m), 0x00010001u);
                const uint32_t cold = pk_min(pk_subsat(pk_subsat(lo, ce[j]), m), 0x00010001u);
                cnt[i][j] += hot + (cold << 8);
            }
            __builtin_amdgcn_sched_barrier(0);  // one row at a time: interleaving the rows only costs registers
        }
#pragma unroll
        for (int k = 0; k < kRows; k++) cur[k] = nxt[k];
    }

    // the map of this lane's 8 x kDefBand pixels, and the counts of hot / cold pixels
    const bool laneOut = lane >= 1 && lane <= kDefLanes - 2;
    uint32_t nHot = 0, nCold = 0;
#pragma unroll
    for (int i = 0; i < kDefBand; i++) {
        const int y = y0 + i;
        uint32_t b = 0;  // 4 map bytes
#pragma unroll
        for (int j = 0; j < kDefWords; j++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint32_t c = (cnt[i][j] >> (16 * h)) & 0xffffu;
                const int x = col + 2 * j + h;
                const bool in = laneOut && y < g.height && x >= 0 && x < g.width;
                const uint32_t v = !in ? 0u : ((int)(c & 0xffu) >= g.minVotes ? 1u : ((int)(c >> 8) >= g.minVotes ? 2u : 0u));
                nHot += v == 1u;
                nCold += v == 2u;
                b |= v << (8 * (2 * j + h));
            }
        if (!laneOut || y >= g.height) continue;
        uint8_t* out = map + (size_t)y * (size_t)g.mapPitch;
        if (g.mapVec) {  // (uniform) width % 4 == 0: the lane lies inside the frame or outside it
            if (col < g.width) *(uint32_t*)(out + col) = b;
        } else {
#pragma unroll
            for (int k = 0; k < kDefLaneCols; k++)
                if (col + k < g.width) out[col + k] = (uint8_t)(b >> (8 * k));
        }
    }
    if (counts) {  // (uniform)
#pragma unroll
        for (int o = kDefLanes / 2; o > 0; o >>= 1) {
            nHot += __shfl_xor(nHot, o);
            nCold += __shfl_xor(nCold, o);
        }
        if (lane == 0 && nHot) atomicAdd(&counts[0], nHot);
        if (lane == 0 && nCold) atomicAdd(&counts[1], nCold);
    }
}

// ---- repair ---------------------------------------------------------------------------------------------------------------
struct RepGeom {
    int pitch, width, height, nFrames, d, mapPitch;
    int mapVec;  // 16-byte loads of the map (pointer and pitch 16-byte aligned)
};

__device__ __forceinline__ void def_cswap(uint32_t& a, uint32_t& b)
{
    const uint32_t lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

// the new value of pixel (x, y) in every frame: the median of its unflagged same-colour neighbours
__device__ void def_repair_pixel(const RawFramesMut& frames, const RepGeom& g, const uint8_t* map, int x, int y)
{
    size_t off[8];   // byte offsets of the neighbours in a frame
    bool ok[8];
    int n = 0, k = 0;
#pragma unroll
    for (int j = -1; j <= 1; j++)
#pragma unroll
        for (int i = -1; i <= 1; i++) {
            if (i == 0 && j == 0) continue;
            const int nx = x + i * g.d, ny = y + j * g.d;
            const bool in = nx >= 0 && nx < g.width && ny >= 0 && ny < g.height;
            ok[k] = in && map[(size_t)ny * (size_t)g.mapPitch + nx] == 0;
            off[k] = in ? (size_t)ny * (size_t)g.pitch + 2 * (size_t)nx : 0;
            n += ok[k];
            k++;
        }
    if (n == 0) return;  // nothing to take a value from: the pixel stays
    const size_t self = (size_t)y * (size_t)g.pitch + 2 * (size_t)x;
    for (int f = 0; f < g.nFrames; f++) {
        char* base = (char*)frames.p[f];
        uint32_t s[8];  // flagged / missing neighbours sort to the end
#pragma unroll
        for (int q = 0; q < 8; q++) s[q] = ok[q] ? (uint32_t) * (const uint16_t*)(base + off[q]) : 0xffffffffu;
        // sorting network for 8 inputs (19 compare-exchanges)
        def_cswap(s[0], s[1]); def_cswap(s[2], s[3]); def_cswap(s[4], s[5]); def_cswap(s[6], s[7]);
        def_cswap(s[0], s[2]); def_cswap(s[1], s[3]); def_cswap(s[4], s[6]); def_cswap(s[5], s[7]);
        def_cswap(s[1], s[2]); def_cswap(s[5], s[6]); def_cswap(s[0], s[4]); def_cswap(s[3], s[7]);
        def_cswap(s[1], s[5]); def_cswap(s[2], s[6]);
        def_cswap(s[1], s[4]); def_cswap(s[3], s[6]);
        def_cswap(s[2], s[4]); def_cswap(s[3], s[5]);
        def_cswap(s[3], s[4]);
        uint32_t a = 0, b = 0;  // s[n/2 - 1], s[n/2]
#pragma unroll
        for (int q = 0; q < 8; q++) {
            if (q == n / 2 - 1) a = s[q];
            if (q == n / 2) b = s[q];
        }
        const uint32_t v = (n & 1) ? b : (a + b + 1) >> 1;
        *(uint16_t*)(base + self) = (uint16_t)v;
    }
}

__global__ __launch_bounds__(256) void k_defectRepair(RawFramesMut frames, RepGeom g, const uint8_t* map)
{
    const int c16 = (g.width + 15) / 16;  // lanes of one row
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)c16 * g.height) return;
    const int y = (int)(idx / c16), x0 = 16 * (int)(idx % c16);
    const uint8_t* row = map + (size_t)y * (size_t)g.mapPitch;
    uint32_t w[4] = {0, 0, 0, 0};
    if (g.mapVec && x0 + 16 <= g.width) {
        const uint4 v = *(const uint4*)(row + x0);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    } else {
        for (int k = 0; k < 16 && x0 + k < g.width; k++) w[k >> 2] |= (uint32_t)row[x0 + k] << (8 * (k & 3));
    }
    if ((w[0] | w[1] | w[2] | w[3]) == 0) return;
    for (int k = 0; k < 16; k++)
        if ((w[k >> 2] >> (8 * (k & 3))) & 0xffu) def_repair_pixel(frames, g, map, x0 + k, y);
}

// the frames of a vote or a repair: at most kRawMaxFrames (the vote counters hold one byte), any size from one lattice
// neighbourhood (2d + 1) upwards, odd ones included
bool def_common_ok(int nFrames, const uint16_t* const* frames, int pitch, int width, int height, int mono)
{
    const int d = mono ? 1 : 2;
    return width >= 2 * d + 1 && height >= 2 * d + 1 && raw_frames_ok(nFrames, kRawMaxFrames, frames, pitch, width);
}

}  // namespace

extern "C" int mfsr_detectDefects(int nFrames, const uint16_t* const* frames, int pitch, int width, int height, int mono,
                                  int threshold, int spread, int minVotes, uint8_t* mapDev, int mapPitch, uint32_t* countsDev,
                                  mfsr_stream_t stream)
{
    // host validation first: nothing below touches the device before every argument has passed
    MFSR_REQUIRE(def_common_ok(nFrames, frames, pitch, width, height, mono));
    MFSR_REQUIRE(threshold >= 0 && threshold <= 65535 && spread >= 0 && spread <= 16);
    MFSR_REQUIRE(minVotes > nFrames / 2 && minVotes <= nFrames);
    MFSR_REQUIRE(mapDev != nullptr && mapPitch >= width);
    MFSR_REQUIRE(countsDev == nullptr || ((uintptr_t)countsDev & 3) == 0);

    const bool vec = raw_aligned(nFrames, frames, pitch, 8) && (width % kDefLaneCols) == 0;
    const RawFrames t = raw_table(nFrames, frames);
    DefGeom g;
    g.pitch = pitch;
    g.width = width;
    g.height = height;
    g.nFrames = nFrames;
    g.nStrips = (int)mfsr_cdiv(width, kDefStripCols);
    g.nBands = (int)mfsr_cdiv(height, kDefBand);
    g.threshold4 = 4 * threshold;
    g.spread = spread;
    g.minVotes = minVotes;
    g.mapPitch = mapPitch;
    g.mapVec = (width % kDefLaneCols) == 0 && (mapPitch % 4) == 0 && ((uintptr_t)mapDev & 3) == 0;

    if (countsDev) MFSR_HIP_TRY(hipMemsetAsync(countsDev, 0, 2 * sizeof(uint32_t), mfsr_s(stream)));
    const dim3 grid(mfsr_cdiv((long long)g.nStrips * g.nBands, kDefWavesPerBlock)), block(kDefWavesPerBlock * kDefLanes);
    if (mono) {
        if (vec)
            hipLaunchKernelGGL((k_defectVotes<1, true>), grid, block, 0, mfsr_s(stream), t, g, mapDev, countsDev);
        else
            hipLaunchKernelGGL((k_defectVotes<1, false>), grid, block, 0, mfsr_s(stream), t, g, mapDev, countsDev);
    } else {
        if (vec)
            hipLaunchKernelGGL((k_defectVotes<2, true>), grid, block, 0, mfsr_s(stream), t, g, mapDev, countsDev);
        else
            hipLaunchKernelGGL((k_defectVotes<2, false>), grid, block, 0, mfsr_s(stream), t, g, mapDev, countsDev);
    }
    return mfsr_launch_status("k_defectVotes");
}

extern "C" int mfsr_repairDefects(int nFrames, uint16_t* const* frames, int pitch, int width, int height, int mono,
                                  const uint8_t* mapDev, int mapPitch, mfsr_stream_t stream)
{
    MFSR_REQUIRE(def_common_ok(nFrames, frames, pitch, width, height, mono));
    MFSR_REQUIRE(mapDev != nullptr && mapPitch >= width);

    const RawFramesMut t = raw_table(nFrames, frames);
    RepGeom g;
    g.pitch = pitch;
    g.width = width;
    g.height = height;
    g.nFrames = nFrames;
    g.d = mono ? 1 : 2;
    g.mapPitch = mapPitch;
    g.mapVec = (mapPitch % 16) == 0 && ((uintptr_t)mapDev & 15) == 0;
    const dim3 block(256), grid(mfsr_cdiv((long long)mfsr_cdiv(width, 16) * height, 256));
    hipLaunchKernelGGL(k_defectRepair, grid, block, 0, mfsr_s(stream), t, g, mapDev);
    return mfsr_launch_status("k_defectRepair");
}
