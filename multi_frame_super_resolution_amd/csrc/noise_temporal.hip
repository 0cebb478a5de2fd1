// noise_temporal.hip -- burst noise calibration: the block statistics of §2.15 taken on the DIFFERENCE of two frames of a burst
// wherever their displacement relative to each other is a whole number of quads.  There both frames sample
// the scene at the same sub-quad phase: texture and aliasing cancel in the difference and what is left is noise, with no
// interpolation, so the device stage stays exact integer arithmetic.  The rule is stated in include/mfsr.h
// (mfsr_noiseStatsTemporal); the tables have the layout of mfsr_noiseStats and equal the numpy restatement of the tests
// (tests/noise_temporal_ref.py) bit for bit, for any launch shape.
//
// Shape (k_noiseStatsTemporal): the blocks of the rectangle are numbered row by row and cut into one contiguous chunk per
// workgroup (one workgroup of 16 waves per CU).  One lane owns one block of the reference grid and walks the pairs j < k of
// the launch in an order that is uniform over the workgroup.  Placement is one 8-byte load of a flow texel per frame and block
// from memory (a plain load at a fixed texel per block: adjacent lanes read texels 4 or 8 apart).  The lane does not keep all
// n placements (64 x 8 bytes would not fit its registers, and the LDS is the histogram's): it holds those of a tile of
// kTempTile frames j and sweeps the later frames k past the tile kTempAhead at a time, so that a step's texel loads are in
// flight together, every texel is read once per tile and not once per frame j, and a wave that accepts nothing in a step goes
// on after one wait.
// Under pure translation a whole wave accepts the same pairs; under rotation, and with any real flow field, the accepted pairs
// differ from lane to lane.  Accepted (block, j, k) go to a queue of the wave in LDS and every 64 of them are worked off one
// per lane: the lane finds its two sites again from the two texels, loads the 16 sample rows, reduces them, and the wave adds
// the terms to the histogram (ballots and shuffles stay outside divergent code).
// B's origin is A's plus 2 s samples = 4 s bytes and A's is 16 s_j bytes off the block grid in x only when s_j.x is a multiple
// of 4, so rows are read as four 32-bit words (ALIGN4: every frame pointer and the pitch are multiples of 4) or eight 16-bit
// samples -- there is no 16-byte path to fall off.
// The histogram is k_noiseStats': 16-bit LDS counters, two to a word.  There a block updates a key once; here one block can
// update the same key once per accepted pair, so the workgroup counts the terms it has added and flushes the histogram to
// memory before a step whose pairs, with what the queues still hold, could take any counter past 65535 (a term adds one to one
// counter of each position q, so a counter never exceeds the terms since the last flush).
#include "raw_stage.hpp"

#include <cmath>

namespace {

constexpr int kNQ = 4, kNL = 64, kNV = 272;
constexpr int kNRows = kNQ * kNL;
constexpr int kNRowWords = kNV / 2;            // 32-bit words of a row in LDS: bins w (low half) and w + 136 (high half)
constexpr int kTempThreads = 1024;
constexpr int kTempWaves = kTempThreads / 64;
constexpr unsigned kTempMaxTerms = 65535;      // accepted terms between two flushes: a 16-bit counter cannot overflow
constexpr int kTempTile = 4;                   // frames j whose placements a lane holds in registers
constexpr int kTempAhead = 8;                  // frames k whose placement is loaded and tested together against them
constexpr int kTempQueue = 128;                // items of a wave's queue: below 64 before a step, at most 64 more after it
constexpr float kTempMaxShift = 16384.0f;      // |0.5 * flow| beyond this (or not finite): the frame is not placed at the block

struct FlowTable {
    const float2* p[kRawMaxFrames];            // NULL: zero flow
};

struct TemporalGeom {
    int n;                   // frames
    int pitch;               // bytes
    int width, height;
    int bx0, by0, nbx, nby;  // rectangle in blocks
    unsigned total, chunk;   // blocks of the launch, blocks per workgroup
    int flowW, flowH, flowPitch;
    float tol;
    int black16[4];          // 16 * black[q]
    int span[4];             // 16 * (sat - black[q])
    float inv[4];            // 64 / span[q]
    int sat;
};

// where the lane's block lies and which texel of a flow field it reads (a byte offset)
__device__ __forceinline__ void temporal_block(const TemporalGeom& g, unsigned i, int& bx, int& by, size_t& texel)
{
    by = g.by0 + (int)(i / (unsigned)g.nbx);
    bx = g.bx0 + (int)(i % (unsigned)g.nbx);
    const int fx = (int)(((long long)(8 * bx + 4) * g.flowW) / g.width), fy = (int)(((long long)(8 * by + 4) * g.flowH) / g.height);
    texel = (size_t)fy * (size_t)g.flowPitch + 8 * (size_t)fx;
}

// 0.5 * the block's texel of the flow field p (NULL: zero flow); placed: finite and within kTempMaxShift
__device__ __forceinline__ bool temporal_place(const float2* p, size_t texel, float2& h)
{
    h = make_float2(0.0f, 0.0f);
    if (p == nullptr) return true;
    const float2 v = *(const float2*)((const char*)p + texel);
    const float2 t = make_float2(0.5f * v.x, 0.5f * v.y);
    const bool placed = fabsf(t.x) <= kTempMaxShift && fabsf(t.y) <= kTempMaxShift;  // (false for NaN and for +-inf)
    if (placed) h = t;                                           // (no site is derived from any other texel)
    return placed;
}

// the sites of a pair at block (bx, by): A's origin from hj, B's from d = hk - hj; whether d is within tol of a whole number of
// quads on both axes (false for a tie of roundf: tol < 0.5) and both blocks lie inside the frame
__device__ __forceinline__ bool temporal_sites(const TemporalGeom& g, int bx, int by, float2 hj, float2 hk, int& ax, int& ay, int& cx, int& cy)
{
    ax = 8 * bx + 2 * (int)roundf(hj.x);
    ay = 8 * by + 2 * (int)roundf(hj.y);
    const float dx = hk.x - hj.x, dy = hk.y - hj.y;
    const float rx = roundf(dx), ry = roundf(dy);
    cx = ax + 2 * (int)rx;
    cy = ay + 2 * (int)ry;
    const bool phase = fabsf(dx - rx) <= g.tol && fabsf(dy - ry) <= g.tol;
    const bool inside = ax >= 0 && ax + 8 <= g.width && ay >= 0 && ay + 8 <= g.height && cx >= 0 && cx + 8 <= g.width && cy >= 0 &&
                        cy + 8 <= g.height;
    return phase && inside;
}

// row k of the 8 x 8 samples at p: 4 words, x even in the low half
template <bool ALIGN4>
__device__ __forceinline__ uint4 temporal_row(const char* p, int pitch, int k)
{
    const char* row = p + (size_t)k * (size_t)pitch;
    if (ALIGN4) {
        const uint32_t* s = (const uint32_t*)row;
        return make_uint4(s[0], s[1], s[2], s[3]);
    }
    const uint16_t* s = (const uint16_t*)row;
    return make_uint4((uint32_t)s[0] | ((uint32_t)s[1] << 16), (uint32_t)s[2] | ((uint32_t)s[3] << 16),
                      (uint32_t)s[4] | ((uint32_t)s[5] << 16), (uint32_t)s[6] | ((uint32_t)s[7] << 16));
}

// every non-zero counter to the tables with one atomic, a row's term count and level sum with one each; `clear`: the counters
// are zeroed for the terms that follow (the caller puts a barrier before and after)
__device__ __forceinline__ void temporal_flush(uint32_t* sHist, unsigned long long* sSum, uint32_t* hist, unsigned long long* levelSum,
                                               unsigned long long* count, bool clear)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int row = wave; row < kNRows; row += kTempWaves) {
        uint32_t n = 0;
#pragma unroll
        for (int k = 0; k < (kNRowWords + 63) / 64; k++) {
            const int w = 64 * k + lane;
            const uint32_t c = w < kNRowWords ? sHist[row * kNRowWords + w] : 0u;
            const uint32_t lo = c & 0xffffu, hi = c >> 16;
            if (lo) atomicAdd(&hist[(size_t)row * kNV + w], lo);
            if (hi) atomicAdd(&hist[(size_t)row * kNV + kNRowWords + w], hi);
            if (clear && c) sHist[row * kNRowWords + w] = 0;
            n += lo + hi;
        }
        n = wave_sum(n);
        if (lane == 0 && n != 0) {
            atomicAdd(&count[row], (unsigned long long)n);
            atomicAdd(&levelSum[row], sSum[row]);
            if (clear) sSum[row] = 0;
        }
    }
}

// The first `cnt` (1 .. 64) items of the wave's queue, one per lane: the lane finds its block's two sites again, loads the 16
// rows, reduces them and the wave adds the terms to the LDS histogram.  Returns the terms added (uniform over the wave).
template <bool ALIGN4>
__device__ __forceinline__ unsigned temporal_drain(const TemporalGeom& g, const uint16_t* const* sFrames, const float2* const* sFlows,
                                                   const uint2* queue, unsigned cnt, uint32_t* sHist, unsigned long long* sSum)
{
    const int lane = threadIdx.x & 63;
    uint32_t S[4] = {0, 0, 0, 0}, top = 0xffffffffu;
    unsigned long long D[4] = {0, 0, 0, 0};
    if ((unsigned)lane < cnt) {
        const uint2 item = queue[lane];
        const int j = (int)(item.y & 0xffu), k = (int)(item.y >> 8);
        int bx, by, ax, ay, cx, cy;
        size_t texel;
        float2 hj, hk;
        temporal_block(g, item.x, bx, by, texel);
        temporal_place(sFlows[j], texel, hj);
        temporal_place(sFlows[k], texel, hk);
        if (temporal_sites(g, bx, by, hj, hk, ax, ay, cx, cy)) {  // (it was when the item was queued: the same arithmetic)
            const char* pa = (const char*)sFrames[j] + (size_t)ay * (size_t)g.pitch + 2 * (size_t)ax;
            const char* pb = (const char*)sFrames[k] + (size_t)cy * (size_t)g.pitch + 2 * (size_t)cx;
            top = 0;
#pragma unroll 2                                                 // (a quad row's 4 loads in flight: all 16 would not fit the registers)
            for (int r = 0; r < 8; r++) {
                const int q = 2 * (r & 1);                       // row parity: positions q (x even) and q + 1 (x odd)
                const uint4 A = temporal_row<ALIGN4>(pa, g.pitch, r), B = temporal_row<ALIGN4>(pb, g.pitch, r);
                const uint32_t wa[4] = {A.x, A.y, A.z, A.w};
                const uint32_t wb[4] = {B.x, B.y, B.z, B.w};
                int te[4], to[4];
                uint32_t se = 0, so = 0;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const uint32_t ae = wa[c] & 0xffffu, ao = wa[c] >> 16, be = wb[c] & 0xffffu, bo = wb[c] >> 16;
                    top = max(top, max(max(ae, ao), max(be, bo)));
                    se += ae;
                    so += ao;
                    te[c] = (int)ae - (int)be;
                    to[c] = (int)ao - (int)bo;
                }
                S[q] += se;
                S[q + 1] += so;
                const long long de0 = te[0] - te[1], de1 = te[2] - te[3];  // (|.| <= 131070: the square needs 64 bits)
                const long long do0 = to[0] - to[1], do1 = to[2] - to[3];
                D[q] += (unsigned long long)(de0 * de0) + (unsigned long long)(de1 * de1);
                D[q + 1] += (unsigned long long)(do0 * do0) + (unsigned long long)(do1 * do1);
            }
        }
    }
    const bool ok = top < (uint32_t)g.sat;                       // (a lane without an item: top = 2^32 - 1)
    const unsigned long long okMask = __ballot(ok);
    if (okMask == 0) return 0;                                   // (uniform over the wave)
    const int first = __ffsll((long long)okMask) - 1;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        // level bin: floor(t * 64 / span), t < span <= 2^20 -- a float estimate (off by at most one), made exact
        const uint32_t t = (uint32_t)clampi((int)S[q] - g.black16[q], 0, g.span[q] - 1);
        uint32_t l = (uint32_t)((float)t * g.inv[q]);
        l = min(l, 63u);
        l -= (l * (uint32_t)g.span[q] > 64u * t) ? 1u : 0u;
        l += ((l + 1u) * (uint32_t)g.span[q] <= 64u * t) ? 1u : 0u;
        // variance bin: D below 16, then 8 sub-bins per octave; D reaches 2^38, the last bin takes what is beyond its range
        const int ex = 63 - __clzll((long long)(D[q] | 1ull));
        uint32_t v = D[q] < 16ull ? (uint32_t)D[q] : (uint32_t)(16 + 8 * (ex - 4)) + (uint32_t)((D[q] >> (ex - 3)) & 7ull);
        v = min(v, (uint32_t)(kNV - 1));
        const uint32_t row = (uint32_t)q * kNL + l;
        const uint32_t key = row * kNV + v;
        const uint32_t word = row * kNRowWords + (v >= (uint32_t)kNRowWords ? v - kNRowWords : v);
        const uint32_t one = v >= (uint32_t)kNRowWords ? 0x10000u : 1u;
        const uint32_t row0 = __shfl(row, first), key0 = __shfl(key, first);
        const bool sameRow = __ballot(ok && row != row0) == 0, sameKey = __ballot(ok && key != key0) == 0;
        if (sameRow) {                                           // one level for the whole wave: one add of the wave's sum
            const uint32_t s = wave_sum(ok ? S[q] : 0u);
            if (lane == first) atomicAdd(&sSum[row], (unsigned long long)s);
        } else if (ok)
            atomicAdd(&sSum[row], (unsigned long long)S[q]);
        if (sameKey) {                                           // (at most 64 in one add, within the bound on the terms)
            if (lane == first) atomicAdd(&sHist[word], one * (uint32_t)__popcll(okMask));
        } else if (ok)
            atomicAdd(&sHist[word], one);
    }
    return (unsigned)__popcll(okMask);
}

template <bool ALIGN4>
__global__ __launch_bounds__(kTempThreads) void k_noiseStatsTemporal(RawFrames frames, FlowTable flows, TemporalGeom g, uint32_t* hist,
                                                                      unsigned long long* levelSum, unsigned long long* count)
{
    __shared__ uint32_t sHist[kNRows * kNRowWords];
    __shared__ unsigned long long sSum[kNRows];
    __shared__ uint2 sQueue[kTempWaves][kTempQueue];             // per wave: accepted (block, j | k << 8)
    __shared__ const uint16_t* sFrames[kRawMaxFrames];           // the two tables, for lanes that index them on their own
    __shared__ const float2* sFlows[kRawMaxFrames];
    __shared__ unsigned sTerms;                                  // terms added since the last flush
    for (int k = threadIdx.x; k < kNRows * kNRowWords; k += kTempThreads) sHist[k] = 0;
    for (int k = threadIdx.x; k < kNRows; k += kTempThreads) sSum[k] = 0;
    if (threadIdx.x < kRawMaxFrames) {
        sFrames[threadIdx.x] = frames.p[threadIdx.x];
        sFlows[threadIdx.x] = flows.p[threadIdx.x];
    }
    if (threadIdx.x == 0) sTerms = 0;
    __syncthreads();

    const unsigned c0 = blockIdx.x * g.chunk;                    // (the host makes every chunk non-empty)
    const unsigned c1 = min(c0 + g.chunk, g.total);
    const int lane = threadIdx.x & 63;
    uint2* queue = sQueue[threadIdx.x >> 6];
    unsigned queued = 0;                                         // items in the wave's queue (uniform over the wave, below 64
                                                                 // between two steps)
    // Before a step that can queue `fresh` items: the terms it can add are those and what the 16 queues still hold.  Where
    // that could take a counter past its range, the histogram goes to memory first.  Uniform over the workgroup.
    auto make_room = [&](unsigned fresh) {
        const unsigned before = sTerms;
        __syncthreads();                                         // (every wave has read sTerms before any wave adds to it)
        if (before + (unsigned)(kTempWaves * 63) + fresh > kTempMaxTerms) {
            temporal_flush(sHist, sSum, hist, levelSum, count, true);
            if (threadIdx.x == 0) sTerms = 0;
            __syncthreads();
        }
    };
    for (unsigned i0 = c0; i0 < c1; i0 += kTempThreads) {        // (uniform over the workgroup)
        const unsigned live = min(c1 - i0, (unsigned)kTempThreads);
        const bool valid = threadIdx.x < live;
        const unsigned i = valid ? i0 + threadIdx.x : c1 - 1;    // (a lane past the end re-reads the last block's texels)
        int bx, by;
        size_t texel;
        temporal_block(g, i, bx, by, texel);
        for (int j0 = 0; j0 + 1 < g.n; j0 += kTempTile) {        // (uniform) a tile of frames j, their placements in registers
            float2 hj[kTempTile];
            bool placedJ[kTempTile];
#pragma unroll
            for (int t = 0; t < kTempTile; t++)
                placedJ[t] = temporal_place(flows.p[min(j0 + t, g.n - 1)], texel, hj[t]) && valid && j0 + t < g.n;
            for (int k0 = j0 + 1; k0 < g.n; k0 += kTempAhead) {  // (uniform) kTempAhead frames k against the tile
                make_room(live * (unsigned)(kTempTile * kTempAhead));
                // the pair tests of the step at once: the texel loads of its frames are in flight together, and a wave that
                // accepts nothing -- the common case -- goes on after one wait
                uint32_t mine = 0, any = 0;                      // bit kTempAhead * t + u: the pair (j0 + t, k0 + u)
                {
                    float2 hk[kTempAhead];
                    bool placedK[kTempAhead];
#pragma unroll
                    for (int u = 0; u < kTempAhead; u++)
                        placedK[u] = temporal_place(flows.p[min(k0 + u, g.n - 1)], texel, hk[u]) && k0 + u < g.n;
#pragma unroll
                    for (int t = 0; t < kTempTile; t++)
#pragma unroll
                        for (int u = 0; u < kTempAhead; u++) {
                            int ax, ay, cx, cy;
                            const bool acc = placedJ[t] && placedK[u] && k0 + u > j0 + t && temporal_sites(g, bx, by, hj[t], hk[u], ax, ay, cx, cy);
                            mine |= (acc ? 1u : 0u) << (kTempAhead * t + u);
                            any |= (__ballot(acc) != 0 ? 1u : 0u) << (kTempAhead * t + u);
                        }
                }
                // accepted pairs go to the wave's queue, and every 64 of them are worked off one per lane: under rotation the
                // lanes accept different pairs, and the 16 row loads of a pair would otherwise run for one lane at a time
                unsigned terms = 0;                              // of this wave in this step
                for (uint32_t rest = any; rest != 0; rest &= rest - 1u) {  // (uniform)
                    const int bit = __ffs((int)rest) - 1;
                    const unsigned pair = (unsigned)(j0 + bit / kTempAhead) | ((unsigned)(k0 + bit % kTempAhead) << 8);
                    const bool acc = ((mine >> bit) & 1u) != 0;
                    const unsigned long long mask = __ballot(acc);
                    if (acc) queue[queued + (unsigned)__popcll(mask & ((1ull << lane) - 1ull))] = make_uint2(i, pair);
                    queued += (unsigned)__popcll(mask);
                    if (queued >= 64u) {
                        __threadfence_block();                   // (the wave's own writes, before its lanes read each other's)
                        terms += temporal_drain<ALIGN4>(g, sFrames, sFlows, queue, 64u, sHist, sSum);
                        const unsigned left = queued - 64u;      // below 64: they move to the front
                        uint2 keep = make_uint2(0u, 0u);
                        if ((unsigned)lane < left) keep = queue[64 + lane];
                        __threadfence_block();
                        if ((unsigned)lane < left) queue[lane] = keep;
                        queued = left;
                    }
                }
                if (lane == 0 && terms != 0) atomicAdd(&sTerms, terms);
                __syncthreads();                                 // (sTerms is complete before the next step reads it)
            }
        }
    }
    make_room(0u);
    __threadfence_block();
    if (queued != 0) temporal_drain<ALIGN4>(g, sFrames, sFlows, queue, queued, sHist, sSum);
    __syncthreads();
    temporal_flush(sHist, sSum, hist, levelSum, count, false);
}

}  // namespace

extern "C" int mfsr_noiseStatsTemporal(int nFrames, const uint16_t* const* frames, int rowBytes, int w, int h,
                                       const mfsr_float2* const* flows, int flowRowBytes, int flowW, int flowH, const int32_t black[4],
                                       int sat, const int32_t rect[4], float tol, uint32_t* histDev, long long* levelSumDev,
                                       long long* countDev, mfsr_stream_t stream)
{
    const int pitch = rowBytes, width = w, height = h, flowPitch = flowRowBytes;
    // host validation first: nothing below touches the device before every argument has passed
    MFSR_REQUIRE(nFrames >= 2);
    MFSR_REQUIRE(raw_even_ok(width, height) && raw_frames_ok(nFrames, kRawMaxFrames, frames, pitch, width));
    MFSR_REQUIRE(flows != nullptr);
    MFSR_REQUIRE((flowW == width / 2 && flowH == height / 2) || (flowW == width && flowH == height));
    MFSR_REQUIRE((long long)flowPitch >= 8LL * flowW && (flowPitch & 7) == 0);
    for (int k = 0; k < nFrames; k++) MFSR_REQUIRE(((uintptr_t)flows[k] & 7) == 0);
    MFSR_REQUIRE(tol >= 0.0f && tol <= 0.25f);  // (false for NaN)
    MFSR_REQUIRE(0 < sat && sat <= 65535 && black != nullptr);
    for (int q = 0; q < 4; q++) MFSR_REQUIRE(black[q] >= 0 && black[q] < sat);
    MFSR_REQUIRE(rect != nullptr && histDev != nullptr && levelSumDev != nullptr && countDev != nullptr);
    MFSR_REQUIRE(((uintptr_t)histDev & 3) == 0 && ((uintptr_t)levelSumDev & 7) == 0 && ((uintptr_t)countDev & 7) == 0);
    const int gw = width / 8, gh = height / 8;  // the block grid: a partial block at the right or bottom edge is not in it
    const int bx0 = rect[0], by0 = rect[1], bx1 = rect[2], by1 = rect[3];
    MFSR_REQUIRE(bx0 >= 0 && bx0 < bx1 && bx1 <= gw && by0 >= 0 && by0 < by1 && by1 <= gh);
    const long long total = (long long)(bx1 - bx0) * (by1 - by0);
    const long long pairs = (long long)nFrames * (nFrames - 1) / 2;
    MFSR_REQUIRE(total < (1LL << 31) && pairs * total < (1LL << 31));  // (the u32 histogram cannot overflow)
    const bool aligned4 = raw_aligned(nFrames, frames, pitch, 4);
    const RawFrames t = raw_table(nFrames, frames);
    FlowTable ft = {};
    for (int k = 0; k < nFrames; k++) ft.p[k] = (const float2*)flows[k];

    TemporalGeom g;
    g.n = nFrames;
    g.pitch = pitch;
    g.width = width;
    g.height = height;
    g.bx0 = bx0;
    g.by0 = by0;
    g.nbx = bx1 - bx0;
    g.nby = by1 - by0;
    g.total = (unsigned)total;
    g.flowW = flowW;
    g.flowH = flowH;
    g.flowPitch = flowPitch;
    g.tol = tol;
    for (int q = 0; q < 4; q++) {
        g.black16[q] = 16 * black[q];
        g.span[q] = 16 * (sat - black[q]);
        g.inv[q] = 64.0f / (float)g.span[q];
    }
    g.sat = sat;
    // one chunk per CU, no workgroup without a full round of blocks
    long long groups = mfsr_device_cus();
    const long long rounds = (total + kTempThreads - 1) / kTempThreads;
    groups = groups < rounds ? groups : rounds;
    g.chunk = (unsigned)((total + groups - 1) / groups);
    const unsigned blocks = (unsigned)((total + g.chunk - 1) / g.chunk);  // every chunk non-empty

    MFSR_HIP_TRY(hipMemsetAsync(histDev, 0, sizeof(uint32_t) * kNRows * kNV, mfsr_s(stream)));
    MFSR_HIP_TRY(hipMemsetAsync(levelSumDev, 0, sizeof(long long) * kNRows, mfsr_s(stream)));
    MFSR_HIP_TRY(hipMemsetAsync(countDev, 0, sizeof(long long) * kNRows, mfsr_s(stream)));
    const dim3 grid(blocks), block(kTempThreads);
    if (aligned4)
        hipLaunchKernelGGL(k_noiseStatsTemporal<true>, grid, block, 0, mfsr_s(stream), t, ft, g, histDev,
                           (unsigned long long*)levelSumDev, (unsigned long long*)countDev);
    else
        hipLaunchKernelGGL(k_noiseStatsTemporal<false>, grid, block, 0, mfsr_s(stream), t, ft, g, histDev,
                           (unsigned long long*)levelSumDev, (unsigned long long*)countDev);
    return mfsr_launch_status("k_noiseStatsTemporal");
}
