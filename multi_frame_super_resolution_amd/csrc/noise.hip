// noise.hip -- noise-model calibration: block statistics of raw frames on the device, and the fit of the affine noise model
// var = alpha * I + beta from them on the host.
//
// The rule is stated in include/mfsr.h (mfsr_noiseStats / mfsr_noise_fit).  The device stage is exact integer arithmetic: its
// three tables equal the numpy restatement of the tests bit for bit, for any launch shape.
//
// Shape (k_noiseStats): the blocks of the rectangle of all frames are numbered frame by frame, row by row, and cut into one
// contiguous chunk per workgroup (one workgroup of 16 waves per CU, as many workgroups as CUs).  One lane owns one block (8
// raw rows x one 16-byte load, adjacent lanes adjacent blocks: 1 KiB per wave and row); the 8 rows of its next block are in
// flight while a block is reduced, and every load is unconditional (a lane past the chunk's end re-reads the chunk's last
// block and takes no part in the updates).
// Updates never go to memory one by one.  Each workgroup keeps the whole histogram in LDS as 16-bit counters, two to a
// 32-bit word (4 x 64 x 272 x 2 B = 136 KiB; a chunk has at most 65535 blocks, so no counter can overflow and no carry can
// cross into the neighbour), plus the 256 level sums as 64-bit words, and adds into them with LDS atomics.  A wave whose 64
// blocks all fall on one key (a flat, clipped or synthetic frame: the contention case) adds once, from one lane.  At the end
// of its chunk the workgroup adds every non-zero counter to the tables in memory with one vector atomic each; the block count
// of a (q, level) row is the sum of the row's counters, taken in the same sweep.  Word w of a row holds bins w and w + 136, so
// that the lanes of one atomic instruction address one contiguous run and the half of a row an image does not reach (its
// variances span a few octaves) costs no instruction at all.
#include "raw_stage.hpp"

#include <cmath>

namespace {

constexpr int kNQ = 4, kNL = 64, kNV = 272;
constexpr int kNRows = kNQ * kNL;              // (q, level) rows of the tables
constexpr int kNRowWords = kNV / 2;            // 32-bit words of a row in LDS: bins w (low half) and w + 136 (high half)
constexpr int kNoiseThreads = 1024;
constexpr int kNoiseWaves = kNoiseThreads / 64;
constexpr int kNoiseMaxChunk = 65535;          // blocks per workgroup: a 16-bit counter cannot overflow
constexpr double kChi2x2 = 14.6882;            // 2 x the median of chi-square with 8 degrees of freedom
constexpr double kChi2x2Temporal = 29.3764;    // 4 x that median: D of a difference of two frames

struct NoiseGeom {
    int pitch;               // bytes
    int bx0, by0, nbx, nby;  // rectangle in blocks
    unsigned total, chunk;   // blocks of the launch, blocks per workgroup
    int black16[4];          // 16 * black[q]
    int span[4];             // 16 * (sat - black[q])
    float inv[4];            // 64 / span[q]
    int sat;
};

// raw rows 8*by .. 8*by + 7 of block i (one 16-byte piece each: 4 words, x even in the low half)
template <bool VEC>
__device__ __forceinline__ void noise_load(const RawFrames& frames, const NoiseGeom& g, unsigned i, uint4 r[8])
{
    const unsigned perFrame = (unsigned)g.nbx * (unsigned)g.nby;
    const unsigned f = i / perFrame, j = i - f * perFrame;
    const unsigned by = j / (unsigned)g.nbx, bx = j - by * (unsigned)g.nbx;
    const char* p = (const char*)frames.p[f] + (size_t)(8 * (g.by0 + (int)by)) * (size_t)g.pitch + 16 * (size_t)(g.bx0 + (int)bx);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const char* row = p + (size_t)k * (size_t)g.pitch;
        if (VEC)
            r[k] = *(const uint4*)row;
        else {
            const uint16_t* s = (const uint16_t*)row;
            r[k] = make_uint4((uint32_t)s[0] | ((uint32_t)s[1] << 16), (uint32_t)s[2] | ((uint32_t)s[3] << 16),
                              (uint32_t)s[4] | ((uint32_t)s[5] << 16), (uint32_t)s[6] | ((uint32_t)s[7] << 16));
        }
    }
}

// VEC: every frame pointer and the pitch are 16-byte aligned (16-byte loads); otherwise 16-bit loads
template <bool VEC>
__global__ __launch_bounds__(kNoiseThreads) void k_noiseStats(RawFrames frames, NoiseGeom g, uint32_t* hist,
                                                               unsigned long long* levelSum, unsigned long long* count)
{
    __shared__ uint32_t sHist[kNRows * kNRowWords];
    __shared__ unsigned long long sSum[kNRows];
    for (int k = threadIdx.x; k < kNRows * kNRowWords; k += kNoiseThreads) sHist[k] = 0;
    for (int k = threadIdx.x; k < kNRows; k += kNoiseThreads) sSum[k] = 0;
    __syncthreads();

    const unsigned c0 = blockIdx.x * g.chunk;                    // (the host makes every chunk non-empty)
    const unsigned c1 = min(c0 + g.chunk, g.total);
    const int lane = threadIdx.x & 63;
    uint4 cur[8], nxt[8];
    noise_load<VEC>(frames, g, min(c0 + threadIdx.x, c1 - 1), cur);
    for (unsigned i0 = c0; i0 < c1; i0 += kNoiseThreads) {       // (uniform over the workgroup)
        const unsigned i = i0 + threadIdx.x;
        noise_load<VEC>(frames, g, min(i + kNoiseThreads, c1 - 1), nxt);
        // a block: S and D of its four quad positions, and whether all 64 samples are below sat
        uint32_t S[4] = {0, 0, 0, 0}, top = 0;
        unsigned long long D[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int q = 2 * (k & 1);                           // row parity: positions q (x even) and q + 1 (x odd)
            const uint32_t w[4] = {cur[k].x, cur[k].y, cur[k].z, cur[k].w};
            int e[4], o[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                e[c] = (int)(w[c] & 0xffffu);
                o[c] = (int)(w[c] >> 16);
                top = max(top, (uint32_t)max(e[c], o[c]));
            }
            S[q] += (uint32_t)(e[0] + e[1] + e[2] + e[3]);
            S[q + 1] += (uint32_t)(o[0] + o[1] + o[2] + o[3]);
            const uint32_t de0 = (uint32_t)abs(e[0] - e[1]), de1 = (uint32_t)abs(e[2] - e[3]);
            const uint32_t do0 = (uint32_t)abs(o[0] - o[1]), do1 = (uint32_t)abs(o[2] - o[3]);
            D[q] += (unsigned long long)de0 * de0;               // (each square is below 2^32, the sum of 8 is not)
            D[q] += (unsigned long long)de1 * de1;
            D[q + 1] += (unsigned long long)do0 * do0;
            D[q + 1] += (unsigned long long)do1 * do1;
        }
        const bool ok = i < c1 && top < (uint32_t)g.sat;
        const unsigned long long okMask = __ballot(ok);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            // level bin: floor(t * 64 / span), t < span <= 2^20 -- a float estimate (off by at most one), made exact
            const uint32_t t = (uint32_t)clampi((int)S[q] - g.black16[q], 0, g.span[q] - 1);
            uint32_t l = (uint32_t)((float)t * g.inv[q]);
            l = min(l, 63u);
            l -= (l * (uint32_t)g.span[q] > 64u * t) ? 1u : 0u;
            l += ((l + 1u) * (uint32_t)g.span[q] <= 64u * t) ? 1u : 0u;
            // variance bin: D below 16, then 8 sub-bins per octave
            const int ex = 63 - __clzll((long long)(D[q] | 1ull));
            const uint32_t v = D[q] < 16ull ? (uint32_t)D[q] : (uint32_t)(16 + 8 * (ex - 4)) + (uint32_t)((D[q] >> (ex - 3)) & 7ull);
            const uint32_t row = (uint32_t)q * kNL + l;
            const uint32_t key = row * kNV + v;
            const uint32_t word = row * kNRowWords + (v >= (uint32_t)kNRowWords ? v - kNRowWords : v);
            const uint32_t one = v >= (uint32_t)kNRowWords ? 0x10000u : 1u;
            if (okMask == 0) continue;                           // (uniform over the wave)
            const int first = __ffsll((long long)okMask) - 1;
            const uint32_t row0 = __shfl(row, first), key0 = __shfl(key, first);
            const bool sameRow = __ballot(ok && row != row0) == 0, sameKey = __ballot(ok && key != key0) == 0;
            if (sameRow) {                                       // one level for the whole wave: one add of the wave's sum
                const uint32_t s = wave_sum(ok ? S[q] : 0u);
                if (lane == first) atomicAdd(&sSum[row], (unsigned long long)s);
            } else if (ok)
                atomicAdd(&sSum[row], (unsigned long long)S[q]);
            if (sameKey) {                                       // (then at most 64 in one add: no carry, as below)
                if (lane == first) atomicAdd(&sHist[word], one * (uint32_t)__popcll(okMask));
            } else if (ok)
                atomicAdd(&sHist[word], one);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) cur[k] = nxt[k];
    }
    __syncthreads();

    // flush: every non-zero counter with one atomic, a row's block count and level sum with one each
    const int wave = threadIdx.x >> 6;
    for (int row = wave; row < kNRows; row += kNoiseWaves) {
        uint32_t n = 0;
#pragma unroll
        for (int k = 0; k < (kNRowWords + 63) / 64; k++) {
            const int w = 64 * k + lane;
            const uint32_t c = w < kNRowWords ? sHist[row * kNRowWords + w] : 0u;
            const uint32_t lo = c & 0xffffu, hi = c >> 16;
            if (lo) atomicAdd(&hist[(size_t)row * kNV + w], lo);
            if (hi) atomicAdd(&hist[(size_t)row * kNV + kNRowWords + w], hi);
            n += lo + hi;
        }
        n = wave_sum(n);
        if (lane == 0 && n != 0) {
            atomicAdd(&count[row], (unsigned long long)n);
            atomicAdd(&levelSum[row], sSum[row]);
        }
    }
}

// [lo, hi) of the D values of variance bin v
void noise_bin_bounds(int v, double& lo, double& hi)
{
    if (v < 16) {
        lo = (double)v;
        hi = (double)(v + 1);
        return;
    }
    const int e = 4 + (v - 16) / 8, m = (v - 16) % 8;
    lo = (double)((long long)(8 + m) << (e - 3));
    hi = (double)((long long)(9 + m) << (e - 3));
}

}  // namespace

extern "C" int mfsr_noiseStats(int nFrames, const uint16_t* const* frames, int pitch, int width, int height, const int32_t black[4],
                               int sat, const int32_t rect[4], uint32_t* histDev, long long* levelSumDev, long long* countDev,
                               mfsr_stream_t stream)
{
    // host validation first: nothing below touches the device before every argument has passed
    MFSR_REQUIRE(raw_even_ok(width, height) && raw_frames_ok(nFrames, kRawMaxFrames, frames, pitch, width));
    MFSR_REQUIRE(0 < sat && sat <= 65535 && black != nullptr);
    for (int q = 0; q < 4; q++) MFSR_REQUIRE(black[q] >= 0 && black[q] < sat);
    MFSR_REQUIRE(rect != nullptr && histDev != nullptr && levelSumDev != nullptr && countDev != nullptr);
    MFSR_REQUIRE(((uintptr_t)histDev & 3) == 0 && ((uintptr_t)levelSumDev & 7) == 0 && ((uintptr_t)countDev & 7) == 0);
    const int gw = width / 8, gh = height / 8;  // the block grid: a partial block at the right or bottom edge is not in it
    const int bx0 = rect[0], by0 = rect[1], bx1 = rect[2], by1 = rect[3];
    MFSR_REQUIRE(bx0 >= 0 && bx0 < bx1 && bx1 <= gw && by0 >= 0 && by0 < by1 && by1 <= gh);
    const bool aligned16 = raw_aligned(nFrames, frames, pitch, 16);
    const RawFrames t = raw_table(nFrames, frames);
    const long long total = (long long)nFrames * (bx1 - bx0) * (by1 - by0);
    MFSR_REQUIRE(total < (1LL << 31));

    NoiseGeom g;
    g.pitch = pitch;
    g.bx0 = bx0;
    g.by0 = by0;
    g.nbx = bx1 - bx0;
    g.nby = by1 - by0;
    g.total = (unsigned)total;
    for (int q = 0; q < 4; q++) {
        g.black16[q] = 16 * black[q];
        g.span[q] = 16 * (sat - black[q]);
        g.inv[q] = 64.0f / (float)g.span[q];
    }
    g.sat = sat;
    // one chunk per CU, no chunk longer than a 16-bit counter holds, no workgroup without a full round of blocks
    long long groups = mfsr_device_cus();
    const long long rounds = (total + kNoiseThreads - 1) / kNoiseThreads;
    groups = groups < rounds ? groups : rounds;
    const long long need = (total + kNoiseMaxChunk - 1) / kNoiseMaxChunk;
    groups = groups > need ? groups : need;
    g.chunk = (unsigned)((total + groups - 1) / groups);
    const unsigned blocks = (unsigned)((total + g.chunk - 1) / g.chunk);  // every chunk non-empty

    MFSR_HIP_TRY(hipMemsetAsync(histDev, 0, sizeof(uint32_t) * kNRows * kNV, mfsr_s(stream)));
    MFSR_HIP_TRY(hipMemsetAsync(levelSumDev, 0, sizeof(long long) * kNRows, mfsr_s(stream)));
    MFSR_HIP_TRY(hipMemsetAsync(countDev, 0, sizeof(long long) * kNRows, mfsr_s(stream)));
    const dim3 grid(blocks), block(kNoiseThreads);
    if (aligned16)
        hipLaunchKernelGGL(k_noiseStats<true>, grid, block, 0, mfsr_s(stream), t, g, histDev, (unsigned long long*)levelSumDev,
                           (unsigned long long*)countDev);
    else
        hipLaunchKernelGGL(k_noiseStats<false>, grid, block, 0, mfsr_s(stream), t, g, histDev, (unsigned long long*)levelSumDev,
                           (unsigned long long*)countDev);
    return mfsr_launch_status("k_noiseStats");
}

// Host only.  The operations, one by one, are those of DESIGN.md §2.15 (the tests restate them in numpy).  divisor: what the
// median of D is divided by to give the variance -- kChi2x2 for the blocks of one frame, twice that for the difference of two
// frames (§2.22: the pair differences of a difference have four times the variance, mfsr_noise_fit_temporal).
static int noise_fit_rule(const uint32_t* hist, const long long* levelSum, const long long* count, const int32_t black[4],
                          const float white[4], int minBlocks, double divisor, double* alpha, double* beta, int32_t* status,
                          int32_t* points)
{
    MFSR_REQUIRE(hist != nullptr && levelSum != nullptr && count != nullptr && black != nullptr && white != nullptr);
    MFSR_REQUIRE(alpha != nullptr && beta != nullptr && status != nullptr);
    MFSR_REQUIRE(minBlocks >= 1);
    for (int q = 0; q < 4; q++) MFSR_REQUIRE(black[q] >= 0 && black[q] <= 65535 && white[q] > 0.0f && std::isfinite(white[q]));
    double sw = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, xmin = 0, xmax = 0;
    int n = 0;
    for (int q = 0; q < kNQ; q++)
        for (int l = 0; l < kNL; l++) {
            const long long c = count[q * kNL + l];
            if (c < (long long)minBlocks) continue;
            const uint32_t* h = hist + ((size_t)q * kNL + l) * kNV;
            const double rank = 0.5 * (double)c;
            double cum = 0, med = 0;
            bool found = false;
            for (int v = 0; v < kNV; v++) {
                const double hv = (double)h[v];
                if (hv > 0.0 && cum + hv >= rank) {
                    double lo, hi;
                    noise_bin_bounds(v, lo, hi);
                    med = lo + (rank - cum) / hv * (hi - lo);
                    found = true;
                    break;
                }
                cum += hv;
            }
            if (!found) continue;  // (a count the histogram does not back)
            const double varDn = med / divisor;
            const double wq = (double)white[q];
            const double x = ((double)levelSum[q * kNL + l] / (16.0 * (double)c) - (double)black[q]) / wq;
            const double t = varDn - 1.0 / 12.0;
            const double y = (t > 0.0 ? t : 0.0) / (wq * wq);
            const double w = (double)c;
            sw += w;
            sx += w * x;
            sy += w * y;
            sxx += w * x * x;
            sxy += w * x * y;
            xmin = n == 0 || x < xmin ? x : xmin;
            xmax = n == 0 || x > xmax ? x : xmax;
            n++;
        }
    if (points) *points = n;
    *alpha = 0.0;
    *beta = 0.0;
    if (n < 4 || xmax - xmin < 0.125) {
        *status = 2;
        return MFSR_OK;
    }
    const double den = sw * sxx - sx * sx;
    double a = (sw * sxy - sx * sy) / den;
    double b = (sy - a * sx) / sw;
    if (b < 0.0) {
        b = 0.0;
        a = sxy / sxx;
    }
    *alpha = a;
    *beta = b;
    *status = a > 0.0 ? 0 : 3;
    return MFSR_OK;
}

extern "C" int mfsr_noise_fit(const uint32_t* hist, const long long* levelSum, const long long* count, const int32_t black[4],
                              const float white[4], int minBlocks, double* alpha, double* beta, int32_t* status, int32_t* points)
{
    return noise_fit_rule(hist, levelSum, count, black, white, minBlocks, kChi2x2, alpha, beta, status, points);
}

extern "C" int mfsr_noise_fit_temporal(const uint32_t* hist, const long long* levelSum, const long long* count,
                                       const int32_t black[4], const float white[4], int minBlocks, double* alpha, double* beta,
                                       int32_t* status, int32_t* points)
{
    return noise_fit_rule(hist, levelSum, count, black, white, minBlocks, kChi2x2Temporal, alpha, beta, status, points);
}
