// image_stats.hip -- statistics of the merged image for auto white balance and auto tone: 12-bit
// codes of the pixel after step 1 of the rendered finish (section 2.19), two 4096-bin histograms (a luma key and the channel
// maximum), and channel sums over all pixels and over a "neutral" set.  The rule is stated in include/mfsr.h
// (mfsr_imageStats).  The codes come from float32 + - * with -ffp-contract=off (the Makefile) and everything after them is
// integer arithmetic, so the table equals the numpy restatement of the tests (tests/image_stats_ref.py) word for word, for any
// launch shape, and stripes or windows of an image add up to the whole image's table.  gfx950, wave64.
//
// Shape (k_imageStats, the structure of k_noiseStats): a read-only stream of 12 B (the image form) or 24 B (the finish form:
// accumulator and weight) per pixel.  One workgroup of 16 waves per CU takes a contiguous chunk of rows.  A lane owns four
// consecutive pixels of a row -- 48 contiguous bytes, three 16-byte loads where they are 16-byte aligned (a dense row whose
// first byte is), 12-byte loads otherwise or at a partial quad at the row's end.  Both histograms stay in LDS for the whole
// chunk as 32-bit counters (2 x 4096 x 4 B = 32 KiB; a launch has fewer than 2^31 pixels, so a counter cannot overflow) and are
// updated with LDS adds; when every live lane of a wave holds the same key (a flat, clipped or black image: 64 adds to one
// address would serialise) one lane adds the lane count.  The seven sums and the neutral count are kept per lane in 64 bits,
// reduced over the wave with shuffles and over the workgroup in LDS.  At the end of its chunk the workgroup sweeps the table
// once: contiguous lanes add the non-zero counters and the eight leading words to memory with 64-bit vector atomic adds.
#include "stats_common.hpp"

namespace {

constexpr int kBins = 4096;                    // codes 0 .. 4095

static_assert(MFSR_IMAGE_STATS_WORDS == 8 + 2 * kBins, "the table of include/mfsr.h");

struct StatsArgs {
    float m[9];
    int useMatrix;
    int lo, hi, chromaTol;
    int width, height, pitch;                  // of the launch; pitch of `in`, or of the accumulator and the weight image
    int rowsPerGroup;
};

// one LDS add per live lane, or one for the whole wave where every live lane holds the same key.  Called by all lanes of the
// wave (the ballots and the shuffle stay outside divergent code).
__device__ __forceinline__ void hist_add(uint32_t* hist, int key, bool live)
{
    const u64 mask = __ballot(live);
    if (mask == 0) return;                     // (uniform over the wave)
    const int first = __ffsll((long long)mask) - 1;
    const int key0 = __shfl(key, first);
    if (__ballot(live && key != key0) == 0) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[key0], (uint32_t)__popcll(mask));
    } else if (live)
        atomicAdd(&hist[key], 1u);
}

// FINISH = 0: `a` is the image.  FINISH = 1: `a` is the accumulator, `b` the weight image, and the pixel is finish_value's.
template <int FINISH>
__global__ void __launch_bounds__(kStatsThreads)
    k_imageStats(const pix3* __restrict__ a, const pix3* __restrict__ b, FinishSrc f, StatsArgs s, u64* __restrict__ stats)
{
    __shared__ uint32_t sHist[2 * kBins];      // the luma key's counters, then the maximum's
    __shared__ u64 sLead[8];                   // words 0 .. 7 of the table
    for (int k = threadIdx.x; k < 2 * kBins; k += kStatsThreads) sHist[k] = 0;
    if (threadIdx.x < 8) sLead[threadIdx.x] = 0;
    __syncthreads();

    const int r0 = blockIdx.x * s.rowsPerGroup;                  // (the host makes every chunk non-empty)
    const int r1 = min(r0 + s.rowsPerGroup, s.height);
    const unsigned upr = (unsigned)(s.width + kStatsPpl - 1) / kStatsPpl;  // quads of a row; upr * height < 2^31
    const unsigned q0 = (unsigned)r0 * upr, q1 = (unsigned)r1 * upr;
    u64 nNeutral = 0, sumN[3] = {0, 0, 0}, sumA[3] = {0, 0, 0};
    for (unsigned base = q0; base < q1; base += kStatsThreads) {  // (uniform over the workgroup)
        const unsigned u = base + threadIdx.x;
        const bool live = u < q1;
        int keyY[kStatsPpl], keyM[kStatsPpl];
        int x0 = 0;
        if (live) {
            const int y = (int)(u / upr);
            x0 = (int)(u % upr) * kStatsPpl;
            pix3 p[kStatsPpl];
            load_quad(row_ptr(a, s.pitch, y), x0, s.width, p);
            if (FINISH) {
                pix3 w[kStatsPpl];
                load_quad(row_ptr(b, s.pitch, y), x0, s.width, w);
#pragma unroll
                for (int k = 0; k < kStatsPpl; k++) p[k] = finish_value(p[k], w[k], x0 + k, y, f);
            }
#pragma unroll
            for (int k = 0; k < kStatsPpl; k++) {
                const pix3 q = s.useMatrix ? matrix_pixel(p[k], s.m) : p[k];  // uniform
                const int c0 = quantize1(q.x, kMaxCode), c1 = quantize1(q.y, kMaxCode), c2 = quantize1(q.z, kMaxCode);
                keyY[k] = (54 * c0 + 183 * c1 + 19 * c2 + 128) >> 8;
                const int hiC = max(c0, max(c1, c2)), loC = min(c0, min(c1, c2));
                keyM[k] = hiC;
                if (x0 + k < s.width) {
                    bool neutral = s.lo <= loC && hiC <= s.hi;
                    if (s.chromaTol > 0)
                        neutral = neutral && 256 * abs(c0 - c1) <= s.chromaTol * c1 && 256 * abs(c2 - c1) <= s.chromaTol * c1;
                    sumA[0] += (u64)c0;
                    sumA[1] += (u64)c1;
                    sumA[2] += (u64)c2;
                    if (neutral) {
                        nNeutral += 1;
                        sumN[0] += (u64)c0;
                        sumN[1] += (u64)c1;
                        sumN[2] += (u64)c2;
                    }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < kStatsPpl; k++) keyY[k] = keyM[k] = 0;
        }
#pragma unroll
        for (int k = 0; k < kStatsPpl; k++) {
            const bool in = live && x0 + k < s.width;
            hist_add(sHist, keyY[k], in);
            hist_add(sHist + kBins, keyM[k], in);
        }
    }
    // the lane sums: over the wave with shuffles, over the workgroup in LDS
    const u64 lead[8] = {0, wave_sum64(nNeutral), wave_sum64(sumN[0]), wave_sum64(sumN[1]), wave_sum64(sumN[2]),
                         wave_sum64(sumA[0]), wave_sum64(sumA[1]), wave_sum64(sumA[2])};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 1; k < 8; k++)
            if (lead[k]) atomicAdd(&sLead[k], lead[k]);
    }
    if (threadIdx.x == 0) sLead[0] = (u64)(r1 - r0) * (u64)s.width;
    __syncthreads();
    // one sweep: contiguous lanes, contiguous words
    if (threadIdx.x < 8 && sLead[threadIdx.x]) atomicAdd(&stats[threadIdx.x], sLead[threadIdx.x]);
    for (int k = threadIdx.x; k < 2 * kBins; k += kStatsThreads) {
        const uint32_t c = sHist[k];
        if (c) atomicAdd(&stats[8 + k], (u64)c);
    }
}

int stats_validate(const mfsr_image_stats_params* p, int w, int h, int rowBytes, const uint64_t* statsDev)
{
    MFSR_REQUIRE(p != nullptr && statsDev != nullptr && ((uintptr_t)statsDev & 7) == 0);
    MFSR_REQUIRE(w > 0 && h > 0 && (long long)w * h < (1LL << 31));
    MFSR_REQUIRE((long long)rowBytes >= 12LL * w && (rowBytes & 3) == 0);
    MFSR_REQUIRE(0 <= p->lo && p->lo <= p->hi && p->hi <= kBins - 1);
    MFSR_REQUIRE(0 <= p->chromaTol && p->chromaTol <= 65536);
    MFSR_REQUIRE(p->reserved[0] == 0 && p->reserved[1] == 0 && p->reserved[2] == 0);
    if (p->useMatrix)
        for (int i = 0; i < 9; i++) MFSR_REQUIRE(std::isfinite(p->matrix[i]) && fabsf(p->matrix[i]) <= 256.0f);
    return MFSR_OK;
}

// one chunk of rows per CU, no workgroup with less than one round of its lanes (where the image has that many rows)
StatsArgs stats_args(const mfsr_image_stats_params* p, int w, int h, int rowBytes, unsigned* blocks)
{
    StatsArgs s;
    for (int i = 0; i < 9; i++) s.m[i] = p->matrix[i];
    s.useMatrix = p->useMatrix != 0;
    s.lo = p->lo;
    s.hi = p->hi;
    s.chromaTol = p->chromaTol;
    s.width = w;
    s.height = h;
    s.pitch = rowBytes;
    const int upr = (w + kStatsPpl - 1) / kStatsPpl;
    const int minRows = (kStatsThreads + upr - 1) / upr;
    int rows = (int)mfsr_cdiv(h, mfsr_device_cus());
    rows = rows < minRows ? minRows : rows;
    s.rowsPerGroup = rows < h ? rows : h;
    *blocks = mfsr_cdiv(h, s.rowsPerGroup);  // every chunk non-empty
    return s;
}

}  // namespace

extern "C" int mfsr_imageStats(const mfsr_float3* in, int inRowBytes, int w, int h, const mfsr_image_stats_params* params,
                               uint64_t* statsDev, mfsr_stream_t stream)
{
    // host validation first: nothing below touches the device before every argument has passed
    MFSR_REQUIRE(in != nullptr && ((uintptr_t)in & 3) == 0);
    if (int rc = stats_validate(params, w, h, inRowBytes, statsDev)) return rc;
    unsigned blocks = 0;
    const StatsArgs s = stats_args(params, w, h, inRowBytes, &blocks);
    const FinishSrc none = FinishSrc();
    hipLaunchKernelGGL(k_imageStats<0>, dim3(blocks), dim3(kStatsThreads), 0, mfsr_s(stream), (const pix3*)in, (const pix3*)nullptr,
                       none, s, (u64*)statsDev);
    return mfsr_launch_status("k_imageStats");
}

extern "C" int mfsr_finishStats(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                                int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, int w, int h,
                                float threshold, int colOffset, int rowOffset, int fullWidth, int fullHeight,
                                const mfsr_image_stats_params* params, uint64_t* statsDev, mfsr_stream_t stream)
{
    if (int rc = finish_check_src(finalImg, weight, imgRowBytes, fallback, fbRowBytes, fbW, fbH, w, h, colOffset, rowOffset, fullWidth,
                                  fullHeight))
        return rc;
    // (its own: the quad loads want the three images dword-aligned)
    MFSR_REQUIRE(((uintptr_t)finalImg & 3) == 0 && ((uintptr_t)weight & 3) == 0 && ((uintptr_t)fallback & 3) == 0);
    if (int rc = stats_validate(params, w, h, imgRowBytes, statsDev)) return rc;
    unsigned blocks = 0;
    const StatsArgs s = stats_args(params, w, h, imgRowBytes, &blocks);
    const FinishSrc f = finish_src(fallback, fbRowBytes, fbW, fbH, u0, u1, v0, v1, threshold, colOffset, rowOffset, fullWidth, fullHeight);
    hipLaunchKernelGGL(k_imageStats<1>, dim3(blocks), dim3(kStatsThreads), 0, mfsr_s(stream), (const pix3*)finalImg,
                       (const pix3*)weight, f, s, (u64*)statsDev);
    return mfsr_launch_status("k_imageStats");
}

// ---- the fits (host only, double precision; no contraction, so a float64 numpy restatement differs only through pow and log)
extern "C" int mfsr_awb_gains(const uint64_t* statsHost, long long minCount, float gains[3], int32_t* status)
{
    MFSR_REQUIRE(statsHost != nullptr && gains != nullptr && status != nullptr);
    gains[0] = gains[1] = gains[2] = 1.0f;
    const uint64_t n = statsHost[1], s0 = statsHost[2], s1 = statsHost[3], s2 = statsHost[4];
    if ((minCount > 0 && n < (uint64_t)minCount) || s0 == 0 || s1 == 0 || s2 == 0) {
        *status = 1;
        return MFSR_OK;
    }
    *status = 0;
    const double g[2] = {(double)s1 / (double)s0, (double)s1 / (double)s2};
    for (int k = 0; k < 2; k++) {
        double v = g[k];
        if (v < 0.125 || v > 8.0) {
            v = v < 0.125 ? 0.125 : 8.0;
            *status = 2;
        }
        gains[2 * k] = (float)v;
    }
    return MFSR_OK;
}

namespace {
// the smallest k with cum(k) >= target (4095 when the table never gets there)
int rank_bin(const uint64_t* hist, uint64_t target)
{
    uint64_t cum = 0;
    for (int k = 0; k < kBins; k++) {
        cum += hist[k];
        if (cum >= target) return k;
    }
    return kBins - 1;
}
double srgb_d(double v) { return v <= 0.0031308 ? 12.92 * v : 1.055 * pow(v > 1e-300 ? v : 1e-300, 1.0 / 2.4) - 0.055; }
}  // namespace

extern "C" int mfsr_tone_fit(const uint64_t* statsHost, const mfsr_tone_params* tp, int toneSize, float* lutHost, double* black,
                             double* white, double* gamma, int32_t* status)
{
    MFSR_REQUIRE(statsHost != nullptr && tp != nullptr && status != nullptr);
    MFSR_REQUIRE(toneSize >= 1 && toneSize <= 65536);
    MFSR_REQUIRE(tp->pLo >= 0.0 && tp->pLo <= 1.0 && tp->pHi >= 0.0 && tp->pHi <= 1.0);  // (false for NaN)
    MFSR_REQUIRE(tp->maxGain >= 1.0 && tp->maxGain <= 65536.0 && tp->mid < 1.0);
    const uint64_t N = statsHost[0];
    MFSR_REQUIRE(N > 0 && N < (1ull << 40));
    const uint64_t tLo = (uint64_t)(tp->pLo * (double)N), tHi = (uint64_t)((1.0 - tp->pHi) * (double)N);
    const uint64_t* histY = statsHost + 8;
    const uint64_t* histM = statsHost + 8 + kBins;
    const int kLo = rank_bin(histY, tLo + 1);          // cumY(k) > tLo
    const int kHi = rank_bin(histM, N - (tHi < N ? tHi : N));
    const int kMed = rank_bin(histY, (N + 1) / 2);
    const double b = (double)kLo / 4095.0;
    double span = (double)kHi / 4095.0 - b;
    *status = 0;
    if (span < 1.0 / tp->maxGain) {
        span = 1.0 / tp->maxGain;
        *status = 1;
    }
    auto u = [&](double v) {
        const double t = (v - b) / span;
        return t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    };
    const double um = u((double)kMed / 4095.0);
    double g = 1.0;
    if (tp->mid > 0.0 && um > 0.0 && um < 1.0) {
        g = log(tp->mid) / log(um);
        g = g < 0.5 ? 0.5 : (g > 2.0 ? 2.0 : g);
    }
    if (lutHost)
        for (int k = 0; k <= toneSize; k++) {
            const double t = u((double)k / (double)toneSize);
            lutHost[k] = (float)srgb_d(g == 1.0 ? t : pow(t, g));
        }
    if (black) *black = b;
    if (white) *white = b + span;
    if (gamma) *gamma = g;
    return MFSR_OK;
}

extern "C" int mfsr_auto_defaults(long long pixels, mfsr_auto_params* ap)
{
    MFSR_REQUIRE(ap != nullptr && pixels >= 0);
    memset(ap, 0, sizeof(*ap));
    ap->awb = ap->tone = 1;
    ap->lo = 64;
    ap->hi = 3967;
    ap->chromaTol = 64;
    ap->iterations = 2;
    ap->minCount = pixels / 64;
    ap->toneParams.pLo = 0.001;
    ap->toneParams.pHi = 0.999;
    ap->toneParams.maxGain = 8.0;
    ap->toneParams.mid = 0.18;
    ap->toneSize = 4096;
    return MFSR_OK;
}
