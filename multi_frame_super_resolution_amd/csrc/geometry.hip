// geometry.hip -- the geometric finish: any output size, lens distortion and lateral chromatic
// aberration as one resample of the value the finish holds -- per output pixel and per channel a source coordinate (a cubic
// polynomial in r^2 around the optical centre) and a bilinear or Catmull-Rom kernel -- then matrix, tone and the store of the
// four single-plane formats.  From the accumulators (mfsr_finishGeometry) and from a float image (mfsr_geometryImage): one
// tile body.  gfx950, wave64.
//
// Every step is float32 + - * fmaxf fminf floorf with -ffp-contract=off (the Makefile) in the order include/mfsr.h writes it, so
// the numpy restatement (tests/geometry_ref.py) is bit-exact.  The source pixel is finish_value_at's (finish_common.hpp), the
// store is render_span's (render_common.hpp): neither is restated.
//
// A workgroup of 256 lanes owns a kTW x kTH = 64 x 16 tile of output pixels (a lane: one pixel of four rows, or, RGB8, four
// consecutive pixels of one row, as render_span stores them):
//   1. every lane computes the (ix, iy) of its pixels' three channels;
//   2. the block reduces them to the exact bounding box of the clamped source taps: whole-wave min / max (cross-lane
//      shuffles), then one LDS step across the four waves;
//   3. if the box fits the stage (kSW x kSH = 96 x 32 source pixels), the block evaluates the source value ONCE per source pixel
//      of the box into LDS -- three planes of kSH rows, kSP = 97 floats apart -- with coalesced row reads;
//   4. all taps are then read from LDS.
// The box comes from the lanes' own integers, so it is exact for any mapping: no analytic bound on the distortion is relied on.
// A block whose box exceeds the stage (strong distortion, a large step) takes a block-uniform slow path that reads every tap
// through the same fetch from memory: the same bits.  MFSR_GEOMETRY_STAGE=0 sends every block that way (A/B).
// LDS: 3 * 32 * 97 * 4 = 37248 B + 64 B for the box: four workgroups (16 waves) on a CU's 160 KB.  Planar, not pix3: the taps of
// one channel at consecutive output pixels are consecutive floats (ds_read_b32, 32 banks: conflict-free at steps up to 1;
// RGB8's four-pixel lanes stride 4 floats and pay 2-way), and the three channels of one pixel sit in different source pixels as
// soon as a lateral scale is set.  The odd row pitch keeps the two rows of an RGB8 half-wave on different banks.
#include <climits>

#include "stencil_host.hpp"

namespace {

constexpr int kTW = 64, kTH = 16, kLanes = 256, kWaves = kLanes / MFSR_WAVE;
constexpr int kSW = 96, kSH = 32, kSP = kSW + 1;

// GeoArgs.flags.  kStage clear: every block takes the slow path; kSame: the three rows of k are equal, so one source coordinate
// serves the three channels
constexpr int kStage = 1, kSame = 2;

struct GeoArgs {
    float ocx, ocy, scx, scy, stepX, stepY, rnorm2;
    float k[3][4];
    int srcW, srcH;
    int colOffset, rowOffset;  // the launch's pixel (0, 0) in the full output
    int flags;                 // kStage | kSame (one word: the kernels are short of scalar registers)
};

struct Tap {
    int i;    // floor of the source coordinate, -1 .. n
    float f;  // its fraction, [0, 1)
};

__device__ __forceinline__ Tap geo_axis(float centre, float d, float m, int n)
{
    float u = (centre + d * m) - 0.5f;
    u = fminf(fmaxf(u, -1.0f), (float)n);
    Tap t;
    t.i = (int)floorf(u);
    t.f = u - (float)t.i;
    return t;
}

// the source coordinates of the channels at pixel (X, Y) of the full output: of all three, or (the three are equal: kSame) of
// channel 0 alone, the other entries then being left alone
__device__ __forceinline__ void geo_coords(int X, int Y, const GeoArgs& g, Tap (&tx)[3], Tap (&ty)[3], bool all = true)
{
    const float dx = (((float)X + 0.5f) - g.ocx) * g.stepX;
    const float dy = (((float)Y + 0.5f) - g.ocy) * g.stepY;
    const float rho = (dx * dx + dy * dy) * g.rnorm2;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (c > 0 && !all) break;
        const float m = ((g.k[c][3] * rho + g.k[c][2]) * rho + g.k[c][1]) * rho + g.k[c][0];
        tx[c] = geo_axis(g.scx, dx, m, g.srcW);
        ty[c] = geo_axis(g.scy, dy, m, g.srcH);
    }
}

__device__ __forceinline__ void cubic_weights(float f, float (&w)[4])
{
    w[0] = ((-0.5f * f + 1.0f) * f - 0.5f) * f;
    w[1] = ((1.5f * f - 2.5f) * f) * f + 1.0f;
    w[2] = ((-1.5f * f + 2.0f) * f + 0.5f) * f;
    w[3] = ((0.5f * f - 0.5f) * f) * f;
}

// o of channel c; s(c, i, j): the cleaned source value at the CLAMPED source pixel (i, j).  CLAMP = false: the caller knows that
// no tap of the block leaves the source (the taps are then constant offsets from one address)
template <int FILTER, bool CLAMP, class S>
__device__ __forceinline__ float geo_channel(int c, Tap tx, Tap ty, const GeoArgs& g, const S& s)
{
    const int xm = g.srcW - 1, ym = g.srcH - 1;
    auto cx = [&](int i) { return CLAMP ? min(max(i, 0), xm) : i; };
    auto cy = [&](int j) { return CLAMP ? min(max(j, 0), ym) : j; };
    if constexpr (FILTER == MFSR_GEO_BILINEAR) {
        const int i0 = cx(tx.i), i1 = cx(tx.i + 1);
        float h[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int jj = cy(ty.i + j);
            const float a = s(c, i0, jj), b = s(c, i1, jj);
            h[j] = a + (b - a) * tx.f;
        }
        return h[0] + (h[1] - h[0]) * ty.f;
    } else {
        float w[4], wy[4], h[4];
        cubic_weights(tx.f, w);
        cubic_weights(ty.f, wy);
        int ii[4];
#pragma unroll
        for (int i = 0; i < 4; i++) ii[i] = cx(tx.i - 1 + i);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int jj = cy(ty.i - 1 + j);
            h[j] = (w[0] * s(c, ii[0], jj) + w[1] * s(c, ii[1], jj)) + (w[2] * s(c, ii[2], jj) + w[3] * s(c, ii[3], jj));
        }
        return (wy[0] * h[0] + wy[1] * h[1]) + (wy[2] * h[2] + wy[3] * h[3]);
    }
}

template <int FILTER, bool CLAMP, class S>
__device__ __forceinline__ pix3 geo_pixel(int X, int Y, const GeoArgs& g, const S& s)
{
    Tap tx[3], ty[3];
    pix3 o;
    if (g.flags & kSame) {  // uniform: one coordinate, one set of weights and tap addresses for the three channels (the same bits)
        geo_coords(X, Y, g, tx, ty, false);
        o.x = geo_channel<FILTER, CLAMP>(0, tx[0], ty[0], g, s);
        o.y = geo_channel<FILTER, CLAMP>(1, tx[0], ty[0], g, s);
        o.z = geo_channel<FILTER, CLAMP>(2, tx[0], ty[0], g, s);
    } else {
        geo_coords(X, Y, g, tx, ty);
        o.x = geo_channel<FILTER, CLAMP>(0, tx[0], ty[0], g, s);
        o.y = geo_channel<FILTER, CLAMP>(1, tx[1], ty[1], g, s);
        o.z = geo_channel<FILTER, CLAMP>(2, tx[2], ty[2], g, s);
    }
    return o;
}

__device__ __forceinline__ float geo_clean(float v) { return isnan(v) ? 0.0f : v; }

__device__ __forceinline__ float pick(pix3 p, int c) { return c == 0 ? p.x : (c == 1 ? p.y : p.z); }

// The slow path's pixel: every tap through fetch(x, y) from memory, the same operations in the same order.  The channels and
// the rows of the kernel are real loops (values picked by comparison, no indexed registers): fetch is finish_value_at in the
// finish kernel, and 48 inlined copies of it would not fit the registers.
template <int FILTER, class Fetch>
__device__ __forceinline__ pix3 geo_pixel_slow(int X, int Y, const GeoArgs& g, const Fetch& fetch)
{
    constexpr bool cubic = FILTER == MFSR_GEO_CUBIC;
    constexpr int N = cubic ? 4 : 2, B = cubic ? 1 : 0;
    const int xm = g.srcW - 1, ym = g.srcH - 1;
    Tap tx[3], ty[3];
    geo_coords(X, Y, g, tx, ty);
    pix3 o = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int c = 0; c < 3; c++) {
        Tap ax, ay;
        ax.i = c == 0 ? tx[0].i : (c == 1 ? tx[1].i : tx[2].i);
        ax.f = c == 0 ? tx[0].f : (c == 1 ? tx[1].f : tx[2].f);
        ay.i = c == 0 ? ty[0].i : (c == 1 ? ty[1].i : ty[2].i);
        ay.f = c == 0 ? ty[0].f : (c == 1 ? ty[1].f : ty[2].f);
        float w[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wy[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (cubic) {
            cubic_weights(ax.f, w);
            cubic_weights(ay.f, wy);
        }
        float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f, h3 = 0.0f;
#pragma unroll 1
        for (int j = 0; j < N; j++) {
            const int jj = min(max(ay.i - B + j, 0), ym);
            float v[N];
#pragma unroll
            for (int i = 0; i < N; i++) v[i] = geo_clean(pick(fetch(min(max(ax.i - B + i, 0), xm), jj), c));
            float h;
            if constexpr (cubic)
                h = (w[0] * v[0] + w[1] * v[1]) + (w[2] * v[2] + w[3] * v[3]);
            else
                h = v[0] + (v[1] - v[0]) * ax.f;
            h0 = j == 0 ? h : h0;
            h1 = j == 1 ? h : h1;
            h2 = j == 2 ? h : h2;
            h3 = j == 3 ? h : h3;
        }
        float oc;
        if constexpr (cubic)
            oc = (wy[0] * h0 + wy[1] * h1) + (wy[2] * h2 + wy[3] * h3);
        else
            oc = h0 + (h1 - h0) * ay.f;
        o.x = c == 0 ? oc : o.x;
        o.y = c == 1 ? oc : o.y;
        o.z = c == 2 ? oc : o.z;
    }
    return o;
}

// the lane's pixels of the tile; pixel(X, Y): o at pixel (X, Y) of the full output
template <int FORMAT, class Pixel>
__device__ __forceinline__ void geo_store(const Pixel& pixel, pix3* outImg, int outPitch, uint8_t* out, int outRowBytes, int width,
                                          int height, const GeoArgs& g, const RenderArgs& r, const float* lut)
{
    constexpr int PPL = Fmt<FORMAT>::ppl, lanesX = kTW / PPL, rowsPerPass = kLanes / lanesX;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW + (tid % lanesX) * PPL;
    for (int ly = tid / lanesX; ly < kTH; ly += rowsPerPass) {
        const int y = blockIdx.y * kTH + ly;
        if (x0 >= width || y >= height) continue;
        pix3 t[PPL];
#pragma unroll
        for (int k = 0; k < PPL; k++) {
            t[k] = {0.0f, 0.0f, 0.0f};
            if (x0 + k < width) t[k] = pixel(x0 + k + g.colOffset, y + g.rowOffset);
        }
        auto src = [&](int x) {
            pix3 q = t[0];
#pragma unroll
            for (int k = 1; k < PPL; k++)
                if (x - x0 == k) q = t[k];
            return q;
        };
        render_span<FORMAT>(src, outImg ? row_ptr(outImg, outPitch, y) : nullptr, out ? out + (size_t)outRowBytes * (size_t)y : nullptr,
                            x0, width, r, lut);
    }
}

// The tile of the workgroup.  load(x, y): what memory holds at source pixel (x, y), 0 <= x < srcW, 0 <= y < srcH; value(raw, x,
// y): the source value of it.  s_st: the stage, three planes of kSH x kSP floats; s_box: kWaves x 4 ints.
template <int FORMAT, int FILTER, class Load, class Value>
__device__ __forceinline__ void geo_tile(const Load& load, const Value& value, float* s_st, int* s_box, pix3* outImg, int outPitch, uint8_t* out,
                                         int outRowBytes, int width, int height, const GeoArgs& g, const RenderArgs& r, const float* lut)
{
    constexpr int PPL = Fmt<FORMAT>::ppl, lanesX = kTW / PPL, rowsPerPass = kLanes / lanesX;
    constexpr int kBefore = FILTER == MFSR_GEO_CUBIC ? 1 : 0, kAfter = FILTER == MFSR_GEO_CUBIC ? 2 : 1;
    const int tid = threadIdx.x;
    auto fetch = [&](int x, int y) { return value(load(x, y), x, y); };
    auto slow = [&](int X, int Y) { return geo_pixel_slow<FILTER>(X, Y, g, fetch); };
    int bx0 = 0, by0 = 0, bw = 0, bh = 0;
    bool fits = false, inside = false;  // inside: no tap of the block leaves the source
    if (g.flags & kStage) {  // uniform (MFSR_GEOMETRY_STAGE=0: no box, every block reads its taps from memory)
        // 1. the lane's own (ix, iy), all channels of all its pixels
        int x0 = INT_MAX, x1 = INT_MIN, y0 = INT_MAX, y1 = INT_MIN;
        {
            const int px0 = blockIdx.x * kTW + (tid % lanesX) * PPL;
            for (int ly = tid / lanesX; ly < kTH; ly += rowsPerPass) {
                const int y = blockIdx.y * kTH + ly;
#pragma unroll
                for (int k = 0; k < PPL; k++) {
                    const bool valid = px0 + k < width && y < height;
                    Tap tx[3], ty[3];
                    geo_coords(px0 + k + g.colOffset, y + g.rowOffset, g, tx, ty, !(g.flags & kSame));
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        if (c > 0 && (g.flags & kSame)) break;  // uniform
                        x0 = valid ? min(x0, tx[c].i) : x0;
                        x1 = valid ? max(x1, tx[c].i) : x1;
                        y0 = valid ? min(y0, ty[c].i) : y0;
                        y1 = valid ? max(y1, ty[c].i) : y1;
                    }
                }
            }
        }
        // 2. the block's box: whole-wave min / max, then across the waves through LDS
#pragma unroll
        for (int o = MFSR_WAVE / 2; o > 0; o >>= 1) {
            x0 = min(x0, __shfl_xor(x0, o));
            x1 = max(x1, __shfl_xor(x1, o));
            y0 = min(y0, __shfl_xor(y0, o));
            y1 = max(y1, __shfl_xor(y1, o));
        }
        if ((tid & (MFSR_WAVE - 1)) == 0) {
            int* b = s_box + 4 * (tid / MFSR_WAVE);
            b[0] = x0;
            b[1] = x1;
            b[2] = y0;
            b[3] = y1;
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            x0 = min(x0, s_box[4 * w]);
            x1 = max(x1, s_box[4 * w + 1]);
            y0 = min(y0, s_box[4 * w + 2]);
            y1 = max(y1, s_box[4 * w + 3]);
        }
        // (every lane holds the same four values: make them scalars).  The taps reach kBefore before and kAfter after the floor and
        // are clamped one by one; clamping is monotone, so the box of the clamped taps is the clamped box.  A tile has a valid pixel
        // (the grid covers width x height), so the box is not empty.
        bx0 = min(max(__builtin_amdgcn_readfirstlane(x0) - kBefore, 0), g.srcW - 1);
        by0 = min(max(__builtin_amdgcn_readfirstlane(y0) - kBefore, 0), g.srcH - 1);
        bw = min(max(__builtin_amdgcn_readfirstlane(x1) + kAfter, 0), g.srcW - 1) - bx0 + 1;
        bh = min(max(__builtin_amdgcn_readfirstlane(y1) + kAfter, 0), g.srcH - 1) - by0 + 1;
        fits = bw <= kSW && bh <= kSH;
        inside = __builtin_amdgcn_readfirstlane(x0) - kBefore >= 0 && __builtin_amdgcn_readfirstlane(x1) + kAfter <= g.srcW - 1 &&
                 __builtin_amdgcn_readfirstlane(y0) - kBefore >= 0 && __builtin_amdgcn_readfirstlane(y1) + kAfter <= g.srcH - 1;
    }
    if (!fits) {  // uniform: the box does not fit the stage
        geo_store<FORMAT>(slow, outImg, outPitch, out, outRowBytes, width, height, g, r, lut);
        return;
    }
    // 3. the source value once per source pixel of the box, row by row (consecutive lanes: consecutive pixels of a row).  The
    // flat index advances by kLanes = q * bw + rem pixels a step.  Four steps at a time: their loads are all issued before the
    // first value is formed (a step's loads would otherwise wait for the previous step's: five to twelve memory latencies in a
    // row, with sixteen waves a CU to hide them).
    {
        constexpr int kBatch = 4;
        const int q = kLanes / bw, rem = kLanes - q * bw;
        int ly = tid / bw, lx = tid - ly * bw;
        while (ly < bh) {
            int px[kBatch], py[kBatch];
            decltype(load(0, 0)) raw[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; k++) {
                px[k] = lx;
                py[k] = ly;
                if (ly < bh) raw[k] = load(bx0 + lx, by0 + ly);
                lx += rem;
                ly += q;
                if (lx >= bw) {
                    lx -= bw;
                    ly++;
                }
            }
#pragma unroll
            for (int k = 0; k < kBatch; k++) {
                if (py[k] >= bh) continue;
                const pix3 p = value(raw[k], bx0 + px[k], by0 + py[k]);
                float* d = s_st + py[k] * kSP + px[k];
                d[0] = geo_clean(p.x);
                d[kSH * kSP] = geo_clean(p.y);
                d[2 * kSH * kSP] = geo_clean(p.z);
            }
        }
    }
    __syncthreads();
    // 4. the taps from LDS
    auto tap = [&](int c, int i, int j) { return s_st[c * (kSH * kSP) + (j - by0) * kSP + (i - bx0)]; };
    if (inside) {  // uniform: the clamps are identities
        auto staged = [&](int X, int Y) { return geo_pixel<FILTER, false>(X, Y, g, tap); };
        geo_store<FORMAT>(staged, outImg, outPitch, out, outRowBytes, width, height, g, r, lut);
    } else {
        auto staged = [&](int X, int Y) { return geo_pixel<FILTER, true>(X, Y, g, tap); };
        geo_store<FORMAT>(staged, outImg, outPitch, out, outRowBytes, width, height, g, r, lut);
    }
}

template <int FORMAT, int LDS, int FILTER>
__global__ void __launch_bounds__(kLanes)
    k_geometryImage(const pix3* __restrict__ in, int inPitch, pix3* __restrict__ outImg, int outPitch, uint8_t* __restrict__ out,
                    int outRowBytes, int width, int height, GeoArgs g, RenderArgs r)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    __shared__ float s_st[3 * kSH * kSP];
    __shared__ int s_box[4 * kWaves];
    const float* lut = stage_lut<LDS>(r, s_lut);
    auto load = [&](int x, int y) { return row_ptr(in, inPitch, y)[x]; };
    auto value = [&](pix3 raw, int, int) { return raw; };
    geo_tile<FORMAT, FILTER>(load, value, s_st, s_box, outImg, outPitch, out, outRowBytes, width, height, g, r, lut);
}

template <int FORMAT, int LDS, int FILTER>
__global__ void __launch_bounds__(kLanes)
    k_finishGeometry(const pix3* __restrict__ finalImg, const pix3* __restrict__ weight, int imgPitch, FinishSrc fIn,
                     pix3* __restrict__ outImg, int outPitch, uint8_t* __restrict__ out, int outRowBytes, int width, int height,
                     GeoArgs g, RenderArgs r)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    __shared__ float s_st[3 * kSH * kSP];
    __shared__ int s_box[4 * kWaves];
    const float* lut = stage_lut<LDS>(r, s_lut);
    // the source is the full frame: its place is (0, 0) of srcW x srcH, which the launch arguments already hold (fewer scalars)
    FinishSrc f = fIn;
    f.colOffset = f.rowOffset = 0;
    f.fullWidth = g.srcW;
    f.fullHeight = g.srcH;
    // k_finishRendered's value at the source pixel (finish_value: one definition)
    // (finish_value_at's two loads and finish_value, apart: the stage issues the loads of several pixels first)
    struct Raw {
        pix3 val, w;
    };
    auto load = [&](int x, int y) {
        Raw r;
        r.val = *(const pix3*)((const char*)finalImg + (long long)imgPitch * y + 12LL * x);
        r.w = *(const pix3*)((const char*)weight + (long long)imgPitch * y + 12LL * x);
        return r;
    };
    auto value = [&](const Raw& r, int x, int y) { return finish_value(r.val, r.w, x, y, f); };
    geo_tile<FORMAT, FILTER>(load, value, s_st, s_box, outImg, outPitch, out, outRowBytes, width, height, g, r, lut);
}

// FORMAT_LUT_DISPATCH switches on <FORMAT, LDS>: the filter is bound here
template <int FORMAT, int LDS>
constexpr auto k_geometryImageBilinear = &k_geometryImage<FORMAT, LDS, MFSR_GEO_BILINEAR>;
template <int FORMAT, int LDS>
constexpr auto k_geometryImageCubic = &k_geometryImage<FORMAT, LDS, MFSR_GEO_CUBIC>;
template <int FORMAT, int LDS>
constexpr auto k_finishGeometryBilinear = &k_finishGeometry<FORMAT, LDS, MFSR_GEO_BILINEAR>;
template <int FORMAT, int LDS>
constexpr auto k_finishGeometryCubic = &k_finishGeometry<FORMAT, LDS, MFSR_GEO_CUBIC>;

bool finite_all(const float* v, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// MFSR_GEOMETRY_STAGE=0: every block reads its taps from memory (A/B); read at every call, so that a test can switch it
bool geometry_stage_on() { return !mfsr_env_is0("MFSR_GEOMETRY_STAGE"); }

// what both launch entries ask of the description, the source extent, the rectangle and the render description
int geometry_launch(const mfsr_geometry* g, int srcW, int srcH, int colOffset, int rowOffset, int w, int h, const mfsr_render* render,
                    const mfsr_render* plain, const mfsr_render** use, GeoArgs* a)
{
    if (int rc = mfsr_geometry_validate(g)) return rc;
    MFSR_REQUIRE(srcW >= 1 && srcW <= 32768 && srcH >= 1 && srcH <= 32768);
    MFSR_REQUIRE(g->scx >= -(float)srcW && g->scx <= 2.0f * (float)srcW && g->scy >= -(float)srcH && g->scy <= 2.0f * (float)srcH);
    MFSR_REQUIRE(w > 0 && h > 0 && colOffset >= 0 && rowOffset >= 0 && g->outW - colOffset >= w && g->outH - rowOffset >= h);
    if (int rc = stencil_render(render, plain, use)) return rc;  // (refuses the two-plane formats)
    a->ocx = g->ocx;
    a->ocy = g->ocy;
    a->scx = g->scx;
    a->scy = g->scy;
    a->stepX = g->stepX;
    a->stepY = g->stepY;
    a->rnorm2 = g->rnorm2;
    memcpy(a->k, g->k, sizeof(a->k));
    a->srcW = srcW;
    a->srcH = srcH;
    a->colOffset = colOffset;
    a->rowOffset = rowOffset;
    const bool same = memcmp(g->k[0], g->k[1], sizeof(g->k[0])) == 0 && memcmp(g->k[0], g->k[2], sizeof(g->k[0])) == 0;
    a->flags = (geometry_stage_on() ? kStage : 0) | (same ? kSame : 0);
    return MFSR_OK;
}

}  // namespace

#define GEOMETRY_DISPATCH(KERNEL, filter, format, lds, ...)                                               \
    do {                                                                                                  \
        if ((filter) == MFSR_GEO_CUBIC)                                                                   \
            STENCIL_DISPATCH(KERNEL##Cubic, kTW, kTH, kLanes, format, lds, __VA_ARGS__);                  \
        else                                                                                              \
            STENCIL_DISPATCH(KERNEL##Bilinear, kTW, kTH, kLanes, format, lds, __VA_ARGS__);               \
    } while (0)

extern "C" int mfsr_geometry_tile(int* tileW, int* tileH, int* stageW, int* stageH)
{
    MFSR_REQUIRE(tileW && tileH && stageW && stageH);
    *tileW = kTW;
    *tileH = kTH;
    *stageW = kSW;
    *stageH = kSH;
    return MFSR_OK;
}

extern "C" int mfsr_geometry_validate(const mfsr_geometry* g)
{
    MFSR_REQUIRE(g != nullptr);
    MFSR_REQUIRE(g->outW >= 1 && g->outW <= 32768 && g->outH >= 1 && g->outH <= 32768);
    MFSR_REQUIRE(g->filter == MFSR_GEO_BILINEAR || g->filter == MFSR_GEO_CUBIC);
    MFSR_REQUIRE(finite_all(&g->ocx, 7) && finite_all(&g->k[0][0], 12));  // (ocx .. rnorm2 are seven consecutive floats)
    MFSR_REQUIRE(g->stepX >= 0.125f && g->stepX <= 8.0f && g->stepY >= 0.125f && g->stepY <= 8.0f);
    MFSR_REQUIRE(g->rnorm2 > 0.0f && g->rnorm2 <= 4.0f);
    for (int c = 0; c < 3; c++) {
        MFSR_REQUIRE(fabsf(g->k[c][0] - 1.0f) <= 0.25f);
        for (int i = 1; i < 4; i++) MFSR_REQUIRE(fabsf(g->k[c][i]) <= 4.0f);
    }
    MFSR_REQUIRE(g->ocx >= -(float)g->outW && g->ocx <= 2.0f * (float)g->outW);
    MFSR_REQUIRE(g->ocy >= -(float)g->outH && g->ocy <= 2.0f * (float)g->outH);
    MFSR_REQUIRE(g->scx >= -32768.0f && g->scx <= 65536.0f && g->scy >= -32768.0f && g->scy <= 65536.0f);  // (the launch: its source)
    for (int i = 0; i < 10; i++) MFSR_REQUIRE(g->reserved[i] == 0);
    return MFSR_OK;
}

extern "C" int mfsr_geometry_lens(int srcW, int srcH, int dstW, int dstH, double zoom, const double k[3], const double lateral[2],
                                  int filter, mfsr_geometry* out)
{
    MFSR_REQUIRE(out && k && lateral && srcW >= 1 && srcW <= 32768 && srcH >= 1 && srcH <= 32768 && dstW >= 1 && dstH >= 1);
    MFSR_REQUIRE(std::isfinite(zoom) && zoom > 0.0);
    mfsr_geometry g;
    memset(&g, 0, sizeof(g));
    g.outW = dstW;
    g.outH = dstH;
    g.filter = filter;
    g.ocx = (float)(dstW / 2.0);
    g.ocy = (float)(dstH / 2.0);
    g.scx = (float)(srcW / 2.0);
    g.scy = (float)(srcH / 2.0);
    const double sx = (double)srcW / dstW, sy = (double)srcH / dstH;
    g.stepX = g.stepY = (float)((sx < sy ? sx : sy) / zoom);
    g.rnorm2 = (float)(1.0 / ((srcW / 2.0) * (srcW / 2.0) + (srcH / 2.0) * (srcH / 2.0)));
    for (int c = 0; c < 3; c++) {
        g.k[c][0] = c == 0 ? (float)lateral[0] : (c == 2 ? (float)lateral[1] : 1.0f);
        for (int i = 0; i < 3; i++) g.k[c][1 + i] = (float)k[i];
    }
    if (int rc = mfsr_geometry_validate(&g)) return rc;
    *out = g;
    return MFSR_OK;
}

extern "C" int mfsr_geometry_defaults(int srcW, int srcH, mfsr_geometry* out)
{
    const double none[3] = {0.0, 0.0, 0.0}, one[2] = {1.0, 1.0};
    return mfsr_geometry_lens(srcW, srcH, srcW, srcH, 1.0, none, one, MFSR_GEO_CUBIC, out);
}

extern "C" int mfsr_geometryImage(const mfsr_float3* in, int inRowBytes, int srcW, int srcH, mfsr_float3* outImg, int outImgRowBytes,
                                  void* out, int outRowBytes, const mfsr_render* render, const mfsr_geometry* geometry, int applyGamma,
                                  int colOffset, int rowOffset, int w, int h, mfsr_stream_t stream)
{
    // host validation first: nothing below touches the device before every argument has passed
    MFSR_REQUIRE(in && (outImg || out) && srcW > 0 && srcH > 0 && w > 0 && h > 0);
    MFSR_REQUIRE((long long)inRowBytes >= 12LL * srcW && (inRowBytes & 3) == 0 && ((uintptr_t)in & 3) == 0);
    if (outImg) MFSR_REQUIRE((long long)outImgRowBytes >= 12LL * w && (outImgRowBytes & 3) == 0 && ((uintptr_t)outImg & 3) == 0);
    const mfsr_render plain = mfsr_plain_render();
    GeoArgs ga;
    if (int rc = geometry_launch(geometry, srcW, srcH, colOffset, rowOffset, w, h, render, &plain, &render, &ga)) return rc;
    if (int rc = stencil_outputs_apart(in, image_span(inRowBytes, srcH, 12, srcW), outImg, outImgRowBytes, out, outRowBytes,
                                       render->format, w, h))
        return rc;
    const RenderArgs ra = render_args(render, applyGamma);
    const bool lds = stencil_lut_in_lds(render);
    GEOMETRY_DISPATCH(k_geometryImage, geometry->filter, render->format, lds, (const pix3*)in, inRowBytes, (pix3*)outImg, outImgRowBytes,
                      (uint8_t*)out, outRowBytes, w, h, ga, ra);
    return mfsr_launch_status("geometryImage");
}

extern "C" int mfsr_finishGeometry(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                                   int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, int srcW, int srcH,
                                   mfsr_float3* outImg, int outImgRowBytes, void* out, int outRowBytes, const mfsr_render* render,
                                   const mfsr_geometry* geometry, float threshold, int applyGamma, int colOffset, int rowOffset, int w,
                                   int h, mfsr_stream_t stream)
{
    // every finish's check, on what this launch READS: the whole srcW x srcH source, which is the full frame
    if (int rc = finish_check_src(finalImg, weight, imgRowBytes, fallback, fbRowBytes, fbW, fbH, srcW, srcH, 0, 0, srcW, srcH)) return rc;
    MFSR_REQUIRE((outImg || out) && w > 0 && h > 0);
    MFSR_REQUIRE(((uintptr_t)finalImg & 3) == 0 && ((uintptr_t)weight & 3) == 0);
    if (outImg) MFSR_REQUIRE((long long)outImgRowBytes >= 12LL * w && (outImgRowBytes & 3) == 0 && ((uintptr_t)outImg & 3) == 0);
    const mfsr_render plain = mfsr_plain_render();
    GeoArgs ga;
    if (int rc = geometry_launch(geometry, srcW, srcH, colOffset, rowOffset, w, h, render, &plain, &render, &ga)) return rc;
    for (const void* img : {(const void*)finalImg, (const void*)weight})
        if (int rc = stencil_outputs_apart(img, image_span(imgRowBytes, srcH, 12, srcW), outImg, outImgRowBytes, out, outRowBytes,
                                           render->format, w, h))
            return rc;
    const RenderArgs ra = render_args(render, applyGamma);
    const bool lds = stencil_lut_in_lds(render);
    const FinishSrc f = finish_src(fallback, fbRowBytes, fbW, fbH, u0, u1, v0, v1, threshold, 0, 0, srcW, srcH);
    GEOMETRY_DISPATCH(k_finishGeometry, geometry->filter, render->format, lds, (const pix3*)finalImg, (const pix3*)weight, imgRowBytes,
                      f, (pix3*)outImg, outImgRowBytes, (uint8_t*)out, outRowBytes, w, h, ga, ra);
    return mfsr_launch_status("finishGeometry");
}
