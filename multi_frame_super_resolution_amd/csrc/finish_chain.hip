// finish_chain.hip -- the finish chain: merge-aware denoise (section 2.24), then the unsharp mask
// (section 2.20), then the local-tone gain (section 2.25), then matrix, tone and the store of any output format -- the four
// single-plane ones (section 2.19) and NV12 / P010 (section 2.21) -- in ONE launch on the value the finish holds
// (mfsr_finishChain), and the same tile body on an existing float image with an optional count image (mfsr_chainImage).  Each
// stage is on or off at run time.  gfx950, wave64.
//
// The result is, bit for bit, the composition of the existing whole-image entry points (mfsr_finishDenoised to a float image,
// mfsr_sharpenImage to a float image, then mfsr_localToneImage / mfsr_renderImage / mfsr_renderImageYuv).  Every step is float32
// + - * / fmaxf fminf with -ffp-contract=off (the Makefile) in the order include/mfsr.h writes it.  The per-pixel arithmetic of
// the four stages is shared with those entry points wherever sharing left every kernel's instructions as they were
// (profiles/isa_finish_stage_bodies.txt):
//   yuv_common.hpp     yuv_block, the whole two-plane store, and YuvArgs / yuv_args / check_planes (render_yuv.hip's too);
//   finish_stages.hpp  slice_gain<0>, the whole gain (local_tone.hip's); the denoise's clean_value, clean_count, fade_of and
//                      denoise_inv_tolerance (denoise.hip's); the sharpen's sharpen_clean, sharpen_tap, sharpen_core and
//                      load_span (sharpen.hip's); DenoiseArgs / SharpenArgs and their host fills;
//   finish_value, render_pixel and render_span are finish_common.hpp's and render_common.hpp's, as before.
// STILL RESTATED here, in denoise.hip's and sharpen.hip's order: the denoise's window loop with its tap weight and its blend
// (denoise_at), and the loops of the sharpen's two passes (stage 3, sharpened_span) around the shared steps.  As functions
// called from both files those loops changed the code of k_denoiseImage / k_finishDenoised / k_sharpenImage /
// k_finishSharpened, which the burst's default finishes run; DESIGN.md section 5 has the rows.
// This file's own: how the tile and its halos are staged, the cleaning rule of the first stage that is on (chain_clean), the
// clamped position a halo pixel stands for, and the sharpen-off short cut.
//
// A workgroup of 256 lanes owns a kTW x kTH = 64 x 16 tile of output pixels.  With R = R_d + R_s (at most 3 + 4):
//   A  s_a[3][30][80]  the cleaned value p of the tile plus a halo of R at clamped coordinates, planar; the tile's column 0 at
//                      float kPadA = 8 of a row whatever R is (16-byte aligned)                                   28800 B
//   B  s_b[3][24][72]  d, the denoised value, of the tile plus a halo of R_s; the tile's column 0 at float kPadB = 4
//                      (16-byte aligned: an RGB8 or two-plane lane reads its four columns as one ds_read_b128)      20736 B
//   C  s_h[3][24][64]  the sharpen's horizontal pass on B (tile columns, tile + halo rows)                          18432 B
// C reuses A's storage: the barrier between the denoise stage (reads A, writes B) and the horizontal pass (reads B, writes C) is
// needed anyway, and after it nobody reads A.  49.5 KB a workgroup instead of 68 KB: three workgroups (twelve waves) on a CU's
// 160 KB instead of two.  With the denoise stage off, the staging writes B directly and A is never touched.
//
// Edges: a stage's stencil at a position outside the valid pixels is that stage's value at the clamped position, as the
// composition has it (the sharpen reads the denoised image at a clamped coordinate).  So B at a position q outside the valid
// pixels holds d of clamp(q), computed by the window around clamp(q) in A -- which lies inside A, see the bounds at stage 2 --
// and NOT by the window around q: A at q + delta holds p of clamp(q + delta), which is another pixel than clamp(clamp(q) +
// delta).
#include "finish_stages.hpp"
#include "stencil_host.hpp"
#include "yuv_common.hpp"

namespace {

constexpr int kMaxR = kMaxRd + kMaxRs;
constexpr int kPadA = 8, kAW = kTW + 2 * kPadA, kAH = kTH + 2 * kMaxR;   // 80 x 30
constexpr int kPadB = 4, kBW = kTW + 2 * kPadB, kBH = kTH + 2 * kMaxRs;  // 72 x 24
constexpr int kFloatsA = 3 * kAH * kAW, kFloatsC = 3 * kBH * kTW;
static_assert(kPadA >= kMaxR && kPadB >= kMaxRs && kFloatsC <= kFloatsA, "stage C reuses stage A's storage");
constexpr int FMT_NV12 = MFSR_OUT_NV12, FMT_P010 = MFSR_OUT_P010;

struct ChainArgs {
    // denoise (section 2.24): DenoiseArgs' members
    float gain, alpha, beta, hh;  // hh = strength * strength
    float wHi, rSpan;             // the fade; used when fade != 0
    int fade;
    int Rd;                       // 0 = the stage is off
    // sharpen (section 2.20): SharpenArgs' members
    float k[kMaxRs + 1];
    float amount, threshold;
    int Rs;                       // 0 = the stage is off
    // local tone (section 2.25): the slice
    const float* grid;            // GX GY NZ floats: luma fastest, then x, then y; null = the stage is off
    int nz, nzShift, gx, gy;
    int colOffset, rowOffset;     // the launch's pixel (0, 0) in the full frame
    float invCell, fnz;
    int yLo, yHi;                 // valid rows [yLo, yHi] relative to the launch's first row
};

template <int FORMAT>
struct ChainFmt {
    static constexpr bool yuv = FORMAT == FMT_NV12 || FORMAT == FMT_P010;
    static constexpr int ppl = yuv ? 4 : Fmt<FORMAT>::ppl;  // consecutive pixels of a row one lane owns
    static constexpr int rows = yuv ? 2 : 1;                // rows of a lane's block
};

// the cleaning of the first stage that is on: the denoise's (step 1 of section 2.24), the sharpen's (step 1 of section 2.20),
// or none (the local-tone gain and the render take p as it is)
__device__ __forceinline__ float chain_clean(float p, int Rd, int Rs)
{
    if (Rd) return clean_value(p);  // uniform
    if (Rs) return sharpen_clean(p);
    return p;
}

// ---- steps 2-6 of section 2.24 at the pixel whose cleaned value sits at s_a[.][ay][ac]: the one-pixel-per-lane loop of
// denoise.hip's denoise_tile around the same step functions.  n3: the count before its NaN cleaning.  Called by every lane of a
// wave (`live`: the lane has a position); a wave whose every position has lambda == 0 in every channel skips the stencil.
__device__ __forceinline__ void denoise_at(const float (*s_a)[kAH][kAW], int ay, int ac, bool live, pix3 n3, const ChainArgs& a,
                                           float (&o)[3])
{
    const int R = a.Rd;
    const float nn[3] = {n3.x, n3.y, n3.z};
    float s[3], n[3];
    bool need = false;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        s[c] = s_a[c][ay][ac];
        n[c] = clean_count(nn[c]);
        need = need || (live && fade_of(n[c], a) != 0.0f);
        o[c] = s[c];
    }
    if (!__any(need)) return;
    float rr[3], G = 0.0f, S[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 3; c++) rr[c] = denoise_inv_tolerance(s[c], n[c], a);
#pragma unroll
    for (int dy = -kMaxRd; dy <= kMaxRd; dy++) {
        if (dy < -R || dy > R) continue;  // uniform
        float win[3][2 * kMaxRd + 1];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float* row = &s_a[c][ay + dy][ac - kMaxRd];
#pragma unroll
            for (int q = 0; q < 2 * kMaxRd + 1; q++) win[c][q] = (q - kMaxRd >= -R && q - kMaxRd <= R) ? row[q] : 0.0f;
        }
        float Gr = 0.0f, Sr[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dx = -kMaxRd; dx <= kMaxRd; dx++) {
            if (dx < -R || dx > R) continue;  // uniform
            const float j0 = win[0][kMaxRd + dx], j1 = win[1][kMaxRd + dx], j2 = win[2][kMaxRd + dx];
            const float d0 = j0 - s[0], d1 = j1 - s[1], d2 = j2 - s[2];
            const float t = ((d0 * d0) * rr[0] + (d1 * d1) * rr[1]) + (d2 * d2) * rr[2];
            const float u = fmaxf(1.0f - t, 0.0f);
            const float g = u * u;
            Gr = Gr + g;
            Sr[0] = Sr[0] + g * j0;
            Sr[1] = Sr[1] + g * j1;
            Sr[2] = Sr[2] + g * j2;
        }
        G = G + Gr;
        S[0] = S[0] + Sr[0];
        S[1] = S[1] + Sr[1];
        S[2] = S[2] + Sr[2];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float f = S[c] / G, l = fade_of(n[c], a);
        o[c] = l == 0.0f ? s[c] : s[c] + l * (f - s[c]);
    }
}

// steps 3 and 4 of section 2.20 for the lane's N pixels of tile row ly from column lx0 (sharpen off: d itself)
template <int N>
__device__ __forceinline__ void sharpened_span(const float (*s_b)[kBH][kBW], const float (*s_h)[kBH][kTW], int ly, int lx0,
                                               const ChainArgs& a, float (&o)[N][3])
{
    const int R = a.Rs;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float s[N];
        load_span<N>(&s_b[c][ly + R][lx0 + kPadB], s);
        if (R == 0) {  // uniform
#pragma unroll
            for (int k = 0; k < N; k++) o[k][c] = s[k];
            continue;
        }
        float b[N];
        load_span<N>(&s_h[c][ly + R][lx0], b);
#pragma unroll
        for (int k = 0; k < N; k++) b[k] = a.k[0] * b[k];
        for (int d = 1; d <= R; d++) {
            float up[N], dn[N];
            load_span<N>(&s_h[c][ly + R - d][lx0], up);
            load_span<N>(&s_h[c][ly + R + d][lx0], dn);
#pragma unroll
            for (int k = 0; k < N; k++) b[k] = sharpen_tap(b[k], a.k[d], up[k], dn[k]);
        }
#pragma unroll
        for (int k = 0; k < N; k++) o[k][c] = sharpen_core(s[k], b[k], a);
    }
}

// The tile of the workgroup at (tileX0, tileY0).  fetch(x, y) is p at a valid pixel of the launch (columns [0, width), rows
// [a.yLo, a.yHi]); count(x, y) is n of section 2.24 before its NaN cleaning there.  s_ac: stage A's storage, which stage C
// reuses.  out / outRowBytes: the integer output, the Y plane for a two-plane format; outUV: its chroma plane.
template <int FORMAT, class Fetch, class Count>
__device__ __forceinline__ void chain_tile(const Fetch& fetch, const Count& count, float* s_ac, float (*s_b)[kBH][kBW], pix3* outImg,
                                           int outPitch, uint8_t* out, int outRowBytes, uint8_t* outUV, int uvRowBytes, int width,
                                           int height, const ChainArgs& a, const RenderArgs& r, const YuvArgs& ya, const float* lut)
{
    float (*s_a)[kAH][kAW] = (float (*)[kAH][kAW])s_ac;
    float (*s_h)[kBH][kTW] = (float (*)[kBH][kTW])s_ac;
    const int tid = threadIdx.x, Rd = a.Rd, Rs = a.Rs, R = Rd + Rs;
    const int tileX0 = blockIdx.x * kTW, tileY0 = blockIdx.y * kTH;
    const int bw = kTW + 2 * Rs, bh = kTH + 2 * Rs;  // B's extent: the tile plus the sharpen's halo
    if (Rd) {                                        // uniform
        // 1. cleaned p of the tile + a halo of R at clamped coordinates (beyond the image's last tile too: never stored)
        const int aw = kTW + 2 * R, ah = kTH + 2 * R;
        for (int i = tid; i < aw * ah; i += kLanes) {
            const int ly = i / aw, lx = i - ly * aw;
            const int gx = min(max(tileX0 + lx - R, 0), width - 1);
            const int gy = min(max(tileY0 + ly - R, a.yLo), a.yHi);
            const pix3 p = fetch(gx, gy);
            const int c0 = lx + (kPadA - R);  // (the tile's column 0 at float kPadA of the row)
            s_a[0][ly][c0] = chain_clean(p.x, Rd, Rs);
            s_a[1][ly][c0] = chain_clean(p.y, Rd, Rs);
            s_a[2][ly][c0] = chain_clean(p.z, Rd, Rs);
        }
        __syncthreads();
        // 2. d of the tile + a halo of Rs: at a position outside the valid pixels, d of the clamped position.  That pixel lies
        // between the tile and the position (tileX0 = 0 where a column is < 0, tileX0 <= width - 1; tileY0 = 0 where a row is
        // < yLo <= 0, tileY0 <= height - 1 <= yHi), so its window of Rd lies inside A's halo of Rd + Rs.
        for (int i0 = 0; i0 < bw * bh; i0 += kLanes) {  // (the same trip count for every lane: denoise_at votes per wave)
            const int i = i0 + tid;
            const bool live = i < bw * bh;
            const int by = live ? i / bw : 0, bx = live ? i - by * bw : 0;
            const int cx = min(max(tileX0 + bx - Rs, 0), width - 1);
            const int cy = min(max(tileY0 + by - Rs, a.yLo), a.yHi);
            pix3 n3 = {1.0f, 1.0f, 1.0f};
            if (live) n3 = count(cx, cy);
            float o[3];
            denoise_at(s_a, cy - tileY0 + R, cx - tileX0 + kPadA, live, n3, a, o);
            if (live) {
                const int c0 = bx + (kPadB - Rs);
                s_b[0][by][c0] = o[0];
                s_b[1][by][c0] = o[1];
                s_b[2][by][c0] = o[2];
            }
        }
    } else {
        // 1. (no denoise: d = p) the cleaned p of the tile + a halo of Rs, straight into B
        for (int i = tid; i < bw * bh; i += kLanes) {
            const int by = i / bw, bx = i - by * bw;
            const int gx = min(max(tileX0 + bx - Rs, 0), width - 1);
            const int gy = min(max(tileY0 + by - Rs, a.yLo), a.yHi);
            const pix3 p = fetch(gx, gy);
            const int c0 = bx + (kPadB - Rs);
            s_b[0][by][c0] = chain_clean(p.x, Rd, Rs);
            s_b[1][by][c0] = chain_clean(p.y, Rd, Rs);
            s_b[2][by][c0] = chain_clean(p.z, Rd, Rs);
        }
    }
    __syncthreads();  // B is complete, and A has been read for the last time: C may overwrite it
    if (Rs) {         // uniform
        // 3. the sharpen's horizontal pass on every row of B
        for (int i = tid; i < kTW * bh; i += kLanes) {
            const int ly = i / kTW, lx = i - ly * kTW;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float* row = &s_b[c][ly][lx + kPadB];
                float h = a.k[0] * row[0];
                for (int d = 1; d <= Rs; d++) h = sharpen_tap(h, a.k[d], row[-d], row[d]);
                s_h[c][ly][lx] = h;
            }
        }
        __syncthreads();
    }
    // 4. - 6. the lane's block: the vertical pass and the coring, the gain, then the format's store
    constexpr int PPL = ChainFmt<FORMAT>::ppl, ROWS = ChainFmt<FORMAT>::rows;
    constexpr int lanesX = kTW / PPL, rowsPerPass = (kLanes / lanesX) * ROWS;
    const int lx0 = (tid % lanesX) * PPL, x0 = tileX0 + lx0;
    for (int ly = (tid / lanesX) * ROWS; ly < kTH; ly += rowsPerPass) {
        const int y = tileY0 + ly;
        if (x0 >= width || y >= height) continue;
        float t[ROWS][PPL][3];
#pragma unroll
        for (int row = 0; row < ROWS; row++) {
            sharpened_span<PPL>(s_b, s_h, ly + row, lx0, a, t[row]);
            if (a.grid) {  // uniform: t = s g, the gain looked up with s (step 4 of section 2.26)
                // local_tone.hip's slice_gain in its through-the-cache form, on the chain's own members (cellShift is the
                // statistics' alone).  Built here, inside the branch: built before the loop, the four-pixel kernels grew.
                const SliceArgs slice = {a.grid, {0, a.nz, a.nzShift, a.gx, a.gy, a.colOffset, a.rowOffset}, a.invCell, a.fnz};
                const Tile unstaged = {0, 0, 0};
#pragma unroll
                for (int k = 0; k < PPL; k++) {
                    const pix3 s = {t[row][k][0], t[row][k][1], t[row][k][2]};
                    const float g = slice_gain<0>(s, x0 + k, y + row, r, slice, unstaged, nullptr);
                    t[row][k][0] = s.x * g;
                    t[row][k][1] = s.y * g;
                    t[row][k][2] = s.z * g;
                }
            }
        }
        if constexpr (ChainFmt<FORMAT>::yuv) {
            auto src = [&](int k, int row) { return pix3{t[row][k][0], t[row][k][1], t[row][k][2]}; };
            yuv_block<FORMAT == FMT_NV12 ? 8 : 10>(src, outImg, outPitch, out, outRowBytes, outUV, uvRowBytes, x0, y / 2, width, r, ya, lut);
        } else {
            auto src = [&](int x) {
                pix3 q = {t[0][0][0], t[0][0][1], t[0][0][2]};
#pragma unroll
                for (int k = 1; k < PPL; k++)
                    if (x - x0 == k) q = {t[0][k][0], t[0][k][1], t[0][k][2]};
                return q;
            };
            render_span<FORMAT>(src, outImg ? row_ptr(outImg, outPitch, y) : nullptr,
                                out ? out + (size_t)outRowBytes * (size_t)y : nullptr, x0, width, r, lut);
        }
    }
}

template <int FORMAT, int LDS>
__global__ void __launch_bounds__(kLanes)
    k_chainImage(const pix3* __restrict__ in, int inPitch, const pix3* __restrict__ cnt, int cntPitch, pix3* __restrict__ outImg,
                 int outPitch, uint8_t* __restrict__ out, int outRowBytes, uint8_t* __restrict__ outUV, int uvRowBytes, int width,
                 int height, ChainArgs a, RenderArgs r, YuvArgs ya)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    __shared__ __attribute__((aligned(16))) float s_ac[kFloatsA];
    __shared__ __attribute__((aligned(16))) float s_b[3][kBH][kBW];
    const float* lut = stage_lut<LDS>(r, s_lut);
    auto fetch = [&](int x, int y) { return row_ptr(in, inPitch, y)[x]; };
    auto count = [&](int x, int y) {
        pix3 n = {1.0f, 1.0f, 1.0f};
        if (cnt) n = row_ptr(cnt, cntPitch, y)[x];  // uniform
        return n;
    };
    chain_tile<FORMAT>(fetch, count, s_ac, s_b, outImg, outPitch, out, outRowBytes, outUV, uvRowBytes, width, height, a, r, ya, lut);
}

template <int FORMAT, int LDS>
__global__ void __launch_bounds__(kLanes)
    k_finishChain(const pix3* __restrict__ finalImg, const pix3* __restrict__ weight, int imgPitch, FinishSrc f,
                  pix3* __restrict__ outImg, int outPitch, uint8_t* __restrict__ out, int outRowBytes, uint8_t* __restrict__ outUV,
                  int uvRowBytes, int width, int height, ChainArgs a, RenderArgs r, YuvArgs ya)
{
    __shared__ float s_lut[LDS ? kLdsLutMax + 1 : 1];
    __shared__ __attribute__((aligned(16))) float s_ac[kFloatsA];
    __shared__ __attribute__((aligned(16))) float s_b[3][kBH][kBW];
    const float* lut = stage_lut<LDS>(r, s_lut);
    // k_finishRendered's value (finish_value_at: one definition); y may be negative (rowsAbove)
    auto fetch = [&](int x, int y) { return finish_value_at(finalImg, weight, imgPitch, x, y, f); };
    // step 2 of section 2.24: the count apply_weight_f divided by (y may be negative here too)
    auto count = [&](int x, int y) {
        pix3 n = *(const pix3*)((const char*)weight + (long long)imgPitch * y + 12LL * x);
        if (n.x < f.threshold) n.x += 1;
        if (n.y < f.threshold) n.y += 1;
        if (n.z < f.threshold) n.z += 1;
        return n;
    };
    chain_tile<FORMAT>(fetch, count, s_ac, s_b, outImg, outPitch, out, outRowBytes, outUV, uvRowBytes, width, height, a, r, ya, lut);
}

bool tone_stage_on(const mfsr_finish_chain* c) { return c->useLocalTone != 0; }

// a stage that is off keeps its zeros (R = 0, grid = null)
ChainArgs chain_args(const mfsr_finish_chain* c, const float* gridDev, int yLo, int yHi, int colOffset, int rowOffset, int fullWidth,
                     int fullHeight)
{
    ChainArgs a;
    memset(&a, 0, sizeof(a));
    if (denoise_on(&c->denoise)) {
        const DenoiseArgs d = denoise_args(&c->denoise, yLo, yHi);
        a.gain = d.gain;
        a.alpha = d.alpha;
        a.beta = d.beta;
        a.hh = d.hh;
        a.wHi = d.wHi;
        a.rSpan = d.rSpan;
        a.fade = d.fade;
        a.Rd = d.R;
    }
    if (sharpen_on(&c->sharpen)) {
        const SharpenArgs s = sharpen_args(&c->sharpen, yLo, yHi);
        memcpy(a.k, s.k, sizeof(a.k));
        a.amount = s.amount;
        a.threshold = s.threshold;
        a.Rs = s.R;
    }
    if (tone_stage_on(c)) {
        const mfsr_local_tone* lt = &c->localTone;
        a.grid = gridDev;
        a.nz = lt->bins;
        a.nzShift = ilog2(lt->bins);
        a.gx = (int)mfsr_cdiv(fullWidth, lt->cell);
        a.gy = (int)mfsr_cdiv(fullHeight, lt->cell);
        a.colOffset = colOffset;
        a.rowOffset = rowOffset;
        a.invCell = 1.0f / (float)lt->cell;
        a.fnz = (float)lt->bins;
    }
    a.yLo = yLo;
    a.yHi = yHi;
    return a;
}

// The outputs of a launch of w x h pixels: the format's alignment and length rules (two-plane: even extents and both planes or
// neither), one output at least, and none of them -- the float image, the integer output or Y plane, the chroma plane -- overlaps
// the `readBytes` bytes at `read` (a stencil cannot run in place: stencil_outputs_apart, extended to the chroma plane)
int chain_outputs(const void* read, long long readBytes, const void* outImg, int outImgRowBytes, const void* out, int outRowBytes,
                  const void* outUV, int uvRowBytes, int format, int w, int h)
{
    MFSR_REQUIRE(outImg || out);
    if (!yuv_format(format)) {
        MFSR_REQUIRE(outUV == nullptr);
        return stencil_outputs_apart(read, readBytes, outImg, outImgRowBytes, out, outRowBytes, format, w, h);
    }
    MFSR_REQUIRE((w & 1) == 0 && (h & 1) == 0);
    if (int rc = check_planes(format, out, outRowBytes, outUV, uvRowBytes, w)) return rc;
    if (outImg) MFSR_REQUIRE(!ranges_overlap(read, readBytes, outImg, image_span(outImgRowBytes, h, 12, w)));
    if (out) {
        const long long rowBytes = (format == MFSR_OUT_NV12 ? 1LL : 2LL) * w;
        MFSR_REQUIRE(!ranges_overlap(read, readBytes, out, (long long)outRowBytes * (h - 1) + rowBytes));
        MFSR_REQUIRE(!ranges_overlap(read, readBytes, outUV, (long long)uvRowBytes * (h / 2 - 1) + rowBytes));
    }
    return MFSR_OK;
}

// what both launch entries ask of the description, the grid and the render description (*use: the one of the launch)
int chain_description(const mfsr_finish_chain* chain, const float* gridDev, const mfsr_render* render, const mfsr_render* plain,
                      const mfsr_render** use)
{
    if (int rc = mfsr_finish_chain_validate(chain)) return rc;
    MFSR_REQUIRE(denoise_on(&chain->denoise) || sharpen_on(&chain->sharpen) || tone_stage_on(chain));  // all off: call the plain entries
    MFSR_REQUIRE((gridDev != nullptr) == tone_stage_on(chain) && ((uintptr_t)gridDev & 3) == 0);
    if (!render) render = plain;
    if (int rc = mfsr_render_validate(render)) return rc;
    *use = render;
    return MFSR_OK;
}

}  // namespace

// one launch of KERNEL<format, lds> over the tiles of w x h pixels; w, h and stream are the caller's: the single-plane formats as
// every stencil kernel (FORMAT_LUT_DISPATCH), and the two two-plane ones
#define CHAIN_CASE(KERNEL, F, L, ...) \
    case ((F) << 1) | (L): hipLaunchKernelGGL((KERNEL<F, L>), grid, block, 0, mfsr_s(stream), __VA_ARGS__); break
#define CHAIN_DISPATCH(KERNEL, format, lds, ...)                                               \
    do {                                                                                       \
        const dim3 grid(mfsr_cdiv(w, kTW), mfsr_cdiv(h, kTH)), block(kLanes);                  \
        switch (((format) << 1) | ((lds) ? 1 : 0)) {                                           \
            CHAIN_CASE(KERNEL, MFSR_OUT_NV12, 0, __VA_ARGS__);                                 \
            CHAIN_CASE(KERNEL, MFSR_OUT_NV12, 1, __VA_ARGS__);                                 \
            CHAIN_CASE(KERNEL, MFSR_OUT_P010, 0, __VA_ARGS__);                                 \
            CHAIN_CASE(KERNEL, MFSR_OUT_P010, 1, __VA_ARGS__);                                 \
            default: FORMAT_LUT_DISPATCH(KERNEL, grid, block, format, lds, __VA_ARGS__); break; \
        }                                                                                      \
    } while (0)

extern "C" int mfsr_chain_tile(int* tileW, int* tileH)
{
    MFSR_REQUIRE(tileW && tileH);
    *tileW = kTW;
    *tileH = kTH;
    return MFSR_OK;
}

extern "C" int mfsr_finish_chain_validate(const mfsr_finish_chain* chain)
{
    MFSR_REQUIRE(chain != nullptr);
    if (int rc = mfsr_denoise_validate(&chain->denoise)) return rc;
    if (int rc = mfsr_sharpen_validate(&chain->sharpen)) return rc;
    if (int rc = mfsr_local_tone_validate(&chain->localTone)) return rc;
    MFSR_REQUIRE(chain->useLocalTone == 0 || chain->useLocalTone == 1);
    for (int i = 0; i < 7; i++) MFSR_REQUIRE(chain->reserved[i] == 0);
    return MFSR_OK;
}

extern "C" int mfsr_finish_chain_reach(const mfsr_finish_chain* chain, int* rows)
{
    MFSR_REQUIRE(rows != nullptr);
    if (int rc = mfsr_finish_chain_validate(chain)) return rc;
    *rows = (denoise_on(&chain->denoise) ? chain->denoise.radius : 0) + (sharpen_on(&chain->sharpen) ? chain->sharpen.radius : 0);
    return MFSR_OK;
}

extern "C" int mfsr_chainImage(const mfsr_float3* in, int inRowBytes, const mfsr_float3* count, int countRowBytes, mfsr_float3* outImg,
                               int outImgRowBytes, void* out, int outRowBytes, void* outUV, int uvRowBytes, int w, int h,
                               const mfsr_render* render, int applyGamma, const mfsr_finish_chain* chain, const float* gridDev,
                               int colOffset, int rowOffset, int fullWidth, int fullHeight, mfsr_stream_t stream)
{
    // host validation first: nothing below touches the device before every argument has passed
    if (int rc = stencil_image_args(in, inRowBytes, outImg, outImgRowBytes, out ? out : outUV, w, h)) return rc;
    if (count) MFSR_REQUIRE((long long)countRowBytes >= 12LL * w && (countRowBytes & 3) == 0 && ((uintptr_t)count & 3) == 0);
    const mfsr_render plain = mfsr_plain_render();
    if (int rc = chain_description(chain, gridDev, render, &plain, &render)) return rc;
    MFSR_REQUIRE(rowOffset >= 0 && fullHeight >= rowOffset + h && colOffset >= 0 && fullWidth >= colOffset + w);
    if (int rc = chain_outputs(in, image_span(inRowBytes, h, 12, w), outImg, outImgRowBytes, out, outRowBytes, outUV, uvRowBytes,
                               render->format, w, h))
        return rc;
    if (count)
        if (int rc = chain_outputs(count, image_span(countRowBytes, h, 12, w), outImg, outImgRowBytes, out, outRowBytes, outUV,
                                   uvRowBytes, render->format, w, h))
            return rc;
    const RenderArgs ra = render_args(render, applyGamma);
    const YuvArgs ya = yuv_args(render);
    const ChainArgs ca = chain_args(chain, gridDev, 0, h - 1, colOffset, rowOffset, fullWidth, fullHeight);
    const bool lds = stencil_lut_in_lds(render);
    CHAIN_DISPATCH(k_chainImage, render->format, lds, (const pix3*)in, inRowBytes, (const pix3*)count, countRowBytes, (pix3*)outImg,
                   outImgRowBytes, (uint8_t*)out, outRowBytes, (uint8_t*)outUV, uvRowBytes, w, h, ca, ra, ya);
    return mfsr_launch_status("chainImage");
}

extern "C" int mfsr_finishChain(const mfsr_float3* finalImg, const mfsr_float3* weight, int imgRowBytes, const mfsr_float3* fallback,
                                int fbRowBytes, int fbW, int fbH, float u0, float u1, float v0, float v1, mfsr_float3* outImg,
                                int outImgRowBytes, void* out, int outRowBytes, void* outUV, int uvRowBytes, const mfsr_render* render,
                                int w, int h, float threshold, int applyGamma, int colOffset, int rowOffset, int fullWidth,
                                int fullHeight, const mfsr_finish_chain* chain, const float* gridDev, int rowsAbove, int rowsBelow,
                                mfsr_stream_t stream)
{
    if (int rc = stencil_finish_args(finalImg, weight, imgRowBytes, fallback, fbRowBytes, fbW, fbH, outImg, outImgRowBytes,
                                     out ? out : outUV, w, h, colOffset, rowOffset, fullWidth, fullHeight, rowsAbove, rowsBelow))
        return rc;
    const mfsr_render plain = mfsr_plain_render();
    if (int rc = chain_description(chain, gridDev, render, &plain, &render)) return rc;
    // no output may overlap the accumulator or weight rows the launch reads: its own and the reach's (stencil_finish_apart)
    const long long readBytes = (long long)imgRowBytes * (h - 1 + rowsAbove + rowsBelow) + 12LL * w;
    for (const void* img : {(const void*)finalImg, (const void*)weight})
        if (int rc = chain_outputs((const char*)img - (long long)imgRowBytes * rowsAbove, readBytes, outImg, outImgRowBytes, out,
                                   outRowBytes, outUV, uvRowBytes, render->format, w, h))
            return rc;
    const RenderArgs ra = render_args(render, applyGamma);
    const YuvArgs ya = yuv_args(render);
    const ChainArgs ca = chain_args(chain, gridDev, -rowsAbove, h - 1 + rowsBelow, colOffset, rowOffset, fullWidth, fullHeight);
    const bool lds = stencil_lut_in_lds(render);
    const FinishSrc f = finish_src(fallback, fbRowBytes, fbW, fbH, u0, u1, v0, v1, threshold, colOffset, rowOffset, fullWidth, fullHeight);
    CHAIN_DISPATCH(k_finishChain, render->format, lds, (const pix3*)finalImg, (const pix3*)weight, imgRowBytes, f, (pix3*)outImg,
                   outImgRowBytes, (uint8_t*)out, outRowBytes, (uint8_t*)outUV, uvRowBytes, w, h, ca, ra, ya);
    return mfsr_launch_status("finishChain");
}
