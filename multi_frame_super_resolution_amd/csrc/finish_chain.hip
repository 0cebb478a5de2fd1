// finish_chain.hip -- the finish chain: merge-aware denoise (section 2.24), then the unsharp mask
// (section 2.20), then the local-tone gain (section 2.25), then matrix, tone and the store of any output format -- the four
// single-plane ones (section 2.19) and NV12 / P010 (section 2.21) -- in ONE launch on the value the finish holds
// (mfsr_finishChain), and the same tile body on an existing float image with an optional count image (mfsr_chainImage).  Each
// stage is on or off at run time.  gfx950, wave64.
//
// The result is, bit for bit, the composition of the existing whole-image entry points (mfsr_finishDenoised to a float image,
// mfsr_sharpenImage to a float image, then mfsr_localToneImage / mfsr_renderImage / mfsr_renderImageYuv).  Every step is float32
// + - * / fmaxf fminf with -ffp-contract=off (the Makefile) in the order include/mfsr.h writes it.  The per-pixel arithmetic of
// the four stages is RESTATED here in that order (denoise.hip's window sums, sharpen.hip's two passes and coring,
// local_tone.hip's slice_gain in its through-the-cache form, render_yuv.hip's yuv_block); those files are untouched and their
// kernels compile to the code they always did.  finish_value, render_pixel and render_span are the shared headers' own.
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
#include "stencil_host.hpp"

namespace {

constexpr int kTW = 64, kTH = 16, kLanes = 256;
constexpr int kMaxRd = 3, kMaxRs = 4, kMaxR = kMaxRd + kMaxRs;
constexpr int kPadA = 8, kAW = kTW + 2 * kPadA, kAH = kTH + 2 * kMaxR;   // 80 x 30
constexpr int kPadB = 4, kBW = kTW + 2 * kPadB, kBH = kTH + 2 * kMaxRs;  // 72 x 24
constexpr int kFloatsA = 3 * kAH * kAW, kFloatsC = 3 * kBH * kTW;
static_assert(kPadA >= kMaxR && kPadB >= kMaxRs && kFloatsC <= kFloatsA, "stage C reuses stage A's storage");
constexpr int FMT_NV12 = MFSR_OUT_NV12, FMT_P010 = MFSR_OUT_P010;

struct ChainArgs {
    // denoise (section 2.24)
    float gain, alpha, beta, hh;  // hh = strength * strength
    float wHi, rSpan;             // the fade; used when fade != 0
    int fade;
    int Rd;                       // 0 = the stage is off
    // sharpen (section 2.20)
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

struct YuvArgs {
    float kr, kg, kb, sb, sr;  // Y = (kr c0 + kg c1) + kb c2;  Cb = (c2 - Y) sb;  Cr = (c0 - Y) sr
    float yOff, yScale;        // yq = yOff + yScale * Y
    float cOff, cScale;        // cq = cOff + cScale * C
    float maxCode;             // 2^N - 1
};

template <int FORMAT>
struct ChainFmt {
    static constexpr bool yuv = FORMAT == FMT_NV12 || FORMAT == FMT_P010;
    static constexpr int ppl = yuv ? 4 : Fmt<FORMAT>::ppl;  // consecutive pixels of a row one lane owns
    static constexpr int rows = yuv ? 2 : 1;                // rows of a lane's block
};

// the cleaning of the first stage that is on: the denoise's (step 1 of section 2.24), the sharpen's (step 1 of section 2.20),
// or none (the local-tone gain and the render take p as it is)
__device__ __forceinline__ float clean_value(float p, int Rd, int Rs)
{
    if (Rd) return isnan(p) ? 0.0f : fminf(fmaxf(p, -65536.0f), 65536.0f);  // uniform
    if (Rs) return isnan(p) ? 0.0f : p;
    return p;
}

__device__ __forceinline__ float fade_of(float n, const ChainArgs& a)
{
    return a.fade ? fminf(fmaxf((a.wHi - n) * a.rSpan, 0.0f), 1.0f) : 1.0f;
}

// N consecutive floats of an LDS row; N = 4: one 16-byte read (the address is 16-byte aligned, see the file's header)
template <int N>
__device__ __forceinline__ void load_span(const float* p, float (&v)[N])
{
    if constexpr (N == 4) {
        const float4 q = *(const float4*)p;
        v[0] = q.x;
        v[1] = q.y;
        v[2] = q.z;
        v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = p[k];
    }
}

// ---- section 2.25's gain, the through-the-cache form of local_tone.hip's slice_gain, in its order
struct Axis {
    int i0, i1;
    float a;
};

__device__ __forceinline__ Axis grid_axis(int X, float invCell, int n)
{
    float fx = ((float)X + 0.5f) * invCell - 0.5f;
    fx = fminf(fmaxf(fx, 0.0f), (float)(n - 1));
    Axis r;
    r.i0 = (int)fx;
    r.i1 = min(r.i0 + 1, n - 1);
    r.a = fx - (float)r.i0;
    return r;
}

__device__ __forceinline__ float chain_gain(pix3 p, int x, int y, const RenderArgs& r, const ChainArgs& t)
{
    const pix3 q = r.useMatrix ? matrix_pixel(p, r.m) : p;  // uniform
    const float v0 = isnan(q.x) ? 0.0f : fminf(fmaxf(q.x, 0.0f), 1.0f);
    const float v1 = isnan(q.y) ? 0.0f : fminf(fmaxf(q.y, 0.0f), 1.0f);
    const float v2 = isnan(q.z) ? 0.0f : fminf(fmaxf(q.z, 0.0f), 1.0f);
    const float l = ((54.0f * v0 + 183.0f * v1) + 19.0f * v2) * (1.0f / 256.0f);
    const Axis ax = grid_axis(x + t.colOffset, t.invCell, t.gx);
    const Axis ay = grid_axis(y + t.rowOffset, t.invCell, t.gy);
    float fz = l * t.fnz - 0.5f;
    fz = fminf(fmaxf(fz, 0.0f), (float)(t.nz - 1));
    const int k0 = (int)fz;
    const float az = fz - (float)k0;
    const int k1 = min(k0 + 1, t.nz - 1);
    const float* g0 = t.grid + (((size_t)ay.i0 * t.gx) << t.nzShift);
    const float* g1 = t.grid + (((size_t)ay.i1 * t.gx) << t.nzShift);
    const int o0 = ax.i0 << t.nzShift, o1 = ax.i1 << t.nzShift;
    const float2 c00 = make_float2(g0[o0 + k0], g0[o0 + k1]), c01 = make_float2(g0[o1 + k0], g0[o1 + k1]);
    const float2 c10 = make_float2(g1[o0 + k0], g1[o0 + k1]), c11 = make_float2(g1[o1 + k0], g1[o1 + k1]);
    const float z00 = c00.x + (c00.y - c00.x) * az, z01 = c01.x + (c01.y - c01.x) * az;
    const float z10 = c10.x + (c10.y - c10.x) * az, z11 = c11.x + (c11.y - c11.x) * az;
    const float x0 = z00 + (z01 - z00) * ax.a, x1 = z10 + (z11 - z10) * ax.a;
    return x0 + (x1 - x0) * ay.a;
}

// ---- section 2.21's store, render_yuv.hip's in its order
__device__ __forceinline__ float unit_clamp(float o) { return isnan(o) ? 0.0f : fminf(fmaxf(o, 0.0f), 1.0f); }

__device__ __forceinline__ uint32_t yuv_code(float v, float maxCode) { return (uint32_t)(int)(fminf(fmaxf(v, 0.0f), maxCode) + 0.5f); }

// `n` (2 or 4) samples of codes q[] at `dst`: one wide store when the lane has all four and `wide` (the row's first sample is
// aligned to the store: uniform per row), else sample by sample.  P010 words carry the code in bits 15..6.
template <int BITS>
__device__ __forceinline__ void store_samples(uint8_t* dst, const uint32_t q[4], int n, bool wide)
{
    if constexpr (BITS == 8) {
        if (n == 4 && wide) {
            *(uint32_t*)dst = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < n) dst[k] = (uint8_t)q[k];
        }
    } else {
        uint16_t* d16 = (uint16_t*)dst;
        if (n == 4 && wide) {
            uint2 v;
            v.x = q[0] << 6 | q[1] << 22;
            v.y = q[2] << 6 | q[3] << 22;
            *(uint2*)dst = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < n) d16[k] = (uint16_t)(q[k] << 6);
        }
    }
}

// The 2 x 4 block with top-left pixel (x0, 2 * yPair) of the launch; t[row][k] is the value before step 1 of section 2.19.
// width and height are even, so the block holds 2 or 4 whole columns and both rows.
template <int BITS>
__device__ __forceinline__ void yuv_store(const float (&t)[2][4][3], pix3* outImg, int outPitch, uint8_t* outY, int yRowBytes,
                                          uint8_t* outUV, int uvRowBytes, int x0, int yPair, int width, const RenderArgs& r,
                                          const YuvArgs& ya, const float* lut)
{
    constexpr int BPS = BITS == 8 ? 1 : 2;          // bytes per sample
    constexpr uintptr_t WIDE = BITS == 8 ? 3 : 7;   // alignment mask of the wide store
    const int n = width - x0 >= 4 ? 4 : 2;
    float cb[4], cr[4];  // row 0's chroma, then the 2 x 2 sums
#pragma unroll
    for (int row = 0; row < 2; row++) {
        const int y = 2 * yPair + row;
        pix3* imgRow = outImg ? row_ptr(outImg, outPitch, y) : nullptr;
        uint32_t q[4] = {0, 0, 0, 0};
        float rb[4], rr[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            rb[k] = rr[k] = 0.0f;
            if (k < n) {
                const pix3 in = {t[row][k][0], t[row][k][1], t[row][k][2]};
                const pix3 o = render_pixel(in, r, lut);
                if (imgRow) imgRow[x0 + k] = o;
                const float c0 = unit_clamp(o.x), c1 = unit_clamp(o.y), c2 = unit_clamp(o.z);
                const float Y = (ya.kr * c0 + ya.kg * c1) + ya.kb * c2;
                rb[k] = (c2 - Y) * ya.sb;
                rr[k] = (c0 - Y) * ya.sr;
                q[k] = yuv_code(ya.yOff + ya.yScale * Y, ya.maxCode);
            }
        }
        if (outY) {
            uint8_t* yRow = outY + (size_t)yRowBytes * (size_t)y;
            store_samples<BITS>(yRow + (size_t)x0 * BPS, q, n, ((uintptr_t)yRow & WIDE) == 0);
        }
        // x first, rows second: ((C(x, y) + C(x+1, y)) + (C(x, y+1) + C(x+1, y+1))) * 0.25
        if (row == 0) {
            cb[0] = rb[0] + rb[1];
            cb[1] = rb[2] + rb[3];
            cr[0] = rr[0] + rr[1];
            cr[1] = rr[2] + rr[3];
        } else {
            cb[0] = (cb[0] + (rb[0] + rb[1])) * 0.25f;
            cb[1] = (cb[1] + (rb[2] + rb[3])) * 0.25f;
            cr[0] = (cr[0] + (rr[0] + rr[1])) * 0.25f;
            cr[1] = (cr[1] + (rr[2] + rr[3])) * 0.25f;
        }
    }
    if (!outUV) return;
    uint32_t q[4];
    q[0] = yuv_code(ya.cOff + ya.cScale * cb[0], ya.maxCode);
    q[1] = yuv_code(ya.cOff + ya.cScale * cr[0], ya.maxCode);
    q[2] = yuv_code(ya.cOff + ya.cScale * cb[1], ya.maxCode);
    q[3] = yuv_code(ya.cOff + ya.cScale * cr[1], ya.maxCode);
    // x0 / 2 (Cb, Cr) pairs = x0 samples into the chroma row
    uint8_t* uvRow = outUV + (size_t)uvRowBytes * (size_t)yPair;
    store_samples<BITS>(uvRow + (size_t)x0 * BPS, q, n, ((uintptr_t)uvRow & WIDE) == 0);
}

// ---- steps 2-6 of section 2.24 at the pixel whose cleaned value sits at s_a[.][ay][ac]: denoise.hip's one-pixel-per-lane body.
// n3: the count before its NaN cleaning.  Called by every lane of a wave (`live`: the lane has a position); a wave whose every
// position has lambda == 0 in every channel skips the stencil.
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
        n[c] = isnan(nn[c]) ? 0.0f : nn[c];
        need = need || (live && fade_of(n[c], a) != 0.0f);
        o[c] = s[c];
    }
    if (!__any(need)) return;
    float rr[3], G = 0.0f, S[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float v = fmaxf((a.gain * (a.alpha * fmaxf(s[c], 0.0f) + a.beta)) / fmaxf(n[c], 1e-6f), 1e-20f);
        rr[c] = 1.0f / (a.hh * v);
    }
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
            for (int k = 0; k < N; k++) b[k] = b[k] + a.k[d] * (up[k] + dn[k]);
        }
#pragma unroll
        for (int k = 0; k < N; k++) {
            const float e = s[k] - b[k];
            const float t = fabsf(e) - a.threshold;
            const float g = t > 0.0f ? copysignf(t, e) : 0.0f;
            o[k][c] = s[k] + a.amount * g;
        }
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
            s_a[0][ly][c0] = clean_value(p.x, Rd, Rs);
            s_a[1][ly][c0] = clean_value(p.y, Rd, Rs);
            s_a[2][ly][c0] = clean_value(p.z, Rd, Rs);
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
            s_b[0][by][c0] = clean_value(p.x, Rd, Rs);
            s_b[1][by][c0] = clean_value(p.y, Rd, Rs);
            s_b[2][by][c0] = clean_value(p.z, Rd, Rs);
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
                for (int d = 1; d <= Rs; d++) h = h + a.k[d] * (row[-d] + row[d]);
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
#pragma unroll
                for (int k = 0; k < PPL; k++) {
                    const pix3 s = {t[row][k][0], t[row][k][1], t[row][k][2]};
                    const float g = chain_gain(s, x0 + k, y + row, r, a);
                    t[row][k][0] = s.x * g;
                    t[row][k][1] = s.y * g;
                    t[row][k][2] = s.z * g;
                }
            }
        }
        if constexpr (ChainFmt<FORMAT>::yuv) {
            yuv_store<FORMAT == FMT_NV12 ? 8 : 10>(t, outImg, outPitch, out, outRowBytes, outUV, uvRowBytes, x0, y / 2, width, r, ya, lut);
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

bool denoise_stage_on(const mfsr_finish_chain* c) { return c->denoise.radius != 0 && c->denoise.strength != 0.0f; }
bool sharpen_stage_on(const mfsr_finish_chain* c) { return c->sharpen.radius != 0 && c->sharpen.amount != 0.0f; }
bool tone_stage_on(const mfsr_finish_chain* c) { return c->useLocalTone != 0; }

int ilog2(int v)
{
    int s = 0;
    while ((1 << s) < v) s++;
    return s;
}

ChainArgs chain_args(const mfsr_finish_chain* c, const float* gridDev, int yLo, int yHi, int colOffset, int rowOffset, int fullWidth,
                     int fullHeight)
{
    ChainArgs a;
    memset(&a, 0, sizeof(a));
    if (denoise_stage_on(c)) {
        const mfsr_denoise* d = &c->denoise;
        a.gain = d->gain;
        a.alpha = d->alpha;
        a.beta = d->beta;
        a.hh = d->strength * d->strength;
        a.fade = d->wHi > d->wLo;
        a.wHi = d->wHi;
        a.rSpan = a.fade ? 1.0f / (d->wHi - d->wLo) : 0.0f;
        a.Rd = d->radius;
    }
    if (sharpen_stage_on(c)) {
        const mfsr_sharpen* s = &c->sharpen;
        for (int d = 0; d <= kMaxRs; d++) a.k[d] = d <= s->radius ? s->taps[d] : 0.0f;
        a.amount = s->amount;
        a.threshold = s->threshold;
        a.Rs = s->radius;
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

// render_yuv.hip's constants: the float32 roundings of doubles; the scales are exact in float32
YuvArgs yuv_args(const mfsr_render* r)
{
    static const double K[3][2] = {{0.2126, 0.0722}, {0.299, 0.114}, {0.2627, 0.0593}};  // Kr, Kb: BT.709, BT.601, BT.2020
    YuvArgs a;
    memset(&a, 0, sizeof(a));
    if (!yuv_format(r->format)) return a;
    const int std_ = r->reserved[0] & 3, full = r->reserved[0] & MFSR_YUV_FULL;
    const double kr = K[std_][0], kb = K[std_][1];
    const int bits = r->format == MFSR_OUT_NV12 ? 8 : 10;
    const float m = (float)(1 << (bits - 8)), M = (float)((1 << bits) - 1);
    a.kr = (float)kr;
    a.kg = (float)(1.0 - kr - kb);
    a.kb = (float)kb;
    a.sb = (float)(0.5 / (1.0 - kb));
    a.sr = (float)(0.5 / (1.0 - kr));
    a.yOff = full ? 0.0f : 16.0f * m;
    a.yScale = full ? M : 219.0f * m;
    a.cOff = full ? (float)(1 << (bits - 1)) : 128.0f * m;
    a.cScale = full ? M : 224.0f * m;
    a.maxCode = M;
    return a;
}

// The outputs of a launch of w x h pixels: the format's alignment and length rules (two-plane: even extents and both planes or
// neither), one output at least, and none of them -- the float image, the integer output or Y plane, the chroma plane -- overlaps
// the `readBytes` bytes at `read` (a stencil cannot run in place: stencil_outputs_apart, extended to the chroma plane)
int chain_outputs(const void* read, long long readBytes, const void* outImg, int outImgRowBytes, const void* out, int outRowBytes,
                  const void* outUV, int uvRowBytes, int format, int w, int h)
{
    if (!yuv_format(format)) {
        MFSR_REQUIRE(outUV == nullptr);
        MFSR_REQUIRE(outImg || out);
        return stencil_outputs_apart(read, readBytes, outImg, outImgRowBytes, out, outRowBytes, format, w, h);
    }
    MFSR_REQUIRE((w & 1) == 0 && (h & 1) == 0);
    MFSR_REQUIRE((out != nullptr) == (outUV != nullptr));
    MFSR_REQUIRE(outImg || out);
    const long long bps = format == MFSR_OUT_NV12 ? 1 : 2, rowBytes = bps * w;
    if (out) {
        MFSR_REQUIRE((long long)outRowBytes >= rowBytes && (long long)uvRowBytes >= rowBytes);
        if (format == MFSR_OUT_P010)
            MFSR_REQUIRE(((uintptr_t)out & 1) == 0 && ((uintptr_t)outUV & 1) == 0 && (outRowBytes & 1) == 0 && (uvRowBytes & 1) == 0);
    }
    if (outImg) MFSR_REQUIRE(!ranges_overlap(read, readBytes, outImg, image_span(outImgRowBytes, h, 12, w)));
    if (out) {
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
    MFSR_REQUIRE(denoise_stage_on(chain) || sharpen_stage_on(chain) || tone_stage_on(chain));  // all off: call the plain entries
    MFSR_REQUIRE((gridDev != nullptr) == tone_stage_on(chain) && ((uintptr_t)gridDev & 3) == 0);
    if (!render) render = plain;
    if (int rc = mfsr_render_validate(render)) return rc;
    *use = render;
    return MFSR_OK;
}

}  // namespace

#define CHAIN_CASE(KERNEL, F, L, ...) \
    case ((F) << 1) | (L): hipLaunchKernelGGL((KERNEL<F, L>), grid, block, 0, mfsr_s(stream), __VA_ARGS__); break
// one launch of KERNEL<format, lds> over the tiles of w x h pixels; w, h and stream are the caller's
#define CHAIN_DISPATCH(KERNEL, format, lds, ...)                            \
    do {                                                                    \
        const dim3 grid(mfsr_cdiv(w, kTW), mfsr_cdiv(h, kTH)), block(kLanes); \
        switch (((format) << 1) | ((lds) ? 1 : 0)) {                        \
            CHAIN_CASE(KERNEL, MFSR_OUT_RGB16, 0, __VA_ARGS__);             \
            CHAIN_CASE(KERNEL, MFSR_OUT_RGB16, 1, __VA_ARGS__);             \
            CHAIN_CASE(KERNEL, MFSR_OUT_RGB8, 0, __VA_ARGS__);              \
            CHAIN_CASE(KERNEL, MFSR_OUT_RGB8, 1, __VA_ARGS__);              \
            CHAIN_CASE(KERNEL, MFSR_OUT_RGBA8, 0, __VA_ARGS__);             \
            CHAIN_CASE(KERNEL, MFSR_OUT_RGBA8, 1, __VA_ARGS__);             \
            CHAIN_CASE(KERNEL, MFSR_OUT_RGB10A2, 0, __VA_ARGS__);           \
            CHAIN_CASE(KERNEL, MFSR_OUT_RGB10A2, 1, __VA_ARGS__);           \
            CHAIN_CASE(KERNEL, MFSR_OUT_NV12, 0, __VA_ARGS__);              \
            CHAIN_CASE(KERNEL, MFSR_OUT_NV12, 1, __VA_ARGS__);              \
            CHAIN_CASE(KERNEL, MFSR_OUT_P010, 0, __VA_ARGS__);              \
            CHAIN_CASE(KERNEL, MFSR_OUT_P010, 1, __VA_ARGS__);              \
        }                                                                   \
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
    *rows = (denoise_stage_on(chain) ? chain->denoise.radius : 0) + (sharpen_stage_on(chain) ? chain->sharpen.radius : 0);
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
