// accumulate_fast.hip -- the full-frame warp+fuse kernels of the headline benchmark (x2 and x4),
// restructured for CDNA4.  Same mathematics as accumulateImagesSuperRes (reference
// test_opencv/DeBayerKernels.cu:379-468, full-frame generalisation), accumulators in HBM as in the
// reference (48 B per HR pixel and frame in its one-launch-per-frame structure; these kernels also take
// up to four frames per launch and move the accumulators once for all of them).
//
// Why not the straight port (accumulate.hip): it spends its time in VALU/SALU work, not in HBM -- per tap
// an IEEE division, a 3-way colour branch and a 16-byte certainty load (1.67 ms per 4K frame = 13 % of
// HBM peak).  These kernels remove that work without changing what is computed:
//
//  * 4-pixel strips: one thread owns HR pixels X0..X0+3 of one row; the certainty cell a tap reads is a
//    compile-time function of the pixel's position in the strip (template parameter K).
//  * raw sites instead of taps: the 5x5 HR taps of a pixel fall on 3x3 (x2) or 2x2 (x4) raw pixels.
//    Which site a tap lands on depends on the low bits of (X + round(s*u)); that choice is applied to the
//    WEIGHTS with lane masks (v_and / v_bitop3, no v_cndmask), the raw values enter with a few fma.
//  * no per-tap division: sum raw*w*c and w*c per CFA position, normalise once per pixel:
//    sum((raw-b)/wl * w*c) = (sum(raw*w*c) - b*sum(w*c)) / wl.
//  * no colour branches: sites are summed per CFA-position class (row/column parity relative to the first
//    site); classes map to R/G/B once per pixel (the CFA pattern is a template parameter).
//  * 12 exponentials per pixel instead of 25: w(px,py) = w(-px,-py), v_exp_f32, exponents from sums -- and, with
//    several frames per launch, once per pixel for all of them (pixel-major order: the weights depend on the kernel
//    parameters of the reference only).
//  * LDS tile kernels (fields at the tracking resolution): field / certainty texels, interpolation
//    fractions and the accumulator rows (LDS-DMA) staged per workgroup; see k_accumulate2xTile.
//
// Numerics: the flow rounding is the same expression as in the straight kernel and the oracle; weights
// and per-channel sums are re-associated (pre-scaled exponents, class sums, fma, one normalisation), so
// results agree with the straight kernel to ~1e-6 relative (tests: 3e-5), not bit for bit.  Pixels whose
// taps would be clamped at the frame border, strips with wild flow and strips whose kernel parameters
// are not positive semi-definite take the straight per-pixel arithmetic (margin kernel / in-kernel path).
#include <cstdlib>

#include "accumulate_common.hpp"
#include "finish_common.hpp"
#include "finish_ring.hpp"
#include <type_traits>

namespace {

// CFA packed 2 bits per CFA position a = (yparity << 1) | xparity
template <int CFA>
struct Cfa {
    static constexpr int col(int yp, int xp) { return (CFA >> (2 * ((yp << 1) | xp))) & 3; }
    // position of the (single) red / blue site; -1 if the pattern has none
    static constexpr int pos_of(int c)
    {
        int n = 0, p = -1;
        for (int a = 0; a < 4; a++)
            if (((CFA >> (2 * a)) & 3) == c) {
                n++;
                p = a;
            }
        return n == 1 ? p : -1;
    }
    static constexpr int count(int c)
    {
        int n = 0;
        for (int a = 0; a < 4; a++)
            if (((CFA >> (2 * a)) & 3) == c) n++;
        return n;
    }
};

struct StripLevels {
    float black[3];
    float invWhite[3];
};

__device__ __forceinline__ float sane(float c) { return finitef(c) ? c : 0.0f; }

// fast-path admission: kernel parameters form a positive semi-definite inverse covariance
// (so every tap exponent is >= 0 and every weight is in [0,1]); NaN fails the comparisons
__device__ __forceinline__ bool psd_ok(float kx, float ky, float kz)
{
    return kx >= 0.0f && ky >= 0.0f && kz * kz <= kx * ky && kx < 1e30f && ky < 1e30f;
}

// one HR pixel of a safe strip.  K = position in the strip (compile time).
// MaskF: float mval(int jt, int cell, int ch) -> sanitised certainty of channel ch in mask cell
// `cell` (0..2, relative to the strip) on the mask row that tap row jt reads.
// Per-lane two-way selects are written as bit-field inserts on lane masks (v_bitop3_b32, a plain
// 3-operand VALU op) instead of v_cndmask_b32 + v_cmp: on gfx950 v_cndmask/v_cmp issue at ~0.69x the
// rate of v_add/v_fma/v_bitop3 (tools/ubench/valu_ops.hip: 1.95 vs 1.3 ns per wave-instruction per
// SIMD) and selects are a third of this kernel's instructions.
__device__ __forceinline__ float selm(uint32_t m, float a, float b)  // m == ~0u ? a : b
{
    // one v_bitop3_b32 with truth table 0xCA = (m & a) | (~m & b)
    return __uint_as_float(__builtin_amdgcn_bitop3_b32(m, __float_as_uint(a), __float_as_uint(b), 0xCA));
}

// certainty of the colour under an even (Ee) / odd (Eo) site column of a tap row, from the three channel
// certainties m[] of a mask cell.  mya: lane mask "the site row has absolute y parity 1"; mP: "site
// column 0 has absolute x parity 1".
template <int CFA>
__device__ __forceinline__ void resolve_certainty(uint32_t mya, uint32_t mP, const float (&m)[3], float& Ee, float& Eo)
{
    constexpr bool mono = Cfa<CFA>::count(MFSR_GREEN) == 4;
    if (mono) {
        Ee = Eo = m[MFSR_GREEN];
    } else if (Cfa<CFA>::col(0, 1) == Cfa<CFA>::col(1, 0)) {
        // Bayer, G on the anti-diagonal (RGGB, BGGR): the colour on the diagonal is picked by the y
        // parity alone; even site columns see it when x parity == y parity, else they see G
        const float X = selm(mya, m[Cfa<CFA>::col(1, 1)], m[Cfa<CFA>::col(0, 0)]);
        const uint32_t d = mya ^ mP;  // x parity != y parity
        Ee = selm(d, m[Cfa<CFA>::col(0, 1)], X);
        Eo = selm(d, X, m[Cfa<CFA>::col(0, 1)]);
    } else if (Cfa<CFA>::col(0, 0) == Cfa<CFA>::col(1, 1)) {
        // Bayer, G on the diagonal (GRBG, GBRG)
        const float X = selm(mya, m[Cfa<CFA>::col(1, 0)], m[Cfa<CFA>::col(0, 1)]);
        const uint32_t d = mya ^ mP;
        Ee = selm(d, X, m[Cfa<CFA>::col(0, 0)]);
        Eo = selm(d, m[Cfa<CFA>::col(0, 0)], X);
    } else {
        const float cA = selm(mya, m[Cfa<CFA>::col(1, 0)], m[Cfa<CFA>::col(0, 0)]);  // absolute x parity 0
        const float cB = selm(mya, m[Cfa<CFA>::col(1, 1)], m[Cfa<CFA>::col(0, 1)]);  // absolute x parity 1
        Ee = selm(mP, cB, cA);
        Eo = selm(mP, cA, cB);
    }
}

// relative CFA-position class sums (class (yc, xc) sits at CFA position (yc ^ Q, xc ^ P)) -> R, G, B,
// normalised and added to pixel K of the strip
template <int K, int CFA>
__device__ __forceinline__ void classes_to_channels(const float (&S)[2][2], const float (&W)[2][2], uint32_t mP, uint32_t mQ,
                                                    const StripLevels& lv, float* accP, float* accW)
{
    constexpr bool mono = Cfa<CFA>::count(MFSR_GREEN) == 4;
    auto at_pos = [&](const float(&T)[2][2], int yp, int xp) {
        const float q0 = selm(mP, T[yp][xp ^ 1], T[yp][xp]);          // Q == 0
        const float q1 = selm(mP, T[yp ^ 1][xp ^ 1], T[yp ^ 1][xp]);  // Q == 1
        return selm(mQ, q1, q0);
    };
    float chS[3] = {0, 0, 0}, chW[3] = {0, 0, 0};
    const float totS = (S[0][0] + S[0][1]) + (S[1][0] + S[1][1]);
    const float totW = (W[0][0] + W[0][1]) + (W[1][0] + W[1][1]);
    if (mono) {
        chS[1] = totS;
        chW[1] = totW;
    } else {
        constexpr int pr = Cfa<CFA>::pos_of(MFSR_RED), pb = Cfa<CFA>::pos_of(MFSR_BLUE);
        if ((pr ^ pb) == 3) {
            // red and blue on opposite corners of the 2x2 cell (every Bayer pattern): they are the two
            // classes of one diagonal; which diagonal follows from P ^ Q, which end from Q
            const uint32_t dq = ((pr >> 1) ^ (pr & 1)) ? ~(mP ^ mQ) : (mP ^ mQ);  // all ones: the anti-diagonal classes
            const uint32_t mR = (pr >> 1) ? ~mQ : mQ;                            // all ones: red is the class in row 1
            const float s0 = selm(dq, S[0][1], S[0][0]), s1 = selm(dq, S[1][0], S[1][1]);
            const float w0 = selm(dq, W[0][1], W[0][0]), w1 = selm(dq, W[1][0], W[1][1]);
            chS[0] = selm(mR, s1, s0);
            chS[2] = selm(mR, s0, s1);
            chW[0] = selm(mR, w1, w0);
            chW[2] = selm(mR, w0, w1);
        } else {
            chS[0] = at_pos(S, pr >> 1, pr & 1);
            chW[0] = at_pos(W, pr >> 1, pr & 1);
            chS[2] = at_pos(S, pb >> 1, pb & 1);
            chW[2] = at_pos(W, pb >> 1, pb & 1);
        }
        // weights are in [0,1] on this path (PSD kernel parameters), so the two green positions can be
        // taken as total - red - blue without cancellation trouble
        chS[1] = (totS - chS[0]) - chS[2];
        chW[1] = (totW - chW[0]) - chW[2];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        // (chS - black * chW) / white, added to the strip's sum: two fma
        accP[3 * K + c] = __builtin_fmaf(__builtin_fmaf(-lv.black[c], chW[c], chS[c]), lv.invWhite[c], accP[3 * K + c]);
        accW[3 * K + c] += chW[c];
    }
}

// the 13 unique tap weights of a pixel: n = jt*5+it, w[n] == w[24-n]; exponents pre-scaled by
// -0.5*log2(e) and built from sums (2 adds per weight).  (Building ten of the twelve from products of
// four exponentials -- six v_exp_f32 instead of twelve -- was measured: no gain, 0.642 vs 0.636 ms per
// pair, and it needs a bound on |kz|; the twelve exponentials stay.)
__device__ __forceinline__ void tap_weights13(float kx, float ky, float kz, float (&w)[13])
{
    const float a1 = kx * -0.72134752044448170368f, b1 = ky * -0.72134752044448170368f;
    const float c1 = kz * -0.72134752044448170368f;
    const float A[3] = {0.0f, a1, 4.0f * a1}, B[3] = {0.0f, b1, 4.0f * b1};
#pragma unroll
    for (int n = 0; n < 12; n++) {
        const int py = n / 5 - 2, px = n % 5 - 2;
        const int apx = px < 0 ? -px : px, apy = py < 0 ? -py : py;
        const float d = apx == 0 ? B[apy] : (apy == 0 ? A[apx] : A[apx] + B[apy]);
        // the caller admits only positive semi-definite kernel parameters, so every exponent is <= 0 and
        // every weight in [0, 1]: the non-finite rule of :429-430 cannot fire
        w[n] = __builtin_amdgcn_exp2f(px * py == 0 ? d : d + (float)(2 * px * py) * c1);
    }
    w[12] = 1.0f;
}

// tail of a strip pixel: C[jt][i] = sum over the taps of tap row jt on site column i of weight x certainty -> the nine
// site weights (tap rows 1 and 3 change site row with the y parity bit), class sums, channels
template <int K, int CFA>
__device__ __forceinline__ void strip_pixel_sites(const float (&C)[5][3], const float (&s)[3][3], uint32_t mby, uint32_t nby, uint32_t mP,
                                                   uint32_t mQ, const StripLevels& lv, float* accP, float* accW)
{
    auto andm = [](uint32_t m, float a) { return __uint_as_float(m & __float_as_uint(a)); };
    // site rows: tap row 0, row 1 if by == 0 | row 1 if by == 1, row 2, row 3 if by == 0 | row 3 if by == 1, row 4
    float Om[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        Om[0][i] = C[0][i] + andm(nby, C[1][i]);
        // (C1 & by) + C2 + (C3 & ~by) with one of the two masked terms zero: C2 + (by ? C1 : C3), the same sum (the terms
        // are non-negative, x + 0 is exact) in two instructions instead of four
        Om[1][i] = C[2][i] + selm(mby, C[1][i], C[3][i]);
        Om[2][i] = andm(mby, C[3][i]) + C[4][i];
    }
    // class (yc, xc) = (j & 1, i & 1), relative to (Q, P)
    float S[2][2], W[2][2];
    S[0][0] = __builtin_fmaf(s[2][2], Om[2][2], __builtin_fmaf(s[2][0], Om[2][0], __builtin_fmaf(s[0][2], Om[0][2], s[0][0] * Om[0][0])));
    W[0][0] = (Om[0][0] + Om[0][2]) + (Om[2][0] + Om[2][2]);
    S[0][1] = __builtin_fmaf(s[2][1], Om[2][1], s[0][1] * Om[0][1]);
    W[0][1] = Om[0][1] + Om[2][1];
    S[1][0] = __builtin_fmaf(s[1][2], Om[1][2], s[1][0] * Om[1][0]);
    W[1][0] = Om[1][0] + Om[1][2];
    S[1][1] = s[1][1] * Om[1][1];
    W[1][1] = Om[1][1];

    classes_to_channels<K, CFA>(S, W, mP, mQ, lv, accP, accW);
}

// Second formulation of the same pixel: the dynamic part (which raw site a tap lands on) is
// applied to the WEIGHTS, not to the values.
//  * site sums: out = sum_sites raw[j][i] * Om[j][i], Om[j][i] = sum of w*certainty over the taps on
//    site (j,i).  The CFA-position class of a site is static ((j&1, i&1) relative to (Q,P)), so the
//    value side is 9 fma + 5 add with no selects at all;
//  * tap columns 1 and 3 change site with the x parity bit: their weights are split once per
//    pixel into (w & ~mbx, w & mbx) (5 unique weights, plain v_and), tap rows 1 and 3 are split
//    the same way on the column sums;
//  * per tap row the certainty is resolved to (even site column, odd site column) x (cell) = at most
//    four values instead of one select per tap;
//  * exponents from pre-scaled sums: 2 adds per weight instead of mul+2 adds+mul.
// ~245 VALU instructions per pixel instead of ~330; sums re-associated again (fma), same tolerance.
// EP != 0 (the LDS tile kernel): the certainties are staged in LDS in CFA-position order, so "which channel does this site
// see" is an LDS ADDRESS (a few integer ops per pixel) instead of three v_bitop3 selects per tap row and cell.
//  One dword plane per CFA position, EP bytes apart; mval(jt, cell, ey, ex) with the byte offsets of the y parity
//  (0 or 2 * EP) and of the x parity (0 or EP) -- a value that is 0 or c flips with `^ c` whatever c is.
// strip_pixel_w: the pixel with its 13 tap weights given (they depend on the kernel parameters only, i.e. not on the
// frame: a kernel that takes several frames per launch computes them once per pixel).
// RawF: void rawf(int x0, int y0, float (&s)[3][3]) -> the 3x3 raw sites whose top left one is (x0, y0).
template <int K, int CFA, int EP = 0, typename RawF, typename MaskF>
__device__ __forceinline__ void strip_pixel_w(int X, int Y, int sx, int sy, const float (&w)[13], RawF rawf, MaskF mval,
                                               const StripLevels& lv, float* accP, float* accW)
{
    static_assert(EP == 0 || EP > 4, "EP: 0 (certainty by channel) or the plane stride in bytes");
    const int qx = X + sx - 2, qy = Y + sy - 2;
    const int x0 = qx >> 1, y0 = qy >> 1;
    uint32_t mbx = 0u - (uint32_t)(qx & 1), mby = 0u - (uint32_t)(qy & 1);
    uint32_t nbx = ~mbx, nby = ~mby;
    // opaque to the compiler: it would turn `weight & mask` into v_cndmask_b32 on the parity bit, which issues at 0.63x
    // the rate of v_and_b32 on gfx950 (profiles/r02_ubench_valu_ops.txt)
    asm volatile("" : "+v"(mbx), "+v"(nbx), "+v"(mby), "+v"(nby));
    const uint32_t mP = 0u - (uint32_t)(x0 & 1), mQ = 0u - (uint32_t)(y0 & 1);
    auto andm = [](uint32_t m, float a) { return __uint_as_float(m & __float_as_uint(a)); };

    float s[3][3];
    rawf(x0, y0, s);

    // tap columns 1 and 3: part that joins the lower / the upper site column
    float wl[13], wh[13];
#pragma unroll
    for (int n = 0; n < 13; n++) {
        const int it = n % 5;
        if (it == 1 || it == 3) {
            wl[n] = andm(nbx, w[n]);
            wh[n] = andm(mbx, w[n]);
        }
    }
    // n = 13 (row 2, column 3) mirrors n = 11
    auto W_ = [&](int jt, int it) { const int n = jt * 5 + it; return w[n <= 12 ? n : 24 - n]; };
    auto WL = [&](int jt, int it) { const int n = jt * 5 + it; return wl[n <= 12 ? n : 24 - n]; };
    auto WH = [&](int jt, int it) { const int n = jt * 5 + it; return wh[n <= 12 ? n : 24 - n]; };

    const uint32_t mY13 = mQ ^ mby;  // y parity of tap row 1's site row (complement for row 3)
    constexpr int cellLo = (K + 0 + 2) >> 2;
    auto cidx = [](int it) { return (((K + it + 2) >> 2) == ((K + 2) >> 2)) ? 0 : 1; };

    // EP != 0: plane offsets of the x parity P / ~P and of the y parities Q, ~Q, Q ^ by, ~(Q ^ by)
    uint32_t ex[2] = {0u, 0u}, ey[4] = {0u, 0u, 0u, 0u};
    if constexpr (EP != 0) {
        ex[0] = mP & (uint32_t)EP;
        ex[1] = ex[0] ^ (uint32_t)EP;
        ey[0] = mQ & (uint32_t)(2 * EP);
        ey[1] = ey[0] ^ (uint32_t)(2 * EP);
        ey[2] = mY13 & (uint32_t)(2 * EP);
        ey[3] = ey[2] ^ (uint32_t)(2 * EP);
    }
    float C[5][3];  // per tap row: w * certainty summed per site column
#pragma unroll
    for (int jt = 0; jt < 5; jt++) {
        uint32_t mya;
        if (jt == 0 || jt == 4) mya = mQ;
        if (jt == 2) mya = ~mQ;
        if (jt == 1) mya = mY13;
        if (jt == 3) mya = ~mY13;
        float Ee[2], Eo[2];  // certainty of the colour on even / odd site columns (relative to x0), per cell
        if constexpr (EP != 0) {
            // y parity Q (rows 0, 4), ~Q (row 2), Q ^ by (row 1), ~(Q ^ by) (row 3); even site columns x parity P, odd ~P
            const uint32_t eyj = ey[(jt == 0 || jt == 4) ? 0 : (jt == 2 ? 1 : (jt == 1 ? 2 : 3))];
#pragma unroll
            for (int c = 0; c < 2; c++) {
                Ee[c] = mval(jt, cellLo + c, eyj, ex[0]);
                Eo[c] = mval(jt, cellLo + c, eyj, ex[1]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 2; c++) {
                float m[3];
#pragma unroll
                for (int ch = 0; ch < 3; ch++) m[ch] = mval(jt, cellLo + c, ch);
                resolve_certainty<CFA>(mya, mP, m, Ee[c], Eo[c]);
            }
        }
        // site column 0: tap 0, tap 1 if bx == 0
        C[jt][0] = cidx(0) == cidx(1) ? (W_(jt, 0) + WL(jt, 1)) * Ee[cidx(0)]
                                      : __builtin_fmaf(WL(jt, 1), Ee[cidx(1)], W_(jt, 0) * Ee[cidx(0)]);
        // site column 1: tap 1 if bx == 1, tap 2, tap 3 if bx == 0
        {
            float acc;
            if (cidx(1) == cidx(2))
                acc = (WH(jt, 1) + W_(jt, 2)) * Eo[cidx(1)];
            else
                acc = __builtin_fmaf(W_(jt, 2), Eo[cidx(2)], WH(jt, 1) * Eo[cidx(1)]);
            if (cidx(3) == cidx(1) && cidx(1) == cidx(2))
                acc = ((WH(jt, 1) + W_(jt, 2)) + WL(jt, 3)) * Eo[cidx(1)];
            else
                acc = __builtin_fmaf(WL(jt, 3), Eo[cidx(3)], acc);
            C[jt][1] = acc;
        }
        // site column 2: tap 3 if bx == 1, tap 4
        C[jt][2] = cidx(3) == cidx(4) ? (WH(jt, 3) + W_(jt, 4)) * Ee[cidx(3)]
                                      : __builtin_fmaf(W_(jt, 4), Ee[cidx(4)], WH(jt, 3) * Ee[cidx(3)]);
    }
    strip_pixel_sites<K, CFA>(C, s, mby, nby, mP, mQ, lv, accP, accW);
}

// The same pixel where every certainty texel its wave touches is exactly 1 in every channel (the robustness mask
// saturates at 1 over well-aligned content: most of a typical frame).  strip_pixel_w with Ee = Eo = 1 folded: the
// products with the certainty are exact no-ops, so the column sums of a tap row are sums of WEIGHTS that depend on the
// frame through the x parity bit only -- one select per site column between two sums the caller makes once per pixel
// for all frames (P[r][0..3] = W0+W1, W1+W2, W2+W3, W3+W4 of tap row r = 0, 1, 2; rows 3 and 4 mirror rows 1 and 0).
// No certainty reads, no certainty addresses, 15 selects instead of 45 and/add/mul/fma: bit-identical to strip_pixel_w
// on such a pixel (same sums in the same association; x + 0 and x * 1 are exact).
template <int K, int CFA, typename RawF>
__device__ __forceinline__ void strip_pixel_sat(int X, int Y, int sx, int sy, const float (&w)[13], const float (&P)[3][4], RawF rawf,
                                                 const StripLevels& lv, float* accP, float* accW)
{
    const int qx = X + sx - 2, qy = Y + sy - 2;
    const int x0 = qx >> 1, y0 = qy >> 1;
    uint32_t mbx = 0u - (uint32_t)(qx & 1), mby = 0u - (uint32_t)(qy & 1);
    uint32_t nby = ~mby;
    asm volatile("" : "+v"(mbx), "+v"(mby), "+v"(nby));
    const uint32_t mP = 0u - (uint32_t)(x0 & 1), mQ = 0u - (uint32_t)(y0 & 1);
    float s[3][3];
    rawf(x0, y0, s);
    auto W_ = [&](int jt, int it) { const int n = jt * 5 + it; return w[n <= 12 ? n : 24 - n]; };
    // W(jt, i) + W(jt, i + 1): tap rows 3 and 4 are rows 1 and 0 read backwards (w[n] == w[24 - n])
    auto P_ = [&](int jt, int i) { return jt <= 2 ? P[jt][i] : P[4 - jt][3 - i]; };
    float C[5][3];
#pragma unroll
    for (int jt = 0; jt < 5; jt++) {
        C[jt][0] = selm(mbx, W_(jt, 0), P_(jt, 0));   // tap 0, tap 1 if bx == 0
        C[jt][1] = selm(mbx, P_(jt, 1), P_(jt, 2));   // tap 1 if bx == 1, tap 2, tap 3 if bx == 0
        C[jt][2] = selm(mbx, P_(jt, 3), W_(jt, 4));   // tap 3 if bx == 1, tap 4
    }
    strip_pixel_sites<K, CFA>(C, s, mby, nby, mP, mQ, lv, accP, accW);
}

// P[r][i] = W(r, i) + W(r, i + 1) of tap rows 0..2, in the association strip_pixel_w uses (see strip_pixel_sat)
__device__ __forceinline__ void tap_pair_sums(const float (&w)[13], float (&P)[3][4])
{
    auto W_ = [&](int jt, int it) { const int n = jt * 5 + it; return w[n <= 12 ? n : 24 - n]; };
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int i = 0; i < 4; i++) P[r][i] = W_(r, i) + W_(r, i + 1);
}

template <int K, int CFA, int EP = 0, typename MaskF>
__device__ __forceinline__ void strip_pixel(int X, int Y, int sx, int sy, float kx, float ky, float kz,
                                             const uint16_t* __restrict__ raw, int dimX, MaskF mval,
                                             const StripLevels& lv, float* accP, float* accW)
{
    float w[13];
    tap_weights13(kx, ky, kz, w);
    auto rawf = [&](int x0, int y0, float (&s)[3][3]) {
        const uint16_t* r = raw + (size_t)y0 * dimX + x0;
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) s[j][i] = (float)r[j * dimX + i];
    };
    strip_pixel_w<K, CFA, EP>(X, Y, sx, sy, w, rawf, mval, lv, accP, accW);
}

// Frame margin (HR pixels) that the strip/tile kernels leave to k_accumulateMargin: taps of
// pixels this close to the frame border can be clamped, which the fast path does not handle.
// Handling them in a separate small launch keeps the fast kernels free of divergent border
// waves (a wave with one border strip used to execute both paths: +12 % VALU instructions).
#define STRIP_MARGIN 16
// The margin kernels take branch-free taps with per-colour sums (accumulate_pixel_core<.., .., true>: tap_accumulate_sums,
// 81 -> 55 us per 4-frame margin launch at 4K).  The tile kernels' in-kernel straight path keeps the colour branches: the
// unrolled branch-free taps push those kernels over their register budget.

// SCALE is a template parameter: the straight arithmetic takes floor((x + px + sx) / scale) twenty times per pixel, and an
// integer division by a run-time value is ~40 instructions -- half of this kernel's work when the scale was a kernel argument
// WIN: the part of the ring inside a window (MarginRects), accumulators relative to the window's origin
// SITES: the site-wise body (accumulate_pixel_sites; mfsr_set_margin_sites), else accumulate_pixel_core's 25 taps
template <int SCALE, bool SITES>
__device__ __forceinline__ void margin_pixel_1(int x, int y, const uint16_t* __restrict__ raw, pix3* __restrict__ imgOut,
                                               pix3* __restrict__ totalWeights, const float4* __restrict__ certaintyMask,
                                               const mfsr_tex2d& kernelParam, const mfsr_tex2d& shifts, const Levels3& glv, int dimX,
                                               int dimY, int strideOut, int strideMask, int cfaPacked, int accX0 = 0, int accY0 = 0)
{
    if constexpr (SITES) {
        const float2 pos = margin_pixel_pos<SCALE>(x, y, dimX, dimY);
        const float4 kernel = tex4<ADDR_CLAMP>(kernelParam, pos.x, pos.y);
        float wSym[13];
#pragma unroll
        for (int n = 0; n < 13; n++) wSym[n] = tap_weight<true>(n % 5 - 2, n / 5 - 2, kernel.x, kernel.y, kernel.z);
        pix3 pixel = row_ptr(imgOut, strideOut, y - accY0)[x - accX0];
        pix3 totalWeight = row_ptr(totalWeights, strideOut, y - accY0)[x - accX0];
        accumulate_pixel_sites<SCALE>(x, y, raw, certaintyMask, shifts, glv, dimX, dimY, strideMask, cfaPacked, pos.x, pos.y,
                                      margin_pixel_sums(kernel), [&](int n) { return wSym[n]; }, pixel, totalWeight);
        row_ptr(imgOut, strideOut, y - accY0)[x - accX0] = pixel;
        row_ptr(totalWeights, strideOut, y - accY0)[x - accX0] = totalWeight;
    } else {
        accumulate_pixel_generic<GEOM_FULL, true, true>(x, y, raw, imgOut, totalWeights, certaintyMask, kernelParam, shifts, glv, dimX,
                                                        dimY, SCALE, strideOut, strideMask, cfaPacked, accX0, accY0);
    }
}

template <int SCALE, bool WIN = false, bool SITES = false>
__global__ void __launch_bounds__(256)
    k_accumulateMargin(const uint16_t* __restrict__ raw, pix3* __restrict__ imgOut, pix3* __restrict__ totalWeights,
                       const float4* __restrict__ certaintyMask, mfsr_tex2d kernelParam, mfsr_tex2d shifts, Levels3 glv,
                       int dimX, int dimY, int strideOut, int strideMask, int cfaPacked, int rowBegin, int rowEnd, MarginRects mr)
{
    constexpr int scale = SCALE;
    if constexpr (WIN) {
        int x, y;
        if (!margin_rect_pixel(mr, blockIdx.x * blockDim.x + threadIdx.x, x, y)) return;
        margin_pixel_1<SCALE, SITES>(x, y, raw, imgOut, totalWeights, certaintyMask, kernelParam, shifts, glv, dimX, dimY, strideOut,
                                     strideMask, cfaPacked, mr.accX0, mr.accY0);
        return;
    }
    const int hrW = scale * dimX, hrH = scale * dimY, M = STRIP_MARGIN;
    const int rowLen = hrW - 2;                    // x in [1, hrW-1)
    const int nTop = (M - 1) * rowLen;             // y in [1, M)
    const int nBot = (M - 1) * rowLen;             // y in [hrH-M, hrH-1)
    const int sideLen = 2 * (M - 1);               // x in [1, M) and [hrW-M, hrW-1)
    const int nSide = (hrH - 2 * M) * sideLen;     // y in [M, hrH-M)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    int x, y;
    if (idx < nTop) {
        y = 1 + idx / rowLen;
        x = 1 + idx % rowLen;
    } else if (idx < nTop + nBot) {
        const int r = idx - nTop;
        y = hrH - M + r / rowLen;
        x = 1 + r % rowLen;
    } else if (idx < nTop + nBot + nSide) {
        const int r = idx - nTop - nBot;
        y = M + r / sideLen;
        const int c = r % sideLen;
        x = c < M - 1 ? 1 + c : hrW - M + (c - (M - 1));
    } else {
        return;
    }
    if (y < rowBegin || y >= rowEnd) return;  // HR row window of this launch (stripe-sharded bursts)
    margin_pixel_1<SCALE, SITES>(x, y, raw, imgOut, totalWeights, certaintyMask, kernelParam, shifts, glv, dimX, dimY, strideOut,
                                 strideMask, cfaPacked);
}

// FR = HR pixels per field texel along each axis (4: fields at LR/2, the Bayer
// pipeline; 2: fields at LR, the monochrome pipeline; 0: any size, per-pixel fetch).
// per-frame arguments of the multi-frame kernels
struct TileFrame {
    const uint16_t* raw;
    const float4* mask;
    mfsr_tex2d shifts;
};
template <int NF>
struct TileFrames {
    TileFrame f[NF];
};

// the margin pixels of NF frames in one launch.  The straight arithmetic is a chain of dependent loads (flow, kernel
// parameters, then raw and certainty per tap) on 7.6 K wavefronts at 4K: one thread per (pixel, frame) -- 64 pixels x NF
// frames per workgroup -- keeps the chain one frame long; the frames' sums (each taken from zero) meet in LDS and are
// added to the accumulators in call order by the pixel's first thread, which reads and writes them once.
// The pixel's header once per workgroup (SITES): the tap weights and the `sums` predicate depend on the kernel parameters of
// the reference only -- the same for every frame of the pixel.  The pixel's frame-threads split the 13 weights between them
// (thread n takes weights n, n + NF, ...), put them into LDS and every thread reads them after one barrier: the same values
// as each thread's own, computed once.  Whole workgroups reach the barrier (threads of pixels past the end take part).
struct MarginHeader {
    float w[13][64];
    float pos[2][64];  // margin_pixel_pos: two IEEE divisions
    int sums[64];
};
template <int NF, int SCALE>
__device__ __forceinline__ void margin_header(MarginHeader& h, bool live, int x, int y, int lane, int n, const mfsr_tex2d& kernelParam,
                                              int dimX, int dimY)
{
    if (live) {
        const float2 pos = margin_pixel_pos<SCALE>(x, y, dimX, dimY);
        const float4 kernel = tex4<ADDR_CLAMP>(kernelParam, pos.x, pos.y);
        if (n == 0) {
            h.pos[0][lane] = pos.x;
            h.pos[1][lane] = pos.y;
        }
        for (int k = n; k < 13; k += NF) h.w[k][lane] = tap_weight<true>(k % 5 - 2, k / 5 - 2, kernel.x, kernel.y, kernel.z);
        if (n == 0) h.sums[lane] = margin_pixel_sums(kernel) ? 1 : 0;
    }
    __syncthreads();
}

template <int NF, int SCALE, bool WIN = false, bool SITES = false>
__global__ void __launch_bounds__(64 * NF)
    k_accumulateMarginN(TileFrames<NF> fr, pix3* __restrict__ imgOut, pix3* __restrict__ totalWeights, mfsr_tex2d kernelParam,
                        Levels3 glv, int dimX, int dimY, int strideOut, int strideMask, int cfaPacked, int rowBegin, int rowEnd,
                        MarginRects mr)
{
    constexpr int scale = SCALE;
    __shared__ float sSum[NF][6][64];
    const int hrW = scale * dimX, hrH = scale * dimY, M = STRIP_MARGIN;
    const int rowLen = hrW - 2;
    const int nTop = (M - 1) * rowLen, nBot = (M - 1) * rowLen;
    const int sideLen = 2 * (M - 1);
    const int nSide = (hrH - 2 * M) * sideLen;
    // (SITES: the frame index as the wave-uniform value it is -- the frame's pointers then sit in scalar registers)
    const int lane = threadIdx.x, n = SITES ? __builtin_amdgcn_readfirstlane(threadIdx.y) : threadIdx.y;
    const int idx = blockIdx.x * 64 + lane;
    int x = 0, y = -1;
    if constexpr (WIN) {
        if (!margin_rect_pixel(mr, idx, x, y)) y = -1;
    } else if (idx < nTop) {
        y = 1 + idx / rowLen;
        x = 1 + idx % rowLen;
    } else if (idx < nTop + nBot) {
        const int r = idx - nTop;
        y = hrH - M + r / rowLen;
        x = 1 + r % rowLen;
    } else if (idx < nTop + nBot + nSide) {
        const int r = idx - nTop - nBot;
        y = M + r / sideLen;
        const int c = r % sideLen;
        x = c < M - 1 ? 1 + c : hrW - M + (c - (M - 1));
    }
    const bool live = y >= rowBegin && y < rowEnd && y >= 0;
    const int ax = WIN ? mr.accX0 : 0, ay = WIN ? mr.accY0 : 0;  // accumulator origin
    pix3 pixel = {0.0f, 0.0f, 0.0f}, totalWeight = {0.0f, 0.0f, 0.0f};
    if constexpr (SITES) {
        __shared__ MarginHeader sHdr;
        margin_header<NF, SCALE>(sHdr, live, x, y, lane, n, kernelParam, dimX, dimY);
        if (live) {
            const TileFrame F = fr.f[n];
            accumulate_pixel_sites<SCALE>(x, y, F.raw, F.mask, F.shifts, glv, dimX, dimY, strideMask, cfaPacked, sHdr.pos[0][lane], sHdr.pos[1][lane],
                                          sHdr.sums[lane] != 0, [&](int k) { return sHdr.w[k][lane]; }, pixel, totalWeight);
        }
    } else if (live) {
        TileFrame F = fr.f[0];
#pragma unroll
        for (int m = 1; m < NF; m++)
            if (n == m) F = fr.f[m];
        accumulate_pixel_core<GEOM_FULL, true, true>(x, y, F.raw, F.mask, kernelParam, F.shifts, glv, dimX, dimY, scale,
                                                                strideMask, cfaPacked, pixel, totalWeight);
    }
    sSum[n][0][lane] = pixel.x;
    sSum[n][1][lane] = pixel.y;
    sSum[n][2][lane] = pixel.z;
    sSum[n][3][lane] = totalWeight.x;
    sSum[n][4][lane] = totalWeight.y;
    sSum[n][5][lane] = totalWeight.z;
    __syncthreads();
    if (n == 0 && live) {
        pix3 a = row_ptr(imgOut, strideOut, y - ay)[x - ax];
        pix3 w = row_ptr(totalWeights, strideOut, y - ay)[x - ax];
#pragma unroll
        for (int m = 0; m < NF; m++) {
            a.x += sSum[m][0][lane];
            a.y += sSum[m][1][lane];
            a.z += sSum[m][2][lane];
            w.x += sSum[m][3][lane];
            w.y += sSum[m][4][lane];
            w.z += sSum[m][5][lane];
        }
        row_ptr(imgOut, strideOut, y - ay)[x - ax] = a;
        row_ptr(totalWeights, strideOut, y - ay)[x - ax] = w;
    }
}

// one frame of one strip on the register-resident accumulators (k_accumulate2xStrip)
template <int CFA, int FR>
__device__ __forceinline__ void strip_frame(int tx, int Y, int X0, const uint16_t* __restrict__ raw,
                                            const float4* __restrict__ certaintyMask, const mfsr_tex2d& kernelParam,
                                            const mfsr_tex2d& shifts, const Levels3& glv, const StripLevels& lv, int dimX,
                                            int dimY, int strideMask, int cfaPacked, float* accP, float* accW)
{
    const int hrW = 2 * dimX, hrH = 2 * dimY;
    const float posY = ((float)Y + 0.5f) / (float)hrH;
    int sx[4], sy[4];
    float kx[4], ky[4], kz[4];
    // a strip is "safe" when no tap of its four pixels is clamped at the frame border
    bool safe = true;  // (the frame margin is handled by k_accumulateMargin)
    if (FR == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float posX = ((float)(X0 + k) + 0.5f) / (float)hrW;
            const float4 kp = tex4<ADDR_CLAMP>(kernelParam, posX, posY);
            const float2 sh = tex2<ADDR_CLAMP>(shifts, posX, posY);
            kx[k] = kp.x;
            ky[k] = kp.y;
            kz[k] = kp.z;
            sx[k] = round2i(sh.x * 2.0f);
            sy[k] = round2i(sh.y * 2.0f);
        }
    } else {
        // The four pixels of a strip read the same few field texels: fetch them once
        // (FR=4: 3 columns x 2 rows, FR=2: 4 x 2) and interpolate with exactly the
        // arithmetic of tex_coord/lerp4, so roundf(2*flow) stays bit-identical.
        constexpr int NC = FR == 4 ? 3 : 4;
        const int fw = kernelParam.width, fh = kernelParam.height;  // == shifts' size (checked on the host)
        float yB = posY * (float)fh - 0.5f;
        if (!finitef(yB)) yB = 0.0f;
        const float fy = floorf(yB);
        const float b = yB - fy;
        const int j0 = clampi(f2i(fy), 0, fh - 1), j1 = clampi(f2i(fy) + 1, 0, fh - 1);
        const int cbase = clampi(FR == 4 ? tx - 1 : 2 * tx - 1, 0, fw - NC);
        float K0[NC][3], K1[NC][3], F0[NC][2], F1[NC][2];
        {
            const float4* k0 = row_ptr((const float4*)kernelParam.ptr, kernelParam.pitch, j0) + cbase;
            const float4* k1 = row_ptr((const float4*)kernelParam.ptr, kernelParam.pitch, j1) + cbase;
            const float2* f0 = row_ptr((const float2*)shifts.ptr, shifts.pitch, j0) + cbase;
            const float2* f1 = row_ptr((const float2*)shifts.ptr, shifts.pitch, j1) + cbase;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const float4 u = k0[c], v = k1[c];
                const float2 p = f0[c], q = f1[c];
                K0[c][0] = u.x; K0[c][1] = u.y; K0[c][2] = u.z;
                K1[c][0] = v.x; K1[c][1] = v.y; K1[c][2] = v.z;
                F0[c][0] = p.x; F0[c][1] = p.y;
                F1[c][0] = q.x; F1[c][1] = q.y;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float posX = ((float)(X0 + k) + 0.5f) / (float)hrW;
            float xB = posX * (float)fw - 0.5f;
            if (!finitef(xB)) xB = 0.0f;
            const float fx = floorf(xB);
            const float a = xB - fx;
            // texel column predicted from the strip geometry; verified against the float path
            const int ci = FR == 4 ? (k < 2 ? 0 : 1) : (k == 0 ? 0 : (k == 3 ? 2 : 1));
            safe = safe && (f2i(fx) == cbase + ci) && (cbase + ci + 1 <= fw - 1);
            kx[k] = lerp4(K0[ci][0], K0[ci + 1][0], K1[ci][0], K1[ci + 1][0], a, b);
            ky[k] = lerp4(K0[ci][1], K0[ci + 1][1], K1[ci][1], K1[ci + 1][1], a, b);
            kz[k] = lerp4(K0[ci][2], K0[ci + 1][2], K1[ci][2], K1[ci + 1][2], a, b);
            const float ux = lerp4(F0[ci][0], F0[ci + 1][0], F1[ci][0], F1[ci + 1][0], a, b);
            const float uy = lerp4(F0[ci][1], F0[ci + 1][1], F1[ci][1], F1[ci + 1][1], a, b);
            sx[k] = round2i(ux * 2.0f);
            sy[k] = round2i(uy * 2.0f);
        }
        safe = safe && (f2i(fy) >= 0) && (f2i(fy) + 1 <= fh - 1);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) safe = safe && psd_ok(kx[k], ky[k], kz[k]);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int qx = X0 + k + sx[k] - 2, qy = Y + sy[k] - 2;
        safe = safe && qx >= 0 && ((qx + 4) >> 1) <= dimX - 1 && qy >= 0 && ((qy + 4) >> 1) <= dimY - 1;
        // guard against saturated conversions of wild flow values
        safe = safe && sx[k] > -(1 << 20) && sx[k] < (1 << 20) && sy[k] > -(1 << 20) && sy[k] < (1 << 20);
    }
    if (!safe) {
        // border-free but wild-flow / non-PSD strips: the straight per-pixel arithmetic on the register values
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            const int X = X0 + k;
            if (X >= 1 && X < hrW - 1) {
                pix3 px = {accP[3 * k], accP[3 * k + 1], accP[3 * k + 2]};
                pix3 tw = {accW[3 * k], accW[3 * k + 1], accW[3 * k + 2]};
                accumulate_pixel_core<GEOM_FULL, true>(X, Y, raw, certaintyMask, kernelParam, shifts, glv, dimX, dimY, 2,
                                                       strideMask, cfaPacked, px, tw);
                accP[3 * k] = px.x; accP[3 * k + 1] = px.y; accP[3 * k + 2] = px.z;
                accW[3 * k] = tw.x; accW[3 * k + 1] = tw.y; accW[3 * k + 2] = tw.z;
            }
        }
        return;
    }

    // certainty texels: rows (Y-2)>>2 and (Y+2)>>2, cells tx-1, tx, tx+1; non-finite -> 0 (:438-439)
    const int r0 = (Y - 2) >> 2;
    const int sw = 4 * (r0 + 1) - (Y - 2);  // first tap row that reads mask row r0+1 (1..4), wave-uniform
    float M0[3][3], M1[3][3];
    {
        const float4* m0 = row_ptr(certaintyMask, strideMask, r0) + (tx - 1);
        const float4* m1 = row_ptr(certaintyMask, strideMask, r0 + 1) + (tx - 1);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float4 u = m0[c], v = m1[c];
            M0[c][0] = sane(u.x); M0[c][1] = sane(u.y); M0[c][2] = sane(u.z);
            M1[c][0] = sane(v.x); M1[c][1] = sane(v.y); M1[c][2] = sane(v.z);
        }
    }

    auto mval = [&](int jt, int cell, int ch) {
        // mask row (Y-2+jt)>>2 is r0 for jt < sw and r0+1 otherwise (wave-uniform)
        return jt == 0 ? M0[cell][ch] : (jt == 4 ? M1[cell][ch] : ((jt >= sw) ? M1[cell][ch] : M0[cell][ch]));
    };
    strip_pixel<0, CFA>(X0 + 0, Y, sx[0], sy[0], kx[0], ky[0], kz[0], raw, dimX, mval, lv, accP, accW);
    strip_pixel<1, CFA>(X0 + 1, Y, sx[1], sy[1], kx[1], ky[1], kz[1], raw, dimX, mval, lv, accP, accW);
    strip_pixel<2, CFA>(X0 + 2, Y, sx[2], sy[2], kx[2], ky[2], kz[2], raw, dimX, mval, lv, accP, accW);
    strip_pixel<3, CFA>(X0 + 3, Y, sx[3], sy[3], kx[3], ky[3], kz[3], raw, dimX, mval, lv, accP, accW);

}

// Register-only strip kernel: serves every field resolution (FR) without LDS; NF frames add into the
// accumulators while they sit in registers (one read-modify-write of HBM for both).
// WIN: the columns [wx0, wx1) of a window (colBlock0 = its first 256-pixel column block), accumulators relative to (wx0, wy0)
template <int CFA, int FR, int NF, bool WIN = false>
__global__ void __launch_bounds__(256)
    k_accumulate2xStrip(TileFrames<NF> fr, pix3* __restrict__ imgOut, pix3* __restrict__ totalWeights, mfsr_tex2d kernelParam,
                        Levels3 glv, StripLevels lv, int dimX, int dimY, int strideOut, int strideMask, int cfaPacked, int rowBlock0,
                        int colBlock0, int wx0, int wx1, int wy0)
{
    const int tx = (blockIdx.x + (WIN ? colBlock0 : 0)) * 64 + threadIdx.x;
    const int Y = (blockIdx.y + rowBlock0) * 4 + threadIdx.y;
    const int hrW = 2 * dimX, hrH = 2 * dimY;
    const int X0 = 4 * tx;
    if (X0 < STRIP_MARGIN || X0 >= hrW - STRIP_MARGIN || Y < STRIP_MARGIN || Y >= hrH - STRIP_MARGIN) return;
    if (WIN && (X0 < wx0 || X0 >= wx1)) return;  // (window edges are multiples of 4 pixels: a strip is in or out)

    // accumulators: 4 pixels x 3 channels = 48 contiguous bytes per plane-set
    const size_t accOff = WIN ? (size_t)(Y - wy0) * strideOut + (size_t)(X0 - wx0) * 12 : (size_t)Y * strideOut + (size_t)X0 * 12;
    float4* pP = (float4*)((char*)imgOut + accOff);
    float4* pW = (float4*)((char*)totalWeights + accOff);
    float accP[12], accW[12];
    {
        const float4 a0 = pP[0], a1 = pP[1], a2 = pP[2];
        const float4 b0 = pW[0], b1 = pW[1], b2 = pW[2];
        accP[0] = a0.x; accP[1] = a0.y; accP[2] = a0.z; accP[3] = a0.w;
        accP[4] = a1.x; accP[5] = a1.y; accP[6] = a1.z; accP[7] = a1.w;
        accP[8] = a2.x; accP[9] = a2.y; accP[10] = a2.z; accP[11] = a2.w;
        accW[0] = b0.x; accW[1] = b0.y; accW[2] = b0.z; accW[3] = b0.w;
        accW[4] = b1.x; accW[5] = b1.y; accW[6] = b1.z; accW[7] = b1.w;
        accW[8] = b2.x; accW[9] = b2.y; accW[10] = b2.z; accW[11] = b2.w;
    }
#pragma unroll
    for (int n = 0; n < NF; n++)
        strip_frame<CFA, FR>(tx, Y, X0, fr.f[n].raw, fr.f[n].mask, kernelParam, fr.f[n].shifts, glv, lv, dimX, dimY, strideMask,
                             cfaPacked, accP, accW);
    pP[0] = make_float4(accP[0], accP[1], accP[2], accP[3]);
    pP[1] = make_float4(accP[4], accP[5], accP[6], accP[7]);
    pP[2] = make_float4(accP[8], accP[9], accP[10], accP[11]);
    pW[0] = make_float4(accW[0], accW[1], accW[2], accW[3]);
    pW[1] = make_float4(accW[4], accW[5], accW[6], accW[7]);
    pW[2] = make_float4(accW[8], accW[9], accW[10], accW[11]);
}

// ---- LDS tile kernel (fields at HR/4: the Bayer pipeline) --------------------------------------
// One 64x4 workgroup covers a 256 x 4 HR tile.
//  * The kernel-parameter / flow / certainty texels the tile touches (3 rows x 66 columns each) are
//    staged once in LDS (certainties sanitised, kernel parameters tagged "positive semi-definite"
//    while staging), and so are the per-column and per-row interpolation fractions (one IEEE
//    division per column of the tile instead of one per pixel).
//  * The two accumulator row segments of a wave (3 KiB each) go global -> LDS with
//    global_load_lds (no VGPRs, 1 KiB contiguous per instruction, in flight during the whole tap
//    arithmetic), are updated in LDS and written back in memory order: every accumulator access
//    on the HBM side is a fully used 128-byte line.
#define TILE_COLS 66
// How the tile kernels are laid out; each choice below won its measurement (DESIGN.md section 5 has the tables).
//  * Several frames per launch run in pixel-major order with the tap weights shared by the frames; one frame at HR/4 keeps
//    the frame-major form.
//  * Both accumulator plane-sets are staged at once.  Measured at 4K x 16, four frames per launch: 1.004 ms with both (no
//    spills) against 1.044 - 1.068 ms with one at a time (10 spilled registers and the second plane-set's load exposed).
//  * ALIAS (three and four frames per launch, fields at HR/4): four workgroups per CU.  The weight-sum plane-set is staged
//    over the kernel-parameter and flow texels once every wave is past its last read of them (39 KiB of LDS instead of 48),
//    and the rounded flow of a strip is kept in 8:8 bits per pixel relative to the tile's own rounded flow (8 registers
//    instead of 16; strips more than 127 HR pixels away from it take the straight arithmetic), which fits the 128-register
//    budget of four waves per SIMD.  Its pass 1 has no 16-bit range test on the rounded flow: the 8-bit window implies it
//    (see there; with the test the burst took 6.00 ms).
//  * Frames whose certainty is saturated over the wave's footprint take strip_pixel_sat.
//  * Certainty is staged as four dword planes, one per CFA position ([e][mask row][frame][column]), not as one float4 texel
//    per cell: a tap row's read is then at a 4-byte lane stride (every bank once per 32 lanes for a wave-uniform parity,
//    two-way at worst) where a texel layout's 16-byte stride put the lanes on 8 of the 32 banks (four-way by construction),
//    and the frame's offset (66 dwords per frame) fits the DS offset field.  Same LDS bytes.  Texels: 6.05 against 5.75 ms
//    per burst at 4K x 16 (profiles/r05_tile_layout_ab.txt).
//  * The raw sites are one uniform frame pointer plus one 32-bit lane offset per site row (the loads take the scalar-base
//    form, no 64-bit VALU adds).
//  * The black / white levels stay in kernel-argument SGPRs although an fp32 op with an SGPR operand issues at 0.63x the
//    rate (profiles/r02_ubench_valu_ops.txt): held in VGPRs, at the 128-register cap of the four-frame kernel the six
//    registers come back as spills (32 bytes of scratch against 8, 6 720 static VALU against 6 633) and the burst takes
//    6.13 instead of 5.75 ms.
// Workgroups per CU (= waves per SIMD) the register budget is sized for.  x2: four with fields at HR/4 (one frame: 125
// VGPRs; three and four: the ALIAS layout), three with fields at HR/2 (41 / 49 KB of LDS).  x4: four (one frame: 113 VGPRs;
// three and four: the ALIAS layout), but three with two frames per launch.
constexpr int tile_waves_x2(int /*NF*/, int FR) { return FR == 4 ? 4 : 3; }
constexpr int tile_waves_x4(int NF) { return NF == 2 ? 3 : 4; }
// ---- pieces the tile kernels share (k_accumulate2xTile, k_accumulate2xTileBurst, k_accumulate4xTile) ----
// HPT = HR pixels per kernel-parameter / flow texel: 2 or 4 at x2 (FR), 8 at x4.
// Not every kernel uses every piece: the four-frame instances of k_accumulate2xTile sit at the 128-VGPR cap with one spilled
// register, and moving its fractions, parameter mix, passes 1 and 2, plane staging, plane add or straight loop into a function
// costs them 4 to 76 more bytes of scratch (the burst kernel: parameter mix and passes 1 and 2, 4 to 20 bytes).  Those stay
// inline there; a piece is shared where every instance keeps its registers, scratch and LDS.
typedef const __attribute__((address_space(3))) char* lds_cptr;
typedef const __attribute__((address_space(1))) char* glb_cptr;

// XCD-aware tile order (tilesPerXcd > 0, the default since round 4).  Workgroups are dealt round-robin to the 8 XCDs
// (workgroup i -> XCD i & 7), each with its own L2.  A 256 x 4 tile stages 66 x 3 field texels (kernel parameters, the
// flows and certainties of its frames: 112 B per texel with four frames) of which it owns 64 x 1, and its raw rows
// overlap those of the tiles above and below: in launch order vertically adjacent tiles sit on DIFFERENT XCDs, so every
// one of those re-reads misses its L2 and goes to the fabric (served by the Infinity Cache, counted by the L2's
// memory-side counters): 1.16 GB read per launch beyond the accumulators against 0.30 GB of inputs (PMC, request-size
// counters, profiles/r04_pmc_fuse_xcd.txt).  With the remap XCD k walks its own contiguous band of tiles in row-major
// order, the neighbours are L2 hits, and the launch reads 0.305 GB + the accumulators: exactly its inputs.  The launch
// time does not move (0.86 ms either way: the kernel is not bound by bytes) -- what it buys is 0.87 GB less fabric
// traffic per launch for the kernels running beside it, and a traffic figure that is the algorithmic one.
__device__ __forceinline__ int xcd_tile_index(int pid, int tilesPerXcd)
{
    return tilesPerXcd > 0 ? (pid & 7) * tilesPerXcd + (pid >> 3) : pid;  // tilesPerXcd == 0: launch order (A/B)
}

// Interpolation fraction of HR column (or row) p on an axis of hrN HR pixels and fN field texels: the float path of
// tex_coord, with the texel floor(xB) predicted -- p / HPT - 1 for the first half of a texel's pixels, p / HPT for the
// second -- and verified.  -1: not on the predicted texel, or that texel's right / lower neighbour is outside the field
// (ROW: or the texel itself is above it).
template <int HPT, bool ROW>
__device__ __forceinline__ float texel_fraction(int p, int hrN, int fN)
{
    constexpr int SH = HPT == 8 ? 3 : (HPT == 4 ? 2 : 1);
    const float pos = ((float)p + 0.5f) / (float)hrN;
    float xB = pos * (float)fN - 0.5f;
    if (!finitef(xB)) xB = 0.0f;
    const float fxf = floorf(xB);
    const int pred = (p >> SH) - 1 + ((p & (HPT - 1)) < HPT / 2 ? 0 : 1);
    const bool ok = (f2i(fxf) == pred) && (pred + 1 <= fN - 1) && (!ROW || f2i(fxf) >= 0);
    return ok ? xB - fxf : -1.0f;
}

// texel columns a strip touches, and the left texel of pixel k's pair among them
template <int HPT>
struct StripTexels {
    static constexpr int SC = HPT == 8 ? 2 : (HPT == 4 ? 3 : 4);
    static constexpr int ci(int k) { return HPT == 8 ? 0 : (HPT == 4 ? (k < 2 ? 0 : 1) : (k + 1) >> 1); }
};

// Pass 1, one frame: the whole-pixel flow of the strip's four pixels (SCALE x the flow at f0 / f1, two LDS rows of 2 x SC
// texels, rounded) and the fast-path admission -- every tap inside the frame: 0 <= q and ((q + 4) / SCALE) <= dim - 1  <=>
// (unsigned)q <= SCALE * dim - 5.  `safe` comes in as what the strip's geometry and kernel parameters allow and is returned
// with this frame's tests added.
// RANGE_BITS: the rounded flow must also lie inside that many signed bits (wilder strips take the straight arithmetic): it
// keeps saturated conversions from wrapping back into range.
template <int SCALE, int HPT, int RANGE_BITS>
__device__ __forceinline__ bool strip_flow(bool safe, const float2* f0, const float2* f1, const float (&av)[4], float b, int X0, int Y,
                                           uint32_t xmax, uint32_t ymax, int (&sx)[4], int (&sy)[4])
{
    constexpr int SC = StripTexels<HPT>::SC;
    float2 Ft[2][SC];
#pragma unroll
    for (int c = 0; c < SC; c++) {
        Ft[0][c] = f0[c];
        Ft[1][c] = f1[c];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ci = StripTexels<HPT>::ci(k);
        const float ux = lerp4(Ft[0][ci].x, Ft[0][ci + 1].x, Ft[1][ci].x, Ft[1][ci + 1].x, av[k], b);
        const float uy = lerp4(Ft[0][ci].y, Ft[0][ci + 1].y, Ft[1][ci].y, Ft[1][ci + 1].y, av[k], b);
        sx[k] = round2i(ux * (float)SCALE);
        sy[k] = round2i(uy * (float)SCALE);
        const int qx = X0 + k + sx[k] - 2, qy = Y + sy[k] - 2;
        safe = safe && (uint32_t)(sx[k] + (1 << RANGE_BITS)) < (2u << RANGE_BITS) && (uint32_t)(sy[k] + (1 << RANGE_BITS)) < (2u << RANGE_BITS);
        safe = safe && (uint32_t)qx <= xmax && (uint32_t)qy <= ymax;
    }
    return safe;
}

// A wave's accumulator row segment (3 KiB = 192 chunks of 16 bytes per plane-set) between global memory and its LDS row, in
// memory order: contiguous 1 KiB per instruction.  g is the segment's address in the frame -- or, WIN, the WINDOW's row: the
// chunk at frame-row byte gb then lives at g + gb - winB0 if winB0 <= gb < winB1, and chunks outside the window are neither
// staged nor written back.
template <bool WIN>
struct AccSegment {
    size_t rowBytes;      // bytes of the frame's accumulator row
    size_t segByte;       // first byte of the segment in it
    size_t winB0, winB1;  // WIN: the window's bytes of the row
    int fresh;            // first launch of a burst: the accumulators are defined to be zero and are not read at all
    __device__ __forceinline__ bool inWin(size_t gb) const { return !WIN || (gb >= winB0 && gb + 16 <= winB1); }
    __device__ __forceinline__ char* chunk(char* g, size_t off) const { return WIN ? g + (segByte + off - winB0) : g + off; }
    // global -> LDS: zeroes if fresh, else the asynchronous copy (no VGPRs; the caller waits with vmcnt(0))
    __device__ __forceinline__ void stage(char* g, float4* lds, int lx) const
    {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            if (fresh) {
                lds[j * 64 + lx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            } else {
                const size_t off = (size_t)(j * 64 + lx) * 16;
                if (segByte + off + 16 <= rowBytes && inWin(segByte + off))
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)chunk(g, off),
                                                     (__attribute__((address_space(3))) void*)&lds[j * 64], 16, 0, 0);
            }
        }
    }
    // LDS -> global.  The 16-pixel side margins of the row belong to the margin kernel: their (unchanged) chunks are not
    // written back.  A fresh launch defines them (zero) instead.
    __device__ __forceinline__ void store(const float4* lds, char* g, int lx) const
    {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const size_t off = (size_t)(j * 64 + lx) * 16;
            const size_t gb = segByte + off;
            const bool sideMargin = gb < (size_t)STRIP_MARGIN * 12 || gb + 16 > rowBytes - (size_t)STRIP_MARGIN * 12;
            if (gb + 16 <= rowBytes && (fresh || !sideMargin) && inWin(gb)) *(float4*)chunk(g, off) = lds[j * 64 + lx];
        }
    }
};

// my[0..11] (a lane's 4 pixels x 3 channels of a staged plane) += acc[0..11]
__device__ __forceinline__ void lane_add12(float* my, const float* acc)
{
    float4* my4 = (float4*)my;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        float4 a = my4[j];
        a.x += acc[4 * j + 0]; a.y += acc[4 * j + 1]; a.z += acc[4 * j + 2]; a.w += acc[4 * j + 3];
        my4[j] = a;
    }
}

// A border / wild-flow / non-PSD strip of frame F: the straight per-pixel arithmetic on the lane's staged values (after the
// sums have left the registers: it needs most of them).  These strips are a few per frame.
template <int SCALE>
__device__ __forceinline__ void strip_straight(const TileFrame& F, float* myP, float* myW, int X0, int Y, int hrW, const mfsr_tex2d& kernelParam,
                                               const Levels3& glv, int dimX, int dimY, int strideMask, int cfaPacked)
{
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const int X = X0 + k;
        if (X >= 1 && X < hrW - 1) {
            pix3 px = {myP[3 * k], myP[3 * k + 1], myP[3 * k + 2]};
            pix3 tw = {myW[3 * k], myW[3 * k + 1], myW[3 * k + 2]};
            accumulate_pixel_core<GEOM_FULL, true>(X, Y, F.raw, F.mask, kernelParam, F.shifts, glv, dimX, dimY, SCALE, strideMask,
                                                   cfaPacked, px, tw);
            myP[3 * k] = px.x; myP[3 * k + 1] = px.y; myP[3 * k + 2] = px.z;
            myW[3 * k] = tw.x; myW[3 * k + 1] = tw.y; myW[3 * k + 2] = tw.z;
        }
    }
}

// What the pixel-frame bodies of the x2 pass 2 share, taken once per strip (each body is its own divergent region, the
// compiler does not hoist across them).
// Certainty rows: the LDS address of the row each tap row reads, as opaque 32-bit addresses -- the compiler would otherwise
// split the planes' own address off them and add it back per read as a constant too large for the DS offset field, where
// frame and cell now fit.
template <int NF>
__device__ __forceinline__ void certainty_row_addrs(float (*planes)[3][NF][TILE_COLS], int lx, int ly, uint32_t (&mrowA)[5])
{
#pragma unroll
    for (int jt = 0; jt < 5; jt++) {
        mrowA[jt] = (uint32_t)(uintptr_t)(lds_cptr)&planes[0][((ly + jt - 2) >> 2) + 1][0][lx];
        asm volatile("" : "+v"(mrowA[jt]));
    }
}
// Raw sites: the frames' own pointers (opaque: kept in SGPR pairs, not fetched again by every body).
template <int NF>
__device__ __forceinline__ void raw_bases(const TileFrame* f, glb_cptr (&rawBase)[NF])
{
#pragma unroll
    for (int n = 0; n < NF; n++) {
        rawBase[n] = (glb_cptr)f[n].raw;
        asm volatile("" : "+s"(rawBase[n]));
    }
}
// Bit n: frame n's certainty is exactly 1 on every texel this WAVE reads (its 66 texel columns on the two mask rows its tap
// rows touch); such a frame takes strip_pixel_sat: a wave-uniform (scalar) branch per frame, bit-identical results.
template <int NF>
__device__ __forceinline__ uint32_t saturated_frames(const uint32_t (*unsat)[TILE_COLS], int lx, int ly)
{
    const int r0 = ((ly - 2) >> 2) + 1;  // mask rows ((ly + jt - 2) >> 2) + 1, jt = 0..4: r0 and r0 + 1
    uint32_t u = unsat[r0][lx] | unsat[r0 + 1][lx];
    if (lx < 2) u |= unsat[r0][64 + lx] | unsat[r0 + 1][64 + lx];
    uint32_t satW = 0;
#pragma unroll
    for (int n = 0; n < NF; n++)
        if (__builtin_amdgcn_ballot_w64((u >> n) & 1u) == 0) satW |= 1u << n;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)satW);
}

// (Measured and not kept: the nine raw sites of a body loaded one body ahead -- 161 VGPRs, the address arithmetic twice:
// 0.96 against 0.876 ms per isolated launch.  The round trip of the raw loads is already hidden.)
// NF frames per launch (1 to 4).  Everything that does not depend on the frame is done once for
// both: the accumulator staging and write-back (the 48 B/px/frame of HBM traffic become 24), the
// kernel-parameter mix, the column/row fractions.  The two frames add into the same registers.

// FR = HR pixels per kernel-parameter / flow texel: 4 (the Bayer pipeline: fields at LR/2) or 2 (the monochrome pipeline:
// fields at LR; 130 x 4 texels per tile, four texel columns per strip); the certainty mask is at LR/2 either way.
// WIN (a separate instantiation: the whole-frame kernels keep their code): only the tile columns from tileX0 on are launched,
// the accumulators hold the window [wx0, wx1) x [wy0, ..) only, and the 16-byte accumulator chunks outside it are neither
// staged nor written back (window edges are multiples of 16 pixels = 12 chunks: no chunk straddles one).
template <int CFA, int NF, int FR = 4, bool WIN = false>
__global__ void __launch_bounds__(256, tile_waves_x2(NF, FR))
    k_accumulate2xTile(TileFrames<NF> fr, pix3* __restrict__ imgOut, pix3* __restrict__ totalWeights, mfsr_tex2d kernelParam,
                       Levels3 glv, StripLevels lv, int dimX, int dimY, int strideOut, int strideMask, int cfaPacked,
                       int tilesX, int tilesY, int tilesPerXcd, int fresh, int tileY0, int tileX0, int wx0, int wx1, int wy0)
{
    const int tile = xcd_tile_index((int)blockIdx.x, tilesPerXcd);
    if (tile >= tilesX * tilesY) return;  // whole workgroup (uniform), before any barrier
    const int bIdYrel = tile / tilesX, bIdX = tile - bIdYrel * tilesX + (WIN ? tileX0 : 0);
    const int bIdY = bIdYrel + tileY0;  // tileY0: first tile row of this launch's HR row window
    static_assert(FR == 4 || FR == 2, "field resolution");
    constexpr int FC = 256 / FR + 2, FROWS = 4 / FR + 2;  // field texels a tile touches: 66 x 3 (FR = 4), 130 x 4 (FR = 2)
    // ALIAS: the field texels live in the (not yet staged) weight-sum plane-set; see above
    constexpr bool ALIAS = FR == 4 && NF > 2;
    __shared__ __attribute__((aligned(16))) float4 sAcc[2][4][192];  // both plane-sets staged
    __shared__ float4 sKown[ALIAS ? 1 : FROWS][ALIAS ? 1 : FC];
    __shared__ float2 sFown[ALIAS ? 1 : NF][ALIAS ? 1 : FROWS][ALIAS ? 1 : FC];
    static_assert(!ALIAS || sizeof(float4) * FROWS * FC + sizeof(float2) * NF * FROWS * FC <= sizeof(float4) * 4 * 192, "field texels fit a plane-set");
    float4(*sK)[FC] = ALIAS ? (float4(*)[FC]) & sAcc[1][0][0] : (float4(*)[FC]) & sKown[0][0];  // .w = 1 if the texel is PSD and finite, else 0
    float2(*sF)[FROWS][FC] = ALIAS ? (float2(*)[FROWS][FC])((char*)&sAcc[1][0][0] + sizeof(float4) * FROWS * FC)
                                   : (float2(*)[FROWS][FC]) & sFown[0][0][0];
    // certainty: four dword planes [CFA position][mask row][frame][column] (allocated as 16-byte units)
    __shared__ float4 sCert[NF][3][TILE_COLS];
    float(*sMp)[3][NF][TILE_COLS] = (float(*)[3][NF][TILE_COLS]) & sCert[0][0][0];
    constexpr int EP = 3 * NF * TILE_COLS * 4;  // strip_pixel_w's plane stride
    // stored by CFA position (y parity << 1 | x parity), not by channel: strip_pixel_w<EP> indexes it
    auto stage_cert = [&](int n, int r, int c, const float (&mc)[3]) {
        sMp[0][r][n][c] = mc[Cfa<CFA>::col(0, 0)];
        sMp[1][r][n][c] = mc[Cfa<CFA>::col(0, 1)];
        sMp[2][r][n][c] = mc[Cfa<CFA>::col(1, 0)];
        sMp[3][r][n][c] = mc[Cfa<CFA>::col(1, 1)];
    };
    __shared__ uint32_t sUnsat[3][TILE_COLS];  // bit n: frame n's certainty texel is not (1, 1, 1)
    __shared__ __attribute__((aligned(16))) float sColA[256];  // x fraction per HR column of the tile, -1 = not on the predicted texel
    __shared__ float sRowB[4];                                 // y fraction per HR row of the tile, -1 likewise
    // accumulator staging: per wave and plane-set the wave's 3 KiB row segment, in memory order
    const int lx = threadIdx.x, ly = threadIdx.y;
    const int tx = bIdX * 64 + lx;
    const int Y = bIdY * 4 + ly;
    const int hrW = 2 * dimX, hrH = 2 * dimY;
    const int X0 = 4 * tx;
    const int fw = kernelParam.width, fh = kernelParam.height;  // == hrW/FR, hrH/FR (checked on the host)
    const int mw = dimX / 2, mh = dimY / 2;                       // certainty mask size
    {
        const int t = ly * 64 + lx;
        if constexpr (FR != 4) {
            // fields and certainty on different grids: two staging loops
            for (int i = t; i < FROWS * FC; i += 256) {
                const int r = i / FC, c = i - r * FC;
                const int gy = bIdY * (4 / FR) - 1 + r, gx = bIdX * (256 / FR) - 1 + c;
                const int fy = clampi(gy, 0, fh - 1), fx = clampi(gx, 0, fw - 1);
                float4 k = row_ptr((const float4*)kernelParam.ptr, kernelParam.pitch, fy)[fx];
                k.w = psd_ok(k.x, k.y, k.z) ? 1.0f : 0.0f;
                sK[r][c] = k;
#pragma unroll
                for (int n = 0; n < NF; n++) sF[n][r][c] = row_ptr((const float2*)fr.f[n].shifts.ptr, fr.f[n].shifts.pitch, fy)[fx];
            }
            if (t < 3 * TILE_COLS) {
                const int r = t / TILE_COLS, c = t - r * TILE_COLS;
                const int gy = bIdY - 1 + r, gx = bIdX * 64 - 1 + c;
                uint32_t unsat = 0;
#pragma unroll
                for (int n = 0; n < NF; n++) {
                    const float4 m = row_ptr(fr.f[n].mask, strideMask, clampi(gy, 0, mh - 1))[clampi(gx, 0, mw - 1)];
                    const float mc[3] = {sane(m.x), sane(m.y), sane(m.z)};
                    stage_cert(n, r, c, mc);
                    if (!(mc[0] == 1.0f && mc[1] == 1.0f && mc[2] == 1.0f)) unsat |= 1u << n;
                }
                sUnsat[r][c] = unsat;
            }
        } else if (t < 3 * TILE_COLS) {
            const int r = t / TILE_COLS, c = t - r * TILE_COLS;
            const int gy = bIdY - 1 + r, gx = bIdX * 64 - 1 + c;
            const int fy = clampi(gy, 0, fh - 1), fx = clampi(gx, 0, fw - 1);
            float4 k = row_ptr((const float4*)kernelParam.ptr, kernelParam.pitch, fy)[fx];
            // a bilinear mix of PSD matrices is PSD, so admitting texels admits every pixel between them
            k.w = psd_ok(k.x, k.y, k.z) ? 1.0f : 0.0f;
            sK[r][c] = k;
            uint32_t unsat = 0;
#pragma unroll
            for (int n = 0; n < NF; n++) {
                sF[n][r][c] = row_ptr((const float2*)fr.f[n].shifts.ptr, fr.f[n].shifts.pitch, fy)[fx];
                const float4 m = row_ptr(fr.f[n].mask, strideMask, clampi(gy, 0, mh - 1))[clampi(gx, 0, mw - 1)];
                const float mc[3] = {sane(m.x), sane(m.y), sane(m.z)};
                stage_cert(n, r, c, mc);
                if (!(mc[0] == 1.0f && mc[1] == 1.0f && mc[2] == 1.0f)) unsat |= 1u << n;
            }
            sUnsat[r][c] = unsat;
        }
        {
            // column t of the tile: the float path of tex_coord, texel column predicted and verified
            const int X = bIdX * 256 + t;
            const float posX = ((float)X + 0.5f) / (float)hrW;
            float xB = posX * (float)fw - 0.5f;
            if (!finitef(xB)) xB = 0.0f;
            const float fxf = floorf(xB);
            // texel column floor(xB) as predicted: (X / FR) - 1 for the first half of a texel's pixels, X / FR for the second
            const int txc = FR == 4 ? X >> 2 : X >> 1, ci = FR == 4 ? ((t & 3) < 2 ? 0 : 1) : (t & 1);
            const bool ok = (f2i(fxf) == txc - 1 + ci) && (txc + ci <= fw - 1);
            sColA[t] = ok ? xB - fxf : -1.0f;
        }
        if (t < 4) {
            const int Yr = bIdY * 4 + t;
            const float posY = ((float)Yr + 0.5f) / (float)hrH;
            float yB = posY * (float)fh - 0.5f;
            if (!finitef(yB)) yB = 0.0f;
            const float fyf = floorf(yB);
            const int frr = FR == 4 ? (t < 2 ? 0 : 1) : (t + 1) >> 1;  // LDS row of texel row floor(yB)
            const bool ok = (f2i(fyf) == bIdY * (4 / FR) - 1 + frr) && f2i(fyf) >= 0 && f2i(fyf) + 1 <= fh - 1;
            sRowB[t] = ok ? yB - fyf : -1.0f;
        }
    }
    // asynchronous global -> LDS copy of both accumulator segments; consumed only after the tap arithmetic
    const bool rowLive = Y >= STRIP_MARGIN && Y < hrH - STRIP_MARGIN;
    const size_t rowBytes = (size_t)hrW * 12;
    const size_t segByte = (size_t)bIdX * 3072;
    // WIN: g = the window row; chunk at frame-row byte gb lives at g + gb - winB0 if winB0 <= gb < winB1
    const size_t winB0 = WIN ? (size_t)wx0 * 12 : 0, winB1 = WIN ? (size_t)wx1 * 12 : 0;
    char* gP = WIN ? (char*)imgOut + (size_t)(Y - wy0) * strideOut : (char*)imgOut + (size_t)Y * strideOut + segByte;
    char* gW = WIN ? (char*)totalWeights + (size_t)(Y - wy0) * strideOut : (char*)totalWeights + (size_t)Y * strideOut + segByte;
    auto inWin = [&](size_t gb) { return !WIN || (gb >= winB0 && gb + 16 <= winB1); };
    auto chunk = [&](char* g, size_t off) { return WIN ? g + (segByte + off - winB0) : g + off; };
    // plane-set g (this wave's row segment) -> LDS plane pl: zeroes on the first launch of a burst (the accumulators are
    // defined to be zero and are not read at all), else the asynchronous copy
    auto stage_plane = [&](char* g, int pl) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            if (fresh) {
                sAcc[pl][ly][j * 64 + lx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            } else {
                const size_t off = (size_t)(j * 64 + lx) * 16;
                if (segByte + off + 16 <= rowBytes && inWin(segByte + off))
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)chunk(g, off),
                                                     (__attribute__((address_space(3))) void*)&sAcc[pl][ly][j * 64], 16, 0, 0);
            }
        }
    };
    if (rowLive) {
        stage_plane(gP, 0);
        if (!ALIAS) stage_plane(gW, 1);  // (ALIAS: after the last read of the field texels, below)
    }
    __syncthreads();
    if (!rowLive) return;
    const bool stripLive = X0 >= STRIP_MARGIN && X0 < hrW - STRIP_MARGIN;

    const int fr_ = FR == 4 ? (ly < 2 ? 0 : 1) : (ly + 1) >> 1;
    constexpr int SC = FR == 4 ? 3 : 4;                               // texel columns a strip touches
    const int cb = FR == 4 ? lx : 2 * lx;                             // LDS column of the first of them
    auto ciOf = [](int k) { return FR == 4 ? (k < 2 ? 0 : 1) : (k + 1) >> 1; };  // left texel of pixel k's pair
    const float b = sRowB[ly];
    const float4 av4 = ((const float4*)sColA)[lx];
    const float av[4] = {av4.x, av4.y, av4.z, av4.w};
    const bool geomOk = stripLive && b >= 0.0f && fminf(fminf(av[0], av[1]), fminf(av[2], av[3])) >= 0.0f;

    // kernel parameters of this strip (frame independent): 3 columns x 2 rows of texels
    float kxa[4], kya[4], kza[4];
    bool kOk;
    {
        float4 Kt[2][SC];
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int c = 0; c < SC; c++) Kt[r][c] = sK[fr_ + r][cb + c];
        float kAll = ((Kt[0][0].w * Kt[0][1].w) * (Kt[0][2].w * Kt[1][0].w)) * (Kt[1][1].w * Kt[1][2].w);
        if (SC == 4) kAll *= Kt[0][SC - 1].w * Kt[1][SC - 1].w;
        kOk = kAll > 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int ci = ciOf(k);
            // same four bilinear weights as the flow, summed with fma (no rounding step depends on them)
            const float w00 = (1.0f - av[k]) * (1.0f - b), w10 = av[k] * (1.0f - b), w01 = (1.0f - av[k]) * b, w11 = av[k] * b;
            auto mix = [&](float t00, float t10, float t01, float t11) {
                return __builtin_fmaf(w11, t11, __builtin_fmaf(w01, t01, __builtin_fmaf(w10, t10, w00 * t00)));
            };
            kxa[k] = mix(Kt[0][ci].x, Kt[0][ci + 1].x, Kt[1][ci].x, Kt[1][ci + 1].x);
            kya[k] = mix(Kt[0][ci].y, Kt[0][ci + 1].y, Kt[1][ci].y, Kt[1][ci + 1].y);
            kza[k] = mix(Kt[0][ci].z, Kt[0][ci + 1].z, Kt[1][ci].z, Kt[1][ci + 1].z);
        }
    }

    float accP[12], accW[12];
#pragma unroll
    for (int i = 0; i < 12; i++) accP[i] = accW[i] = 0.0f;
    const uint32_t xmax = (uint32_t)(2 * dimX - 5), ymax = (uint32_t)(2 * dimY - 5);
    uint32_t safeBits = 0;  // bit n: frame n took the fast path
    if constexpr (NF > 1 || FR != 4) {
        // Several frames, pixel-major: the 13 tap weights of a pixel (12 v_exp_f32 and their exponents: a fifth of the
        // pixel's arithmetic) depend on the kernel parameters only, so each pixel takes them ONCE and applies them to
        // both frames before the next pixel starts -- 13 live registers instead of the 4 x 13 a frame-major loop would
        // have to keep (that was 214 VGPRs; recomputing them per frame was the faster frame-major form).
        // Pass 1, per frame: whole-pixel flow of the four pixels (packed 16:16) and the fast-path admission.
        // (ALIAS: 8:8 bits per pixel, sxy[n][0] = the four sx, sxy[n][1] = the four sy; else 16:16 per pixel)
        uint32_t sxy[NF][ALIAS ? 2 : 4];
        // (ALIAS: the 8 bits hold the flow RELATIVE to the rounded flow of the tile's centre texel, a per-frame scalar -- so
        // a large global shift of a frame costs nothing; a strip more than 127 HR pixels away from it takes the straight path)
        int bsx[NF], bsy[NF];
#pragma unroll
        for (int n = 0; n < NF; n++) {
            bsx[n] = bsy[n] = 0;
            if constexpr (ALIAS) {
                sxy[n][0] = sxy[n][1] = 0u;
                const float2 cf = sF[n][1][FC / 2];
                bsx[n] = __builtin_amdgcn_readfirstlane(min(max(round2i(cf.x * 2.0f), -32000), 32000));
                bsy[n] = __builtin_amdgcn_readfirstlane(min(max(round2i(cf.y * 2.0f), -32000), 32000));
            }
            float2 Ft[2][SC];
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int c = 0; c < SC; c++) Ft[r][c] = sF[n][fr_ + r][cb + c];
            bool safe = geomOk && kOk;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int ci = ciOf(k);
                const float ux = lerp4(Ft[0][ci].x, Ft[0][ci + 1].x, Ft[1][ci].x, Ft[1][ci + 1].x, av[k], b);
                const float uy = lerp4(Ft[0][ci].y, Ft[0][ci + 1].y, Ft[1][ci].y, Ft[1][ci + 1].y, av[k], b);
                const int sx = round2i(ux * 2.0f), sy = round2i(uy * 2.0f);
                const int qx = X0 + k + sx - 2, qy = Y + sy - 2;
                // as below, with the rounded flow inside 16 signed bits (wilder strips take the straight arithmetic).
                // ALIAS: that test is implied by the 8-bit window below.  dx = sx - bsx taken modulo 2^32 passes
                // dx + 128 < 256 only if sx is congruent to bsx + d with d in [-128, 127]; |bsx| <= 32000 puts bsx + d in
                // [-32128, 32127], far from wrapping, so the int32 sx IS that value: inside 16 signed bits.  This holds for
                // every int32 sx, saturated conversions of wild flow included.
                if constexpr (!ALIAS)
                    safe = safe && (uint32_t)(sx + (1 << 15)) < (2u << 15) && (uint32_t)(sy + (1 << 15)) < (2u << 15);
                safe = safe && (uint32_t)qx <= xmax && (uint32_t)qy <= ymax;
                if constexpr (ALIAS) {
                    const uint32_t dx = (uint32_t)sx - (uint32_t)bsx[n], dy = (uint32_t)sy - (uint32_t)bsy[n];
                    safe = safe && dx + 128u < 256u && dy + 128u < 256u;
                    sxy[n][0] |= (dx & 0xffu) << (8 * k);
                    sxy[n][1] |= (dy & 0xffu) << (8 * k);
                } else {
                    sxy[n][k] = ((uint32_t)sx & 0xffffu) | ((uint32_t)sy << 16);
                }
            }
            if (safe) safeBits |= 1u << n;
        }
        if constexpr (ALIAS) {
            // every wave of the workgroup is past its reads of sK / sF (the rows outside the frame left before the first
            // barrier as whole workgroups): the weight-sum plane-set may land on them
            __syncthreads();
            stage_plane(gW, 1);
        }
        // Pass 2, per pixel: weights once, then frame after frame.  What the eight pixel-frame bodies share is taken
        // here once (each body is its own divergent region, the compiler does not hoist across them).
        uint32_t mrowA[5];
        certainty_row_addrs<NF>(sMp, lx, ly, mrowA);
        glb_cptr rawBase[NF];
        raw_bases<NF>(fr.f, rawBase);
        const uint32_t rawPitch = (uint32_t)dimX * 2u;  // bytes per raw row
        StripLevels lvv = lv;  // levels in kernel-argument SGPRs (a copy by value: the bodies' code depends on it)
        const uint32_t satW = saturated_frames<NF>(sUnsat, lx, ly);
        auto pixel = [&](auto kc) {
            constexpr int k = decltype(kc)::value;
            if (safeBits == 0) return;
            // this pixel's value sums live here only while the pixel is worked on, then go into the staged plane-set
            // (12 registers fewer across the other pixels; the weight sums have no staged plane yet when NF > 2)
            float aP[12];
            aP[3 * k] = aP[3 * k + 1] = aP[3 * k + 2] = 0.0f;
            float w[13];
            tap_weights13(kxa[k], kya[k], kza[k], w);
            float P[3][4];
            if (satW) tap_pair_sums(w, P);
#pragma unroll
            for (int n = 0; n < NF; n++) {
                if ((safeBits >> n) & 1u) {
                    auto rawf = [&](int x0, int y0, float (&sv)[3][3]) {
                        const uint32_t boff = (uint32_t)(y0 * dimX + x0) * 2u;  // admitted strips: x0, y0 >= 0, inside the frame
#pragma unroll
                        for (int j = 0; j < 3; j++) {
                            // The whole offset in 32 bits, the lane part of the address is one VGPR: off <= (y0 + 2) * dimX * 2
                            // + 2 * x0 lies inside the frame, and tile_kernel_ok() admits frames below 4 GiB only.  Opaque,
                            // so that base + offset is formed in the body that loads -- both bodies of a frame take the same
                            // sites, and an address hoisted above their branch reaches the loads as a 64-bit VGPR pair.
                            uint32_t off = boff + (uint32_t)j * rawPitch;
                            asm volatile("" : "+v"(off));
                            glb_cptr rb = rawBase[n] + off;
#pragma unroll
                            for (int i = 0; i < 3; i++) sv[j][i] = (float)*(const __attribute__((address_space(1))) uint16_t*)(rb + 2 * i);
                        }
                    };
                    auto mval = [&](int jt, int cell, auto... e) {
                        return *(const __attribute__((address_space(3))) float*)(uintptr_t)((mrowA[jt] + ... + e) +
                                                                                             (uint32_t)(n * TILE_COLS + cell) * 4u);
                    };
                    const int sx = ALIAS ? bsx[n] + (int)(int8_t)(sxy[n][0] >> (8 * k)) : (int)(int16_t)(sxy[n][ALIAS ? 0 : k] & 0xffffu);
                    const int sy = ALIAS ? bsy[n] + (int)(int8_t)(sxy[n][1] >> (8 * k)) : (int)sxy[n][ALIAS ? 0 : k] >> 16;
                    if ((satW >> n) & 1u)
                        strip_pixel_sat<k, CFA>(X0 + k, Y, sx, sy, w, P, rawf, lvv, aP, accW);
                    else
                        strip_pixel_w<k, CFA, EP>(X0 + k, Y, sx, sy, w, rawf, mval, lvv, aP, accW);
                }
            }
            if (k == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the staged plane-set has landed (long ago)
            float* myP = (float*)&sAcc[0][ly][0] + lx * 12 + 3 * k;
            myP[0] += aP[3 * k];
            myP[1] += aP[3 * k + 1];
            myP[2] += aP[3 * k + 2];
        };
        pixel(std::integral_constant<int, 0>{});
        pixel(std::integral_constant<int, 1>{});
        pixel(std::integral_constant<int, 2>{});
        pixel(std::integral_constant<int, 3>{});
    } else {
        // One frame, fields at HR/4: the frame-major form
        int sx[4], sy[4];
        if (strip_flow<2, 4, 20>(geomOk && kOk, &sF[0][fr_][lx], &sF[0][fr_ + 1][lx], av, b, X0, Y, xmax, ymax, sx, sy)) {
            safeBits = 1u;
            const uint16_t* raw = fr.f[0].raw;
            // certainty: LDS row of the mask row that tap row jt reads = ((ly + jt - 2) >> 2) + 1; column lx + cell
            auto mval = [&](int jt, int cell, auto... e) {
                const int mr = ((ly + jt - 2) >> 2) + 1;
                return *(const float*)((const char*)&sMp[0][mr][0][lx + cell] + (e + ...));
            };
            strip_pixel<0, CFA, EP>(X0 + 0, Y, sx[0], sy[0], kxa[0], kya[0], kza[0], raw, dimX, mval, lv, accP, accW);
            strip_pixel<1, CFA, EP>(X0 + 1, Y, sx[1], sy[1], kxa[1], kya[1], kza[1], raw, dimX, mval, lv, accP, accW);
            strip_pixel<2, CFA, EP>(X0 + 2, Y, sx[2], sy[2], kxa[2], kya[2], kza[2], raw, dimX, mval, lv, accP, accW);
            strip_pixel<3, CFA, EP>(X0 + 3, Y, sx[3], sy[3], kxa[3], kya[3], kza[3], raw, dimX, mval, lv, accP, accW);
        }
    }
    // staged plane pl += this lane's 4 pixels x 3 channels
    auto add_plane = [&](int pl, const float* acc) {
        float4* my = (float4*)((float*)&sAcc[pl][ly][0] + lx * 12);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            float4 a = my[j];
            a.x += acc[4 * j + 0]; a.y += acc[4 * j + 1]; a.z += acc[4 * j + 2]; a.w += acc[4 * j + 3];
            my[j] = a;
        }
    };
    // border / wild-flow / non-PSD strips of a frame: the straight per-pixel arithmetic on the staged values (after the
    // sums have left the registers: it needs most of them).  These strips are a few per frame.
    auto slow_frames = [&]() {
        float* myP = (float*)&sAcc[0][ly][0] + lx * 12;
        float* myW = (float*)&sAcc[1][ly][0] + lx * 12;
#pragma unroll 1
        for (int n = 0; n < NF; n++) {
            if (!((safeBits >> n) & 1u) && stripLive) {
                // the frame's arguments picked with scalar selects: the argument struct stays in SGPRs
                TileFrame F = fr.f[0];
#pragma unroll
                for (int m = 1; m < NF; m++)
                    if (n == m) F = fr.f[m];
#pragma unroll 1
                for (int k = 0; k < 4; k++) {
                    const int X = X0 + k;
                    if (X >= 1 && X < hrW - 1) {
                        pix3 px = {myP[3 * k], myP[3 * k + 1], myP[3 * k + 2]};
                        pix3 tw = {myW[3 * k], myW[3 * k + 1], myW[3 * k + 2]};
                        accumulate_pixel_core<GEOM_FULL, true>(X, Y, F.raw, F.mask, kernelParam, F.shifts, glv, dimX, dimY, 2,
                                                               strideMask, cfaPacked, px, tw);
                        myP[3 * k] = px.x; myP[3 * k + 1] = px.y; myP[3 * k + 2] = px.z;
                        myW[3 * k] = tw.x; myW[3 * k + 1] = tw.y; myW[3 * k + 2] = tw.z;
                    }
                }
            }
        }
    };
    // staged plane pl back to g in memory order: contiguous 1 KiB per store instruction
    auto store_plane = [&](int pl, char* g) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const size_t off = (size_t)(j * 64 + lx) * 16;
            // the 16-pixel side margins of the row belong to k_accumulateMargin: their (unchanged) chunks are not written
            // back.  A fresh launch defines them (zero) instead.
            const size_t gb = segByte + off;
            const bool sideMargin = gb < (size_t)STRIP_MARGIN * 12 || gb + 16 > rowBytes - (size_t)STRIP_MARGIN * 12;
            if (gb + 16 <= rowBytes && (fresh || !sideMargin) && inWin(gb)) *(float4*)chunk(g, off) = sAcc[pl][ly][j * 64 + lx];
        }
    };
    // staged accumulators must have landed before anyone reads them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    constexpr bool valueSumsStaged = NF > 1 || FR != 4;  // the pixel-major loop has added them already
    if (!valueSumsStaged) add_plane(0, accP);
    add_plane(1, accW);
    if (safeBits != (1u << NF) - 1u) slow_frames();
    store_plane(0, gP);
    store_plane(1, gW);
}

// ---- burst form of the x2 Bayer tile kernel: G groups of four frames in one launch ------------------
// A burst of 16 frames used to be four launches of k_accumulate2xTile<CFA, 4>, each a complete pass over both accumulator
// plane-sets.  Here a workgroup stages its two row segments ONCE (zeroes on a fresh launch, else the global_load_lds copy),
// runs the four-frame group arithmetic of k_accumulate2xTile G times on them -- a rolled loop, each turn stages that group's flow
// and certainty texels and adds the group's sums into the staged planes -- and writes them back ONCE: G - 1 reads and G - 1
// write-backs of 48 B per HR pixel less, and one kernel ramp and tail instead of G.
// Bit identity with the G launches it replaces dictates the structure: a pixel's value sums AND weight sums of a group are
// formed from zero in registers and added to the staged planes at the end of their group (carrying the weight sums across
// groups in registers would be another association), so both planes stay in LDS for the whole launch and the field texels
// cannot borrow the weight plane's bytes (the ALIAS layout): 48.6 KB of LDS, three workgroups per CU, a 168-register budget.
// The admission rules are those of the launches it replaces (the ALIAS form: rounded flow within the 8-bit window around the
// tile's own, 8:8 bits per pixel), so the same strips take the in-kernel straight path; a write-back followed by a read is
// exact, so the straight path sees the same plane values either way.
// What does not depend on the group is taken once per launch: the kernel-parameter texels, the column and row fractions and
// the strip's mixed kernel parameters.  The frames of all groups travel in the kernel arguments, indexed by the (uniform) group.
// Every barrier is reached by whole workgroups: the margin rows leave before the first one, and STRIP_MARGIN is a multiple
// of the tile height, so a workgroup is live or not as a whole.  nGroups (2 .. TILE_BURST_GROUPS) is a kernel argument.
#define TILE_BURST_GROUPS 4
struct BurstFrames {
    TileFrame f[4 * TILE_BURST_GROUPS];
};

// The finishing form (FIN): the launch is the burst's last fuse and the output is the plain uint16_t image, so each live lane
// also finishes its own four pixels from the staged planes -- the arithmetic of k_finishFused without gamma, finish_common.hpp --
// and the wave's 1 536 bytes of RGB leave through its own LDS row in memory order.  The finish pass over both plane-sets
// (24 B read per pixel) is then not run; the ring is k_finishRing's.  A second instance, so that the form without it is the
// kernel it was, instruction for instruction.
template <bool FIN>
struct TileFinish {
};
template <>
struct TileFinish<true> {
    FinishSrc src;    // the fallback image, its window, the threshold; the launch is the whole frame (offsets 0)
    uint16_t* out16;  // dense RGB, hrW x hrH
};

template <int CFA, bool FIN = false>
__global__ void __launch_bounds__(256, 3)
    k_accumulate2xTileBurst(BurstFrames fr, int nGroups, pix3* __restrict__ imgOut, pix3* __restrict__ totalWeights, mfsr_tex2d kernelParam,
                            Levels3 glv, StripLevels lv, int dimX, int dimY, int strideOut, int strideMask, int cfaPacked, int tilesX,
                            int tilesY, int tilesPerXcd, int fresh, TileFinish<FIN> fin)
{
    constexpr int NF = 4, FC = TILE_COLS, FROWS = 3;
    const int tile = xcd_tile_index((int)blockIdx.x, tilesPerXcd);
    if (tile >= tilesX * tilesY) return;  // whole workgroup (uniform), before any barrier
    const int bIdY = tile / tilesX, bIdX = tile - bIdY * tilesX;
    __shared__ __attribute__((aligned(16))) float4 sAcc[2][4][192];
    __shared__ float4 sK[FROWS][FC];  // .w = 1 if the texel is PSD and finite, else 0
    __shared__ float2 sF[NF][FROWS][FC];
    __shared__ __attribute__((aligned(16))) float sMp[4][3][NF][TILE_COLS];  // [CFA position][mask row][frame][column]
    __shared__ uint32_t sUnsat[3][TILE_COLS];
    __shared__ __attribute__((aligned(16))) float sColA[256];
    __shared__ float sRowB[4];
    const int lx = threadIdx.x, ly = threadIdx.y;
    const int t = ly * 64 + lx;
    const int tx = bIdX * 64 + lx;
    const int Y = bIdY * 4 + ly;
    const int hrW = 2 * dimX, hrH = 2 * dimY;
    const int X0 = 4 * tx;
    const int fw = kernelParam.width, fh = kernelParam.height;  // == hrW/4, hrH/4 (checked on the host)
    const int mw = dimX / 2, mh = dimY / 2;
    // flow and certainty texels of group g (and which of them are not saturated)
    auto stage_fields = [&](int g) {
        if (t < 3 * TILE_COLS) {
            const int r = t / TILE_COLS, c = t - r * TILE_COLS;
            const int gy = bIdY - 1 + r, gx = bIdX * 64 - 1 + c;
            const int fy = clampi(gy, 0, fh - 1), fx = clampi(gx, 0, fw - 1);
            uint32_t unsat = 0;
#pragma unroll
            for (int n = 0; n < NF; n++) {
                const TileFrame& F = fr.f[4 * g + n];
                sF[n][r][c] = row_ptr((const float2*)F.shifts.ptr, F.shifts.pitch, fy)[fx];
                const float4 m = row_ptr(F.mask, strideMask, clampi(gy, 0, mh - 1))[clampi(gx, 0, mw - 1)];
                const float mc[3] = {sane(m.x), sane(m.y), sane(m.z)};
                sMp[0][r][n][c] = mc[Cfa<CFA>::col(0, 0)];
                sMp[1][r][n][c] = mc[Cfa<CFA>::col(0, 1)];
                sMp[2][r][n][c] = mc[Cfa<CFA>::col(1, 0)];
                sMp[3][r][n][c] = mc[Cfa<CFA>::col(1, 1)];
                if (!(mc[0] == 1.0f && mc[1] == 1.0f && mc[2] == 1.0f)) unsat |= 1u << n;
            }
            sUnsat[r][c] = unsat;
        }
    };
    if (t < 3 * TILE_COLS) {
        const int r = t / TILE_COLS, c = t - r * TILE_COLS;
        const int fy = clampi(bIdY - 1 + r, 0, fh - 1), fx = clampi(bIdX * 64 - 1 + c, 0, fw - 1);
        float4 k = row_ptr((const float4*)kernelParam.ptr, kernelParam.pitch, fy)[fx];
        k.w = psd_ok(k.x, k.y, k.z) ? 1.0f : 0.0f;
        sK[r][c] = k;
    }
    stage_fields(0);
    sColA[t] = texel_fraction<4, false>(bIdX * 256 + t, hrW, fw);
    if (t < 4) sRowB[t] = texel_fraction<4, true>(bIdY * 4 + t, hrH, fh);
    const bool rowLive = Y >= STRIP_MARGIN && Y < hrH - STRIP_MARGIN;
    const size_t segByte = (size_t)bIdX * 3072;
    const AccSegment<false> seg{(size_t)hrW * 12, segByte, 0, 0, fresh};
    if (rowLive) {
        seg.stage((char*)imgOut + (size_t)Y * strideOut + segByte, &sAcc[0][ly][0], lx);
        seg.stage((char*)totalWeights + (size_t)Y * strideOut + segByte, &sAcc[1][ly][0], lx);
    }
    __syncthreads();
    if (!rowLive) return;
    const bool stripLive = X0 >= STRIP_MARGIN && X0 < hrW - STRIP_MARGIN;

    const int fr_ = ly < 2 ? 0 : 1;
    const float b0 = sRowB[ly];
    const float4 av4 = ((const float4*)sColA)[lx];
    const bool geomOk = stripLive && b0 >= 0.0f && fminf(fminf(av4.x, av4.y), fminf(av4.z, av4.w)) >= 0.0f;

    // kernel parameters of this strip (the same for every frame of every group)
    float kxa[4], kya[4], kza[4];
    bool kOk;
    {
        const float av[4] = {av4.x, av4.y, av4.z, av4.w}, b = b0;
        float4 Kt[2][3];
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) Kt[r][c] = sK[fr_ + r][lx + c];
        const float kAll = ((Kt[0][0].w * Kt[0][1].w) * (Kt[0][2].w * Kt[1][0].w)) * (Kt[1][1].w * Kt[1][2].w);
        kOk = kAll > 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int ci = k < 2 ? 0 : 1;
            const float w00 = (1.0f - av[k]) * (1.0f - b), w10 = av[k] * (1.0f - b), w01 = (1.0f - av[k]) * b, w11 = av[k] * b;
            auto mix = [&](float t00, float t10, float t01, float t11) {
                return __builtin_fmaf(w11, t11, __builtin_fmaf(w01, t01, __builtin_fmaf(w10, t10, w00 * t00)));
            };
            kxa[k] = mix(Kt[0][ci].x, Kt[0][ci + 1].x, Kt[1][ci].x, Kt[1][ci + 1].x);
            kya[k] = mix(Kt[0][ci].y, Kt[0][ci + 1].y, Kt[1][ci].y, Kt[1][ci + 1].y);
            kza[k] = mix(Kt[0][ci].z, Kt[0][ci + 1].z, Kt[1][ci].z, Kt[1][ci + 1].z);
        }
    }
    const uint32_t xmax = (uint32_t)(2 * dimX - 5), ymax = (uint32_t)(2 * dimY - 5);
    constexpr int EP = 3 * NF * TILE_COLS * 4;
    uint32_t mrowA[5];
    certainty_row_addrs<NF>(sMp, lx, ly, mrowA);
    const uint32_t rawPitch = (uint32_t)dimX * 2u;
    float* const myP = (float*)&sAcc[0][ly][0] + lx * 12;
    float* const myW = (float*)&sAcc[1][ly][0] + lx * 12;

#pragma unroll 1
    for (int g = 0; g < nGroups; g++) {
        if (g > 0) {
            __syncthreads();  // every wave is past its reads of the previous group's texels
            stage_fields(g);
            __syncthreads();
        }
        // The tap weights depend on the kernel parameters only, so the compiler would take all 4 x 13 of them (and the pair sums)
        // out of the group loop and spill: opaque per turn, they are recomputed per group as the launches they replace did
#pragma unroll
        for (int k = 0; k < 4; k++) asm volatile("" : "+v"(kxa[k]), "+v"(kya[k]), "+v"(kza[k]));
        // (likewise the bilinear weights of pass 1, which depend on the fractions only)
        float av[4] = {av4.x, av4.y, av4.z, av4.w};
        float b = b0;
#pragma unroll
        for (int k = 0; k < 4; k++) asm volatile("" : "+v"(av[k]));
        asm volatile("" : "+v"(b));
        // Pass 1, per frame: the rules of k_accumulate2xTile's ALIAS form, whose launches this replaces
        uint32_t safeBits = 0;
        uint32_t sxy[NF][2];
        int bsx[NF], bsy[NF];
#pragma unroll
        for (int n = 0; n < NF; n++) {
            sxy[n][0] = sxy[n][1] = 0u;
            const float2 cf = sF[n][1][FC / 2];
            bsx[n] = __builtin_amdgcn_readfirstlane(min(max(round2i(cf.x * 2.0f), -32000), 32000));
            bsy[n] = __builtin_amdgcn_readfirstlane(min(max(round2i(cf.y * 2.0f), -32000), 32000));
            float2 Ft[2][3];
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) Ft[r][c] = sF[n][fr_ + r][lx + c];
            bool safe = geomOk && kOk;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int ci = k < 2 ? 0 : 1;  // left texel of pixel k's pair
                const float ux = lerp4(Ft[0][ci].x, Ft[0][ci + 1].x, Ft[1][ci].x, Ft[1][ci + 1].x, av[k], b);
                const float uy = lerp4(Ft[0][ci].y, Ft[0][ci + 1].y, Ft[1][ci].y, Ft[1][ci + 1].y, av[k], b);
                const int sx = round2i(ux * 2.0f), sy = round2i(uy * 2.0f);
                const int qx = X0 + k + sx - 2, qy = Y + sy - 2;
                safe = safe && (uint32_t)qx <= xmax && (uint32_t)qy <= ymax;
                const uint32_t dx = (uint32_t)sx - (uint32_t)bsx[n], dy = (uint32_t)sy - (uint32_t)bsy[n];
                safe = safe && dx + 128u < 256u && dy + 128u < 256u;  // (implies the rounded flow fits 16 signed bits, see there)
                sxy[n][0] |= (dx & 0xffu) << (8 * k);
                sxy[n][1] |= (dy & 0xffu) << (8 * k);
            }
            if (safe) safeBits |= 1u << n;
        }
        // Pass 2, per pixel: weights once, then frame after frame; the group's weight sums start from zero
        glb_cptr rawBase[NF];
        raw_bases<NF>(&fr.f[4 * g], rawBase);
        const uint32_t satW = saturated_frames<NF>(sUnsat, lx, ly);
        float accW[12];
#pragma unroll
        for (int i = 0; i < 12; i++) accW[i] = 0.0f;
        auto pixel = [&](auto kc) {
            constexpr int k = decltype(kc)::value;
            if (safeBits == 0) return;
            float aP[12];
            aP[3 * k] = aP[3 * k + 1] = aP[3 * k + 2] = 0.0f;
            float w[13];
            tap_weights13(kxa[k], kya[k], kza[k], w);
            float P[3][4];
            if (satW) tap_pair_sums(w, P);
#pragma unroll
            for (int n = 0; n < NF; n++) {
                if ((safeBits >> n) & 1u) {
                    auto rawf = [&](int x0, int y0, float (&sv)[3][3]) {
                        const uint32_t boff = (uint32_t)(y0 * dimX + x0) * 2u;  // admitted strips: x0, y0 >= 0, inside the frame
#pragma unroll
                        for (int j = 0; j < 3; j++) {
                            uint32_t off = boff + (uint32_t)j * rawPitch;
                            asm volatile("" : "+v"(off));
                            glb_cptr rb = rawBase[n] + off;
#pragma unroll
                            for (int i = 0; i < 3; i++) sv[j][i] = (float)*(const __attribute__((address_space(1))) uint16_t*)(rb + 2 * i);
                        }
                    };
                    auto mval = [&](int jt, int cell, auto... e) {
                        return *(const __attribute__((address_space(3))) float*)(uintptr_t)((mrowA[jt] + ... + e) +
                                                                                             (uint32_t)(n * TILE_COLS + cell) * 4u);
                    };
                    const int sx = bsx[n] + (int)(int8_t)(sxy[n][0] >> (8 * k));
                    const int sy = bsy[n] + (int)(int8_t)(sxy[n][1] >> (8 * k));
                    if ((satW >> n) & 1u)
                        strip_pixel_sat<k, CFA>(X0 + k, Y, sx, sy, w, P, rawf, lv, aP, accW);
                    else
                        strip_pixel_w<k, CFA, EP>(X0 + k, Y, sx, sy, w, rawf, mval, lv, aP, accW);
                }
            }
            if (k == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the staged plane-sets have landed (first group)
            myP[3 * k] += aP[3 * k];
            myP[3 * k + 1] += aP[3 * k + 1];
            myP[3 * k + 2] += aP[3 * k + 2];
        };
        pixel(std::integral_constant<int, 0>{});
        pixel(std::integral_constant<int, 1>{});
        pixel(std::integral_constant<int, 2>{});
        pixel(std::integral_constant<int, 3>{});
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (strips that took no fast path have not waited yet)
        lane_add12(myW, accW);
        // refused strips: the straight arithmetic on the staged values, which hold the earlier groups and this group's fast
        // frames -- what the group's own launch would have read
        if (safeBits != (1u << NF) - 1u && stripLive) {
#pragma unroll 1
            for (int n = 0; n < NF; n++) {
                if ((safeBits >> n) & 1u) continue;
                const TileFrame F = fr.f[4 * g + n];
                strip_straight<2>(F, myP, myW, X0, Y, hrW, kernelParam, glv, dimX, dimY, strideMask, cfaPacked);
            }
        }
    }
    // both staged planes back in memory order, once
    // (the row's address is formed again from an opaque copy of Y: kept across the loop, the two pointers were spilled)
    int Yw = Y;
    asm volatile("" : "+v"(Yw));
    seg.store(&sAcc[0][ly][0], (char*)imgOut + (size_t)Yw * strideOut + segByte, lx);
    seg.store(&sAcc[1][ly][0], (char*)totalWeights + (size_t)Yw * strideOut + segByte, lx);
    if constexpr (FIN) {
        // The lane's own 12 value and 12 weight floats (written by this lane or staged by this wave: no barrier), twelve
        // independent divisions, then 24 bytes of RGB into the wave's own value row -- whose plane store has been issued and
        // whose last reads are waited for -- so that the row leaves as whole chunks in memory order.
        uint2* const row16 = (uint2*)&sAcc[0][ly][0];
        if (stripLive) {
            float v[12], w[12];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float4 a = ((const float4*)myP)[j], c = ((const float4*)myW)[j];
                v[4 * j] = a.x; v[4 * j + 1] = a.y; v[4 * j + 2] = a.z; v[4 * j + 3] = a.w;
                w[4 * j] = c.x; w[4 * j + 1] = c.y; w[4 * j + 2] = c.z; w[4 * j + 3] = c.w;
            }
            uint32_t need = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (finish_needs_fallback(pix3{w[3 * k], w[3 * k + 1], w[3 * k + 2]}, fin.src)) need |= 1u << k;
            pix3 fb[4];
#pragma unroll
            for (int k = 0; k < 4; k++) fb[k] = pix3{0.0f, 0.0f, 0.0f};
            if (__builtin_amdgcn_ballot_w64(need != 0) != 0) {  // (wave-uniform: most waves resample nothing)
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if ((need >> k) & 1u) fb[k] = finish_fallback(X0 + k, Yw, fin.src);
            }
            uint16_t q[12];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const pix3 p = finish_weighted(fb[k], pix3{v[3 * k], v[3 * k + 1], v[3 * k + 2]}, pix3{w[3 * k], w[3 * k + 1], w[3 * k + 2]},
                                               fin.src);
                finish_quantize3(p, 65535.0f, &q[3 * k]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every lane has its floats before the row is written over
#pragma unroll
            for (int j = 0; j < 3; j++)
                row16[3 * lx + j] = make_uint2((uint32_t)q[4 * j] | ((uint32_t)q[4 * j + 1] << 16),
                                               (uint32_t)q[4 * j + 2] | ((uint32_t)q[4 * j + 3] << 16));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // the live bytes of the row: everything but the 16 ring pixels (96 bytes) at either end, a whole number of strips
        const size_t rowB = (size_t)hrW * 6, segB = (size_t)bIdX * 1536;
        char* const orow = (char*)fin.out16 + (size_t)Yw * rowB + segB;
        if ((((uintptr_t)fin.out16 | rowB) & 15) == 0) {  // 16-byte chunks where every row starts on one (uniform)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int c = j * 64 + lx;
                const size_t gb = segB + (size_t)c * 16;
                if (c < 96 && gb >= (size_t)STRIP_MARGIN * 6 && gb + 16 <= rowB - (size_t)STRIP_MARGIN * 6)
                    *(uint4*)(orow + (size_t)c * 16) = ((const uint4*)row16)[c];
            }
        } else {  // rows that start on an odd multiple of 8 bytes (hrW = 4 (2 m + 1)): 8-byte chunks
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int c = j * 64 + lx;
                const size_t gb = segB + (size_t)c * 8;
                if (gb >= (size_t)STRIP_MARGIN * 6 && gb + 8 <= rowB - (size_t)STRIP_MARGIN * 6) *(uint2*)(orow + (size_t)c * 8) = row16[c];
            }
        }
    }
}

// The ring of the finishing burst launch: the STRIP_MARGIN pixels along every edge (the margin kernel's pixels and the outermost
// line that nobody accumulates), finished from the accumulators after k_accumulateMarginBurst by the arithmetic of
// k_finishFused (finish_common.hpp).  One thread per ring pixel in the order of finish_ring.hpp; with the tile kernel's
// epilogue every HR pixel is written exactly once.
__global__ void __launch_bounds__(256)
    k_finishRing(const pix3* __restrict__ imgOut, const pix3* __restrict__ totalWeights, int strideOut, FinishSrc src,
                 uint16_t* __restrict__ out16, int hrW, int hrH)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= finish_ring_count(hrW, hrH, STRIP_MARGIN)) return;
    int x, y;
    finish_ring_pixel(i, hrW, hrH, STRIP_MARGIN, x, y);
    const pix3 val = row_ptr(imgOut, strideOut, y)[x];
    const pix3 w = row_ptr(totalWeights, strideOut, y)[x];
    finish_quantize3(finish_value(val, w, x, y, src), 65535.0f, out16 + ((size_t)y * hrW + x) * 3);
}

// The margin pixels of the same G groups in one launch: k_accumulateMarginN<4>'s workgroup (64 pixels x 4 frames, one thread
// per pixel and frame) in a rolled loop over the groups.  A frame's sums are taken from zero and meet in LDS; the pixel's first
// thread reads the accumulators once, adds the frames one after another in call order -- the order of G consecutive launches --
// and writes them once.  Whole workgroups reach every barrier (no thread leaves early).
// (k_accumulateMarginN<4 G> with one thread per (pixel, frame), up to 64 x 16 threads per workgroup, was measured slower
// than the launches it replaces: 233 against 4 x 50 us at 4K x 16)
// Occupancy bound of the SITES form, by measurement (4K x 16): four waves per SIMD with the pixel
// opaque per turn 108 us; three waves (168 registers: the compiler then carries the pixel's cell offsets, phases and texture
// coordinates across the groups, 87 VALU instructions fewer per group) 119 us, three waves and opaque 119 us; five waves
// spill 29 registers (not run).
template <int SCALE, bool SITES = false>
__global__ void __launch_bounds__(256, 4)  // four waves per SIMD as k_accumulateMarginN<4>
    k_accumulateMarginBurst(BurstFrames fr, int nGroups, pix3* __restrict__ imgOut, pix3* __restrict__ totalWeights, mfsr_tex2d kernelParam,
                            Levels3 glv, int dimX, int dimY, int strideOut, int strideMask, int cfaPacked)
{
    constexpr int scale = SCALE, NF = 4;
    __shared__ float sSum[NF][6][64];
    const int hrW = scale * dimX, hrH = scale * dimY, M = STRIP_MARGIN;
    const int rowLen = hrW - 2;
    const int nTop = (M - 1) * rowLen, nBot = (M - 1) * rowLen;
    const int sideLen = 2 * (M - 1);
    const int nSide = (hrH - 2 * M) * sideLen;
    const int lane = threadIdx.x, n = SITES ? __builtin_amdgcn_readfirstlane(threadIdx.y) : threadIdx.y;
    const int idx = blockIdx.x * 64 + lane;
    int x = 0, y = -1;
    if (idx < nTop) {
        y = 1 + idx / rowLen;
        x = 1 + idx % rowLen;
    } else if (idx < nTop + nBot) {
        const int r = idx - nTop;
        y = hrH - M + r / rowLen;
        x = 1 + r % rowLen;
    } else if (idx < nTop + nBot + nSide) {
        const int r = idx - nTop - nBot;
        y = M + r / sideLen;
        const int c = r % sideLen;
        x = c < M - 1 ? 1 + c : hrW - M + (c - (M - 1));
    }
    const bool live = y >= 0;
    const bool first = n == 0 && live;
    pix3 a = {0.0f, 0.0f, 0.0f}, w = {0.0f, 0.0f, 0.0f};
    if (first) {
        a = row_ptr(imgOut, strideOut, y)[x];
        w = row_ptr(totalWeights, strideOut, y)[x];
    }
    __shared__ MarginHeader sHdr;  // (SITES only; an unused __shared__ object takes no LDS)
    if constexpr (SITES) margin_header<NF, SCALE>(sHdr, live, x, y, lane, n, kernelParam, dimX, dimY);
#pragma unroll 1
    for (int g = 0; g < nGroups; g++) {
        pix3 pixel = {0.0f, 0.0f, 0.0f}, totalWeight = {0.0f, 0.0f, 0.0f};
        if constexpr (SITES) {
            // the weights and the predicate come from LDS in every group: nothing of the header is carried across the loop
            // (the pixel opaque per turn, as below: what the compiler would carry across the groups spills 28 registers at
            // the 128 of four waves per SIMD)
            int xg = x, yg = y;
            asm volatile("" : "+v"(xg), "+v"(yg));
            if (live) {
                const TileFrame F = fr.f[4 * g + n];
                accumulate_pixel_sites<SCALE>(xg, yg, F.raw, F.mask, F.shifts, glv, dimX, dimY, strideMask, cfaPacked,
                                              sHdr.pos[0][lane], sHdr.pos[1][lane], sHdr.sums[lane] != 0,
                                              [&](int k) { return sHdr.w[k][lane]; }, pixel, totalWeight);
            }
        } else {
            // (opaque per turn: the compiler would otherwise carry the pixel's 25 tap weights, which depend on the kernel
            // parameters only, across the groups -- and spill 36 registers at the 128 the occupancy allows)
            int xg = x, yg = y;
            asm volatile("" : "+v"(xg), "+v"(yg));
            if (live) {
                TileFrame F = fr.f[4 * g];
#pragma unroll
                for (int m = 1; m < NF; m++)
                    if (n == m) F = fr.f[4 * g + m];
                accumulate_pixel_core<GEOM_FULL, true, true>(xg, yg, F.raw, F.mask, kernelParam, F.shifts, glv, dimX, dimY, scale,
                                                             strideMask, cfaPacked, pixel, totalWeight);
            }
        }
        sSum[n][0][lane] = pixel.x;
        sSum[n][1][lane] = pixel.y;
        sSum[n][2][lane] = pixel.z;
        sSum[n][3][lane] = totalWeight.x;
        sSum[n][4][lane] = totalWeight.y;
        sSum[n][5][lane] = totalWeight.z;
        __syncthreads();
        if (first) {
#pragma unroll
            for (int m = 0; m < NF; m++) {
                a.x += sSum[m][0][lane];
                a.y += sSum[m][1][lane];
                a.z += sSum[m][2][lane];
                w.x += sSum[m][3][lane];
                w.y += sSum[m][4][lane];
                w.z += sSum[m][5][lane];
            }
        }
        __syncthreads();  // the sums are read before the next group overwrites them
    }
    if (first) {
        row_ptr(imgOut, strideOut, y)[x] = a;
        row_ptr(totalWeights, strideOut, y)[x] = w;
    }
}

// ---- x4 ------------------------------------------------------------------------------------------
// The same pixel at scale 4.  The 5x5 HR taps of a pixel fall on 2x2 raw sites: tap column `it` lands
// on site column (ph + it) >> 2 with ph = (X + sx - 2) & 3, i.e. on column 1 iff ph + it >= 4 -- a lane
// mask per tap column (none for it = 0, all for it = 4), applied to the weights as in strip_pixel.
// Each site is its own CFA-position class (relative to the parity of (x0, y0)).  K8 = X & 7 is the
// pixel's position in its certainty cell (8 HR pixels at scale 4), K8 & 3 its position in the strip.
// strip_pixel4_w: the tap weights given (frame independent, see strip_pixel_w); RawF: void rawf(x0, y0, float (&s)[2][2])
template <int K8, int CFA, bool PARITY = false, typename RawF, typename MaskF>
__device__ __forceinline__ void strip_pixel4_w(int X, int Y, int sx, int sy, const float (&w)[13], RawF rawf, MaskF mval,
                                                const StripLevels& lv, float* accP, float* accW)
{
    const int qx = X + sx - 2, qy = Y + sy - 2;
    const int x0 = qx >> 2, y0 = qy >> 2;
    const uint32_t bx0 = 0u - (uint32_t)(qx & 1), bx1 = 0u - (uint32_t)((qx >> 1) & 1);
    const uint32_t by0 = 0u - (uint32_t)(qy & 1), by1 = 0u - (uint32_t)((qy >> 1) & 1);
    // mx[it]: tap column it lands on site column 1 (ph + it >= 4); same for rows
    const uint32_t mx[5] = {0u, bx0 & bx1, bx1, bx0 | bx1, ~0u};
    const uint32_t my[5] = {0u, by0 & by1, by1, by0 | by1, ~0u};
    const uint32_t mP = 0u - (uint32_t)(x0 & 1), mQ = 0u - (uint32_t)(y0 & 1);
    auto andm = [](uint32_t m, float a) { return __uint_as_float(m & __float_as_uint(a)); };

    float s[2][2];
    rawf(x0, y0, s);
    auto W_ = [&](int jt, int it) { const int n = jt * 5 + it; return w[n <= 12 ? n : 24 - n]; };

    // certainty cell column of tap column it, relative to the cell left of the strip's own: 0..2
    auto cellOf = [](int it) { return (K8 + it - 2 + 8) >> 3; };
    constexpr int cellLo = (K8 - 2 + 8) >> 3;
    constexpr bool twoCells = ((K8 + 4 - 2 + 8) >> 3) != cellLo;

    float C[5][2];  // per tap row: w * certainty summed per site column
#pragma unroll
    for (int jt = 0; jt < 5; jt++) {
        const uint32_t mya = mQ ^ my[jt];  // absolute y parity of the site row this tap row lands on
        float Ee[2], Eo[2];
        if constexpr (PARITY) {
            // CFA position (y parity << 1 | x parity) of site column 0 on this tap row; tap row jt sits on site row
            // ((qy & 3) + jt) >> 2, whose parity is Q flipped when that is 1
            const int ph = qy & 3;
            const int flip = jt == 0 ? 0 : (jt == 4 ? 1 : (jt == 1 ? (ph == 3) : (jt == 2 ? (ph >> 1) : (ph != 0))));
            const int e = (((y0 & 1) ^ flip) << 1) | (x0 & 1);
#pragma unroll
            for (int c = 0; c < (twoCells ? 2 : 1); c++) {
                Ee[c] = mval(jt, cellLo + c, e);
                Eo[c] = mval(jt, cellLo + c, e ^ 1);
            }
        } else {
#pragma unroll
            for (int c = 0; c < (twoCells ? 2 : 1); c++) {
                float m[3];
#pragma unroll
                for (int ch = 0; ch < 3; ch++) m[ch] = mval(jt, cellLo + c, ch);
                resolve_certainty<CFA>(mya, mP, m, Ee[c], Eo[c]);
            }
        }
        // weights per (site column, cell), then one multiply with the certainty of that pair
        float lo[2] = {0.0f, 0.0f}, hi[2] = {0.0f, 0.0f};
        bool loUsed[2] = {false, false}, hiUsed[2] = {false, false};
#pragma unroll
        for (int it = 0; it < 5; it++) {
            const int c = cellOf(it) - cellLo;
            const float wt = W_(jt, it);
            if (it < 4) {
                const float v = it == 0 ? wt : andm(~mx[it], wt);
                lo[c] = loUsed[c] ? lo[c] + v : v;
                loUsed[c] = true;
            }
            if (it > 0) {
                const float v = it == 4 ? wt : andm(mx[it], wt);
                hi[c] = hiUsed[c] ? hi[c] + v : v;
                hiUsed[c] = true;
            }
        }
        float c0 = loUsed[0] ? lo[0] * Ee[0] : 0.0f;
        if (twoCells && loUsed[1]) c0 = loUsed[0] ? __builtin_fmaf(lo[1], Ee[1], c0) : lo[1] * Ee[1];
        float c1 = hiUsed[0] ? hi[0] * Eo[0] : 0.0f;
        if (twoCells && hiUsed[1]) c1 = hiUsed[0] ? __builtin_fmaf(hi[1], Eo[1], c1) : hi[1] * Eo[1];
        C[jt][0] = c0;
        C[jt][1] = c1;
    }
    float S[2][2], W[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const float o0 = ((C[0][i] + andm(~my[1], C[1][i])) + andm(~my[2], C[2][i])) + andm(~my[3], C[3][i]);
        const float o1 = ((andm(my[1], C[1][i]) + andm(my[2], C[2][i])) + andm(my[3], C[3][i])) + C[4][i];
        W[0][i] = o0;
        W[1][i] = o1;
        S[0][i] = s[0][i] * o0;
        S[1][i] = s[1][i] * o1;
    }
    classes_to_channels<(K8 & 3), CFA>(S, W, mP, mQ, lv, accP, accW);
}

template <int K8, int CFA, bool PARITY = false, typename MaskF>
__device__ __forceinline__ void strip_pixel4(int X, int Y, int sx, int sy, float kx, float ky, float kz,
                                              const uint16_t* __restrict__ raw, int dimX, MaskF mval,
                                              const StripLevels& lv, float* accP, float* accW)
{
    float w[13];
    tap_weights13(kx, ky, kz, w);
    auto rawf = [&](int x0, int y0, float (&s)[2][2]) {
        const uint16_t* r = raw + (size_t)y0 * dimX + x0;
        s[0][0] = (float)r[0];
        s[0][1] = (float)r[1];
        s[1][0] = (float)r[dimX];
        s[1][1] = (float)r[dimX + 1];
    };
    strip_pixel4_w<K8, CFA, PARITY>(X, Y, sx, sy, w, rawf, mval, lv, accP, accW);
}

// x4 LDS tile kernel (fields at HR/8: the Bayer pipeline at scale 4).  One 64x4 workgroup covers a
// 512 x 2 HR tile: wave (r, h) = (threadIdx.y >> 1, threadIdx.y & 1) owns row r and the strips whose
// position in the 8-pixel certainty cell is h (lane lx -> strip 2*lx + h), so K8 is a compile-time
// constant per wave.  Staging as in the x2 kernel (64 + 2 field texels x 3 rows, column/row fractions,
// accumulator rows through LDS-DMA); the two waves of a row share its staged segment, hence the
// workgroup barriers around the LDS update.
// (three and four frames per launch: four workgroups per CU by the ALIAS layout, see k_accumulate2xTile)
// WIN: as k_accumulate2xTile (window edges are multiples of 16 pixels = 12 chunks of a 512-pixel tile row)
template <int CFA, int NF, bool WIN = false>
__global__ void __launch_bounds__(256, tile_waves_x4(NF))
    k_accumulate4xTile(TileFrames<NF> fr, pix3* __restrict__ imgOut, pix3* __restrict__ totalWeights, mfsr_tex2d kernelParam,
                       Levels3 glv, StripLevels lv, int dimX, int dimY, int strideOut, int strideMask, int cfaPacked,
                       int tilesX, int fresh, int tileY0, int tileX0, int wx0, int wx1, int wy0)
{
    const int bIdYrel = (int)blockIdx.x / tilesX, bIdX = (int)blockIdx.x - bIdYrel * tilesX + (WIN ? tileX0 : 0);
    const int bIdY = bIdYrel + tileY0;  // tileY0: first tile row of this launch's HR row window
    const int hrW = 4 * dimX, hrH = 4 * dimY;
    const int Y0 = 2 * bIdY;
    if (Y0 < STRIP_MARGIN || Y0 >= hrH - STRIP_MARGIN) return;  // whole workgroup (margin rows)
    constexpr bool ALIAS = NF > 2;
    __shared__ __attribute__((aligned(16))) float4 sAcc[2][2][384];  // [plane-set][row][6 KiB row segment]
    __shared__ float4 sKown[ALIAS ? 1 : 3][ALIAS ? 1 : TILE_COLS];
    __shared__ float2 sFown[ALIAS ? 1 : NF][ALIAS ? 1 : 3][ALIAS ? 1 : TILE_COLS];
    static_assert(!ALIAS || sizeof(float4) * 3 * TILE_COLS + sizeof(float2) * NF * 3 * TILE_COLS <= sizeof(float4) * 2 * 384, "field texels fit a plane-set");
    // ALIAS: the field texels live in the weight-sum plane-set's staging area until every wave has read them
    float4(*sK)[TILE_COLS] = ALIAS ? (float4(*)[TILE_COLS]) & sAcc[1][0][0] : (float4(*)[TILE_COLS]) & sKown[0][0];  // .w = 1 if PSD and finite
    float2(*sF)[3][TILE_COLS] = ALIAS ? (float2(*)[3][TILE_COLS])((char*)&sAcc[1][0][0] + sizeof(float4) * 3 * TILE_COLS)
                                      : (float2(*)[3][TILE_COLS]) & sFown[0][0][0];
    __shared__ float4 sM[NF][3][TILE_COLS];
    __shared__ __attribute__((aligned(16))) float sColA[512];
    __shared__ float sRowB[2];
    const int lx = threadIdx.x, ly = threadIdx.y;
    const int r = ly >> 1, h = ly & 1;
    const int X0 = bIdX * 512 + 8 * lx + 4 * h;
    const int Y = Y0 + r;
    const int fw = kernelParam.width, fh = kernelParam.height;  // == hrW/8, hrH/8 (checked on the host)
    const int mw = dimX / 2, mh = dimY / 2;
    const int band = Y0 >> 3;  // field / certainty row of the tile
    {
        const int t = ly * 64 + lx;
        if (t < 3 * TILE_COLS) {
            const int rr = t / TILE_COLS, c = t - rr * TILE_COLS;
            const int gy = band - 1 + rr, gx = bIdX * 64 - 1 + c;
            const int fy = clampi(gy, 0, fh - 1), fx = clampi(gx, 0, fw - 1);
            float4 k = row_ptr((const float4*)kernelParam.ptr, kernelParam.pitch, fy)[fx];
            k.w = psd_ok(k.x, k.y, k.z) ? 1.0f : 0.0f;
            sK[rr][c] = k;
#pragma unroll
            for (int n = 0; n < NF; n++) {
                sF[n][rr][c] = row_ptr((const float2*)fr.f[n].shifts.ptr, fr.f[n].shifts.pitch, fy)[fx];
                const float4 m = row_ptr(fr.f[n].mask, strideMask, clampi(gy, 0, mh - 1))[clampi(gx, 0, mw - 1)];
                const float mc[3] = {sane(m.x), sane(m.y), sane(m.z)};  // by CFA position, see k_accumulate2xTile
                sM[n][rr][c] = make_float4(mc[Cfa<CFA>::col(0, 0)], mc[Cfa<CFA>::col(0, 1)], mc[Cfa<CFA>::col(1, 0)],
                                          mc[Cfa<CFA>::col(1, 1)]);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; u++) sColA[t + 256 * u] = texel_fraction<8, false>(bIdX * 512 + t + 256 * u, hrW, fw);
        if (t < 2) sRowB[t] = texel_fraction<8, true>(Y0 + t, hrH, fh);
    }
    // accumulator rows of the tile -> LDS (wave (r, h) brings half h of row r), asynchronously
    const size_t segByte = (size_t)bIdX * 6144 + (size_t)h * 3072;
    const AccSegment<WIN> seg{(size_t)hrW * 12, segByte, WIN ? (size_t)wx0 * 12 : 0, WIN ? (size_t)wx1 * 12 : 0, fresh};
    char* gP = WIN ? (char*)imgOut + (size_t)(Y - wy0) * strideOut : (char*)imgOut + (size_t)Y * strideOut + segByte;
    char* gW = WIN ? (char*)totalWeights + (size_t)(Y - wy0) * strideOut : (char*)totalWeights + (size_t)Y * strideOut + segByte;
    seg.stage(gP, &sAcc[0][r][h * 192], lx);
    if (!ALIAS) seg.stage(gW, &sAcc[1][r][h * 192], lx);  // (ALIAS: after the last read of the field texels, below)
    __syncthreads();
    const bool stripLive = X0 >= STRIP_MARGIN && X0 < hrW - STRIP_MARGIN;

    const int fr_ = (Y0 & 7) < 4 ? 0 : 1;
    const float b = sRowB[r];
    const float4 av4 = ((const float4*)sColA)[2 * lx + h];
    const float av[4] = {av4.x, av4.y, av4.z, av4.w};
    const bool geomOk = stripLive && b >= 0.0f && fminf(fminf(av[0], av[1]), fminf(av[2], av[3])) >= 0.0f;
    const int cb = lx + h;  // LDS column of the left texel of this strip's texel pair

    float kxa[4], kya[4], kza[4];
    bool kOk;
    {
        float4 Kt[2][2];
#pragma unroll
        for (int r2 = 0; r2 < 2; r2++)
#pragma unroll
            for (int c = 0; c < 2; c++) Kt[r2][c] = sK[fr_ + r2][cb + c];
        kOk = (Kt[0][0].w * Kt[0][1].w) * (Kt[1][0].w * Kt[1][1].w) > 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float w00 = (1.0f - av[k]) * (1.0f - b), w10 = av[k] * (1.0f - b), w01 = (1.0f - av[k]) * b, w11 = av[k] * b;
            auto mix = [&](float t00, float t10, float t01, float t11) {
                return __builtin_fmaf(w11, t11, __builtin_fmaf(w01, t01, __builtin_fmaf(w10, t10, w00 * t00)));
            };
            kxa[k] = mix(Kt[0][0].x, Kt[0][1].x, Kt[1][0].x, Kt[1][1].x);
            kya[k] = mix(Kt[0][0].y, Kt[0][1].y, Kt[1][0].y, Kt[1][1].y);
            kza[k] = mix(Kt[0][0].z, Kt[0][1].z, Kt[1][0].z, Kt[1][1].z);
        }
    }

    float accP[12], accW[12];
#pragma unroll
    for (int i = 0; i < 12; i++) accP[i] = accW[i] = 0.0f;
    const uint32_t xmax = (uint32_t)(4 * dimX - 5), ymax = (uint32_t)(4 * dimY - 5);
    const int yq = Y & 7;
    uint32_t safeBits = 0;
    if constexpr (NF > 1) {
        // pixel-major, as k_accumulate2xTile: per frame the whole-pixel flow of the strip's pixels and the admission, then
        // per pixel the tap weights once and frame after frame
        uint32_t sxy[NF][ALIAS ? 2 : 4];  // (ALIAS: 8:8 bits per pixel, [0] = the four sx, [1] = the four sy, relative to bsx / bsy)
        int bsx[NF], bsy[NF];             // rounded flow of the tile's centre texel (per-frame scalars), see k_accumulate2xTile
#pragma unroll
        for (int n = 0; n < NF; n++) {
            bsx[n] = bsy[n] = 0;
            if constexpr (ALIAS) {
                sxy[n][0] = sxy[n][1] = 0u;
                const float2 cf = sF[n][1][TILE_COLS / 2];
                bsx[n] = __builtin_amdgcn_readfirstlane(min(max(round2i(cf.x * 4.0f), -32000), 32000));
                bsy[n] = __builtin_amdgcn_readfirstlane(min(max(round2i(cf.y * 4.0f), -32000), 32000));
            }
            int sx[4], sy[4];
            bool safe = strip_flow<4, 8, 15>(geomOk && kOk, &sF[n][fr_][cb], &sF[n][fr_ + 1][cb], av, b, X0, Y, xmax, ymax, sx, sy);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if constexpr (ALIAS) {
                    const int dx = sx[k] - bsx[n], dy = sy[k] - bsy[n];
                    safe = safe && (uint32_t)(dx + 128) < 256u && (uint32_t)(dy + 128) < 256u;
                    sxy[n][0] |= ((uint32_t)dx & 0xffu) << (8 * k);
                    sxy[n][1] |= ((uint32_t)dy & 0xffu) << (8 * k);
                } else {
                    sxy[n][k] = ((uint32_t)sx[k] & 0xffffu) | ((uint32_t)sy[k] << 16);
                }
            }
            if (safe) safeBits |= 1u << n;
        }
        if constexpr (ALIAS) {
            __syncthreads();  // every wave is past its reads of sK / sF
            seg.stage(gW, &sAcc[1][r][h * 192], lx);
        }
        const float* certRow[5];
#pragma unroll
        for (int jt = 0; jt < 5; jt++) certRow[jt] = (const float*)&sM[0][(yq + jt - 2 + 8) >> 3][lx];
        const char* siteRow[NF][2];
#pragma unroll
        for (int n = 0; n < NF; n++)
#pragma unroll
            for (int j = 0; j < 2; j++) siteRow[n][j] = (const char*)(fr.f[n].raw + (size_t)j * dimX);
        auto pixel = [&](auto k8c) {
            constexpr int K8 = decltype(k8c)::value, k = K8 & 3;
            if (safeBits == 0) return;
            float w[13];
            tap_weights13(kxa[k], kya[k], kza[k], w);
#pragma unroll
            for (int n = 0; n < NF; n++) {
                if ((safeBits >> n) & 1u) {
                    auto rawf = [&](int x0, int y0, float (&sv)[2][2]) {
                        const uint32_t boff = (uint32_t)(y0 * dimX + x0) * 2u;  // admitted strips: inside the frame
#pragma unroll
                        for (int j = 0; j < 2; j++) {
                            const char* rb = siteRow[n][j] + (size_t)boff;
                            sv[j][0] = (float)*(const uint16_t*)rb;
                            sv[j][1] = (float)*(const uint16_t*)(rb + 2);
                        }
                    };
                    auto mval = [&](int jt, int cell, int e) { return certRow[jt][n * (3 * TILE_COLS * 4) + cell * 4 + e]; };
                    const int sx = ALIAS ? bsx[n] + (int)(int8_t)(sxy[n][0] >> (8 * k)) : (int)(int16_t)(sxy[n][ALIAS ? 0 : k] & 0xffffu);
                    const int sy = ALIAS ? bsy[n] + (int)(int8_t)(sxy[n][1] >> (8 * k)) : (int)sxy[n][ALIAS ? 0 : k] >> 16;
                    strip_pixel4_w<K8, CFA, true>(X0 + k, Y, sx, sy, w, rawf, mval, lv, accP, accW);
                }
            }
        };
        if (h == 0) {
            pixel(std::integral_constant<int, 0>{});
            pixel(std::integral_constant<int, 1>{});
            pixel(std::integral_constant<int, 2>{});
            pixel(std::integral_constant<int, 3>{});
        } else {
            pixel(std::integral_constant<int, 4>{});
            pixel(std::integral_constant<int, 5>{});
            pixel(std::integral_constant<int, 6>{});
            pixel(std::integral_constant<int, 7>{});
        }
    } else {
        // one frame: frame-major
        int sx[4], sy[4];
        if (strip_flow<4, 8, 20>(geomOk && kOk, &sF[0][fr_][cb], &sF[0][fr_ + 1][cb], av, b, X0, Y, xmax, ymax, sx, sy)) {
            safeBits = 1u;
            const uint16_t* raw = fr.f[0].raw;
            // certainty: LDS row of the mask row that tap row jt reads, column lx + cell
            auto mval = [&](int jt, int cell, int e) {
                const int mr = ((yq + jt - 2 + 8) >> 3);
                const float* p = (const float*)&sM[0][mr][lx + cell];
                return p[e];
            };
            if (h == 0) {
                strip_pixel4<0, CFA, true>(X0 + 0, Y, sx[0], sy[0], kxa[0], kya[0], kza[0], raw, dimX, mval, lv, accP, accW);
                strip_pixel4<1, CFA, true>(X0 + 1, Y, sx[1], sy[1], kxa[1], kya[1], kza[1], raw, dimX, mval, lv, accP, accW);
                strip_pixel4<2, CFA, true>(X0 + 2, Y, sx[2], sy[2], kxa[2], kya[2], kza[2], raw, dimX, mval, lv, accP, accW);
                strip_pixel4<3, CFA, true>(X0 + 3, Y, sx[3], sy[3], kxa[3], kya[3], kza[3], raw, dimX, mval, lv, accP, accW);
            } else {
                strip_pixel4<4, CFA, true>(X0 + 0, Y, sx[0], sy[0], kxa[0], kya[0], kza[0], raw, dimX, mval, lv, accP, accW);
                strip_pixel4<5, CFA, true>(X0 + 1, Y, sx[1], sy[1], kxa[1], kya[1], kza[1], raw, dimX, mval, lv, accP, accW);
                strip_pixel4<6, CFA, true>(X0 + 2, Y, sx[2], sy[2], kxa[2], kya[2], kza[2], raw, dimX, mval, lv, accP, accW);
                strip_pixel4<7, CFA, true>(X0 + 3, Y, sx[3], sy[3], kxa[3], kya[3], kza[3], raw, dimX, mval, lv, accP, accW);
            }
        }
    }
    // every wave's part of the staged rows must have landed before any lane updates them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    float* myP = (float*)&sAcc[0][r][0] + (2 * lx + h) * 12;
    float* myW = (float*)&sAcc[1][r][0] + (2 * lx + h) * 12;
    if (safeBits) {
        lane_add12(myP, accP);
        lane_add12(myW, accW);
    }
    if (safeBits != (1u << NF) - 1u && stripLive) {
#pragma unroll 1
        for (int n = 0; n < NF; n++) {
            if ((safeBits >> n) & 1u) continue;
            TileFrame F = fr.f[0];  // picked with scalar selects: the argument struct stays in SGPRs
#pragma unroll
            for (int m = 1; m < NF; m++)
                if (n == m) F = fr.f[m];
            strip_straight<4>(F, myP, myW, X0, Y, hrW, kernelParam, glv, dimX, dimY, strideMask, cfaPacked);
        }
    }
    __syncthreads();
    // write the half-row segments back in memory order
    seg.store(&sAcc[0][r][h * 192], gP, lx);
    seg.store(&sAcc[1][r][h * 192], gW, lx);
}

constexpr int pack_cfa(int c00, int c01, int c10, int c11) { return c00 | (c01 << 2) | (c10 << 4) | (c11 << 6); }

// the 2-bit form of a packed launch word (colours 0..3: the callers refuse the others first)
constexpr int pack_cfa(int cp) { return pack_cfa(cp & 0xff, (cp >> 8) & 0xff, (cp >> 16) & 0xff, (cp >> 24) & 0xff); }
bool cfa_rgb(int cp)  // every colour of the launch word is red, green or blue
{
    for (int i = 0; i < 4; i++)
        if (((cp >> (8 * i)) & 0xff) > MFSR_BLUE) return false;
    return true;
}

bool strip_xcd_remap()  // MFSR_XCD_REMAP=0: launch order (A/B); see k_accumulate2xTile
{
    static const bool on = !mfsr_env_is0("MFSR_XCD_REMAP");
    return on;
}
bool strip_use_tile()  // MFSR_STRIP_TILE=0: the register-only strip kernel instead of the LDS tile kernel (fields at HR/4)
{
    static const bool on = !mfsr_env_is0("MFSR_STRIP_TILE");
    return on;
}
MfsrKnob g_margin_sites;  // mfsr_set_margin_sites / MFSR_MARGIN_SITES=0: the x2 margin kernels' per-tap body (A/B)
bool margin_sites()
{
    return g_margin_sites.get([] { return mfsr_env_is0("MFSR_MARGIN_SITES") ? 0 : 1; }) == 1;
}

// true when the LDS tile kernel serves this geometry (fields at HR/4, whole tiles)
bool tile_kernel_ok(mfsr_tex2d kp, mfsr_tex2d sh, int dimX, int dimY)
{
    const int hrW = 2 * dimX, hrH = 2 * dimY;
    // (the tile kernels address the raw sites with 32-bit byte offsets: frames below 4 GiB)
    return kp.width == sh.width && kp.height == sh.height && kp.width * 4 == hrW && kp.height * 4 == hrH && kp.width >= 4 &&
           (dimX % 4) == 0 && (dimY % 4) == 0 && (uint64_t)dimX * (uint64_t)dimY * 2u < (1ull << 32) && strip_use_tile();
}

// the same for fields at HR/2 (the monochrome pipeline: tracking at the raw resolution)
bool tile_kernel_ok_fr2(mfsr_tex2d kp, mfsr_tex2d sh, int dimX, int dimY)
{
    const int hrW = 2 * dimX, hrH = 2 * dimY;
    return kp.width == sh.width && kp.height == sh.height && kp.width * 2 == hrW && kp.height * 2 == hrH && kp.width >= 4 &&
           (dimX % 4) == 0 && (dimY % 4) == 0 && (uint64_t)dimX * (uint64_t)dimY * 2u < (1ull << 32) && strip_use_tile();
}

// the tile launch of a window: its first tile column (x0 / tileW) and how many it covers (whole frame: 0, all)
struct WinLaunch {
    bool on;              // window-relative accumulators (the WIN instantiations)
    int tileX0, tilesX;   // tile columns of tileW HR pixels
    int x0, x1, y0;
};
WinLaunch win_launch(const HrWindow& w, int hrW, int tileW)
{
    WinLaunch l;
    l.on = w.rel && !(w.x0 == 0 && w.x1 == hrW && w.y0 == 0);
    l.tileX0 = l.on ? w.x0 / tileW : 0;
    l.tilesX = (l.on ? mfsr_cdiv(w.x1, tileW) : mfsr_cdiv(hrW, tileW)) - l.tileX0;
    l.x0 = l.on ? w.x0 : 0;
    l.x1 = l.on ? w.x1 : hrW;
    l.y0 = l.on ? w.y0 : 0;
    return l;
}

template <int CFA, int NF, int FR = 4>
void launch_tile(dim3 grid, dim3 block, hipStream_t st, const TileFrames<NF>& fr, pix3* imgOut, pix3* tw, mfsr_tex2d kp,
                 Levels3 glv, StripLevels lv, int dimX, int dimY, int strideOut, int strideMask, int cfaPacked, int fresh, int tileY0,
                 const WinLaunch& wl)
{
    const int tilesX = (int)grid.x, tilesY = (int)grid.y;
    // (a window: the XCD-aware order is taken over the window's tiles; the order does not change any pixel's bits)
    const int tilesPerXcd = strip_xcd_remap() ? mfsr_cdiv(tilesX * tilesY, 8) : 0;
    const dim3 g1(tilesPerXcd ? 8 * tilesPerXcd : tilesX * tilesY);
    if (wl.on)
        hipLaunchKernelGGL((k_accumulate2xTile<CFA, NF, FR, true>), g1, block, 0, st, fr, imgOut, tw, kp, glv, lv, dimX, dimY,
                           strideOut, strideMask, cfaPacked, tilesX, tilesY, tilesPerXcd, fresh, tileY0, wl.tileX0, wl.x0, wl.x1, wl.y0);
    else
        hipLaunchKernelGGL((k_accumulate2xTile<CFA, NF, FR>), g1, block, 0, st, fr, imgOut, tw, kp, glv, lv, dimX, dimY,
                           strideOut, strideMask, cfaPacked, tilesX, tilesY, tilesPerXcd, fresh, tileY0, 0, 0, 0, 0);
}

template <int CFA, int FR, int NF>
void launch_strip_regs_fr(dim3 grid, dim3 block, hipStream_t st, const TileFrames<NF>& fr, pix3* imgOut, pix3* tw, mfsr_tex2d kp,
                          Levels3 glv, StripLevels lv, int dimX, int dimY, int strideOut, int strideMask, int cfaPacked, int rowBlock0,
                          const WinLaunch& wl)
{
    if (wl.on)
        hipLaunchKernelGGL((k_accumulate2xStrip<CFA, FR, NF, true>), grid, block, 0, st, fr, imgOut, tw, kp, glv, lv, dimX, dimY,
                           strideOut, strideMask, cfaPacked, rowBlock0, wl.tileX0, wl.x0, wl.x1, wl.y0);
    else
        hipLaunchKernelGGL((k_accumulate2xStrip<CFA, FR, NF>), grid, block, 0, st, fr, imgOut, tw, kp, glv, lv, dimX, dimY,
                           strideOut, strideMask, cfaPacked, rowBlock0, 0, 0, 0, 0);
}

template <int CFA, int NF>
void launch_strip_regs(dim3 grid, dim3 block, hipStream_t st, const TileFrames<NF>& fr, pix3* imgOut, pix3* tw, mfsr_tex2d kp,
                       Levels3 glv, StripLevels lv, int dimX, int dimY, int strideOut, int strideMask, int cfaPacked, int rowBlock0,
                       const WinLaunch& wl)
{
    const int hrW = 2 * dimX, hrH = 2 * dimY;
    bool same = true;
    for (int n = 0; n < NF; n++) same = same && kp.width == fr.f[n].shifts.width && kp.height == fr.f[n].shifts.height;
    if (same && kp.width * 4 == hrW && kp.height * 4 == hrH && kp.width >= 4)
        launch_strip_regs_fr<CFA, 4, NF>(grid, block, st, fr, imgOut, tw, kp, glv, lv, dimX, dimY, strideOut, strideMask, cfaPacked,
                                         rowBlock0, wl);
    else if (same && kp.width * 2 == hrW && kp.height * 2 == hrH && kp.width >= 4)
        launch_strip_regs_fr<CFA, 2, NF>(grid, block, st, fr, imgOut, tw, kp, glv, lv, dimX, dimY, strideOut, strideMask, cfaPacked,
                                         rowBlock0, wl);
    else
        launch_strip_regs_fr<CFA, 0, NF>(grid, block, st, fr, imgOut, tw, kp, glv, lv, dimX, dimY, strideOut, strideMask, cfaPacked,
                                         rowBlock0, wl);
}

// zero HR rows [r0, r1) x the launch's columns of the accumulators (one memset over whole rows when the pitch is the row's
// size; a 2-D one otherwise, so that the bytes beyond a row -- or beyond a window's row -- are not touched)
int zero_rows(mfsr_float3* imgOut, mfsr_float3* totalWeights, int strideOut, int r0, int r1, const WinLaunch& wl, hipStream_t st)
{
    const size_t rowB = (size_t)(wl.x1 - wl.x0) * 12, rows = (size_t)(r1 - r0);
    for (int p2 = 0; p2 < 2; p2++) {
        char* base = (p2 ? (char*)totalWeights : (char*)imgOut) + (size_t)(r0 - wl.y0) * strideOut;
        const hipError_t e = rowB == (size_t)strideOut ? hipMemsetAsync(base, 0, rows * strideOut, st)
                                                       : hipMemset2DAsync(base, strideOut, 0, rowB, rows, st);
        if (e != hipSuccess) return -1;
    }
    return 0;
}

// fresh accumulators: the tile kernels write every row of their window outside the top and bottom margin bands
// (rows [0, M) and [hrH - M, hrH)); zero the part of those bands that lies inside the window
int zero_margin_bands(mfsr_float3* imgOut, mfsr_float3* totalWeights, int hrH, int strideOut, int rowBegin, int rowEnd,
                      const WinLaunch& wl, hipStream_t st)
{
    const int bands[2][2] = {{0, STRIP_MARGIN}, {hrH - STRIP_MARGIN, hrH}};
    for (int i = 0; i < 2; i++) {
        const int r0 = bands[i][0] > rowBegin ? bands[i][0] : rowBegin, r1 = bands[i][1] < rowEnd ? bands[i][1] : rowEnd;
        if (r1 <= r0) continue;
        if (zero_rows(imgOut, totalWeights, strideOut, r0, r1, wl, st) != 0) return -1;
    }
    return 0;
}

// number of margin pixels of a frame: the ring of STRIP_MARGIN HR pixels less the outermost one (the kernels' index space)
long long margin_pixel_count(int hrW, int hrH)
{
    const int M = STRIP_MARGIN;
    return 2LL * (M - 1) * (hrW - 2) + (long long)(hrH - 2 * M) * 2 * (M - 1);
}

// The margin kernels (one thread per pixel of the 16-pixel frame margin, the straight per-pixel arithmetic) are small (5.6 K
// waves per 4K frame).  Counters on the per-tap body's 16-frame launch (profiles/r08_pmc_margin.txt): it issues VALU
// instructions in as many wave-cycles as it waits (SQ_ACTIVE_INST_VALU 124 M, SQ_WAIT_INST_ANY 136 M) -- instruction-bound
// as much as latency-bound; the site-wise body issues a third fewer instructions and waits a third as long.  They touch
// accumulator bytes the tile kernel does not (it does not write the side-margin chunks back) and are launched on the
// caller's stream after it.  (Measured and not kept: a side stream, forked before the tile launch and joined after the last
// margin launch -- 8.79 against 8.88 ms per burst, no gain, profiles/r02_ab_margin_overlap.txt.)
// The site-wise body (k_accumulateMargin*<.., SITES = true>) serves x2 with the switch on; it addresses a frame's raw and
// certainty planes with 32-bit offsets, so planes of 2 GiB and more keep the per-tap body.  (x4 keeps the per-tap body: its
// instances of the site-wise body have not been measured.)
template <int SCALE>
bool margin_sites_ok(int dimX, int dimY, int strideMask)
{
    return SCALE == 2 && margin_sites() && (long long)dimX * dimY * 2 < (1LL << 31) &&
           (long long)strideMask * ((dimY + 1) / 2) < (1LL << 31);
}

template <int SCALE>
void launch_margin_1(hipStream_t st, const uint16_t* raw, const mfsr_float4* mask, mfsr_tex2d shifts, pix3* pI, pix3* pT, mfsr_tex2d kp,
                     Levels3 glv, int dimX, int dimY, int strideOut, int strideMask, int cp, int rowBegin, int rowEnd,
                     const WinLaunch& wl, const MarginRects& mr)
{
    auto launch = [&](auto sites) {
        constexpr bool SITES = decltype(sites)::value;
        if (!wl.on)
            hipLaunchKernelGGL((k_accumulateMargin<SCALE, false, SITES>), dim3(mfsr_cdiv(margin_pixel_count(SCALE * dimX, SCALE * dimY), 256)),
                               dim3(256), 0, st, raw, pI, pT, (const float4*)mask, kp, shifts, glv, dimX, dimY, strideOut, strideMask, cp,
                               rowBegin, rowEnd, mr);
        else if (mr.start[4] > 0)
            hipLaunchKernelGGL((k_accumulateMargin<SCALE, true, SITES>), dim3(mfsr_cdiv(mr.start[4], 256)), dim3(256), 0, st, raw, pI, pT,
                               (const float4*)mask, kp, shifts, glv, dimX, dimY, strideOut, strideMask, cp, rowBegin, rowEnd, mr);
    };
    if constexpr (SCALE == 2) {
        if (margin_sites_ok<SCALE>(dimX, dimY, strideMask)) return launch(std::true_type{});
    }
    launch(std::false_type{});
}

// the margin pixels of NF frames in one launch: the whole ring, or the part of it inside a window
template <int NF, int SCALE>
void launch_margin_n(hipStream_t st, const TileFrames<NF>& fr, pix3* pI, pix3* pT, mfsr_tex2d kp, Levels3 glv, int dimX, int dimY,
                     int strideOut, int strideMask, int cp, int rowBegin, int rowEnd, const WinLaunch& wl, const MarginRects& mr)
{
    auto launch = [&](auto sites) {
        constexpr bool SITES = decltype(sites)::value;
        if (!wl.on)
            hipLaunchKernelGGL((k_accumulateMarginN<NF, SCALE, false, SITES>), dim3(mfsr_cdiv(margin_pixel_count(SCALE * dimX, SCALE * dimY), 64)),
                               dim3(64, NF), 0, st, fr, pI, pT, kp, glv, dimX, dimY, strideOut, strideMask, cp, rowBegin, rowEnd, mr);
        else if (mr.start[4] > 0)
            hipLaunchKernelGGL((k_accumulateMarginN<NF, SCALE, true, SITES>), dim3(mfsr_cdiv(mr.start[4], 64)), dim3(64, NF), 0, st, fr, pI,
                               pT, kp, glv, dimX, dimY, strideOut, strideMask, cp, rowBegin, rowEnd, mr);
    };
    if constexpr (SCALE == 2) {
        if (margin_sites_ok<SCALE>(dimX, dimY, strideMask)) return launch(std::true_type{});
    }
    launch(std::false_type{});
}

// black / white levels in the two forms the kernels take
void make_levels(mfsr_float3 white, mfsr_float3 black, Levels3& glv, StripLevels& lv)
{
    const float wl[3] = {white.x, white.y, white.z}, bl[3] = {black.x, black.y, black.z};
    for (int c = 0; c < 3; c++) {
        glv.white[c] = wl[c];
        glv.black[c] = bl[c];
        lv.black[c] = bl[c];
        lv.invWhite[c] = 1.0f / wl[c];
    }
}

// per-frame kernel arguments of the first n frames of a call
void fill_frames(TileFrame* fr, const uint16_t* const* dataIn, const mfsr_float4* const* certaintyMask, const mfsr_tex2d* shifts, int n)
{
    for (int i = 0; i < n; i++) {
        fr[i].raw = dataIn[i];
        fr[i].mask = (const float4*)certaintyMask[i];
        fr[i].shifts = shifts[i];
    }
}

template <int N>
using int_c = std::integral_constant<int, N>;

// f(int_c<CFA>{}) for the packed CFA pattern of the call: the four Bayer patterns and, with MONO, monochrome (a compile-time
// switch: f is not instantiated for a pattern it does not serve).  Any other pattern: 0, "not the fast kernels'".
template <bool MONO, class F>
int for_cfa(int packed, F f)
{
    constexpr int R = MFSR_RED, G = MFSR_GREEN, B = MFSR_BLUE;
    switch (packed) {
        case pack_cfa(R, G, G, B): return f(int_c<pack_cfa(R, G, G, B)>{});  // RGGB
        case pack_cfa(B, G, G, R): return f(int_c<pack_cfa(B, G, G, R)>{});  // BGGR
        case pack_cfa(G, R, B, G): return f(int_c<pack_cfa(G, R, B, G)>{});  // GRBG
        case pack_cfa(G, B, R, G): return f(int_c<pack_cfa(G, B, R, G)>{});  // GBRG
        case pack_cfa(G, G, G, G):
            if constexpr (MONO) return f(int_c<pack_cfa(G, G, G, G)>{});
            return 0;
        default: return 0;
    }
}

}  // namespace

// Returns 1 if the fast kernels were launched for all `nFrames` (1 to 4) frames, 0 if the
// configuration is not one they handle (caller falls back to the straight kernel, or splits a group of
// three or four), -1 if a memset of the fresh-accumulator mode failed.
// With two to four frames the LDS tile kernel fuses all of them in one pass over the accumulators; the other
// geometries take at most two, frame after frame.
int mfsr_try_launch_accumulate2x_strip(int cp, int nFrames, const uint16_t* const* dataIn, mfsr_float3* imgOut,
                                       mfsr_float3* totalWeights, const mfsr_float4* const* certaintyMask,
                                       mfsr_tex2d kernelParam, const mfsr_tex2d* shifts, mfsr_float3 whiteLevel,
                                       mfsr_float3 blackLevel, int dimX, int dimY, int strideOut, int strideMask,
                                       int fresh, int rowBegin, int rowEnd, int colBegin, int colEnd, int relative,
                                       mfsr_stream_t stream)
{
    if (nFrames < 1 || nFrames > 4) return 0;
    if (!cfa_rgb(cp)) return 0;
    const int packed2 = pack_cfa(cp);
    // layout requirements of the vectorised accumulator access
    if ((dimX & 1) || ((uintptr_t)imgOut & 15) || ((uintptr_t)totalWeights & 15) || (strideOut & 15)) return 0;
    if (dimX < 2 * STRIP_MARGIN || dimY < 2 * STRIP_MARGIN) return 0;
    Levels3 glv;
    StripLevels lv;
    make_levels(whiteLevel, blackLevel, glv, lv);
    const int hrW = 2 * dimX, hrH = 2 * dimY;
    // HR row window [rowBegin, rowEnd): whole 4-row tile rows (the caller aligns it to 16 rows or the frame's end); columns
    // [colBegin, colEnd): the 256-pixel tile columns that meet them
    const int rowBlock0 = rowBegin / 4, rowBlocks = mfsr_cdiv(rowEnd, 4) - rowBlock0;
    const WinLaunch wlc = win_launch(HrWindow{colBegin, rowBegin, colEnd, rowEnd, relative}, hrW, 256);
    dim3 block(64, 4), grid(wlc.tilesX, rowBlocks);
    const MarginRects mr = margin_rects(hrW, hrH, STRIP_MARGIN, HrWindow{colBegin, rowBegin, colEnd, rowEnd, relative});
    hipStream_t st = mfsr_s(stream);
    pix3* pI = (pix3*)imgOut;
    pix3* pT = (pix3*)totalWeights;
    // two to four frames in one pass over the accumulators: the LDS tile kernel's geometry only
    bool pair = nFrames >= 2;
    for (int n = 0; n < nFrames; n++) pair = pair && tile_kernel_ok(kernelParam, shifts[n], dimX, dimY);
    // the monochrome pipeline (fields at the raw resolution = HR/2): its own instantiation of the tile kernel, one or two frames
    constexpr int kMono = pack_cfa(MFSR_GREEN, MFSR_GREEN, MFSR_GREEN, MFSR_GREEN);
    bool mono2 = packed2 == kMono && nFrames <= 2;
    for (int n = 0; n < nFrames; n++) mono2 = mono2 && tile_kernel_ok_fr2(kernelParam, shifts[n], dimX, dimY);
    if (nFrames > 2 && !pair) return 0;  // the caller splits the group
    // fresh accumulators ("as if zeroed", never read): the tile kernels write every row outside the top
    // and bottom margin bands themselves, the bands are zeroed here; the other kernels get a full memset
    const bool tileFirst = pair || mono2 || (nFrames == 1 && tile_kernel_ok(kernelParam, shifts[0], dimX, dimY));
    int tileFresh = 0;
    if (fresh) {
        if (tileFirst) {
            tileFresh = 1;
            if (zero_margin_bands(imgOut, totalWeights, hrH, strideOut, rowBegin, rowEnd, wlc, st) != 0) return -1;
        } else {
            if (zero_rows(imgOut, totalWeights, strideOut, rowBegin, rowEnd, wlc, st) != 0) return -1;
        }
    }
    auto launch_margin = [&](int n) {
        launch_margin_1<2>(st, dataIn[n], certaintyMask[n], shifts[n], pI, pT, kernelParam, glv, dimX, dimY, strideOut, strideMask, cp,
                           rowBegin, rowEnd, wlc, mr);
    };
    // NF frames at field resolution FR: the tile kernel, then their margin pixels in one launch (one frame: the single-frame
    // margin kernel)
    auto launch_group = [&](auto cfaTag, auto nfTag, auto frTag) {
        constexpr int CFA = decltype(cfaTag)::value, NF = decltype(nfTag)::value, FR = decltype(frTag)::value;
        TileFrames<NF> fr;
        fill_frames(fr.f, dataIn, certaintyMask, shifts, NF);
        launch_tile<CFA, NF, FR>(grid, block, st, fr, pI, pT, kernelParam, glv, lv, dimX, dimY, strideOut, strideMask, cp, tileFresh,
                                 rowBlock0, wlc);
        if (NF == 1)
            launch_margin(0);
        else
            launch_margin_n<NF, 2>(st, fr, pI, pT, kernelParam, glv, dimX, dimY, strideOut, strideMask, cp, rowBegin, rowEnd, wlc, mr);
    };
    if (mono2) {
        if (nFrames == 1) launch_group(int_c<kMono>{}, int_c<1>{}, int_c<2>{});
        if (nFrames == 2) launch_group(int_c<kMono>{}, int_c<2>{}, int_c<2>{});
        return 1;
    }
    return for_cfa<true>(packed2, [&](auto cfaTag) {
        constexpr int CFA = decltype(cfaTag)::value;
        if (pair) {
            if (nFrames == 2) launch_group(cfaTag, int_c<2>{}, int_c<4>{});
            if (nFrames == 3) launch_group(cfaTag, int_c<3>{}, int_c<4>{});
            if (nFrames == 4) launch_group(cfaTag, int_c<4>{}, int_c<4>{});
        } else if (nFrames == 2) {
            TileFrames<2> fr;
            fill_frames(fr.f, dataIn, certaintyMask, shifts, 2);
            launch_strip_regs<CFA, 2>(grid, block, st, fr, pI, pT, kernelParam, glv, lv, dimX, dimY, strideOut, strideMask, cp, rowBlock0,
                                      wlc);
            launch_margin(0);
            launch_margin(1);
        } else if (tile_kernel_ok(kernelParam, shifts[0], dimX, dimY)) {
            launch_group(cfaTag, int_c<1>{}, int_c<4>{});
        } else {
            TileFrames<1> fr;
            fill_frames(fr.f, dataIn, certaintyMask, shifts, 1);
            launch_strip_regs<CFA, 1>(grid, block, st, fr, pI, pT, kernelParam, glv, lv, dimX, dimY, strideOut, strideMask, cp, rowBlock0,
                                      wlc);
            launch_margin(0);
        }
        return 1;
    });
}

// The burst form: nFrames = 8, 12 or 16 frames (whole groups of four, Bayer, fields at HR/4, the whole frame) in ONE tile
// launch (k_accumulate2xTileBurst) and ONE margin launch; bit for bit what nFrames / 4 calls of the function above give.
// Returns 1 if launched, 0 if the configuration is not the burst kernel's (nothing was touched), -1 if a memset of the
// fresh-accumulator mode failed.
int mfsr_try_launch_accumulate2x_burst(int cp, int nFrames, const uint16_t* const* dataIn, mfsr_float3* imgOut,
                                       mfsr_float3* totalWeights, const mfsr_float4* const* certaintyMask,
                                       mfsr_tex2d kernelParam, const mfsr_tex2d* shifts, mfsr_float3 whiteLevel,
                                       mfsr_float3 blackLevel, int dimX, int dimY, int strideOut, int strideMask, int fresh,
                                       const mfsr_float3* fallback, int fbPitch, int fbW, int fbH, float u0, float u1, float v0,
                                       float v1, float threshold, uint16_t* out16, mfsr_stream_t stream)
{
    if (nFrames < 8 || nFrames > 4 * TILE_BURST_GROUPS || (nFrames & 3)) return 0;
    const int packed2 = pack_cfa(cp);
    if ((dimX & 1) || ((uintptr_t)imgOut & 15) || ((uintptr_t)totalWeights & 15) || (strideOut & 15)) return 0;
    if (dimX < 2 * STRIP_MARGIN || dimY < 2 * STRIP_MARGIN) return 0;
    for (int n = 0; n < nFrames; n++)
        if (!tile_kernel_ok(kernelParam, shifts[n], dimX, dimY)) return 0;
    Levels3 glv;
    StripLevels lv;
    make_levels(whiteLevel, blackLevel, glv, lv);
    const int hrW = 2 * dimX, hrH = 2 * dimY;
    const WinLaunch wlc = win_launch(HrWindow{0, 0, hrW, hrH, 0}, hrW, 256);
    const int tilesX = wlc.tilesX, tilesY = mfsr_cdiv(hrH, 4);
    const int tilesPerXcd = strip_xcd_remap() ? mfsr_cdiv(tilesX * tilesY, 8) : 0;
    const dim3 block(64, 4), g1(tilesPerXcd ? 8 * tilesPerXcd : tilesX * tilesY);
    hipStream_t st = mfsr_s(stream);
    pix3* pI = (pix3*)imgOut;
    pix3* pT = (pix3*)totalWeights;
    BurstFrames fr;
    fill_frames(fr.f, dataIn, certaintyMask, shifts, nFrames);
    for (int n = nFrames; n < 4 * TILE_BURST_GROUPS; n++) fr.f[n] = fr.f[0];  // (never read: nGroups bounds the loop)
    // the finishing form (out16): the whole frame's plain finish, the launch's pixel (0, 0) is the image's
    const FinishSrc src = finish_src(fallback, fbPitch, fbW, fbH, u0, u1, v0, v1, threshold, 0, 0, hrW, hrH);
    // monochrome and other patterns are not the burst kernel's: 0
    const int rc = for_cfa<false>(packed2, [&](auto cfaTag) {
        constexpr int CFA = decltype(cfaTag)::value;
        // fresh accumulators: the tile kernel writes every row outside the top and bottom margin bands, which are zeroed here
        if (fresh && zero_margin_bands(imgOut, totalWeights, hrH, strideOut, 0, hrH, wlc, st) != 0) return -1;
        if (out16)
            hipLaunchKernelGGL((k_accumulate2xTileBurst<CFA, true>), g1, block, 0, st, fr, nFrames / 4, pI, pT, kernelParam, glv, lv, dimX,
                               dimY, strideOut, strideMask, cp, tilesX, tilesY, tilesPerXcd, fresh ? 1 : 0, TileFinish<true>{src, out16});
        else
            hipLaunchKernelGGL((k_accumulate2xTileBurst<CFA>), g1, block, 0, st, fr, nFrames / 4, pI, pT, kernelParam, glv, lv, dimX, dimY,
                               strideOut, strideMask, cp, tilesX, tilesY, tilesPerXcd, fresh ? 1 : 0, TileFinish<false>{});
        return 1;
    });
    if (rc != 1) return rc;
    // the margin pixels of all frames in one launch, the frames' sums (each from zero) added to the accumulator value one after
    // another in call order -- the order of the launches it replaces
    if (margin_sites_ok<2>(dimX, dimY, strideMask))
        hipLaunchKernelGGL((k_accumulateMarginBurst<2, true>), dim3(mfsr_cdiv(margin_pixel_count(hrW, hrH), 64)), dim3(64, 4), 0, st, fr,
                           nFrames / 4, pI, pT, kernelParam, glv, dimX, dimY, strideOut, strideMask, cp);
    else
        hipLaunchKernelGGL((k_accumulateMarginBurst<2, false>), dim3(mfsr_cdiv(margin_pixel_count(hrW, hrH), 64)), dim3(64, 4), 0, st, fr,
                           nFrames / 4, pI, pT, kernelParam, glv, dimX, dimY, strideOut, strideMask, cp);
    // the ring's finish, from the accumulators the margin launch has just completed
    if (out16)
        hipLaunchKernelGGL(k_finishRing, dim3((unsigned)mfsr_cdiv(finish_ring_count(hrW, hrH, STRIP_MARGIN), 256)), dim3(256), 0, st, pI, pT,
                           strideOut, src, out16, hrW, hrH);
    return 1;
}

extern "C" int mfsr_set_margin_sites(int enable)
{
    g_margin_sites.set(enable ? 1 : 0);
    return MFSR_OK;
}

// x4: returns 1 if the x4 tile kernel took the nFrames (1 to 4) frames, 0 if the geometry is not its
// (fields at HR/8, even dimensions); the caller then uses the straight kernel.
int mfsr_try_launch_accumulate4x_tile(int cp, int nFrames, const uint16_t* const* dataIn, mfsr_float3* imgOut,
                                      mfsr_float3* totalWeights, const mfsr_float4* const* certaintyMask,
                                      mfsr_tex2d kernelParam, const mfsr_tex2d* shifts, mfsr_float3 whiteLevel,
                                      mfsr_float3 blackLevel, int dimX, int dimY, int strideOut, int strideMask,
                                      int fresh, int rowBegin, int rowEnd, int colBegin, int colEnd, int relative,
                                      mfsr_stream_t stream)
{
    if (nFrames < 1 || nFrames > 4 || !strip_use_tile()) return 0;
    if (!cfa_rgb(cp)) return 0;
    const int packed2 = pack_cfa(cp);
    const int hrW = 4 * dimX, hrH = 4 * dimY;
    if ((dimX & 1) || (dimY & 1) || ((uintptr_t)imgOut & 15) || ((uintptr_t)totalWeights & 15) || (strideOut & 15)) return 0;
    if (hrW < 4 * STRIP_MARGIN || hrH < 4 * STRIP_MARGIN) return 0;
    for (int n = 0; n < nFrames; n++)
        if (!(kernelParam.width == shifts[n].width && kernelParam.height == shifts[n].height && kernelParam.width * 8 == hrW &&
              kernelParam.height * 8 == hrH && kernelParam.width >= 4))
            return 0;
    Levels3 glv;
    StripLevels lv;
    make_levels(whiteLevel, blackLevel, glv, lv);
    hipStream_t st = mfsr_s(stream);
    pix3* pI = (pix3*)imgOut;
    pix3* pT = (pix3*)totalWeights;
    // HR row window [rowBegin, rowEnd): whole 2-row tile rows; columns [colBegin, colEnd): the 512-pixel tile columns that meet them
    const int tileY0 = rowBegin / 2;
    const WinLaunch wlc = win_launch(HrWindow{colBegin, rowBegin, colEnd, rowEnd, relative}, hrW, 512);
    const MarginRects mr = margin_rects(hrW, hrH, STRIP_MARGIN, HrWindow{colBegin, rowBegin, colEnd, rowEnd, relative});
    const int tilesX = wlc.tilesX, tilesY = mfsr_cdiv(rowEnd, 2) - tileY0;
    const dim3 block(64, 4), grid(tilesX * tilesY);
    if (fresh) {  // the top and bottom margin bands are the only rows the tile kernel does not write
        if (zero_margin_bands(imgOut, totalWeights, hrH, strideOut, rowBegin, rowEnd, wlc, st) != 0) return -1;
    }
    // NF frames: the tile kernel, then their margin pixels in one launch (one frame: the single-frame margin kernel)
    auto launch_group = [&](auto cfaTag, auto nfTag) {
        constexpr int CFA = decltype(cfaTag)::value, NF = decltype(nfTag)::value;
        TileFrames<NF> fr;
        fill_frames(fr.f, dataIn, certaintyMask, shifts, NF);
        if (wlc.on)
            hipLaunchKernelGGL((k_accumulate4xTile<CFA, NF, true>), grid, block, 0, st, fr, pI, pT, kernelParam, glv, lv, dimX, dimY,
                               strideOut, strideMask, cp, tilesX, fresh ? 1 : 0, tileY0, wlc.tileX0, wlc.x0, wlc.x1, wlc.y0);
        else
            hipLaunchKernelGGL((k_accumulate4xTile<CFA, NF>), grid, block, 0, st, fr, pI, pT, kernelParam, glv, lv, dimX, dimY, strideOut,
                               strideMask, cp, tilesX, fresh ? 1 : 0, tileY0, 0, 0, 0, 0);
        if (NF == 1)
            launch_margin_1<4>(st, dataIn[0], certaintyMask[0], shifts[0], pI, pT, kernelParam, glv, dimX, dimY, strideOut, strideMask, cp,
                               rowBegin, rowEnd, wlc, mr);
        else
            launch_margin_n<NF, 4>(st, fr, pI, pT, kernelParam, glv, dimX, dimY, strideOut, strideMask, cp, rowBegin, rowEnd, wlc, mr);
    };
    return for_cfa<true>(packed2, [&](auto cfaTag) {
        if (nFrames == 1) launch_group(cfaTag, int_c<1>{});
        if (nFrames == 2) launch_group(cfaTag, int_c<2>{});
        if (nFrames == 3) launch_group(cfaTag, int_c<3>{});
        if (nFrames == 4) launch_group(cfaTag, int_c<4>{});
        return 1;
    });
}
