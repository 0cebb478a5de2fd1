// margin_sites.hpp -- the integer mapping of the site-wise straight body (accumulate_pixel_sites, accumulate_common.hpp):
// which raw site and which certainty cell each of the five taps of an axis reads.  Plain integer code for host and device, so
// that the kernels and the host check (tests/test_margin_sites_cpu.py) use one definition.
//
// Along one axis the straight arithmetic reads, for tap it = 0..4 (px = it - 2) of output pixel x with flow sx at scale S,
//     raw coordinate   clamp(floor((x + px + sx) / S), 0, dim - 1)
//     certainty cell   clamp(floor((x + px) / S), 0, dim - 1) / 2
// Five consecutive HR positions fall on (S + 3) / S + 1 consecutive raw sites (3 at x2, 2 at x4) and on at most two certainty
// cells (a cell is 2 S >= 4 HR pixels wide).  With u = x + sx - 2 = S * base + phase (0 <= phase < S) tap `it` reads site
// (phase + it) / S = it / S + carry, where carry = (phase + it % S >= S) depends on the lane only when it % S != 0.  The clamp
// is monotone, so clamping the site's coordinate equals clamping each tap's.
#pragma once

#if defined(__HIPCC__)
#define MFSR_SITES_HD __host__ __device__ __forceinline__
#else
#define MFSR_SITES_HD inline
#endif

// floor(a / S), S > 0, any a (accumulate_common.hpp: floordiv_pos)
template <int S>
MFSR_SITES_HD int margin_floordiv(int a)
{
    const int q = a / S;
    return (a % S < 0) ? q - 1 : q;
}

MFSR_SITES_HD int margin_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// raw sites the five taps of an axis fall on
template <int S>
struct MarginSites {
    static constexpr int count = (S + 3) / S + 1;
};

// one axis of a pixel: first (unclamped) raw site of tap 0 and tap 0's position in it; u0 = x + sx - 2
template <int S>
MFSR_SITES_HD void margin_axis(int u0, int& base, int& phase)
{
    base = margin_floordiv<S>(u0);
    phase = u0 - base * S;
}

// tap -> site: margin_tap_site_lo (compile time) + margin_tap_carry (0 for every lane when it % S == 0)
template <int S>
MFSR_SITES_HD constexpr int margin_tap_site_lo(int it)
{
    return it / S;
}
template <int S>
MFSR_SITES_HD constexpr bool margin_tap_carry_varies(int it)
{
    return it % S != 0;
}
template <int S>
MFSR_SITES_HD int margin_tap_carry(int phase, int it)
{
    return (phase + it % S >= S) ? 1 : 0;
}
template <int S>
MFSR_SITES_HD int margin_tap_site(int phase, int it)
{
    return margin_tap_site_lo<S>(it) + margin_tap_carry<S>(phase, it);
}

// site -> clamped raw column or row
MFSR_SITES_HD int margin_site_coord(int base, int site, int dim) { return margin_clamp(base + site, 0, dim - 1); }

// site -> CFA position (the index of cfa_at: bits ((row & 1) * 2 + (col & 1)) * 8 of the packed pattern) of a clamped site
MFSR_SITES_HD int margin_site_cfa_pos(int row, int col) { return ((row & 1) << 1) | (col & 1); }

// certainty cells of one axis: the two (clamped) cells the taps can read and tap 0's position in the first; x0 = x - 2.
// clamp(floor(a / S), 0, dim - 1) / 2 == clamp(floor(a / 2S), 0, (dim - 1) / 2): the halving is monotone, too.
template <int S>
MFSR_SITES_HD void margin_cert_axis(int x0, int dim, int (&cell)[2], int& phase)
{
    const int c = margin_floordiv<2 * S>(x0);
    phase = x0 - c * 2 * S;
    cell[0] = margin_clamp(c, 0, (dim - 1) / 2);
    cell[1] = margin_clamp(c + 1, 0, (dim - 1) / 2);
}

// tap -> certainty cell (0 or 1 of margin_cert_axis); tap 0 always reads cell 0, a tap with it >= 2 S always cell 1
template <int S>
MFSR_SITES_HD int margin_tap_cell(int phase, int it)
{
    return (phase + it >= 2 * S) ? 1 : 0;
}
template <int S>
MFSR_SITES_HD constexpr bool margin_tap_cell_varies(int it)
{
    return it != 0 && it < 2 * S;
}
