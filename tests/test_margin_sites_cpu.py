"""The integer mapping of the site-wise margin body (csrc/margin_sites.hpp) against the per-tap expressions of
accumulate_pixel_core (accumulate_common.hpp), exhaustively, in a stand-alone host program built with AddressSanitizer and
UBSan: scale 2 and 4, raw dimensions 32 and 34, every HR position of the frame, flows of -70 .. 70 HR pixels (sites far beyond
both borders), all five taps of an axis.  The mapping is separable, so one axis is checked (columns and rows use the same
functions); the CFA position is checked on every (row, column) of the frame."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi_frame_super_resolution_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "margin_sites.hpp"

// accumulate_common.hpp: floordiv_pos, clampi; common.hpp: cfa_at's index
static int floordiv_pos(int a, int s) { int q = a / s; return (a % s < 0) ? q - 1 : q; }
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int cfa_index(int y, int x) { return ((y & 1) << 1) | (x & 1); }

static long long checked = 0;
static int failures = 0;
static void fail(const char* what, int S, int dim, int x, int sx, int it, int got, int want)
{
    if (failures++ < 20) std::printf("%s: scale %d dim %d x %d sx %d tap %d: %d, per tap %d\n", what, S, dim, x, sx, it, got, want);
}

template <int S>
static void axis(int dim)
{
    constexpr int NS = MarginSites<S>::count;
    for (int x = 0; x < S * dim; x++) {
        int cell[2], q;
        margin_cert_axis<S>(x - 2, dim, cell, q);
        if (q < 0 || q >= 2 * S) fail("certainty phase", S, dim, x, 0, 0, q, 0);
        for (int it = 0; it < 5; it++) {
            const int px = it - 2;
            const int want = clampi(floordiv_pos(x + px, S), 0, dim - 1) / 2;  // maskRow[ppxA / 2], row ppy / 2
            const int c = margin_tap_cell<S>(q, it);
            if (c != 0 && c != 1) fail("certainty cell index", S, dim, x, 0, it, c, 0);
            if (!margin_tap_cell_varies<S>(it) && c != (it != 0 ? 1 : 0)) fail("fixed certainty cell", S, dim, x, 0, it, c, it != 0);
            if (cell[c & 1] != want) fail("certainty cell", S, dim, x, 0, it, cell[c & 1], want);
            checked++;
        }
        for (int sx = -70; sx <= 70; sx++) {
            int base, phase;
            margin_axis<S>(x + sx - 2, base, phase);
            if (phase < 0 || phase >= S) fail("phase", S, dim, x, sx, 0, phase, 0);
            for (int it = 0; it < 5; it++) {
                const int px = it - 2;
                const int want = clampi(floordiv_pos(x + px + sx, S), 0, dim - 1);  // ppsxA / ppsy
                const int site = margin_tap_site<S>(phase, it);
                const int carry = margin_tap_carry<S>(phase, it);
                if (site < 0 || site >= NS) fail("site index", S, dim, x, sx, it, site, NS);
                if (site != margin_tap_site_lo<S>(it) + carry) fail("site = lo + carry", S, dim, x, sx, it, site, carry);
                if (!margin_tap_carry_varies<S>(it) && carry != 0) fail("fixed carry", S, dim, x, sx, it, carry, 0);
                if (carry && margin_tap_site_lo<S>(it) + 1 >= NS) fail("carry past the last site", S, dim, x, sx, it, site, NS);
                const int got = margin_site_coord(base, site, dim);
                if (got != want) fail("site coordinate", S, dim, x, sx, it, got, want);
                // the CFA position of the tap is that of its (clamped) site, in either role
                for (int other = 0; other < 2; other++) {
                    if (margin_site_cfa_pos(got, other) != cfa_index(want, other)) fail("CFA position (row)", S, dim, x, sx, it, got, want);
                    if (margin_site_cfa_pos(other, got) != cfa_index(other, want)) fail("CFA position (column)", S, dim, x, sx, it, got, want);
                }
                checked++;
            }
        }
    }
    for (int r = 0; r < dim; r++)
        for (int c = 0; c < dim; c++)
            if (margin_site_cfa_pos(r, c) != cfa_index(r, c)) fail("CFA position", S, dim, c, r, 0, margin_site_cfa_pos(r, c), cfa_index(r, c));
}

int main()
{
    static_assert(MarginSites<2>::count == 3 && MarginSites<4>::count == 2, "sites per axis");
    for (int dim : {32, 34}) {
        axis<2>(dim);
        axis<4>(dim);
    }
    std::printf("checked %lld failures %d\n", checked, failures);
    return failures ? 1 : 0;
}
"""


def test_site_mapping_equals_the_per_tap_expressions(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check of margin_sites.hpp"
    src = tmp_path / "margin_sites_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "margin_sites_check"
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    # 2 scales x 2 dims: (S * dim) positions x (5 certainty taps + 141 flows x 5 taps)
    want = sum(s * d * (5 + 141 * 5) for s in (2, 4) for d in (32, 34))
    assert f"checked {want} failures 0" in p.stdout, p.stdout
