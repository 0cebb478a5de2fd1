// finish_ring.hpp -- the pixels the finishing burst tile kernel (accumulate_fast.hip, k_accumulate2xTileBurst<CFA, true>) does
// not finish: the ring of M HR pixels along every edge of the frame, outermost line included.  Plain integer code for host and
// device, so that k_finishRing and the host check (tests/test_finish_ring_cpu.py) use one definition.
//
// Index order: the top band row by row (M rows of hrW pixels), the bottom band likewise, then for every row between them its M
// left and its M right pixels.  The tile kernel's live pixels are rows M .. hrH - M - 1, columns M .. hrW - M - 1 (hrW a
// multiple of 4: whole four-pixel strips), so ring and live pixels together cover the frame exactly once.
#pragma once

#if defined(__HIPCC__)
#define MFSR_RING_HD __host__ __device__ __forceinline__
#else
#define MFSR_RING_HD inline
#endif

// hrW, hrH >= 2 M
MFSR_RING_HD long long finish_ring_count(int hrW, int hrH, int M) { return 2LL * M * hrW + 2LL * M * (hrH - 2 * M); }

// pixel i of the ring, 0 <= i < finish_ring_count
MFSR_RING_HD void finish_ring_pixel(long long i, int hrW, int hrH, int M, int& x, int& y)
{
    const long long band = (long long)M * hrW;
    if (i < 2 * band) {
        const int bottom = i >= band ? 1 : 0;
        const int r = (int)(i - bottom * band);
        const int row = r / hrW;
        x = r - row * hrW;
        y = bottom ? hrH - M + row : row;
        return;
    }
    const long long s = i - 2 * band;
    const int row = (int)(s / (2 * M));
    const int c = (int)(s - (long long)row * (2 * M));
    y = M + row;
    x = c < M ? c : hrW - 2 * M + c;
}
