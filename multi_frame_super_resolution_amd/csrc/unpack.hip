// unpack.hip -- packed 10 / 12-bit raw frames widened to the uint16_t samples every other stage reads.
//
// The four layouts are stated bit by bit in include/mfsr.h (mfsr_unpackRaw): MIPI CSI-2 RAW10 / RAW12 (the low bits of a group
// of samples collected in its last byte) and the big-endian bit stream of DNG / TIFF.  Everything is integer and exact: the
// results equal the numpy restatement of the tests (tests/packed_ref.py) bit for bit, for any launch shape.
//
// k_unpackRaw: one lane per 16 samples of a row (20 source bytes at 10 bits, 24 at 12 bits; 32 destination bytes), one launch
// for all frames, shaped like k_applyGains.  VEC (every source row 4-byte aligned, every destination row 16-byte aligned): a
// whole lane loads its 5 / 6 dwords, takes the bytes out of the registers with constant shifts (v_bfe_u32), and stores two
// 16-byte pieces; the lane the row's end cuts goes group by group.  Otherwise every lane goes group by group with byte loads
// and 16-bit stores.  A group is 4 samples in 5 bytes or 2 samples in 3 bytes and the width is a whole number of groups, so
// no lane reads a byte beyond width * bits / 8 of its row (line padding is never read) or writes beyond 2 * width.
#include "raw_stage.hpp"

namespace {

constexpr int kUnpackThreads = 256;
constexpr int kUnpackSamples = 16;  // samples of one lane

typedef RawFramesT<const uint8_t> PackedFrames;

struct UnpackGeom {
    int rowBytes, pitch, width, height;
    int lanesPerRow;
};

// one group: BITS == 10: 5 bytes -> 4 samples; BITS == 12: 3 bytes -> 2 samples
template <int BITS, bool BE>
__device__ __forceinline__ void unpack_group(const uint32_t* B, uint32_t* P)
{
    if (BITS == 10) {
        if (BE) {
            P[0] = (B[0] << 2) | (B[1] >> 6);
            P[1] = ((B[1] & 63u) << 4) | (B[2] >> 4);
            P[2] = ((B[2] & 15u) << 6) | (B[3] >> 2);
            P[3] = ((B[3] & 3u) << 8) | B[4];
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) P[j] = (B[j] << 2) | ((B[4] >> (2 * j)) & 3u);
        }
    } else {
        if (BE) {
            P[0] = (B[0] << 4) | (B[1] >> 4);
            P[1] = ((B[1] & 15u) << 8) | B[2];
        } else {
            P[0] = (B[0] << 4) | (B[2] & 15u);
            P[1] = (B[1] << 4) | (B[2] >> 4);
        }
    }
}

template <int BITS, bool BE, bool VEC>
__global__ __launch_bounds__(kUnpackThreads) void k_unpackRaw(PackedFrames packed, RawFramesMut frames, UnpackGeom g)
{
    constexpr int kGroupBytes = BITS == 10 ? 5 : 3, kGroupSamples = BITS == 10 ? 4 : 2;
    constexpr int kLaneBytes = kUnpackSamples * BITS / 8;  // 20 / 24
    constexpr int kLaneGroups = kUnpackSamples / kGroupSamples;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)g.lanesPerRow * g.height) return;
    const int y = (int)(idx / g.lanesPerRow), c = (int)(idx % g.lanesPerRow);
    const uint8_t* src = packed.p[blockIdx.y] + (size_t)y * (size_t)g.rowBytes + (size_t)c * kLaneBytes;
    char* dst = (char*)frames.p[blockIdx.y] + (size_t)y * (size_t)g.pitch + (size_t)c * (2 * kUnpackSamples);
    const int n = min(kUnpackSamples, g.width - kUnpackSamples * c);  // samples of this lane: whole groups, >= 1
    if (VEC && n == kUnpackSamples) {
        uint32_t w[kLaneBytes / 4];
#pragma unroll
        for (int i = 0; i < kLaneBytes / 4; i++) w[i] = ((const uint32_t*)src)[i];
        uint32_t P[kUnpackSamples];
#pragma unroll
        for (int k = 0; k < kLaneGroups; k++) {
            uint32_t B[kGroupBytes];
#pragma unroll
            for (int i = 0; i < kGroupBytes; i++) {
                const int at = k * kGroupBytes + i;
                B[i] = (w[at >> 2] >> (8 * (at & 3))) & 0xffu;
            }
            unpack_group<BITS, BE>(B, P + k * kGroupSamples);
        }
        uint4* out = (uint4*)dst;
        out[0] = make_uint4(P[0] | (P[1] << 16), P[2] | (P[3] << 16), P[4] | (P[5] << 16), P[6] | (P[7] << 16));
        out[1] = make_uint4(P[8] | (P[9] << 16), P[10] | (P[11] << 16), P[12] | (P[13] << 16), P[14] | (P[15] << 16));
        return;
    }
    uint16_t* out = (uint16_t*)dst;
    for (int k = 0; k * kGroupSamples < n; k++) {
        uint32_t B[kGroupBytes], P[kGroupSamples];
#pragma unroll
        for (int i = 0; i < kGroupBytes; i++) B[i] = src[k * kGroupBytes + i];
        unpack_group<BITS, BE>(B, P);
#pragma unroll
        for (int j = 0; j < kGroupSamples; j++) out[k * kGroupSamples + j] = (uint16_t)P[j];
    }
}

int pack_bits(int packing)
{
    return packing == MFSR_PACK_MIPI10 || packing == MFSR_PACK_BE10 ? 10 : (packing == MFSR_PACK_MIPI12 || packing == MFSR_PACK_BE12 ? 12 : 0);
}

template <int BITS, bool BE>
void launch_unpack(bool vec, dim3 grid, hipStream_t s, const PackedFrames& p, const RawFramesMut& t, const UnpackGeom& g)
{
    const dim3 block(kUnpackThreads);
    if (vec)
        hipLaunchKernelGGL((k_unpackRaw<BITS, BE, true>), grid, block, 0, s, p, t, g);
    else
        hipLaunchKernelGGL((k_unpackRaw<BITS, BE, false>), grid, block, 0, s, p, t, g);
}

}  // namespace

extern "C" int mfsr_packed_row_bytes(int packing, int width)
{
    const int bits = pack_bits(packing);
    MFSR_REQUIRE(bits != 0 && width > 0 && (width % (bits == 10 ? 4 : 2)) == 0);
    const long long bytes = (long long)width * bits / 8;
    MFSR_REQUIRE(bytes <= INT_MAX);
    return (int)bytes;
}

extern "C" int mfsr_unpackRaw(int nFrames, const uint8_t* const* packed, int rowBytes, int packing, uint16_t* const* frames, int pitch,
                              int width, int height, mfsr_stream_t stream)
{
    // host validation first: nothing below touches the device before every argument has passed
    const int dense = mfsr_packed_row_bytes(packing, width);
    MFSR_REQUIRE(dense > 0 && rowBytes >= dense && height > 0);
    MFSR_REQUIRE(raw_frames_ok(nFrames, kRawMaxFrames, frames, pitch, width) && packed != nullptr);
    for (int k = 0; k < nFrames; k++) MFSR_REQUIRE(packed[k] != nullptr);
    UnpackGeom g;
    g.rowBytes = rowBytes;
    g.pitch = pitch;
    g.width = width;
    g.height = height;
    g.lanesPerRow = (int)mfsr_cdiv(width, kUnpackSamples);
    const long long blocks = ((long long)g.lanesPerRow * height + kUnpackThreads - 1) / kUnpackThreads;
    MFSR_REQUIRE(blocks <= INT_MAX);
    const bool vec = raw_aligned(nFrames, packed, rowBytes, 4) && raw_aligned(nFrames, frames, pitch, 16);
    const PackedFrames p = raw_table(nFrames, packed);
    const RawFramesMut t = raw_table(nFrames, frames);
    const dim3 grid((unsigned)blocks, (unsigned)nFrames);
    switch (packing) {
    case MFSR_PACK_MIPI10: launch_unpack<10, false>(vec, grid, mfsr_s(stream), p, t, g); break;
    case MFSR_PACK_MIPI12: launch_unpack<12, false>(vec, grid, mfsr_s(stream), p, t, g); break;
    case MFSR_PACK_BE10: launch_unpack<10, true>(vec, grid, mfsr_s(stream), p, t, g); break;
    default: launch_unpack<12, true>(vec, grid, mfsr_s(stream), p, t, g); break;
    }
    return mfsr_launch_status("k_unpackRaw");
}
