"""Numpy restatement of the four packed raw layouts (include/mfsr.h), both directions, written from
the table there and not from the kernel or from synth.pack_raw: the MIPI layouts byte by byte, the big-endian ones as what they
are -- the samples' bits, most significant first, strung together and cut into bytes."""
import numpy as np

NONE, MIPI10, MIPI12, BE10, BE12 = 0, 1, 2, 3, 4
BITS = {MIPI10: 10, MIPI12: 12, BE10: 10, BE12: 12}
ALL = (MIPI10, MIPI12, BE10, BE12)


def group(packing):
    """(samples, bytes) of one group"""
    return (4, 5) if BITS[packing] == 10 else (2, 3)


def dense_row_bytes(packing, width):
    return width * BITS[packing] // 8


def pack_ref(frame, packing, row_bytes=None, fill=0):
    """uint16 [H, W] -> uint8 [H, row_bytes]; bytes beyond the dense row are `fill`"""
    frame = np.asarray(frame).astype(np.uint32)
    h, w = frame.shape
    bits = BITS[packing]
    gs, gb = group(packing)
    assert w % gs == 0 and int(frame.max(initial=0)) < (1 << bits)
    dense = dense_row_bytes(packing, w)
    rb = dense if row_bytes is None else row_bytes
    assert rb >= dense
    out = np.full((h, rb), fill, np.uint8)
    if packing in (BE10, BE12):
        # bit stream: every sample's `bits` bits, most significant first
        b = ((frame[:, :, None] >> np.arange(bits - 1, -1, -1, dtype=np.uint32)) & 1).astype(np.uint8)
        out[:, :dense] = np.packbits(b.reshape(h, w * bits), axis=1, bitorder="big")
        return out
    P = frame.reshape(h, w // gs, gs)
    B = np.zeros((h, w // gs, gb), np.uint32)
    if packing == MIPI10:
        for j in range(4):
            B[:, :, j] = P[:, :, j] >> 2
            B[:, :, 4] |= (P[:, :, j] & 3) << (2 * j)
    else:
        B[:, :, 0] = P[:, :, 0] >> 4
        B[:, :, 1] = P[:, :, 1] >> 4
        B[:, :, 2] = (P[:, :, 0] & 15) | ((P[:, :, 1] & 15) << 4)
    out[:, :dense] = B.reshape(h, dense).astype(np.uint8)
    return out


def unpack_ref(packed, packing, width):
    """uint8 [H, >= dense] -> uint16 [H, width]; bytes beyond the dense row are not looked at"""
    packed = np.asarray(packed, np.uint8)
    h = packed.shape[0]
    bits = BITS[packing]
    gs, gb = group(packing)
    assert width % gs == 0
    dense = dense_row_bytes(packing, width)
    rows = packed[:, :dense]
    if packing in (BE10, BE12):
        b = np.unpackbits(rows, axis=1, bitorder="big").reshape(h, width, bits).astype(np.uint32)
        return (b << np.arange(bits - 1, -1, -1, dtype=np.uint32)).sum(axis=2).astype(np.uint16)
    B = rows.reshape(h, width // gs, gb).astype(np.uint32)
    P = np.zeros((h, width // gs, gs), np.uint32)
    if packing == MIPI10:
        for j in range(4):
            P[:, :, j] = (B[:, :, j] << 2) | ((B[:, :, 4] >> (2 * j)) & 3)
    else:
        P[:, :, 0] = (B[:, :, 0] << 4) | (B[:, :, 2] & 15)
        P[:, :, 1] = (B[:, :, 1] << 4) | (B[:, :, 2] >> 4)
    return P.reshape(h, width).astype(np.uint16)


# Known answers, worked out by hand from the table: (packing, samples of one row, its bytes).  Every group has all-distinct
# samples whose high and low parts differ, so that a swapped pair, a reversed nibble or a reversed order of the low bits shows.
KNOWN = [
    # 0x2A5 = 10 1010 0101: >>2 = 0xA9, &3 = 1; 0x13E: 0x4F, 2; 0x3C3: 0xF0, 3; 0x058: 0x16, 0 -> B4 = 1 | 2<<2 | 3<<4 | 0<<6 = 0x39
    # 0x003, 0x001, 0x3FE, 0x002: >>2 = 0, 0, 0xFF, 0; &3 = 3, 1, 2, 2 -> B4 = 3 | 1<<2 | 2<<4 | 2<<6 = 0xA7
    (MIPI10, [0x2A5, 0x13E, 0x3C3, 0x058, 0x003, 0x001, 0x3FE, 0x002],
     [0xA9, 0x4F, 0xF0, 0x16, 0x39, 0x00, 0x00, 0xFF, 0x00, 0xA7]),
    # 0xABC, 0x123: B0 = 0xAB, B1 = 0x12, B2 = 0xC | 0x3<<4 = 0x3C;  0x00F, 0xF00: 0x00, 0xF0, 0x0F
    (MIPI12, [0xABC, 0x123, 0x00F, 0xF00], [0xAB, 0x12, 0x3C, 0x00, 0xF0, 0x0F]),
    # 1010100101 0100111110 1111000011 0001011000 -> 10101001 01010011 11101111 00001100 01011000
    # 0000000011 0000000001 1111111110 0000000010 -> 00000000 11000000 00011111 11111000 00000010
    (BE10, [0x2A5, 0x13E, 0x3C3, 0x058, 0x003, 0x001, 0x3FE, 0x002],
     [0xA9, 0x53, 0xEF, 0x0C, 0x58, 0x00, 0xC0, 0x1F, 0xF8, 0x02]),
    # 0xABC 0x123 -> AB C1 23
    (BE12, [0xABC, 0x123, 0x00F, 0xF00], [0xAB, 0xC1, 0x23, 0x00, 0xFF, 0x00]),
]
