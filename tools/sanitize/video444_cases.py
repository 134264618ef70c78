#!/usr/bin/env python3
"""The cases of tools/sanitize/video444_host.cpp, made by the numpy statement of the 4:4:4 stages (pipeline.pack_video444 /
unpack_video444): every format and container over the shapes and the three layouts of tests/test_gpu_video444.py.

    python tools/sanitize/video444_cases.py OUT_FILE

One record per case, little endian: 9 uint32 (format code, width, height, depth, container bits, pitch, the buffer's offset
from a 256-byte boundary, then the byte counts of the video buffer and of the planes) and four blobs: the video buffer to
unpack (garbage wherever unpacking must not look, pitch slack included), the planes that must come out, the planes to pack
(values outside the range among them), and the buffer that must come out of packing into a destination pre-filled with 0x5A."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from openjph_amd.pipeline import VIDEO444_FORMATS, pack_video444, video444_layout   # noqa: E402

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
HEIGHTS = (1, 2, 3, 5)
WIDE = (6149, 5)
# (name, depth, containers): every format, both ends of a column somewhere, every instantiation (field width x container)
KERNELS = (("v410", 10, (16, 32)), ("y410", 10, (16, 32)), ("r210", 10, (16, 32)), ("r10k", 10, (16, 32)), ("v410", 1, (16,)),
           ("y4xx", 9, (16, 32)), ("y412", 12, (16,)), ("y416", 16, (16, 32)),
           ("ayuv", 8, (8, 16, 32)), ("bgra", 8, (8, 16, 32)), ("rgba", 8, (8, 16, 32)), ("argb", 8, (8, 16, 32)), ("bgra", 5, (8,)))
NP_DT = {8: np.uint8, 16: np.uint16, 32: np.int32}
FILL = 0x5A


def garbage(buf, fmt, depth, rng):
    """a copy of a packed buffer with random bits wherever unpacking must not look: padding, alpha, the low bits of a Y4XX word"""
    code = VIDEO444_FORMATS[fmt][0]
    out = buf.copy()
    if code in (0x21, 0x24):                                   # bits 0-1 of the dword: v410 little endian, r10k big endian
        out[:, (0 if code == 0x21 else 3)::4] |= rng.integers(0, 4, out[:, 0::4].shape).astype(np.uint8)
    elif code in (0x22, 0x23):                                 # bits 30-31
        i = 3 if code == 0x22 else 0
        out[:, i::4] = (out[:, i::4] & 0x3F) | (rng.integers(0, 4, out[:, i::4].shape) << 6).astype(np.uint8)
    elif code == 0x25:
        w16 = out.view("<u2")
        if depth < 16:
            w16 |= rng.integers(0, 1 << (16 - depth), w16.shape).astype(np.uint16)
        w16[:, 3::4] = rng.integers(0, 1 << 16, w16[:, 3::4].shape)
    else:
        i = 0 if code == 0x29 else 3
        out[:, i::4] = rng.integers(0, 256, out[:, i::4].shape)
    return out


def layouts(fmt, w, h):
    """(pitch, offset of the buffer from a 256-byte boundary)"""
    row = video444_layout(fmt, w, h)[0]
    e = row // w
    yield row, 0                                               # tight
    yield row + 3 * e, e                                       # one pixel off 16 bytes, and the alignment changes row by row
    yield -(-row // 256) * 256, 0                              # a multiple of 256


def pitched(rows, pitch, fill_rng):
    """[n, row_bytes] -> the bytes of a buffer of that pitch, without slack behind the last row; the slack: FILL or random"""
    n, row = rows.shape
    out = np.full((n, pitch), FILL, np.uint8) if fill_rng is None else fill_rng.integers(0, 256, (n, pitch)).astype(np.uint8)
    out[:, :row] = rows
    return out.reshape(-1)[: pitch * (n - 1) + row]


def main(path):
    rng = np.random.default_rng(444)
    n = 0
    with open(path, "wb") as f:
        for fmt, depth, containers in KERNELS:
            code = VIDEO444_FORMATS[fmt][0]
            for w, h in [(w, h) for w in WIDTHS for h in HEIGHTS] + [WIDE]:
                planes = [rng.integers(0, 1 << depth, (h, w)).astype(np.int64) for _ in range(3)]
                dirty = garbage(pack_video444(planes, fmt, depth), fmt, depth, rng)
                for cont in containers:
                    want_planes = np.concatenate([p.reshape(-1) for p in planes]).astype(NP_DT[cont])
                    lo, hi = (-70000, 70000) if cont == 32 else (0, 1 << cont)
                    src = [np.where(rng.integers(0, 4, p.shape) == 0, rng.integers(lo, hi, p.shape), p) for p in planes]
                    packed = pack_video444(src, fmt, depth)
                    src_flat = np.concatenate([p.reshape(-1) for p in src]).astype(NP_DT[cont])
                    for pitch, off in layouts(fmt, w, h):
                        blobs = [pitched(dirty, pitch, rng), want_planes.view(np.uint8), src_flat.view(np.uint8), pitched(packed, pitch, None)]
                        f.write(struct.pack("<9I", code, w, h, depth, cont, pitch, off, blobs[0].size, blobs[1].size))
                        for b in blobs:
                            f.write(np.ascontiguousarray(b).tobytes())
                        n += 1
    print("%d cases -> %s" % (n, path))


if __name__ == "__main__":
    main(sys.argv[1])
