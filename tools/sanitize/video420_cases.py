#!/usr/bin/env python3
"""The cases of tools/sanitize/video420_host.cpp, made by the numpy statement of the 4:2:0 stages (pipeline.pack_video420 /
unpack_video420): every format and container over the shapes and the three layouts of tests/test_gpu_video420.py.

    python tools/sanitize/video420_cases.py OUT_FILE

One record per case, little endian: 12 uint32 (format code, width, height, depth, container bits, luma pitch, chroma pitch,
the luma and the chroma plane's offset from a 256-byte boundary, then the byte counts of a video plane pair's blobs: luma,
chroma, and of the planes) and six blobs: the video luma and chroma plane to unpack (garbage wherever unpacking must not
look, pitch slack included), the planes that must come out, the planes to pack (values outside the range among them), and the
luma and chroma plane that must come out of packing into a destination pre-filled with 0x5A."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from openjph_amd.pipeline import VIDEO420_FORMATS, pack_video420, video420_layout   # noqa: E402

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
HEIGHTS = (1, 2, 3, 5)
WIDE = (6149, 5)
KERNELS = (("nv12", 8, (8, 16, 32)), ("nv21", 8, (8, 16, 32)), ("nv12", 5, (8,)), ("p010", 10, (16, 32)), ("p012", 12, (16,)), ("p016", 16, (16, 32)))
NP_DT = {8: np.uint8, 16: np.uint16, 32: np.int32}
FILL = 0x5A


def layouts(fmt, w, h):
    row, off, _ = video420_layout(fmt, w, h)
    e = 4 if VIDEO420_FORMATS[fmt][0] == 0x13 else 2
    yield row, row, 0, off % 256                               # tight
    yield row + 3 * e, row + 3 * e, 0, e                       # alignment changes row by row, the chroma plane one element off 16 bytes
    p = -(-row // 256) * 256
    yield p, p + 256, 0, 0                                     # both pitches a multiple of 256


def pitched(rows, pitch, fill_rng):
    """[n, row_bytes] -> the bytes of a plane of that pitch, without slack behind the last row; the slack: FILL or random"""
    n, row = rows.shape
    out = np.full((n, pitch), FILL, np.uint8) if fill_rng is None else fill_rng.integers(0, 256, (n, pitch)).astype(np.uint8)
    out[:, :row] = rows
    return out.reshape(-1)[: pitch * (n - 1) + row]


def main(path):
    rng = np.random.default_rng(420)
    n = 0
    with open(path, "wb") as f:
        for fmt, depth, containers in KERNELS:
            code = VIDEO420_FORMATS[fmt][0]
            for w, h in [(w, h) for w in WIDTHS for h in HEIGHTS] + [WIDE]:
                cw, ch = (w + 1) // 2, (h + 1) // 2
                planes = [rng.integers(0, 1 << depth, s).astype(np.int64) for s in ((h, w), (ch, cw), (ch, cw))]
                buf = pack_video420(planes, fmt, depth)
                dirty = buf.copy()                             # garbage where unpacking must not look
                if code == 0x13:
                    w16 = dirty.view("<u2")
                    if depth < 16:
                        w16 |= rng.integers(0, 1 << (16 - depth), w16.shape).astype(np.uint16)
                    if w & 1:
                        w16[:h, w] = rng.integers(0, 1 << 16, h)
                elif w & 1:
                    dirty[:h, w] = rng.integers(0, 256, h)
                for cont in containers:
                    want_planes = np.concatenate([p.reshape(-1) for p in planes]).astype(NP_DT[cont])
                    lo, hi = (-70000, 70000) if cont == 32 else (0, 1 << cont)
                    src = [np.where(rng.integers(0, 4, p.shape) == 0, rng.integers(lo, hi, p.shape), p) for p in planes]
                    packed = pack_video420(src, fmt, depth)
                    src_flat = np.concatenate([p.reshape(-1) for p in src]).astype(NP_DT[cont])
                    for lp, cp, loff, coff in layouts(fmt, w, h):
                        blobs = [pitched(dirty[:h], lp, rng), pitched(dirty[h:], cp, rng), want_planes.view(np.uint8), src_flat.view(np.uint8),
                                 pitched(packed[:h], lp, None), pitched(packed[h:], cp, None)]
                        f.write(struct.pack("<12I", code, w, h, depth, cont, lp, cp, loff, coff, blobs[0].size, blobs[1].size, blobs[2].size))
                        for b in blobs:
                            f.write(np.ascontiguousarray(b).tobytes())
                        n += 1
    print("%d cases -> %s" % (n, path))


if __name__ == "__main__":
    main(sys.argv[1])
