"""4:4:4 packed video (ojphgpu.h section 7d) on the host: the bit layouts of the formats as byte strings written by hand from
the table, through pipeline.pack_video444 / unpack_video444; ojphgpu_video444_layout against the table; round trips at both
ends of every depth column, the clamp, the positions unpacking must not look at, and the names, depths and shapes the numpy
pair refuses."""
import ctypes as C

import numpy as np
import pytest

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 97)
HEIGHTS = (1, 2, 3, 5)
# name, OJPHGPU_VIDEO_* constant, bytes of a pixel, the depths tried: both ends of the format's column (a name that fixes one: it)
FORMATS = (("v410", 0x21, 4, (1, 10)), ("y410", 0x22, 4, (1, 10)), ("r210", 0x23, 4, (1, 10)), ("r10k", 0x24, 4, (1, 10)),
           ("y4xx", 0x25, 8, (9, 16)), ("y412", 0x25, 8, (12,)), ("y416", 0x25, 8, (16,)),
           ("ayuv", 0x26, 4, (1, 8)), ("bgra", 0x27, 4, (1, 8)), ("rgba", 0x28, 4, (1, 8)), ("argb", 0x29, 4, (1, 8)))


def random_planes444(rng, width, height, depth):
    return [rng.integers(0, 1 << depth, (height, width)).astype(np.int32) for _ in range(3)]


def garbage_in_padding444(rng, buf, fmt, depth):
    """-> a copy of the [H, row_bytes] buffer with random bits wherever unpacking must not look: the padding bits of a dword, the
    alpha, the low bits of every Y4XX word.  Written from the table of section 7d, byte by byte."""
    b = buf.copy()
    if fmt == "v410":                                         # bits 0-1 of a little-endian dword: of its first byte
        b[:, 0::4] |= rng.integers(0, 4, b[:, 0::4].shape).astype(np.uint8)
    elif fmt == "r10k":                                       # bits 0-1 of a big-endian dword: of its last byte
        b[:, 3::4] |= rng.integers(0, 4, b[:, 3::4].shape).astype(np.uint8)
    elif fmt == "y410":                                       # bits 30-31 of a little-endian dword: the top of its last byte
        b[:, 3::4] = (b[:, 3::4] & 0x3F) | (rng.integers(0, 4, b[:, 3::4].shape) << 6).astype(np.uint8)
    elif fmt == "r210":                                       # bits 30-31 of a big-endian dword: the top of its first byte
        b[:, 0::4] = (b[:, 0::4] & 0x3F) | (rng.integers(0, 4, b[:, 0::4].shape) << 6).astype(np.uint8)
    elif fmt in ("y4xx", "y412", "y416"):
        w16 = b.view("<u2")
        if depth < 16:
            w16 |= rng.integers(0, 1 << (16 - depth), w16.shape).astype(np.uint16)
        w16[:, 3::4] = rng.integers(0, 1 << 16, w16[:, 3::4].shape)
    else:                                                     # the alpha byte
        i = 0 if fmt == "argb" else 3
        b[:, i::4] = rng.integers(0, 256, b[:, i::4].shape)
    return b


# (format, depth, components 0 1 2, the pixel's bytes) -- by hand from the table:
#   v410  Cb << 2 | Y << 12 | Cr << 22 = 0xAA8 | 0x155000 | 0xFFC00000 = 0xFFD55AA8, little endian
#   y410  Cb | Y << 10 | Cr << 20 | 3 << 30 = 0x2AA | 0x55400 | 0x3FF00000 | 0xC0000000 = 0xFFF556AA, little endian
#   r210  R << 20 | G << 10 | B = 0x15500000 | 0xAA800 | 0x3FF = 0x155AABFF, BIG endian
#   r10k  R << 22 | G << 12 | B << 2 = 0x55400000 | 0x2AA000 | 0xFFC = 0x556AAFFC, BIG endian
#   y412  words Cb << 4, Y << 4, Cr << 4, 0xFFF0;  y416  words Cb, Y, Cr, 0xFFFF
VECTORS = (("v410", 10, (0x155, 0x2AA, 0x3FF), "A8 5A D5 FF"),
           ("y410", 10, (0x155, 0x2AA, 0x3FF), "AA 56 F5 FF"),
           ("r210", 10, (0x155, 0x2AA, 0x3FF), "15 5A AB FF"),
           ("r10k", 10, (0x155, 0x2AA, 0x3FF), "55 6A AF FC"),
           ("v410", 10, (1, 0, 0), "00 10 00 00"),
           ("r210", 10, (0, 0, 1), "00 00 00 01"),
           ("y412", 12, (0x123, 0x456, 0x789), "60 45 30 12 90 78 F0 FF"),
           ("y4xx", 12, (0x123, 0x456, 0x789), "60 45 30 12 90 78 F0 FF"),
           ("y416", 16, (0x1234, 0xABCD, 0x00FF), "CD AB 34 12 FF 00 FF FF"),
           ("y4xx", 9, (0x1FF, 1, 0x100), "80 00 80 FF 00 80 80 FF"),
           ("ayuv", 8, (1, 2, 3), "03 02 01 FF"),
           ("bgra", 8, (1, 2, 3), "03 02 01 FF"),
           ("rgba", 8, (1, 2, 3), "01 02 03 FF"),
           ("argb", 8, (1, 2, 3), "FF 01 02 03"))


def test_the_bit_layouts_both_ways():
    from openjph_amd.pipeline import pack_video444, unpack_video444
    for fmt, depth, comps, text in VECTORS:
        want = bytes.fromhex(text)
        planes = [np.array([[c]]) for c in comps]
        got = pack_video444(planes, fmt, depth)
        assert got.dtype == np.uint8 and got.shape == (1, len(want)) and got.tobytes() == want, (fmt, got.tobytes().hex())
        back = unpack_video444(np.frombuffer(want, np.uint8), fmt, 1, 1, depth)
        assert [int(p[0, 0]) for p in back] == list(comps) and all(p.shape == (1, 1) for p in back), fmt
    # two rows of two pixels: pixels follow each other in a row, rows follow each other
    planes = [np.array([[1, 2], [3, 4]]), np.array([[5, 6], [7, 8]]), np.array([[9, 10], [11, 12]])]
    want = bytes([1, 5, 9, 255, 2, 6, 10, 255, 3, 7, 11, 255, 4, 8, 12, 255])
    assert pack_video444(planes, "rgba").tobytes() == want and pack_video444(planes, "rgba").shape == (2, 8)
    # the default depths: the one a name fixes, else the widest of the column
    assert pack_video444([np.array([[5000]])] * 3, "v410").tobytes() == bytes.fromhex("FC FF FF FF")
    assert pack_video444([np.array([[70000]])] * 3, "y4xx").tobytes() == b"\xff" * 8
    assert pack_video444([np.array([[70000]])] * 3, "y412").tobytes() == bytes.fromhex("F0 FF") * 4
    assert pack_video444([np.array([[300]])] * 3, "bgra").tobytes() == b"\xff" * 4


def test_video444_layout_against_the_table():
    from openjph_amd import capi
    from openjph_amd.pipeline import VIDEO444_FORMATS, video444_layout
    assert sorted(VIDEO444_FORMATS) == sorted(f for f, _, _, _ in FORMATS)
    assert (capi.VIDEO_V410, capi.VIDEO_Y410, capi.VIDEO_R210, capi.VIDEO_R10K, capi.VIDEO_Y4XX, capi.VIDEO_AYUV, capi.VIDEO_BGRA, capi.VIDEO_RGBA,
            capi.VIDEO_ARGB) == (0x21, 0x22, 0x23, 0x24, 0x25, 0x26, 0x27, 0x28, 0x29)
    L = capi.lib()
    row, total = C.c_uint32(), C.c_uint64()
    for fmt, code, pixel, _ in FORMATS:
        assert VIDEO444_FORMATS[fmt][0] == code
        for w in WIDTHS:
            for h in HEIGHTS:
                assert L.ojphgpu_video444_layout(code, w, h, C.byref(row), C.byref(total)) == capi.OK
                assert (row.value, total.value) == (pixel * w, pixel * w * h) == video444_layout(fmt, w, h)
    for code in (0, 1, 3, 5, 0x11, 0x13, 0x20, 0x2A, -1):    # the codes of sections 7b and 7c among them
        assert L.ojphgpu_video444_layout(code, 6, 2, C.byref(row), C.byref(total)) == capi.E_INVALID
    assert L.ojphgpu_video444_layout(0x21, 0, 2, C.byref(row), C.byref(total)) == capi.E_INVALID
    assert L.ojphgpu_video444_layout(0x25, 6, 0, C.byref(row), C.byref(total)) == capi.E_INVALID
    assert L.ojphgpu_video444_layout(0x21, 6, 2, None, C.byref(total)) == capi.E_INVALID
    assert L.ojphgpu_video444_layout(0x21, 6, 2, C.byref(row), None) == capi.E_INVALID
    assert L.ojphgpu_video444_layout(0x21, 1 << 30, 2, C.byref(row), C.byref(total)) == capi.E_INVALID      # row_bytes beyond 32 bits
    assert L.ojphgpu_video444_layout(0x25, 1 << 29, 2, C.byref(row), C.byref(total)) == capi.E_INVALID
    assert L.ojphgpu_video444_layout(0x21, (1 << 30) - 1, 2, C.byref(row), C.byref(total)) == capi.OK and total.value == 2 * 4 * ((1 << 30) - 1)
    # the 4:2:2 and the 4:2:0 entry points keep refusing the new codes
    off = C.c_uint64()
    for code in range(0x21, 0x2A):
        assert L.ojphgpu_video_layout(code, 6, 2, C.byref(row), C.byref(total)) == capi.E_INVALID
        assert L.ojphgpu_video420_layout(code, 6, 2, C.byref(row), C.byref(off), C.byref(total)) == capi.E_INVALID


@pytest.mark.parametrize("fmt,code,pixel,depth", [(f, c, p, d) for f, c, p, ds in FORMATS for d in ds])
def test_round_trips_clamp_and_ignored_padding(fmt, code, pixel, depth):
    from openjph_amd.pipeline import pack_video444, unpack_video444
    rng = np.random.default_rng(code * 100 + depth)
    top = (1 << depth) - 1
    for w in WIDTHS:
        for h in HEIGHTS:
            planes = random_planes444(rng, w, h, depth)
            planes[0][0, 0], planes[1][0, 0], planes[2][-1, -1] = top, 0, top
            buf = pack_video444(planes, fmt, depth)
            assert buf.dtype == np.uint8 and buf.shape == (h, pixel * w)
            for a, b in zip(unpack_video444(buf, fmt, w, h, depth), planes):
                assert a.shape == b.shape and np.array_equal(a, b)
            # garbage in every position unpacking must not look at: the planes do not change
            dirty = garbage_in_padding444(rng, buf, fmt, depth)
            for a, b in zip(unpack_video444(dirty, fmt, w, h, depth), planes):
                assert np.array_equal(a, b)
            # values below 0 and above 2^b - 1 in int32 planes pack as 0 and 2^b - 1
            over = [rng.choice(np.array([1 << depth, (1 << depth) + 5, -1, -70000], np.int32), p.shape) for p in planes]
            clamped = [np.where(p < 0, 0, top) for p in over]
            assert pack_video444(over, fmt, depth).tobytes() == pack_video444(clamped, fmt, depth).tobytes()
            for a, b in zip(unpack_video444(pack_video444(over, fmt, depth), fmt, w, h, depth), clamped):
                assert np.array_equal(a, b)


def test_refused_names_depths_and_shapes():
    from openjph_amd.pipeline import pack_video, pack_video420, pack_video444, unpack_video444, video444_format, video444_layout
    planes = [np.zeros((4, 6), int)] * 3
    assert pack_video444(planes, "y412", 12).shape == (4, 48)
    assert video444_format("y416", None) == (0x25, 16) and video444_format("r10k", None) == (0x24, 10) and video444_format("argb", 3) == (0x29, 3)
    for fmt, depth in (("y412", 10), ("y416", 12), ("v410", 11), ("y410", 12), ("r210", 0), ("r10k", 16), ("y4xx", 8), ("y4xx", 17), ("ayuv", 9),
                       ("bgra", 10), ("rgba", 0), ("argb", 16)):
        with pytest.raises(ValueError):
            pack_video444(planes, fmt, depth)
    for fmt in ("v210", "uyvy", "y210", "nv12", "p010", "rgb24", "r12l"):      # 4:2:2 and 4:2:0 names among them
        with pytest.raises(ValueError):
            pack_video444(planes, fmt, 8)
        with pytest.raises(ValueError):
            video444_layout(fmt, 6, 4)
    with pytest.raises(ValueError):
        video444_layout("v410", 0, 4)
    with pytest.raises(ValueError):
        video444_layout("v410", 6, 0)
    with pytest.raises(ValueError):                           # sub-sampled chroma planes
        pack_video444([planes[0], np.zeros((4, 3), int), np.zeros((4, 3), int)], "v410")
    with pytest.raises(ValueError):
        pack_video444(planes[:2], "v410")
    with pytest.raises(ValueError):                           # a buffer of another size
        unpack_video444(np.zeros(95, np.uint8), "v410", 6, 4)
    with pytest.raises(ValueError):
        unpack_video444(np.zeros(96, np.uint8), "y416", 6, 4)
    for fmt in ("v410", "y410", "r210", "bgra", "y416"):      # the 4:2:2 and the 4:2:0 pair keep refusing the new names
        with pytest.raises(ValueError):
            pack_video([planes[0], np.zeros((4, 3), int), np.zeros((4, 3), int)], fmt, 8)
        with pytest.raises(ValueError):
            pack_video420([planes[0], np.zeros((2, 3), int), np.zeros((2, 3), int)], fmt, 8)
