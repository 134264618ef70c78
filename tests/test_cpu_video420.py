"""4:2:0 video buffers (ojphgpu.h section 7c) on the host: the fixed vectors of the formats through pipeline.pack_video420 /
unpack_video420, ojphgpu_video420_layout against the table of the formats, round trips, the clamp, the padding positions
unpacking must not look at, and the names, depths and shapes the numpy pair refuses."""
import ctypes as C

import numpy as np
import pytest

WIDTHS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 97)
HEIGHTS = (1, 2, 3, 5)
# name, OJPHGPU_VIDEO_* constant, bit depth
FORMATS = (("nv12", 0x11, 8), ("nv21", 0x12, 8), ("p010", 0x13, 10), ("p012", 0x13, 12), ("p016", 0x13, 16), ("p0xx", 0x13, 9))


def row_bytes_of(code, width):
    return (4 if code == 0x13 else 2) * ((width + 1) // 2)


def random_planes420(rng, width, height, depth):
    cw, ch = (width + 1) // 2, (height + 1) // 2
    return [rng.integers(0, 1 << depth, s).astype(np.int32) for s in ((height, width), (ch, cw), (ch, cw))]


def garbage_in_padding420(rng, buf, fmt, width, height, depth):
    """-> a copy of the [H + ch, row_bytes] buffer with random bits wherever unpacking must not look: the sample behind an odd
    luma row, the low bits of every P0XX word"""
    from openjph_amd.pipeline import VIDEO420_FORMATS
    b = buf.copy()
    if VIDEO420_FORMATS[fmt][0] == 0x13:
        w16 = b.view("<u2")
        if depth < 16:
            w16 |= rng.integers(0, 1 << (16 - depth), w16.shape).astype(np.uint16)
        if width & 1:
            w16[:height, width] = rng.integers(0, 1 << 16, height)
    elif width & 1:
        b[:height, width] = rng.integers(0, 256, height)
    return b


def test_the_fixed_vectors_both_ways():
    from openjph_amd.pipeline import pack_video420, unpack_video420
    planes = [np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]]), np.array([[10, 11], [12, 13]]), np.array([[20, 21], [22, 23]])]
    luma = [1, 2, 3, 0, 4, 5, 6, 0, 7, 8, 9, 0]
    for fmt, chroma in (("nv12", [10, 20, 11, 21, 12, 22, 13, 23]), ("nv21", [20, 10, 21, 11, 22, 12, 23, 13])):
        got = pack_video420(planes, fmt, 8)
        assert got.dtype == np.uint8 and got.shape == (5, 4) and got.reshape(-1).tolist() == luma + chroma
        for a, b in zip(unpack_video420(np.array(luma + chroma, np.uint8), fmt, 3, 3, 8), planes):
            assert a.shape == b.shape and np.array_equal(a, b)
    planes = [np.array([[1, 1023]]), np.array([[512]]), np.array([[4]])]
    words = np.array([0x0040, 0xFFC0, 0x8000, 0x0100], "<u2")
    for fmt, depth in (("p010", None), ("p010", 10), ("p0xx", 10)):
        got = pack_video420(planes, fmt, depth)
        assert got.shape == (2, 4) and got.tobytes() == words.tobytes()
        for a, b in zip(unpack_video420(words, fmt, 2, 1, depth), planes):
            assert np.array_equal(a, b)


def test_video420_layout_against_the_table():
    from openjph_amd import capi
    from openjph_amd.pipeline import video420_layout
    L = capi.lib()
    row, off, total = C.c_uint32(), C.c_uint64(), C.c_uint64()
    for fmt, code, _ in FORMATS:
        for w in WIDTHS:
            for h in HEIGHTS:
                assert L.ojphgpu_video420_layout(code, w, h, C.byref(row), C.byref(off), C.byref(total)) == capi.OK
                rb, ch = row_bytes_of(code, w), (h + 1) // 2
                assert (row.value, off.value, total.value) == (rb, rb * h, rb * (h + ch)) == video420_layout(fmt, w, h)
    for code in (0, 5, 1, 0x14, -1):                          # 1: a 4:2:2 code
        assert L.ojphgpu_video420_layout(code, 6, 2, C.byref(row), C.byref(off), C.byref(total)) == capi.E_INVALID
    assert L.ojphgpu_video420_layout(0x11, 0, 2, C.byref(row), C.byref(off), C.byref(total)) == capi.E_INVALID
    assert L.ojphgpu_video420_layout(0x13, 6, 0, C.byref(row), C.byref(off), C.byref(total)) == capi.E_INVALID
    assert L.ojphgpu_video420_layout(0x11, 6, 2, None, C.byref(off), C.byref(total)) == capi.E_INVALID
    assert L.ojphgpu_video420_layout(0x11, 6, 2, C.byref(row), None, C.byref(total)) == capi.E_INVALID
    assert L.ojphgpu_video420_layout(0x11, 6, 2, C.byref(row), C.byref(off), None) == capi.E_INVALID
    # the 4:2:2 entry point keeps refusing the new codes, as it refuses 5
    two = C.c_uint64()
    for code in (0x11, 0x12, 0x13):
        assert L.ojphgpu_video_layout(code, 6, 2, C.byref(row), C.byref(two)) == capi.E_INVALID


@pytest.mark.parametrize("fmt,code,depth", FORMATS)
def test_round_trips_clamp_and_ignored_padding(fmt, code, depth):
    from openjph_amd.pipeline import pack_video420, unpack_video420
    rng = np.random.default_rng(code * 100 + depth)
    for w in WIDTHS:
        for h in HEIGHTS:
            planes = random_planes420(rng, w, h, depth)
            buf = pack_video420(planes, fmt, depth)
            assert buf.dtype == np.uint8 and buf.shape == (h + (h + 1) // 2, row_bytes_of(code, w))
            for a, b in zip(unpack_video420(buf, fmt, w, h, depth), planes):
                assert a.shape == b.shape and np.array_equal(a, b)
            if w & 1:                                         # the padding luma sample is zero
                es = 2 if code == 0x13 else 1
                assert not buf[:h, w * es: (w + 1) * es].any()
            # garbage in every padding position: the planes do not change
            dirty = garbage_in_padding420(rng, buf, fmt, w, h, depth)
            for a, b in zip(unpack_video420(dirty, fmt, w, h, depth), planes):
                assert np.array_equal(a, b)
            # values below 0 and above 2^b - 1 pack as 0 and 2^b - 1
            over = [rng.choice(np.array([1 << depth, (1 << depth) + 5, -1, -70000]), p.shape) for p in planes]
            clamped = [np.where(p < 0, 0, (1 << depth) - 1) for p in over]
            assert pack_video420(over, fmt, depth).tobytes() == pack_video420(clamped, fmt, depth).tobytes()
            for a, b in zip(unpack_video420(pack_video420(over, fmt, depth), fmt, w, h, depth), clamped):
                assert np.array_equal(a, b)


def test_refused_names_depths_and_shapes():
    from openjph_amd.pipeline import pack_video, pack_video420, unpack_video420, video420_layout
    planes = [np.zeros((4, 6), int), np.zeros((2, 3), int), np.zeros((2, 3), int)]
    assert pack_video420(planes, "p012", 12).shape == (6, 12)
    with pytest.raises(ValueError):
        pack_video420(planes, "p012", 10)
    with pytest.raises(ValueError):
        pack_video420(planes, "nv12", 10)
    with pytest.raises(ValueError):
        pack_video420(planes, "p0xx", 8)
    with pytest.raises(ValueError):
        pack_video420(planes, "uyvy", 8)                       # a 4:2:2 name
    with pytest.raises(ValueError):
        pack_video420(planes, "i420", 8)
    with pytest.raises(ValueError):
        unpack_video420(np.zeros(36, np.uint8), "nv16", 6, 4, 8)
    with pytest.raises(ValueError):
        video420_layout("v210", 6, 4)
    with pytest.raises(ValueError):
        video420_layout("nv12", 0, 4)
    with pytest.raises(ValueError):                           # 4:2:2-shaped chroma planes
        pack_video420([planes[0], np.zeros((4, 3), int), np.zeros((4, 3), int)], "nv12", 8)
    with pytest.raises(ValueError):
        pack_video420([planes[0], planes[1], np.zeros((2, 2), int)], "nv12", 8)
    with pytest.raises(ValueError):                           # a buffer of another size
        unpack_video420(np.zeros(35, np.uint8), "nv12", 6, 4, 8)
    with pytest.raises(ValueError):                           # and the 4:2:2 pair keeps refusing the new names
        pack_video([planes[0], np.zeros((4, 3), int), np.zeros((4, 3), int)], "nv12", 8)
