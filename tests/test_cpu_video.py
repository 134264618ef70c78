"""4:2:2 video buffers (ojphgpu.h section 7b) on the host: the fixed vectors of the formats through pipeline.pack_video /
unpack_video, ojphgpu_video_layout against the table of the formats, round trips, the clamp, and the padding positions
unpacking must not look at."""
import ctypes as C

import numpy as np
import pytest

WIDTHS = (1, 2, 5, 6, 7, 47, 48, 49, 96, 97)
HEIGHTS = (1, 3)
# name, OJPHGPU_VIDEO_* constant, bit depth
FORMATS = (("uyvy", 1, 8), ("yuy2", 2, 8), ("v210", 3, 10), ("y210", 4, 10), ("y212", 4, 12), ("y216", 4, 16))


def row_bytes_of(code, width):
    cw = (width + 1) // 2
    return {1: 4 * cw, 2: 4 * cw, 3: 128 * ((width + 47) // 48), 4: 8 * cw}[code]


def random_planes(rng, width, height, depth):
    cw = (width + 1) // 2
    return [rng.integers(0, 1 << depth, (height, w)).astype(np.int32) for w in (width, cw, cw)]


def garbage_in_padding(rng, buf, fmt, width, depth):
    """-> a copy of the [H, row_bytes] buffer with random bits wherever unpacking must not look: the second luma of an odd
    row's last pair, the fields and groups a v210 row is padded with, bits 30-31 of every v210 dword, the low bits of every
    Y2XX word"""
    from openjph_amd.pipeline import VIDEO_FORMATS
    code = VIDEO_FORMATS[fmt][0]
    b = buf.copy()
    h, cw = b.shape[0], (width + 1) // 2
    if code in (1, 2):
        if width & 1:
            b[:, 4 * (cw - 1) + (3 if code == 1 else 2)] = rng.integers(0, 256, h)
    elif code == 4:
        w16 = b.view("<u2")
        w16 |= rng.integers(0, 1 << (16 - depth), w16.shape).astype(np.uint16)
        if width & 1:
            w16[:, 4 * (cw - 1) + 2] = rng.integers(0, 1 << 16, h)
    else:
        d = b.view("<u4")
        d |= (rng.integers(0, 4, d.shape).astype(np.uint32) << 30)
        # field q of a row (three to a dword) belongs to pair q // 4 as Cb Y0 Cr Y1
        q = np.arange(d.shape[1] * 3)
        pad = (q // 4 >= cw) | ((q // 4 == cw - 1) & (q % 4 == 3) & bool(width & 1))
        junk = np.where(pad[None, :], rng.integers(0, 1024, (h, q.size)), 0).astype(np.uint32).reshape(h, -1, 3)
        d |= junk[:, :, 0] | junk[:, :, 1] << 10 | junk[:, :, 2] << 20
    return b


def test_the_fixed_vectors_both_ways():
    from openjph_amd.pipeline import pack_video, unpack_video
    planes = [np.arange(64, 70)[None], np.array([[512, 513, 514]]), np.array([[768, 769, 770]])]
    want = np.zeros(128, np.uint8)
    want[:16] = np.array([0x30010200, 0x04280441, 0x20210F01, 0x045C0844], "<u4").view(np.uint8)
    got = pack_video(planes, "v210", 10)
    assert got.dtype == np.uint8 and got.shape == (1, 128) and got.tobytes() == want.tobytes()
    for a, b in zip(unpack_video(want, "v210", 6, 1, 10), planes):
        assert np.array_equal(a, b)
    planes = [np.array([[1, 2, 3]]), np.array([[10, 11]]), np.array([[20, 21]])]
    for fmt, row in (("uyvy", [10, 1, 20, 2, 11, 3, 21, 0]), ("yuy2", [1, 10, 2, 20, 3, 11, 0, 21])):
        assert pack_video(planes, fmt, 8).tolist() == [row]
        for a, b in zip(unpack_video(np.array(row, np.uint8), fmt, 3, 1, 8), planes):
            assert np.array_equal(a, b)
    planes = [np.array([[1, 1023]]), np.array([[512]]), np.array([[4]])]
    words = np.array([0x0040, 0x8000, 0xFFC0, 0x0100], "<u2")
    for fmt in ("y210", "y2xx"):
        assert pack_video(planes, fmt, 10).tobytes() == words.tobytes()
        for a, b in zip(unpack_video(words, fmt, 2, 1, 10), planes):
            assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        pack_video(planes, "y212", 10)
    with pytest.raises(ValueError):
        pack_video(planes, "v210", 12)
    with pytest.raises(ValueError):
        pack_video(planes, "nv12", 8)


def test_video_layout_against_the_table():
    from openjph_amd import capi
    from openjph_amd.pipeline import video_layout
    L = capi.lib()
    row, total = C.c_uint32(), C.c_uint64()
    for fmt, code, _ in FORMATS:
        for w in WIDTHS:
            for h in HEIGHTS:
                assert L.ojphgpu_video_layout(code, w, h, C.byref(row), C.byref(total)) == capi.OK
                assert (row.value, total.value) == (row_bytes_of(code, w), row_bytes_of(code, w) * h) == video_layout(fmt, w, h)
    for code, w, h in ((0, 6, 1), (5, 6, 1), (1, 0, 1), (3, 6, 0), (-1, 6, 1)):
        assert L.ojphgpu_video_layout(code, w, h, C.byref(row), C.byref(total)) == capi.E_INVALID
    assert L.ojphgpu_video_layout(1, 6, 1, None, C.byref(total)) == capi.E_INVALID
    assert L.ojphgpu_video_layout(1, 6, 1, C.byref(row), None) == capi.E_INVALID


@pytest.mark.parametrize("fmt,code,depth", FORMATS)
def test_round_trips_clamp_and_ignored_padding(fmt, code, depth):
    from openjph_amd.pipeline import pack_video, unpack_video
    rng = np.random.default_rng(code * 100 + depth)
    for w in WIDTHS:
        for h in HEIGHTS:
            planes = random_planes(rng, w, h, depth)
            buf = pack_video(planes, fmt, depth)
            assert buf.dtype == np.uint8 and buf.shape == (h, row_bytes_of(code, w))
            for a, b in zip(unpack_video(buf, fmt, w, h, depth), planes):
                assert a.shape == b.shape and np.array_equal(a, b)
            # garbage in every padding position: the planes do not change
            dirty = garbage_in_padding(rng, buf, fmt, w, depth)
            for a, b in zip(unpack_video(dirty, fmt, w, h, depth), planes):
                assert np.array_equal(a, b)
            # 2^b and -1 pack as 2^b - 1 and 0
            over = [np.where(rng.integers(0, 2, p.shape) == 1, 1 << depth, -1) for p in planes]
            clamped = [np.where(p < 0, 0, (1 << depth) - 1) for p in over]
            assert pack_video(over, fmt, depth).tobytes() == pack_video(clamped, fmt, depth).tobytes()
            for a, b in zip(unpack_video(pack_video(over, fmt, depth), fmt, w, h, depth), clamped):
                assert np.array_equal(a, b)
