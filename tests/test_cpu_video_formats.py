"""The per-format rules of the video buffers (ojphgpu.h sections 7b - 7d) as one literal table, written by hand from the header's
prose, and the two tables of the code held against it: the C one through ojphgpu_video_format_info and the three layout
calls, the Python one (pipeline) through its names, its depth columns, its default depths and its layouts."""
import ctypes as C

import pytest

# name: (OJPHGPU_VIDEO_* code, family, chroma cell (sub_x, sub_y), the depth the name fixes, lowest and highest depth of the column,
# smallest container, alignment of a video pointer and of a pitch (0: rows follow each other at row_bytes, the entry points take
# no pitch), bytes per unit of pixels: row_bytes = unit_bytes * ceil(width / unit_pixels))
TABLE = {
    # 7b: one packed buffer, 16-byte aligned; 8-bit containers with the two byte formats only
    "uyvy": (0x01, 422, (2, 1), None, 1, 8, 8, 16, 0, 4, 2),
    "yuy2": (0x02, 422, (2, 1), None, 1, 8, 8, 16, 0, 4, 2),
    "v210": (0x03, 422, (2, 1), None, 1, 10, 16, 16, 0, 128, 48),
    "y2xx": (0x04, 422, (2, 1), None, 9, 16, 16, 16, 0, 8, 2),
    "y210": (0x04, 422, (2, 1), 10, 9, 16, 16, 16, 0, 8, 2),
    "y212": (0x04, 422, (2, 1), 12, 9, 16, 16, 16, 0, 8, 2),
    "y216": (0x04, 422, (2, 1), 16, 9, 16, 16, 16, 0, 8, 2),
    # 7c: two planes; pointers and pitches are multiples of the chroma pair
    "nv12": (0x11, 420, (2, 2), None, 1, 8, 8, 2, 2, 2, 2),
    "nv21": (0x12, 420, (2, 2), None, 1, 8, 8, 2, 2, 2, 2),
    "p0xx": (0x13, 420, (2, 2), None, 9, 16, 16, 4, 4, 4, 2),
    "p010": (0x13, 420, (2, 2), 10, 9, 16, 16, 4, 4, 4, 2),
    "p012": (0x13, 420, (2, 2), 12, 9, 16, 16, 4, 4, 4, 2),
    "p016": (0x13, 420, (2, 2), 16, 9, 16, 16, 4, 4, 4, 2),
    # 7d: one word per pixel; the pointer and the pitch are multiples of it
    "v410": (0x21, 444, (1, 1), None, 1, 10, 16, 4, 4, 4, 1),
    "y410": (0x22, 444, (1, 1), None, 1, 10, 16, 4, 4, 4, 1),
    "r210": (0x23, 444, (1, 1), None, 1, 10, 16, 4, 4, 4, 1),
    "r10k": (0x24, 444, (1, 1), None, 1, 10, 16, 4, 4, 4, 1),
    "y4xx": (0x25, 444, (1, 1), None, 9, 16, 16, 8, 8, 8, 1),
    "y412": (0x25, 444, (1, 1), 12, 9, 16, 16, 8, 8, 8, 1),
    "y416": (0x25, 444, (1, 1), 16, 9, 16, 16, 8, 8, 8, 1),
    "ayuv": (0x26, 444, (1, 1), None, 1, 8, 8, 4, 4, 4, 1),
    "bgra": (0x27, 444, (1, 1), None, 1, 8, 8, 4, 4, 4, 1),
    "rgba": (0x28, 444, (1, 1), None, 1, 8, 8, 4, 4, 4, 1),
    "argb": (0x29, 444, (1, 1), None, 1, 8, 8, 4, 4, 4, 1),
}
# the depth a name stands for when none is given: the one it fixes; 4:4:4: the widest of the column; nv12 / nv21: 8; None: refused
DEFAULT_DEPTH = {name: (t[3] if t[3] is not None else (t[5] if t[1] == 444 else (8 if name in ("nv12", "nv21") else None))) for name, t in TABLE.items()}


def table_layout(name, w, h):
    """-> (row_bytes, chroma_offset, frame_bytes) by the table's arithmetic; chroma_offset 0 without a second plane"""
    _, family, _, _, _, _, _, _, _, unit_bytes, unit_pixels = TABLE[name]
    row = unit_bytes * (-(-w // unit_pixels))
    return (row, row * h, row * (h + (h + 1) // 2)) if family == 420 else (row, 0, row * h)


def accepts(name, cell, depth, container):
    """the rule of the two _set_video setters on a plan of three unsigned components of one depth whose chroma cell is `cell`"""
    _, _, fcell, fixed, lo, hi, min_container, *_ = TABLE[name]
    return fcell == cell and fixed in (None, depth) and lo <= depth <= hi and container >= depth and container >= min_container


def c_layout(L, family, code, w, h):
    """the family's layout call -> its return code, (row_bytes, chroma_offset, frame_bytes)"""
    row, off, total = C.c_uint32(), C.c_uint64(), C.c_uint64()
    if family == 420:
        rc = L.ojphgpu_video420_layout(code, w, h, C.byref(row), C.byref(off), C.byref(total))
    else:
        rc = getattr(L, "ojphgpu_video_layout" if family == 422 else "ojphgpu_video444_layout")(code, w, h, C.byref(row), C.byref(total))
    return rc, (row.value, off.value, total.value)


def test_the_table_itself():
    rows = {}
    for t in TABLE.values():                                   # the names of one code differ in the depth they fix, in nothing else
        rows.setdefault(t[0], set()).add(t[:3] + t[4:])
    assert len(TABLE) == 24 and len(rows) == 16 and all(len(r) == 1 for r in rows.values())


def test_format_info_is_the_table():
    from openjph_amd import capi
    L = capi.lib()
    info = capi.VideoInfo()
    codes = {t[0]: t for t in TABLE.values()}
    for code in range(-1, 0x31):
        rc = L.ojphgpu_video_format_info(code, C.byref(info))
        if code not in codes:
            assert rc == capi.E_INVALID, code
            continue
        _, family, cell, _, lo, hi, min_container, palign, pitch_align, _, _ = codes[code]
        assert rc == capi.OK, code
        got = (info.family, (info.sub_x, info.sub_y), info.min_depth, info.max_depth, info.min_container_bits, info.pointer_align, info.pitch_align)
        assert got == (family, cell, lo, hi, min_container, palign, pitch_align), (code, got)
        assert L.ojphgpu_video_format_info(code, None) == capi.E_INVALID


def test_the_python_table_is_the_table():
    from openjph_amd import pipeline
    assert sorted(pipeline._VIDEO_TABLE) == sorted(TABLE)
    for name, (code, family, _, fixed, lo, hi, _, _, _, unit_bytes, unit_pixels) in TABLE.items():
        assert tuple(pipeline._VIDEO_TABLE[name]) == (code, family, fixed, lo, hi, DEFAULT_DEPTH[name], unit_bytes, unit_pixels), name
    for family, derived in ((422, pipeline.VIDEO_FORMATS), (420, pipeline.VIDEO420_FORMATS), (444, pipeline.VIDEO444_FORMATS)):
        assert derived == {name: (t[0], t[3]) for name, t in TABLE.items() if t[1] == family}
    assert pipeline.VIDEO_FORMATS == {"uyvy": (1, None), "yuy2": (2, None), "v210": (3, None), "y2xx": (4, None), "y210": (4, 10), "y212": (4, 12),
                                      "y216": (4, 16)}
    assert pipeline.VIDEO420_FORMATS == {"nv12": (0x11, None), "nv21": (0x12, None), "p0xx": (0x13, None), "p010": (0x13, 10), "p012": (0x13, 12),
                                         "p016": (0x13, 16)}
    assert pipeline.VIDEO444_FORMATS == {"v410": (0x21, None), "y410": (0x22, None), "r210": (0x23, None), "r10k": (0x24, None), "y4xx": (0x25, None),
                                         "y412": (0x25, 12), "y416": (0x25, 16), "ayuv": (0x26, None), "bgra": (0x27, None), "rgba": (0x28, None),
                                         "argb": (0x29, None)}


def test_layouts_of_both_tables_against_the_arithmetic():
    from openjph_amd import capi, pipeline
    L = capi.lib()
    py = {422: pipeline.video_layout, 420: pipeline.video420_layout, 444: pipeline.video444_layout}
    for name, t in TABLE.items():
        code, family = t[0], t[1]
        for w in (1, 2, 3, 47, 48, 49):
            for h in (1, 2, 3):
                row, off, total = table_layout(name, w, h)
                assert c_layout(L, family, code, w, h) == (capi.OK, (row, off, total)), (name, w, h)
                assert tuple(py[family](name, w, h)) == ((row, off, total) if family == 420 else (row, total)), (name, w, h)
                for other in {422, 420, 444} - {family}:
                    assert c_layout(L, other, code, w, h)[0] == capi.E_INVALID, (name, other)


def test_depth_columns_and_default_depths():
    from openjph_amd import pipeline
    fn = {422: pipeline.video_format, 420: pipeline.video420_format, 444: pipeline.video444_format}
    for name, (code, family, _, fixed, lo, hi, *_) in TABLE.items():
        for depth in range(0, 18):
            if lo <= depth <= hi and fixed in (None, depth):
                assert fn[family](name, depth) == (code, depth), (name, depth)
            else:
                with pytest.raises(ValueError):
                    fn[family](name, depth)
        if DEFAULT_DEPTH[name] is None:
            with pytest.raises(ValueError):
                fn[family](name, None)
        else:
            assert fn[family](name, None) == (code, DEFAULT_DEPTH[name]), name
        for other in {422, 420, 444} - {family}:               # a name of another family
            with pytest.raises(ValueError):
                fn[other](name, fixed if fixed is not None else hi)
