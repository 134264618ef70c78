"""The chroma stage without a device (include/ojphgpu.h section 7f): pipeline.rechroma_plane / rechroma_frame, the numpy statement
of ojphgpu_frame_rechroma, against a plain double loop and against the two rules it joins (resample_plane at phase 0,
ycc_to_rgb's doubling); and the plan judgement of the pipes' set_video_chroma (ojphgpu_video_chroma_fit)."""
import itertools

import numpy as np
import pytest

from openjph_amd import capi, pipeline
from tests.chroma_cases import CELLS, PAIRS, RGB_NAMES, YCC_FORMATS, plane_loop, plane_shapes

SIZES = [(w, h) for w in range(1, 10) for h in range(1, 8)]   # of the luma plane
# per direction same / halve / double: the eight pairings that are not a copy, the unchanged direction at factor 1
NON_IDENTITY = [(s, d) for s, d in PAIRS if s != d and not (s[0] == d[0] == 2) and not (s[1] == d[1] == 2)]


def test_the_eight_pairings():
    modes = {((d[0] == 2 * s[0]) - (s[0] == 2 * d[0]), (d[1] == 2 * s[1]) - (s[1] == 2 * d[1])) for s, d in NON_IDENTITY}
    assert len(NON_IDENTITY) == 8 and modes == set(itertools.product((-1, 0, 1), repeat=2)) - {(0, 0)}


@pytest.mark.parametrize("s,d", [p for p in PAIRS if p[0] != p[1]], ids=lambda c: "%d%d" % c)
def test_plane_against_a_double_loop(s, d):
    rng = np.random.default_rng(CELLS.index(s) * 4 + CELLS.index(d))
    for w, h in SIZES:
        q = rng.integers(0, 1 << 16, plane_shapes(w, h, s)[1])
        got = pipeline.rechroma_plane(q, s, d, (w, h))
        assert got.dtype == np.int64 and got.shape == plane_shapes(w, h, d)[1]
        assert got.tolist() == plane_loop(q.tolist(), s, d, w, h), (s, d, w, h)


def test_identity_is_a_copy_and_the_frame_keeps_luma():
    rng = np.random.default_rng(5)
    for (w, h), c in itertools.product(SIZES, CELLS):
        planes = [rng.integers(-9, 1 << 12, sh) for sh in plane_shapes(w, h, c)]
        for a, b in zip(pipeline.rechroma_frame(planes, c, c), planes):
            assert np.array_equal(a, b)
        for d in CELLS:
            out = pipeline.rechroma_frame(planes, c, d)
            assert np.array_equal(out[0], planes[0]) and [p.shape for p in out] == plane_shapes(w, h, d)


@pytest.mark.parametrize("fx,fy", [(2, 1), (1, 2), (2, 2)])
def test_halving_is_resample_plane_at_phase_0(fx, fy):
    rng = np.random.default_rng(fx * 10 + fy)
    for w, h in SIZES + [(37, 19)]:
        q = rng.integers(-(1 << 20), 1 << 20, (h, w))
        assert np.array_equal(pipeline.rechroma_plane(q, (1, 1), (fx, fy), (w, h)), pipeline.resample_plane(q, fx, fy))


@pytest.mark.parametrize("fx,fy", [(2, 1), (1, 2), (2, 2)])
def test_doubling_is_the_rule_of_ycc_to_rgb(fx, fy):
    """a constant plane stays that constant; and through ycc_to_rgb with a table that passes Cb on: the same samples"""
    rng = np.random.default_rng(fx * 10 + fy)
    kk = (fx == 2) + (fy == 2)
    passes_cb = pipeline.ColourTable(((0, 1 << 16, 0),) * 3, (0, 0, 0), (0, 0, 0), ((1 << 31) - 1,) * 3, 16)
    for w, h in SIZES + [(37, 19)]:
        shape = plane_shapes(w, h, (fx, fy))[1]
        for v in (0, 1, 777, 65535, -5):
            assert np.array_equal(pipeline.rechroma_plane(np.full(shape, v), (fx, fy), (1, 1), (w, h)), np.full((h, w), v))
        q = rng.integers(0, 1 << 16, shape)
        got = pipeline.rechroma_plane(q, (fx, fy), (1, 1), (w, h))
        assert got.shape == (h, w)
        rgb = pipeline.ycc_to_rgb([np.zeros((h, w), np.int64), q, q], passes_cb, fx, fy)     # (m . v + 2^(15 + kk)) >> (16 + kk), v = Cb's sum << 16
        assert np.array_equal(got, rgb[0]), (w, h, kk)


def test_outputs_stay_between_the_smallest_and_the_largest_input():
    rng = np.random.default_rng(9)
    lo, hi = -2 ** 31, 2 ** 31 - 1
    for (w, h), (s, d) in itertools.product(SIZES, PAIRS):
        shape = plane_shapes(w, h, s)[1]
        for q in (rng.integers(0, 1 << 16, shape), rng.integers(lo, hi + 1, shape), rng.integers(-1000, 3, shape),
                  np.where(rng.integers(0, 2, shape) == 1, hi, lo), np.full(shape, hi), np.full(shape, lo)):
            got = pipeline.rechroma_plane(q, s, d, (w, h))
            assert got.min() >= q.min() and got.max() <= q.max(), (w, h, s, d)


def test_statement_refusals():
    p = np.zeros((2, 2), np.int64)
    for s, d in (((0, 1), (1, 1)), ((1, 1), (3, 1)), ((4, 1), (2, 1)), ((1, 1), (1, 0))):
        with pytest.raises(ValueError):
            pipeline.rechroma_plane(p, s, d)
    with pytest.raises(ValueError):
        pipeline.rechroma_plane(p, (2, 2), (1, 1), (5, 4))          # a 3 x 2 plane, not 2 x 2
    with pytest.raises(ValueError):
        pipeline.rechroma_frame([p, p], (1, 1), (2, 1))
    assert pipeline.rechroma_plane(p, (2, 2), (1, 1)).shape == (4, 4)


# ---- the plan judgement of the pipes' set_video_chroma (ojphgpu_video_chroma_fit): what needs no device
W, H = 66, 34


def _plan(depth=10, rev=True, cell=(1, 1), w=W, h=H, **kw):
    from tests.video_cases import make_plan
    return make_plan(w, h, depth, rev, cell, num_decomps=2, **kw)


def _depth_of(fmt):
    """a depth of the format's column (the one its name fixes, else its default, else the column's top)"""
    _, _, fixed, lo, hi, default, _, _ = pipeline._VIDEO_TABLE[fmt]
    return fixed or default or hi


def _buffer_bytes(fmt, w, h):
    cell = pipeline.video_cell(fmt)
    return (pipeline.video420_layout if cell == (2, 2) else pipeline.video_layout if cell == (2, 1) else pipeline.video444_layout)(fmt, w, h)[-1]


@pytest.mark.parametrize("decoding", [False, True])
@pytest.mark.parametrize("fmt", YCC_FORMATS)
def test_plan_judgement_passes_every_format_on_every_plan(fmt, decoding):
    depth, fcell = _depth_of(fmt), pipeline.video_cell(fmt)
    for pcell, (w, h) in itertools.product(CELLS, ((66, 34), (37, 19), (1, 1))):
        plan = _plan(depth=depth, cell=pcell, w=w, h=h)
        got = pipeline.video_chroma_fit(plan, fmt, 16, decoding)
        wh = w * h
        fc, pc = [-(-w // c[0]) * -(-h // c[1]) for c in (fcell, pcell)]
        f_off, p_off = (0, wh, wh + fc), (0, wh, wh + pc)
        assert (got["w"], got["h"]) == (w, h) and got["bytes"] == _buffer_bytes(fmt, w, h)
        if fcell == pcell:                                      # the plain hand-over: no stage
            assert got["src_cell"] == got["dst_cell"] == pcell and got["src_off"] == got["dst_off"] == p_off
        elif decoding:
            assert (got["src_cell"], got["dst_cell"], got["src_off"], got["dst_off"]) == (pcell, fcell, p_off, f_off)
        else:
            assert (got["src_cell"], got["dst_cell"], got["src_off"], got["dst_off"]) == (fcell, pcell, f_off, p_off)
        assert p_off == tuple(plan.comp_info(c)["frame_off"] for c in range(3))
    # 32-bit containers pass both ways: the stage takes int32, the pack kernels clamp
    pipeline.video_chroma_fit(_plan(depth=depth, cell=(2, 2) if fcell != (2, 2) else (1, 1)), fmt, 32, decoding)
    # an even image offset keeps phase 0 on both sides
    pipeline.video_chroma_fit(_plan(depth=depth, cell=(1, 1) if fcell != (1, 1) else (2, 2), image_offset=(2, 4)), fmt, 16, decoding)


def _refused(plan, fmt, container=16, decoding=False, mode="cosited"):
    with pytest.raises(capi.OjphError) as e:
        pipeline.video_chroma_fit(plan, fmt, container, decoding, mode)
    return e.value.code == capi.E_INVALID


@pytest.mark.parametrize("decoding", [False, True])
def test_plan_judgement_refusals(decoding):
    for fmt in RGB_NAMES:                                       # they hold R, G, B: colour= is their way
        for cell in CELLS:
            assert _refused(_plan(depth=10 if fmt in ("r210", "r10k") else 8, cell=cell), fmt, 16, decoding)
    # a depth outside the format's column, or not the one the name fixes; a container narrower than the format takes or the depth
    for fmt, depth, container in (("uyvy", 10, 16), ("nv12", 10, 16), ("v210", 12, 16), ("v410", 12, 16), ("ayuv", 9, 16), ("y2xx", 8, 16),
                                  ("p0xx", 8, 16), ("y4xx", 8, 16), ("y210", 12, 16), ("p010", 12, 16), ("y416", 12, 16), ("v210", 10, 8),
                                  ("y2xx", 12, 8), ("v210", 17, 32)):
        for cell in CELLS:
            assert _refused(_plan(depth=depth, cell=cell), fmt, container, decoding), (fmt, depth, container, cell)
    for kw in (dict(signs=[False, True, True]), dict(is_signed=True), dict(bit_depths=[10, 8, 8]), dict(bit_depths=[10, 10, 9]), dict(num_comps=4),
               dict(num_comps=1), dict(downsampling=[(1, 1), (4, 1), (4, 1)]), dict(downsampling=[(1, 1), (1, 4), (1, 4)]),
               dict(downsampling=[(1, 1), (2, 1), (1, 1)]), dict(downsampling=[(1, 1), (2, 2), (2, 1)]), dict(downsampling=[(2, 1), (2, 1), (2, 1)])):
        for fmt in ("v210", "v410", "p010"):
            assert _refused(_plan(depth=10, **kw), fmt, 16, decoding), (kw, fmt)
    # an odd image offset in a direction where EITHER side's cell is 2 -- the format's (v210: x, p010: x and y) or the plan's
    for fmt, cell, off, refused in (("v210", (1, 1), (1, 0), True), ("v210", (1, 1), (0, 1), False), ("v210", (2, 2), (0, 1), True),
                                    ("v210", (1, 2), (0, 3), True), ("v410", (2, 1), (1, 0), True), ("v410", (2, 1), (0, 1), False),
                                    ("v410", (1, 2), (0, 1), True), ("v410", (1, 2), (1, 0), False), ("p010", (1, 1), (0, 1), True),
                                    ("p010", (1, 1), (1, 0), True), ("p010", (2, 1), (3, 5), True), ("v210", (2, 1), (1, 0), True),
                                    ("v410", (1, 1), (1, 1), False)):
        plan = _plan(depth=10, cell=cell, image_offset=off)
        if refused:
            assert _refused(plan, fmt, 16, decoding), (fmt, cell, off)
        else:
            pipeline.video_chroma_fit(plan, fmt, 16, decoding)
    # the mode, the plan, the container, the format's code
    L, plan = capi.lib(), _plan(cell=(2, 2))
    assert L.ojphgpu_video_chroma_fit(plan.handle, 16, decoding, 0x03, capi.CHROMA_COSITED, None, None) == capi.OK
    for mode in (0, 2, -1, 7):
        assert L.ojphgpu_video_chroma_fit(plan.handle, 16, decoding, 0x03, mode, None, None) == capi.E_INVALID
    assert L.ojphgpu_video_chroma_fit(None, 16, decoding, 0x03, capi.CHROMA_COSITED, None, None) == capi.E_INVALID
    for container in (0, 12, 64):
        assert L.ojphgpu_video_chroma_fit(plan.handle, container, decoding, 0x03, capi.CHROMA_COSITED, None, None) == capi.E_INVALID
    for code in (0, 0x05, 0x14, 0x20, 0x2A, 0x23, 0x27):
        assert L.ojphgpu_video_chroma_fit(plan.handle, 16, decoding, code, capi.CHROMA_COSITED, None, None) == capi.E_INVALID


def _view_plan(cell, skip, region, w=W, h=H, depth=8):
    """a parsed plan restricted to a view, from a codestream made on the CPU"""
    from openjph_amd.plan import parse_codestream
    from tests import cpu_pipeline as cp
    rng = np.random.default_rng(w + h)
    planes = [rng.integers(0, 1 << depth, sh).astype(np.int32) for sh in plane_shapes(w, h, cell)]
    cs = cp.encode(planes, size=(w, h), bit_depth=depth, reversible=True, num_decomps=2, downsampling=[(1, 1), cell, cell])[0]
    pl = parse_codestream(cs)
    if skip:
        pl.restrict_resolution(*skip)
    if region is not None:
        pl.restrict_region(*region)
    return pl


def test_plan_judgement_of_views():
    """a reduced resolution always passes; a window when its first column / row is even in every direction where either side's
    cell is 2; both together: an origin that is a multiple of 2^(skip + 1) there"""
    for fmt, cell, skip, region, ok in (
            ("uyvy", (2, 2), (1, 1), None, True), ("nv12", (1, 1), (1, 1), None, True), ("ayuv", (2, 1), (2, 2), None, True),
            ("nv12", (2, 1), None, (4, 6, 20, 10), True), ("nv12", (2, 1), None, (4, 5, 20, 10), False), ("nv12", (2, 1), None, (5, 4, 20, 10), False),
            ("uyvy", (2, 2), None, (4, 5, 20, 10), False), ("uyvy", (1, 1), None, (4, 5, 20, 10), True), ("uyvy", (1, 1), None, (5, 4, 20, 10), False),
            ("uyvy", (1, 2), None, (4, 5, 20, 10), False), ("ayuv", (2, 1), None, (5, 4, 20, 10), False), ("ayuv", (2, 1), None, (4, 5, 20, 10), True),
            ("ayuv", (1, 2), None, (5, 4, 20, 10), True),
            ("nv12", (2, 1), (1, 1), (8, 4, 20, 12), True), ("nv12", (2, 1), (1, 1), (8, 6, 20, 12), False), ("nv12", (2, 1), (1, 1), (6, 4, 20, 12), False),
            ("uyvy", (1, 1), (1, 1), (6, 5, 20, 12), False), ("uyvy", (1, 1), (1, 1), (4, 6, 20, 12), True), ("ayuv", (2, 2), (1, 1), (4, 6, 20, 12), False)):
        plan = _view_plan(cell, skip, region)
        if ok:
            got = pipeline.video_chroma_fit(plan, fmt, 16, True)
            assert (got["w"], got["h"]) == (plan.comp_info(0)["w"], plan.comp_info(0)["h"]) and got["dst_cell"] == pipeline.video_cell(fmt)
        else:
            assert _refused(plan, fmt, 16, True), (fmt, cell, skip, region)
