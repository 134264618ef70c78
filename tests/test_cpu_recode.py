"""The recoder without a GPU (include/ojphgpu.h section 5e): the fit in numpy against values written out by hand, the output
parameters under every view, the contract stated with the oracle pipeline (tests/recode_cases.py cpu_recode) against the
fixture made from the reference (tests/golden/recode.json), and what creation refuses, as far as plans alone show it."""
import json
import os

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd.pipeline import fit_container, fit_frame
from openjph_amd.plan import Plan, make_params, parse_codestream, recode_params
from tests import rate_cases as rc
from tests import recode_cases as rcc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "recode.json")))
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
_sources = {}


def source(src):
    if src not in _sources:
        _sources[src] = rcc.cpu_source(src)
    return _sources[src]


def fit1(values, bs, bo, signed=False):
    return fit_frame([np.array(values, np.int64)], [bs], [bo], [signed])[0]


# ---------------------------------------------------------------------------------------------
# 1. the fit
# ---------------------------------------------------------------------------------------------
def test_fit_rounds_half_up_at_every_shift():
    for s in range(1, 9):
        half, one = 1 << (s - 1), 1 << s
        v = [0, half - 1, half, half + 1, one - 1, one, one + half - 1, one + half, 5 * one + half]
        want = [0, 0, 1, 1, 1, 1, 1, 2, 6]
        assert fit1(v, 8 + s, 8).tolist() == want, s
        # negative ties go up as well (an arithmetic shift): -0.5 -> 0, -1.5 -> -1, -2.5 -> -2
        v = [-half, -half - 1, -one - half, -one - half - 1, -2 * one - half, -one, -1]
        want = [0, -1, -1, -2, -2, -1, 0]
        assert fit1(v, 8 + s, 8, signed=True).tolist() == want, s


def test_fit_clamps_also_without_a_shift():
    assert fit1([-2, -1, 0, 1, 254, 255, 256, 257], 8, 8).tolist() == [0, 0, 0, 1, 254, 255, 255, 255]
    assert fit1([-130, -129, -128, -127, 126, 127, 128, 129], 8, 8, signed=True).tolist() == [-128, -128, -128, -127, 126, 127, 127, 127]
    assert fit1([-1, 0, 4094, 4095, 4096], 12, 12).tolist() == [0, 0, 4094, 4095, 4095]
    # 16 bits: the container saturates at the depth, a 12-bit component in a 16-bit container at 4095
    assert fit1([65534, 65535, 65536], 16, 16).tolist() == [65534, 65535, 65535]
    # a shift down brings a sample past its range back inside or not: 4096 >> 2 = 1024 is past 10 bits
    assert fit1([4093, 4094, 4095, 4096, 4097, 4098], 12, 10).tolist() == [1023, 1023, 1023, 1023, 1023, 1023]
    assert fit1([4089, 4090], 12, 10).tolist() == [1022, 1023]
    # a shift up: 255 << 2 = 1020, 256 << 2 = 1024 clamped
    assert fit1([-1, 0, 1, 255, 256], 8, 10).tolist() == [0, 0, 4, 1020, 1023]


def test_fit_at_the_ends_of_int32():
    assert fit1([I32_MIN, I32_MAX], 16, 8).tolist() == [0, 255]                        # (v + 128) >> 8 in 64 bits: no wrap
    assert fit1([I32_MIN, I32_MAX], 16, 8, signed=True).tolist() == [-128, 127]
    assert fit1([I32_MIN, I32_MAX], 8, 16).tolist() == [0, 65535]                      # v << 8 in 64 bits
    assert fit1([I32_MIN, I32_MAX], 8, 16, signed=True).tolist() == [-32768, 32767]
    assert fit1([I32_MIN, I32_MAX, I32_MAX - 1], 32, 31).tolist() == [0, 2 ** 30, 2 ** 30 - 1]   # round half up past int32
    assert fit1([I32_MIN, I32_MAX], 24, 24, signed=True).tolist() == [-2 ** 23, 2 ** 23 - 1]
    assert fit1([I32_MIN, I32_MAX], 1, 32, signed=True).tolist() == [I32_MIN, I32_MAX]  # << 31, clamped


def test_fit_containers():
    assert [fit_container(d) for d in ([8], [1, 8], [9], [8, 16], [17], [8, 31])] == [8, 8, 16, 16, 32, 32]
    g = fit_frame([np.zeros((2, 2), np.int32)] * 3, [12, 12, 12], [8, 10, 8], [False, True, False])
    assert [q.dtype for q in g] == [np.uint16, np.int16, np.uint16]
    g = fit_frame([np.zeros((2, 2), np.int32)] * 2, [12, 12], [8, 8], [False, True])
    assert [q.dtype for q in g] == [np.uint8, np.int8]
    assert fit_frame([np.zeros((2, 2), np.int32)], [12], [20], [False])[0].dtype == np.int32


# ---------------------------------------------------------------------------------------------
# 2. the output's parameters
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(rcc.CASES) + list(rcc.REFUSED))
def test_recode_params_under_every_view(case):
    c = rcc.CASES.get(case) or rcc.REFUSED[case]
    cs = source(c["source"])
    src = rcc.view_plan(cs, c["view"])
    p = recode_params(src, **c["out"])
    kw, (w, h) = rcc.out_make_kwargs(case)
    want = make_params(w, h, int(src.params.num_comps), **kw)
    for f in ("width", "height", "num_comps", "bit_depth", "is_signed", "reversible", "num_decomps", "block_w", "block_h", "color_transform",
              "prog_order", "image_x0", "image_y0", "tile_x0", "tile_y0", "tlm"):
        assert getattr(p, f) == getattr(want, f), f            # (a parsed plan names its one tile by its size: the plans tell)
    if "qstep" in c["out"]:
        assert p.qstep == want.qstep
    out, ref = Plan(p), Plan(want)
    nc = int(p.num_comps)
    assert [out.comp_info(k) for k in range(nc)] == [ref.comp_info(k) for k in range(nc)]
    assert [out.comp_format(k) for k in range(nc)] == [ref.comp_format(k) for k in range(nc)]
    assert [(src.comp_info(k)["w"], src.comp_info(k)["h"]) for k in range(nc)] == [(out.comp_info(k)["w"], out.comp_info(k)["h"]) for k in range(nc)]
    assert (out.num_tiles, out.num_bands, out.num_blocks, out.arena_elems) == (ref.num_tiles, ref.num_bands, ref.num_blocks, ref.arena_elems)
    assert np.array_equal(out.blocks[["band", "x0", "y0", "w", "h"]], ref.blocks[["band", "x0", "y0", "w", "h"]])
    if c.get("mode", ("plain",)) == ("plain",):              # (a codestream does not carry its base step: a search brings its own)
        assert np.array_equal(out.bands, ref.bands) and np.array_equal(out.blocks, ref.blocks)
    if c["view"]:
        assert out.num_tiles == 1 and p.tile_w == 0 and p.tile_h == 0


def test_recode_params_overrides():
    cs = source(("C", False, rcc.SRC_INDEX))
    src = parse_codestream(cs)
    p = recode_params(src, tile=(64, 64), num_decomps=2, prog_order="CPRL", tlm=False, bit_depths=[10, 9, 8], tileparts="R")
    assert (p.tile_w, p.tile_h, p.num_decomps, p.prog_order, p.tlm, p.reserved[1]) == (64, 64, 2, capi.PROG_ORDERS["CPRL"], 0, 1)
    assert [Plan(p).comp_format(k)[0] for k in range(3)] == [10, 9, 8]
    assert (p.block_w, p.block_h) == (32, 32)                # (the source's)
    p = recode_params(src, bit_depth=12)
    assert [Plan(p).comp_format(k)[0] for k in range(3)] == [12, 12, 12]
    with pytest.raises(TypeError):
        recode_params(src, width=10)


# ---------------------------------------------------------------------------------------------
# 3. the contract against the fixture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(rcc.CASES))
def test_cpu_recode_is_the_fixture(case):
    c = rcc.CASES[case]
    cs = source(c["source"])
    g = GOLD["cases"][case]
    assert (rcc.sha(cs), len(cs)) == (g["source"]["sha256"], g["source"]["len"])
    G, _, out = rcc.cpu_fitted(cs, c["view"], c["out"])
    assert [list(q.shape) for q in G] == g["frame"]["shapes"]
    assert rcc.frame_digest(G) == g["frame"]["sha256"]
    if c["ref"]:
        got = rcc.cpu_encode_planes(out, G)
        assert (rcc.sha(got), len(got)) == (g["output"]["sha256"], g["output"]["len"])


def test_rewrap_is_the_direct_encode():
    """a reversible source carried through the sample domain: the encode of the original image with the output's parameters"""
    from tests import cpu_pipeline as cp
    img, _ = rc.case_image("D")
    direct = cp.encode(img, **rcc.out_make_kwargs("rewrapD")[0])[0]
    g = GOLD["cases"]["rewrapD"]["output"]
    assert (rcc.sha(direct), len(direct)) == (g["sha256"], g["len"])


def test_the_clamp_has_something_to_do():
    """the fixture's irreversible sources decode to samples past their range: without the clamp G would differ"""
    c = rcc.CASES["cropA"]
    cs = source(c["source"])
    from tests import cpu_pipeline as cp
    dec = cp.decode(cs)[0]
    assert int(dec.max()) > 4095 or int(dec.min()) < 0


# ---------------------------------------------------------------------------------------------
# 4. what creation refuses, through the plans alone (no device is reached: the plans are judged first)
# ---------------------------------------------------------------------------------------------
def create(src, out):
    import ctypes as C
    h = C.c_void_p()
    rc_ = capi.lib().ojphgpu_recoder_create(src.handle if src is not None else None, out.handle if out is not None else None, 0, None, C.byref(h))
    assert not h.value
    return rc_


def test_creation_refusals():
    cs = source(("A", False, rcc.SRC_INDEX))
    src = parse_codestream(cs)
    good = recode_params(src, qstep=rcc.Q150)
    assert create(None, Plan(good)) == capi.E_INVALID and create(src, None) == capi.E_INVALID
    assert create(Plan(good), Plan(good)) == capi.E_INVALID             # a source that is not a parsed plan
    assert create(src, parse_codestream(cs)) == capi.E_INVALID          # an output that is
    wider = make_params(313, 200, 3, bit_depth=12, reversible=False, qstep=rcc.Q150)
    assert create(src, Plan(wider)) == capi.E_INVALID                   # another size: nothing is resampled
    assert create(src, Plan(make_params(312, 200, 1, bit_depth=12))) == capi.E_INVALID           # another component count
    assert create(src, Plan(recode_params(src, qstep=rcc.Q150, signs=[False, True, False], color_transform=False))) == capi.E_INVALID   # signedness changes
    assert create(src, Plan(recode_params(src, qstep=rcc.Q150, downsampling=[(1, 1), (2, 2), (2, 2)], color_transform=False))) == capi.E_INVALID
    # the 64-bit sample path, on the output's side
    deep = Plan(recode_params(src, reversible=True, bit_depth=32, color_transform=False))
    assert any(deep.comp_style(k)["wide"] for k in range(3))
    assert create(src, deep) == capi.E_INVALID
    # a view against the whole frame's output, and a window whose origin is no sample of the chroma
    half = rcc.view_plan(cs, dict(skip_res=1))
    assert create(half, Plan(good)) == capi.E_INVALID
    c = rcc.REFUSED["cropEodd"]
    e = source(c["source"])
    odd = rcc.view_plan(e, c["view"])
    assert create(odd, Plan(recode_params(odd, **c["out"]))) == capi.E_INVALID
    kw, (w, h) = rcc.out_make_kwargs("cropEodd")
    assert create(odd, Plan(make_params(w, h, 3, **kw))) == capi.E_INVALID
    odd_y = rcc.view_plan(e, dict(region=(20, 11, 100, 76)))
    assert create(odd_y, Plan(recode_params(odd_y, **c["out"]))) == capi.E_INVALID
    odd_k = rcc.view_plan(e, dict(skip_res=1, region=(22, 12, 100, 76)))   # even, but no multiple of 2 * 2^1
    assert create(odd_k, Plan(recode_params(odd_k, **c["out"]))) == capi.E_INVALID
