"""The resampling recoder without a GPU (include/ojphgpu.h section 5e, "a resampling recode"): the numpy statement of the
filter (pipeline.resample_plane) against values written out by hand and against the canvas rule, the table the recoder
uploads (ojphgpu_recoder_resample_table) for every accepted pair of plans, every refusal, and the contract stated with the
oracle pipeline (tests/resample_cases.py cpu_recode_resampled) -- against the fixture made from the reference
(tests/golden/recode_resample.json) where it exists."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd.codec import resample_table
from openjph_amd.pipeline import fit_frame, resample_frame, resample_plane
from openjph_amd.plan import Plan, make_params, parse_codestream, recode_params
from tests import cpu_pipeline as cp
from tests import recode_cases as rcc
from tests import resample_cases as rsc
from tests.synth import synth_image

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD_PATH = os.path.join(HERE, "golden", "recode_resample.json")
GOLD = json.load(open(GOLD_PATH)) if os.path.exists(GOLD_PATH) else None
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------
# 1. the statement
# ---------------------------------------------------------------------------------------------
def test_values_written_out_by_hand():
    row = np.array([[10, 20, 40, 80, 160]])
    # phase 0: centres 0, 2, 4; the left neighbour of 0 and the right one of 4 are the samples themselves
    assert resample_plane(row, 2, 1).tolist() == [[(10 + 20 + 20 + 2) >> 2, (20 + 80 + 80 + 2) >> 2, (80 + 320 + 160 + 2) >> 2]]
    # phase 1: centres 1, 3
    assert resample_plane(row, 2, 1, px=1).tolist() == [[(10 + 40 + 40 + 2) >> 2, (40 + 160 + 160 + 2) >> 2]]
    col = row.T
    assert resample_plane(col, 1, 2).tolist() == [[13], [45], [140]] and resample_plane(col, 1, 2, py=1).tolist() == [[23], [90]]
    # both ways: one rounding of the sixteenths, not two of the quarters
    q = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 0]])
    assert resample_plane(q, 2, 2).tolist() == [[(9 + 8) >> 4, 0], [0, 0]]           # weights (1 + 2)(1 + 2) on the corner
    q = np.array([[0, 0, 0], [0, 2, 0], [0, 0, 0]])                                   # 2 at (1, 1): weight 1 for every output
    assert resample_plane(q, 2, 2).tolist() == [[0, 0], [0, 0]]                       # (2 + 8) >> 4; two roundings would give 1
    assert resample_plane(q, 2, 1).tolist() == [[0, 0], [1, 1], [0, 0]]
    # negative ties round up, as the fit's shift does
    assert resample_plane(np.array([[-2, 0, 0]]), 2, 1).tolist() == [[(-6 + 2) >> 2, 0]]
    assert resample_plane(np.array([[-1, -1, 0]]), 2, 1).tolist() == [[-1, 0]]       # -3/4 -> -1, -1/4 -> 0
    assert resample_plane(np.arange(12).reshape(3, 4), 1, 1).tolist() == np.arange(12).reshape(3, 4).tolist()
    for bad in ((3, 1, 0, 0), (1, 4, 0, 0), (2, 2, 2, 0), (0, 1, 0, 0)):
        with pytest.raises(ValueError):
            resample_plane(row, *bad)


def test_size_rule_is_the_canvas():
    """a component of XRsiz dx over [X0, X0 + W) halved is the component of XRsiz 2 dx over the same canvas"""
    up = lambda a, b: -(-a // b)
    for x0 in range(9):
        for w in range(1, 12):
            for dx in (1, 2):
                xs0, xs1 = up(x0, dx), up(x0 + w, dx)
                xo0, xo1 = up(x0, 2 * dx), up(x0 + w, 2 * dx)
                ws, px = xs1 - xs0, xs0 & 1
                q = np.zeros((ws, ws), np.int32)
                assert resample_plane(q, 2, 1, px=px).shape == (ws, xo1 - xo0), (x0, w, dx)
                assert resample_plane(q, 1, 2, py=px).shape == (xo1 - xo0, ws), (x0, w, dx)
                assert resample_plane(q, 2, 2, px, px).shape == (xo1 - xo0, xo1 - xo0)
                # and output sample i stands on reference-grid column (xo0 + i) * 2 dx == (xs0 + 2 i + px) * dx
                assert all((xo0 + i) * 2 * dx == (xs0 + 2 * i + px) * dx for i in range(xo1 - xo0))
    assert resample_plane(np.zeros((3, 1), np.int32), 2, 1, px=1).shape == (3, 0)    # an empty output is legal
    assert resample_plane(np.zeros((1, 3), np.int32), 2, 2, py=1).shape == (0, 2)


def test_no_half_sample_shift_and_constants():
    x = np.arange(23)
    ramp = np.tile(8 * x, (9, 1))
    for px in (0, 1):
        got = resample_plane(ramp, 2, 1, px=px)
        i = np.arange(got.shape[1])
        assert np.array_equal(got[:, 1:-1], np.tile(8 * (2 * i + px), (9, 1))[:, 1:-1])
        got = resample_plane(ramp.T, 1, 2, py=px)
        assert np.array_equal(got[1:-1], np.tile(8 * (2 * i + px), (9, 1)).T[1:-1])
        got = resample_plane(ramp, 2, 2, px, px)
        assert np.array_equal(got[:, 1:-1], np.tile(8 * (2 * i + px), (got.shape[0], 1))[:, 1:-1])
    for v in (0, 1, -1, 1023, I32_MAX, I32_MIN):
        q = np.full((7, 10), v, np.int64)
        for fx, fy, px, py in ((2, 1, 0, 0), (1, 2, 0, 1), (2, 2, 1, 0), (2, 2, 1, 1)):
            got = resample_plane(q, fx, fy, px, py)
            assert got.dtype == np.int64 and got.size and (got == v).all()           # 16 * INT32_MAX + 8 needs 64 bits
    planes = [np.ones((4, 6), np.int32), np.full((4, 6), 5, np.int32)]
    got = resample_frame(planes, [(1, 1), (2, 2)])
    assert [q.shape for q in got] == [(4, 6), (2, 3)] and (got[1] == 5).all()
    assert resample_frame(planes, [(2, 1), (1, 2)], [(1, 0), (0, 1)])[0].shape == (4, 3)


# ---------------------------------------------------------------------------------------------
# 2. the table the recoder uploads
# ---------------------------------------------------------------------------------------------
_small = {}


def small_source(downsampling, image_offset=(0, 0), w=37, h=23, bd=8):
    """a small three-component source of the oracle pipeline with a chroma format and an image offset"""
    key = (tuple(downsampling), image_offset, w, h, bd)
    if key not in _small:
        up = lambda a, b: -(-a // b)
        x0, y0 = image_offset
        rng = np.random.default_rng(5)
        planes = [rng.integers(0, 1 << bd, size=(up(y0 + h, dy) - up(y0, dy), up(x0 + w, dx) - up(x0, dx))).astype(np.int32)
                  for dx, dy in downsampling]
        _small[key] = cp.encode(planes, size=(w, h), bit_depth=bd, reversible=True, num_decomps=2, color_transform=False,
                                downsampling=list(downsampling), image_offset=image_offset)[0]
    return _small[key]


def check_table(src, out, want_factors, want_phases):
    tab = resample_table(src, out)
    nc = int(out.params.num_comps)
    assert len(tab) == nc
    assert rsc.factors_and_phases(src, out) == (want_factors, want_phases)
    for c in range(nc):
        a, b, t = src.comp_info(c), out.comp_info(c), tab[c]
        (fx, fy), (px, py) = want_factors[c], want_phases[c]
        assert (int(t["src_first"]), int(t["dst_first"])) == (a["frame_off"], b["frame_off"])
        assert (int(t["src_w"]), int(t["src_h"]), int(t["dst_w"]), int(t["dst_h"])) == (a["w"], a["h"], b["w"], b["h"])
        assert (int(t["fx"]), int(t["fy"]), int(t["px"]), int(t["py"])) == (fx, fy, px, py)
        assert resample_plane(np.zeros((a["h"], a["w"]), np.int8), fx, fy, px, py).shape == (b["h"], b["w"])
        (bs, _), (bo, sg) = src.comp_format(c), out.comp_format(c)
        lo, hi = (-(1 << (bo - 1)), (1 << (bo - 1)) - 1) if sg else (0, (1 << bo) - 1)
        assert (int(t["shift"]), int(t["lo"]), int(t["hi"])) == (bs - bo, lo, hi)
    return tab


Z = (0, 0)


def test_table_444_to_422_and_420():
    cs = small_source([(1, 1)] * 3)
    src = parse_codestream(cs)
    check_table(src, Plan(recode_params(src, downsampling=rsc.S422)), [(1, 1), (2, 1), (2, 1)], [Z, Z, Z])
    tab = check_table(src, Plan(recode_params(src, downsampling=rsc.S420, bit_depth=6)), [(1, 1), (2, 2), (2, 2)], [Z, Z, Z])
    assert [int(t["dst_first"]) for t in tab] == [0, 37 * 23, 37 * 23 + 19 * 12] and int(tab[2]["src_first"]) == 2 * 37 * 23
    # halving every component is legal as well: the rule does not single out chroma
    check_table(src, Plan(recode_params(src, downsampling=[(2, 2)] * 3)), [(2, 2)] * 3, [Z, Z, Z])
    check_table(src, Plan(recode_params(src, downsampling=[(1, 2), (2, 1), (1, 1)])), [(1, 2), (2, 1), (1, 1)], [Z, Z, Z])
    # nothing resampled: the table is the fit's
    tab = check_table(src, Plan(recode_params(src, bit_depth=7)), [(1, 1)] * 3, [Z, Z, Z])
    assert all(int(t["shift"]) == 1 for t in tab)
    # and NONE gives the same table for what ojphgpu_recoder_create takes
    assert resample_table(src, Plan(recode_params(src, bit_depth=7)), None).tobytes() == tab.tobytes()


def test_table_422_to_420():
    src = parse_codestream(small_source(rsc.S422))
    check_table(src, Plan(recode_params(src, downsampling=rsc.S420)), [(1, 1), (1, 2), (1, 2)], [Z, Z, Z])
    check_table(src, Plan(recode_params(src, downsampling=[(1, 1), (4, 1), (4, 2)])), [(1, 1), (2, 1), (2, 2)], [Z, Z, Z])


def test_table_phases_of_an_image_offset():
    src = parse_codestream(small_source([(1, 1)] * 3, image_offset=(3, 5)))
    assert (src.comp_info(1)["x0"], src.comp_info(1)["y0"]) == (3, 5)
    check_table(src, Plan(recode_params(src, downsampling=rsc.S420)), [(1, 1), (2, 2), (2, 2)], [Z, (1, 1), (1, 1)])
    check_table(src, Plan(recode_params(src, downsampling=rsc.S422)), [(1, 1), (2, 1), (2, 1)], [Z, (1, 0), (1, 0)])
    src = parse_codestream(small_source(rsc.S422, image_offset=(3, 5)))       # chroma origin ceil(3 / 2) = 2: phase 0 across
    check_table(src, Plan(recode_params(src, downsampling=[(1, 1), (4, 2), (4, 2)])), [(1, 1), (2, 2), (2, 2)], [Z, (0, 1), (0, 1)])
    src = parse_codestream(small_source([(1, 1)] * 3, image_offset=(2, 4)))
    check_table(src, Plan(recode_params(src, downsampling=rsc.S420)), [(1, 1), (2, 2), (2, 2)], [Z, Z, Z])


def test_table_under_views():
    cs = small_source([(1, 1)] * 3, w=75, h=51)
    half = rcc.view_plan(cs, dict(skip_res=1))
    assert (half.comp_info(0)["w"], half.comp_info(0)["h"]) == (38, 26)
    check_table(half, Plan(recode_params(half, downsampling=rsc.S422)), [(1, 1), (2, 1), (2, 1)], [Z, Z, Z])
    win = rcc.view_plan(cs, dict(region=(10, 6, 41, 33)))
    assert win.comp_info(1)["x0"] == 10                      # the view keeps its place in the source; the output starts at 0
    check_table(win, Plan(recode_params(win, downsampling=rsc.S420)), [(1, 1), (2, 2), (2, 2)], [Z, Z, Z])
    both = rcc.view_plan(cs, dict(skip_res=1, region=(12, 8, 41, 33)))       # a multiple of 2 * 2^1 both ways
    check_table(both, Plan(recode_params(both, downsampling=rsc.S420)), [(1, 1), (2, 2), (2, 2)], [Z, Z, Z])


@pytest.mark.parametrize("case", list(rsc.CASES) + list(rsc.MORE))
def test_table_of_every_case(case):
    c = rsc.CASES.get(case) or rsc.MORE[case]
    src = rcc.view_plan(rsc.source(case), c["view"])
    out = Plan(recode_params(src, **c["out"]))
    f, p = rsc.factors_and_phases(src, out)
    check_table(src, out, f, p)
    assert any(x != (1, 1) for x in f)
    if case == "offsetB":
        assert p == [(1, 1)]


# ---------------------------------------------------------------------------------------------
# 3. refusals (no device is reached: the plans are judged first)
# ---------------------------------------------------------------------------------------------
def table_rc(src, out, resample=capi.RESAMPLE_COSITED, cap=16):
    tab = (capi.ResampleComp * 16)()
    n = C.c_uint32(99)
    rc_ = capi.lib().ojphgpu_recoder_resample_table(src.handle if src is not None else None, out.handle if out is not None else None, resample,
                                                    tab, cap, C.byref(n))
    assert rc_ == capi.OK or n.value == 0
    return rc_


def create_rc(src, out, resample=capi.RESAMPLE_COSITED):
    h = C.c_void_p()
    rc_ = capi.lib().ojphgpu_recoder_create_resampled(src.handle if src is not None else None, out.handle if out is not None else None,
                                                      resample, 0, None, C.byref(h))
    assert not h.value
    return rc_


def refused(src, out, resample=capi.RESAMPLE_COSITED):
    return table_rc(src, out, resample) == capi.E_INVALID and create_rc(src, out, resample) == capi.E_INVALID


def test_refusals_of_the_resampling_rule():
    cs = small_source([(1, 1)] * 3)
    src = parse_codestream(cs)
    ok = Plan(recode_params(src, downsampling=rsc.S420))
    assert table_rc(src, ok) == capi.OK
    assert refused(src, Plan(recode_params(src, downsampling=[(1, 1), (4, 1), (4, 1)])))        # a factor of 4
    assert refused(src, Plan(recode_params(src, downsampling=[(1, 1), (2, 4), (2, 2)])))
    sub = parse_codestream(small_source(rsc.S420))
    assert refused(sub, Plan(recode_params(sub, downsampling=rsc.S422)))                        # upsampling down the rows
    assert refused(sub, Plan(recode_params(sub, downsampling=[(1, 1)] * 3)))
    assert refused(sub, Plan(recode_params(sub, downsampling=[(1, 1), (4, 1), (4, 2)])))        # halved across, doubled down
    # NONE keeps today's meaning: sizes that differ are refused, whatever the filter could do
    assert refused(src, ok, capi.RESAMPLE_NONE)
    assert refused(src, ok, 2) and refused(src, ok, -1)                                          # no such filter
    assert table_rc(src, ok, cap=2) == capi.E_INVALID                                            # a table too short
    # the sizes must be the canvas's: an output one column wider, with the right sub-sampling
    p = recode_params(src, downsampling=rsc.S420)
    wide = make_params(39, 23, 3, bit_depth=8, reversible=True, num_decomps=2, color_transform=False, downsampling=rsc.S420)
    assert Plan(wide).comp_info(1)["w"] == Plan(p).comp_info(1)["w"] + 1 and refused(src, Plan(wide))
    # windows: the origin must be a sample of every OUTPUT component
    big = small_source([(1, 1)] * 3, w=75, h=51)
    for region in ((11, 6, 40, 32), (10, 7, 40, 32)):
        odd = rcc.view_plan(big, dict(region=region))
        assert table_rc(odd, Plan(recode_params(odd))) == capi.OK                                # (fine for a 4:4:4 output)
        assert refused(odd, Plan(recode_params(odd, downsampling=rsc.S420)))
    odd = rcc.view_plan(big, dict(region=(11, 6, 40, 32)))
    assert table_rc(odd, Plan(recode_params(odd, downsampling=[(1, 1), (1, 2), (1, 2)]))) == capi.OK   # x0 odd, halved down only
    odd_k = rcc.view_plan(big, dict(skip_res=1, region=(10, 8, 40, 32)))                         # even, but no multiple of 2 * 2^1
    assert refused(odd_k, Plan(recode_params(odd_k, downsampling=rsc.S422)))
    # a proxy of a source with an odd image offset: the view has no offset left to carry the phase
    off = rcc.view_plan(small_source([(1, 1)] * 3, image_offset=(2, 4), w=75, h=51), dict(skip_res=1))
    assert refused(off, Plan(recode_params(off, downsampling=rsc.S420)))


def test_creation_refusals_through_the_new_entry_point():
    """what tests/test_cpu_recode.py test_creation_refusals lists, asked of ojphgpu_recoder_create_resampled"""
    cs = rcc.cpu_source(("A", False, rcc.SRC_INDEX))
    src = parse_codestream(cs)
    good = recode_params(src, qstep=rcc.Q150)
    for mode in (capi.RESAMPLE_NONE, capi.RESAMPLE_COSITED):
        assert create_rc(None, Plan(good), mode) == capi.E_INVALID and create_rc(src, None, mode) == capi.E_INVALID
        assert refused(Plan(good), Plan(good), mode)                        # a source that is not a parsed plan
        assert refused(src, parse_codestream(cs), mode)                     # an output that is
        wider = make_params(313, 200, 3, bit_depth=12, reversible=False, qstep=rcc.Q150)
        assert refused(src, Plan(wider), mode)                              # another size
        assert refused(src, Plan(make_params(312, 200, 1, bit_depth=12)), mode)                 # another component count
        assert refused(src, Plan(recode_params(src, qstep=rcc.Q150, signs=[False, True, False], color_transform=False)), mode)
        deep = Plan(recode_params(src, reversible=True, bit_depth=32, color_transform=False))   # the 64-bit sample path
        assert refused(src, deep, mode)
        half = rcc.view_plan(cs, dict(skip_res=1))
        assert refused(half, Plan(good), mode)                              # a view against the whole frame's output
        c = rcc.REFUSED["cropEodd"]
        e = rcc.cpu_source(c["source"])
        for view in (c["view"], dict(region=(20, 11, 100, 76)), dict(skip_res=1, region=(22, 12, 100, 76))):
            odd = rcc.view_plan(e, view)
            assert refused(odd, Plan(recode_params(odd, **c["out"])), mode)
    # 4:2:0 out of 4:4:4: refused by the old entry point's rule, accepted by the new one's (judged here by the table alone)
    sub = Plan(recode_params(src, qstep=rcc.Q150, downsampling=rsc.S420, color_transform=False))
    assert refused(src, sub, capi.RESAMPLE_NONE) and table_rc(src, sub) == capi.OK
    # the colour transform over sub-sampled chroma: the output plan itself says no
    with pytest.raises(Exception):
        Plan(recode_params(src, qstep=rcc.Q150, downsampling=rsc.S420))


# ---------------------------------------------------------------------------------------------
# 4. the contract on the oracle pipeline
# ---------------------------------------------------------------------------------------------
def psnr(a, b, peak):
    d = np.concatenate([(np.asarray(x, np.float64) - np.asarray(y, np.float64)).ravel() for x, y in zip(a, b)])
    return 10 * np.log10(peak * peak / max(float((d * d).mean()), 1e-12))


@pytest.mark.parametrize("case", list(rsc.CASES))
def test_cpu_recode_resampled(case):
    c = rsc.CASES[case]
    cs = rsc.source(case)
    G, params, out = rsc.cpu_fitted_resampled(cs, c["view"], c["out"])
    nc = int(params.num_comps)
    ds = c["out"]["downsampling"]
    assert [(out.comp_info(k)["dx"], out.comp_info(k)["dy"]) for k in range(nc)] == ds
    got = rsc.cpu_recode_resampled(cs, c["view"], c["out"])
    back, plan = cp.decode(got)
    assert [(plan.comp_info(k)["dx"], plan.comp_info(k)["dy"]) for k in range(nc)] == ds
    assert [q.shape for q in back] == [q.shape for q in G]
    # the output codes G: what decodes from it is G up to the output's own quantisation -- a base step of 2^(-1 - 150/16)
    # of the range, under one LSB of a 10-bit sample, weighted over three 9/7 levels: above 50 dB with margin
    bo = out.comp_format(0)[0]
    assert psnr(back, G, (1 << bo) - 1) > 50.0
    if GOLD is not None and case in GOLD["cases"]:
        g = GOLD["cases"][case]
        assert (rcc.sha(cs), len(cs)) == (g["source"]["sha256"], g["source"]["len"])
        assert [list(q.shape) for q in G] == g["frame"]["shapes"] and rcc.frame_digest(G) == g["frame"]["sha256"]
        assert (rcc.sha(got), len(got)) == (g["output"]["sha256"], g["output"]["len"])


def test_a_reversible_output_carries_the_resampled_frame_exactly():
    """G = fit(resample(decode)) coded reversibly decodes to G: the statement's frame is what the output holds"""
    img = synth_image(3, 45, 67, 10, seed=3)
    cs = cp.encode(img, bit_depth=10, reversible=True, num_decomps=3, color_transform=False)[0]
    for ds in (rsc.S422, rsc.S420):
        kw = dict(downsampling=ds, bit_depth=8)
        G, _, out = rsc.cpu_fitted_resampled(cs, {}, kw)
        want = fit_frame(resample_frame(list(img), [(dx, dy) for dx, dy in ds]), [10] * 3, [8] * 3, [False] * 3)
        assert all(np.array_equal(a, b) for a, b in zip(G, want))
        back, _ = cp.decode(rsc.cpu_recode_resampled(cs, {}, kw))
        assert all(np.array_equal(a, b) for a, b in zip(back, G))
