"""The transcoder's host side (include/ojphgpu.h section 5d; no GPU needed): the oracle statement of the contract
(tests/transcode_cases.py cpu_transcode) against the fixture made from the reference (tests/golden/transcode.json), and
ojphgpu_plan_create_transcode -- what it accepts and every item it refuses."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd import plan as planmod
from openjph_amd.plan import Plan, make_params, parse_codestream
from tests import cpu_pipeline as cp
from tests import rate_cases as rc
from tests import transcode_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "transcode.json")))
IDS = [tc.case_id(n, r) for n, r in tc.CASES]
_sources = {}


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def source(name, rev):
    """(codestream, parsed plan, the planes its blocks decode to) of a case, made once"""
    key = tc.case_id(name, rev)
    if key not in _sources:
        cs = tc.cpu_encode(name, tc.src_kwargs(name, rev))
        _sources[key] = (cs,) + tc.cpu_source_planes(cs)
    return _sources[key]


def refused(src, params):
    h = C.c_void_p()
    rc_ = capi.lib().ojphgpu_plan_create_transcode(src.handle, C.byref(params), C.byref(h))
    assert (rc_ == capi.OK) == bool(h.value), "a plan is handed out exactly on success"
    if h.value:
        capi.lib().ojphgpu_plan_destroy(h)
    return rc_ == capi.E_INVALID


# ---------------------------------------------------------------------------------------------
# the helper and the fixture (these pass without the feature: they pin what the feature is tested against)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rev", tc.CASES, ids=IDS)
def test_fixture_is_cpu_transcode(name, rev):
    g = GOLD["cases"][tc.case_id(name, rev)]
    cs, _, arena = source(name, rev)
    assert (sha(cs), len(cs)) == (g["source"]["sha256"], g["source"]["len"])     # the reference's source codestream
    assert sorted(g["targets"]) == sorted(tc.targets(rev))
    for tg, (_, _, identity) in tc.targets(rev).items():
        kw = tc.out_kwargs(name, rev, tg)
        got = tc.cpu_transcode_planes(arena, tc.case_params(name, kw))
        assert (sha(got), len(got)) == (g["targets"][tg]["sha256"], g["targets"][tg]["len"]), tg
        assert g["targets"][tg]["identity"] == identity
        if identity:                                         # ... which the fixture took from the reference's direct encode
            assert got == tc.cpu_encode(name, kw), tg
        else:
            assert got != tc.cpu_encode(name, kw), tg


@pytest.mark.parametrize("name", tc.IRV)
def test_fixture_budgets(name):
    g = GOLD["cases"][tc.case_id(name, False)]
    _, _, arena = source(name, False)
    inr, below, above = rc.budgets(name)
    assert sorted(g["budgets"]) == sorted(str(b) for b in inr) and len(g["sizes"]) == rc.GRID
    assert below < g["sizes"][0] and above > max(g["sizes"])
    for b in inr:
        e = g["budgets"][str(b)]
        j = e["j"]
        assert e["bytes"] == g["sizes"][j] <= b < g["sizes"][j + 1] == e["bytes_finer"]
        for k in (j, j + 1):
            kw = tc.out_kwargs(name, False, "frac", rc.grid_qstep(k))
            assert len(tc.cpu_transcode_planes(arena, tc.case_params(name, kw))) == g["sizes"][k]


# ---------------------------------------------------------------------------------------------
# ojphgpu_plan_create_transcode
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rev", tc.CASES, ids=IDS)
def test_plan_accepts_every_target(name, rev):
    _, src, _ = source(name, rev)
    assert src.params.qstep == 0                             # the base step is not in a codestream
    for tg in tc.targets(rev):
        p = planmod.transcode_params(src, **tc.transcode_kwargs(rev, tg))
        got = planmod.transcode_plan(src, p)
        want = Plan(tc.case_params(name, tc.out_kwargs(name, rev, tg)))
        assert got.arena_elems == want.arena_elems == src.arena_elems
        for table in ("bands", "blocks", "levels"):
            assert np.array_equal(getattr(got, table), getattr(want, table)), (tg, table)
        assert (got.num_precincts, got.parts_per_tile) == (want.num_precincts, want.parts_per_tile)
        for k in ("plane_off", "pitch", "x0", "y0", "w", "h"):
            assert np.array_equal(got.bands[k], src.bands[k]), (tg, k)
    # everything that may change, at once
    p = planmod.transcode_params(src, qstep=None if rev else 0.01, block=(16, 16), prog_order="LRCP", precincts=[(64, 64), (128, 128)],
                                 tlm=True, tileparts="R")
    got = planmod.transcode_plan(src, p)
    assert got.parts_per_tile > 1 and got.num_precincts >= src.num_precincts and got.num_blocks > src.num_blocks
    assert got.params.tlm == 1 and got.params.prog_order == capi.PROG_ORDERS["LRCP"] and got.params.precinct_exps[1] == 0x77
    # an irreversible output without a step is a plan (for a transcoder with a budget)
    if not rev:
        planmod.transcode_plan(src, planmod.transcode_params(src, block=(32, 32)))


def _set(field, value, index=None):
    def f(p):
        if index is None:
            setattr(p, field, value)
        else:
            getattr(p, field)[index] = value
    return f


def _coc(p):
    p.coc[0].rank = 1; p.coc[0].num_decomps = 2; p.coc[0].log_block_w = p.coc[0].log_block_h = 5


OTHER_DIFFERENCES = {
    "width": _set("width", 311), "height": _set("height", 201), "image_offset": _set("image_x0", 1), "tile_offset": _set("tile_y0", 1),
    "tile_w": _set("tile_w", 128), "tile_h": _set("tile_h", 64), "components": _set("num_comps", 2), "depth": _set("bit_depth", 11),
    "comp_depth": _set("comp_depth", 10, 1), "sign": _set("is_signed", 1), "comp_sign": _set("comp_sign", 2, 2),
    "sub_sampling": _set("comp_dx", 2, 1), "wavelet": _set("reversible", 1), "decompositions": _set("num_decomps", 3),
    "colour_transform": _set("color_transform", 0), "nlt": _set("nlt_default", 1), "coc": _coc, "causal": _set("reserved", 1, 0),
    "qfactor": _set("reserved", 50, 2), "comp_qfactor": _set("qcc_qfactor", 50, 0), "atk_wavelet": _set("wavelet", 2),
}


@pytest.mark.parametrize("what", sorted(OTHER_DIFFERENCES))
def test_plan_refuses_any_other_difference(what):
    _, src, _ = source("A", False)
    p = planmod.transcode_params(src, qstep=0.01, block=(32, 32))
    assert not refused(src, p)
    OTHER_DIFFERENCES[what](p)
    assert refused(src, p), what
    with pytest.raises(capi.OjphError) as ei:
        planmod.transcode_plan(src, p)
    assert ei.value.code == capi.E_INVALID


def test_plan_refuses_a_source_that_was_not_parsed():
    kw = tc.src_kwargs("B", False)
    built = Plan(tc.case_params("B", kw))
    assert refused(built, planmod.transcode_params(built, qstep=0.01))


def test_plan_refuses_a_restricted_source():
    cs, _, _ = source("A", False)
    for restrict in (lambda pl: pl.restrict_resolution(1), lambda pl: pl.restrict_resolution(1, 0), lambda pl: pl.restrict_region(8, 8, 100, 60)):
        src = parse_codestream(cs)
        p = planmod.transcode_params(src, qstep=0.01)
        assert not refused(src, p)
        restrict(src)
        assert refused(src, planmod.transcode_params(src, qstep=0.01))
        assert refused(src, p)


@pytest.mark.parametrize("kw", [dict(bit_depth=8, wavelet=2, atk={2: dict(steps=[(1, 2, 2), (-1, 1, 1)])}),
                                dict(bit_depth=8, num_comps=2, coc={1: dict(reversible=True, dfs=0, block=(32, 32))}, dfs={0: [1, 2, 3, 1, 0]})],
                         ids=["atk", "dfs"])
def test_plan_refuses_part2(kw):
    nc = kw.pop("num_comps", 1)
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (nc, 96, 130)).astype(np.int32)
    cs = cp.encode(img, **kw)[0]
    src = parse_codestream(cs)
    assert any(src.comp_style(c)["general"] for c in range(nc))
    assert refused(src, planmod.transcode_params(src, block=(32, 32), qstep=0.01))


def test_plan_refuses_the_64_bit_sample_path():
    rng = np.random.default_rng(6)
    img = rng.integers(0, 1 << 31, (1, 48, 70)).astype(np.int64).astype(np.int32)
    cs = cp.encode(img, bit_depth=32, reversible=True, num_decomps=2)[0]
    src = parse_codestream(cs)
    assert src.comp_style(0)["wide"]
    assert refused(src, planmod.transcode_params(src, block=(32, 32)))


def test_plan_refuses_a_step_for_a_reversible_output():
    _, src, _ = source("D", True)
    assert not refused(src, planmod.transcode_params(src, block=(32, 32)))
    assert refused(src, planmod.transcode_params(src, block=(32, 32), qstep=0.01))


def test_plan_refuses_a_reversible_source_with_more_guard_bits():
    """a foreign source may carry more guard bits than this library writes: its bands' K_max is then above the output's"""
    cs, src, _ = source("D", True)
    raw = bytearray(cs)
    at = raw.index(b"\xff\x5c")                              # QCD: marker, Lqcd, Sqcd = guard bits << 5 | style
    assert at < 200 and raw[at + 4] >> 5 == 1
    raw[at + 4] = (2 << 5) | (raw[at + 4] & 0x1F)
    more = parse_codestream(bytes(raw))
    assert np.array_equal(more.bands["K_max"], src.bands["K_max"] + 1)
    assert refused(more, planmod.transcode_params(more, block=(32, 32)))


def test_the_new_symbols_are_bound_and_exported():
    names = ["ojphgpu_plan_create_transcode"] + ["ojphgpu_transcoder_" + s for s in
                                                 ("create", "set_budget", "submit", "finish", "rate_info", "timing", "destroy")]
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "ojphgpu.h")).read()
    L = C.CDLL(capi.LIB_PATH)
    for n in names:
        assert n in capi.SIGNATURES and hasattr(L, n) and n + "(" in hdr, n
