"""The search of a byte budget started from a guess (ojphgpu_rate_search_hint, include/ojphgpu.h section 5b): what the frame
pipelines call with the previous frame's answer.  Driven by the reference's recorded codestream lengths
(tests/golden/rate_sizes.json) and the hostile tables of tests/test_cpu_rate.py.  No GPU needed.

The hinted trials are the hint, the neighbour its result points to and, when that one points the same way, the index beyond
it; then the search goes on as ojphgpu_rate_search does: led by the model when there are histograms, by halving when there
are none."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd import plan as planmod
from openjph_amd.plan import Plan, make_params
from tests import cpu_pipeline as cp
from tests import rate_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "rate_sizes.json")))
NAMES = sorted(rc.CASES)

_HISTS = {}


def case_hists(name):
    if name not in _HISTS:
        c = rc.CASES[name]
        pl = Plan(make_params(c["w"], c["h"], c["nc"], **rc.case_kwargs(name)))
        img, _ = rc.case_image(name)
        _HISTS[name] = (pl, rc.plan_hists(pl, cp.forward_stages(pl, img)))
    return _HISTS[name]


def certify(info, size, budget):
    j = info["grid_index"]
    assert size(j) <= budget, (j, size(j), budget)
    assert j == rc.GRID - 1 or size(j + 1) > budget, (j, size(j + 1), budget)
    assert info["bytes"] == size(j)
    assert info["bytes_finer"] == (size(j + 1) if j + 1 < rc.GRID else 0)
    assert info["qstep"] == rc.grid_qstep(j)


def search(pl, hist, budget, size, hint):
    asked = []

    def fn(j):
        asked.append(j)
        return size(j)
    try:
        info = planmod.rate_search(pl, hist, budget, fn, hint=hint)
    except capi.OjphError as e:
        info = dict(e.info, error=e.code)
    assert len(set(asked)) == len(asked), "an index was asked twice: %s" % asked
    assert info["passes"] == len(asked) <= 16, asked
    assert info["first_guess"] == asked[0]
    if hint is not None:
        assert asked[0] == hint
    return info, asked


def golden_j(name, budget):
    return GOLD["cases"][name]["budgets"][str(budget)]["j"]


@pytest.mark.parametrize("with_hist", [True, False], ids=["model", "no_hist"])
@pytest.mark.parametrize("name", NAMES)
def test_hint_at_and_beside_the_answer(name, with_hist):
    pl, hist = case_hists(name)
    if not with_hist:
        hist = None
    sizes = GOLD["cases"][name]["sizes"]
    size = lambda j: sizes[j]
    inr, below, above = rc.budgets(name)
    for b in inr + [above]:
        js = golden_j(name, b)
        info, asked = search(pl, hist, b, size, js)
        assert "error" not in info and info["grid_index"] == js
        certify(info, size, b)
        if js == rc.GRID - 1:
            assert info["passes"] == 1 and asked == [js]
        else:
            assert info["passes"] == 2 and asked == [js, js + 1]
        for hint in (js - 1, js + 1):
            if not 0 <= hint < rc.GRID:
                continue
            info, asked = search(pl, hist, b, size, hint)
            assert "error" not in info and info["grid_index"] == js
            certify(info, size, b)
            print(name, b, "hint", hint, "j*", js, "asked", asked)
            assert info["passes"] <= 3, asked
            assert asked == ([js + 1, js] if hint == js + 1 else [js - 1, js, js + 1][:info["passes"]])


@pytest.mark.parametrize("with_hist", [True, False], ids=["model", "no_hist"])
@pytest.mark.parametrize("name", NAMES)
def test_every_hint_finds_the_answer(name, with_hist):
    pl, hist = case_hists(name)
    if not with_hist:
        hist = None
    sizes = GOLD["cases"][name]["sizes"]
    size = lambda j: sizes[j]
    inr, below, above = rc.budgets(name)
    worst = 0
    for b in inr + [above]:
        for hint in range(rc.GRID):
            info, asked = search(pl, hist, b, size, hint)
            assert "error" not in info
            certify(info, size, b)
            assert info["grid_index"] == golden_j(name, b)
            assert info["first_guess"] == hint
            if len(asked) > 1 and rc.GRID > asked[1] >= 0:
                assert asked[1] == (hint + 1 if sizes[hint] <= b else hint - 1)
            worst = max(worst, info["passes"])
    print(name, "most passes over every hint:", worst)
    for hint in (0, 100, 240):
        info, asked = search(pl, hist, below, size, hint)
        assert info.get("error") == capi.E_BUDGET and 0 in asked
        assert info["first_guess"] == hint


def hostile_tables():
    sizes = GOLD["cases"]["A"]["sizes"]
    rng = np.random.default_rng(5)
    dip = list(sizes)
    for j in range(100, 110):
        dip[j] = sizes[90]                                   # a table that is not monotone
    tables = [("golden", sizes), ("dip", dip)]
    for at in (0, 1, 57, 239, 240):
        tables.append(("step at %d" % at, [10 if j < at else 10 ** 9 for j in range(rc.GRID)]))
    tables.append(("flat", [1000] * rc.GRID))
    tables.append(("random", [int(v) for v in rng.integers(1, 10 ** 6, rc.GRID)]))
    return tables


@pytest.mark.parametrize("label,tab", hostile_tables(), ids=[t[0].replace(" ", "_") for t in hostile_tables()])
def test_hostile_inputs_stay_within_the_cap_with_every_hint(label, tab):
    pl, hist = case_hists("A")
    sizes = GOLD["cases"]["A"]["sizes"]
    rng = np.random.default_rng(5)
    hists = [None, np.zeros_like(hist), rng.integers(0, 2 ** 32, hist.shape, dtype=np.uint64).astype(np.uint32),
             np.full_like(hist, 0xFFFFFFFF), hist]
    worst = 0
    for h in hists:
        for budget in (5, 1000, 37440, sizes[90], 10 ** 6, 10 ** 12):
            for hint in range(rc.GRID):
                info, asked = search(pl, h, budget, lambda j: tab[j], hint)
                worst = max(worst, info["passes"])
                if "error" in info:
                    assert info["error"] == capi.E_BUDGET and tab[0] > budget, (label, budget, hint)
                else:
                    certify(info, lambda j: tab[j], budget)
    print("most passes over", label, "with every hint:", worst)


def test_a_failing_size_function_comes_back_as_it_is():
    pl, hist = case_hists("A")
    with pytest.raises(capi.OjphError) as e:
        planmod.rate_search(pl, hist, 1000, lambda j: capi.E_HIP, hint=17)
    assert e.value.code == capi.E_HIP


def test_no_hint_is_the_plain_search():
    lib = capi.lib()
    for name in NAMES:
        pl, hist = case_hists(name)
        sizes = GOLD["cases"][name]["sizes"]
        inr, below, above = rc.budgets(name)
        for h in (hist, None):
            for b in inr + [above, below]:
                plain = []
                cb = capi.SIZE_FN(lambda user, j: (plain.append(int(j)), sizes[j])[1])
                info = capi.RateInfo()
                rc0 = lib.ojphgpu_rate_search(pl.handle, None if h is None else h.ctypes.data, b, cb, None, C.byref(info))
                got, asked = search(pl, h, b, lambda j: sizes[j], None)
                assert asked == plain
                assert got.get("error", capi.OK) == rc0
                assert all(got[k] == getattr(info, k) for k, _ in capi.RateInfo._fields_)
                # ... and so is the C entry point with its "no hint" value
                again = []
                cb2 = capi.SIZE_FN(lambda user, j: (again.append(int(j)), sizes[j])[1])
                info2 = capi.RateInfo()
                rc2 = lib.ojphgpu_rate_search_hint(pl.handle, None if h is None else h.ctypes.data, b, -1, cb2, None, C.byref(info2))
                assert rc2 == rc0 and again == plain


def test_hints_off_the_grid_are_refused():
    pl, hist = case_hists("B")
    for hint in (rc.GRID, rc.GRID + 1, 10 ** 6, -2, -(2 ** 31), 2 ** 31 + 5, 2 ** 32 + 7, -(2 ** 32) + 3):
        asked = []
        with pytest.raises(capi.OjphError) as e:
            planmod.rate_search(pl, hist, 10 ** 5, lambda j: (asked.append(j), 1000)[1], hint=hint)
        assert e.value.code == capi.E_INVALID and not asked, hint
    pl = Plan(make_params(64, 64, 3, bit_depth=8, reversible=True))
    with pytest.raises(capi.OjphError) as e:
        planmod.rate_search(pl, None, 1000, lambda j: 1, hint=5)
    assert e.value.code == capi.E_INVALID
