"""Encoding to a byte budget, the host side (include/ojphgpu.h section 5b): the grid of base steps and ojphgpu_rate_search,
driven by the reference's own codestream lengths (tests/golden/rate_sizes.json, written by tests/golden/make_rate_golden.py)
and by histograms taken with numpy over the oracle's sub-band planes.  No GPU needed."""
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


def case_plan(name, qstep=-1.0):
    c = rc.CASES[name]
    return Plan(make_params(c["w"], c["h"], c["nc"], **rc.case_kwargs(name, qstep)))


_HISTS = {}


def case_hists(name):
    if name not in _HISTS:
        pl = case_plan(name)
        img, _ = rc.case_image(name)
        _HISTS[name] = (pl, rc.plan_hists(pl, cp.forward_stages(pl, img)))
    return _HISTS[name]


def certify(info, size, budget):
    """the contract of a budgeted encode, whatever search found the index"""
    j = info["grid_index"]
    assert size(j) <= budget, (j, size(j), budget)
    assert j == rc.GRID - 1 or size(j + 1) > budget, (j, size(j + 1), budget)
    assert info["bytes"] == size(j)
    assert info["bytes_finer"] == (size(j + 1) if j + 1 < rc.GRID else 0)
    assert info["qstep"] == rc.grid_qstep(j)


def search(pl, hist, budget, size):
    asked = []

    def fn(j):
        asked.append(j)
        return size(j)
    try:
        info = planmod.rate_search(pl, hist, budget, fn)
    except capi.OjphError as e:
        info = dict(e.info, error=e.code)
    assert len(set(asked)) == len(asked), "an index was asked twice: %s" % asked
    assert info["passes"] == len(asked) <= 16, asked
    assert info["first_guess"] == asked[0]
    return info, asked


def test_grid_is_the_formula_bit_for_bit():
    q = [planmod.rate_grid_qstep(j) for j in range(rc.GRID)]
    assert capi.RATE_GRID == rc.GRID == 241 and capi.STATS_BINS == rc.BINS == 80
    for j in range(rc.GRID):
        assert np.float32(q[j]).tobytes() == np.float32(2.0 ** (-1.0 - j / 16.0)).tobytes(), j
        assert q[j] == rc.grid_qstep(j)
    assert all(q[j] > q[j + 1] for j in range(rc.GRID - 1))
    assert q[0] == 0.5 and q[240] == 2.0 ** -16
    with pytest.raises(capi.OjphError):
        planmod.rate_grid_qstep(rc.GRID)


def test_golden_table_is_what_the_issue_measured():
    for name in NAMES:
        sizes = GOLD["cases"][name]["sizes"]
        assert len(sizes) == rc.GRID and all(a <= b for a, b in zip(sizes, sizes[1:]))
        inr, below, above = rc.budgets(name)
        assert below < sizes[0] and sizes[-1] < above and all(sizes[0] < b < sizes[-1] for b in inr)


@pytest.mark.parametrize("name", NAMES)
def test_search_against_the_reference_lengths(name):
    pl, hist = case_hists(name)
    sizes = GOLD["cases"][name]["sizes"]
    inr, below, above = rc.budgets(name)
    for b in inr + [above]:
        info, asked = search(pl, hist, b, lambda j: sizes[j])
        assert "error" not in info
        certify(info, lambda j: sizes[j], b)
        assert info["grid_index"] == GOLD["cases"][name]["budgets"][str(b)]["j"]
    info, asked = search(pl, hist, above, lambda j: sizes[j])
    assert info["grid_index"] == rc.GRID - 1 and info["bytes_finer"] == 0
    info, asked = search(pl, hist, below, lambda j: sizes[j])
    assert info.get("error") == capi.E_BUDGET and 0 in asked


def test_search_over_the_oracle_pipeline():
    """size_fn = the CPU model of the whole encoder at qstep(j): the lengths it gives are the reference's"""
    name = "B"
    pl, hist = case_hists(name)
    img, _ = rc.case_image(name)
    sizes = GOLD["cases"][name]["sizes"]
    budget = rc.budgets(name)[0][1]
    seen = {}

    def size(j):
        if j not in seen:
            seen[j] = len(cp.encode(img, **rc.case_kwargs(name, rc.grid_qstep(j)))[0])
        return seen[j]
    info, asked = search(pl, hist, budget, size)
    certify(info, size, budget)
    assert all(seen[j] == sizes[j] for j in seen)


def test_search_over_the_live_reference():
    """where the reference has been built: size_fn = its generic build, encoding"""
    from oracle import refbind
    if not refbind.available(generic=True):
        return                                              # (the golden table above is the same reference, recorded)
    ref = refbind.Ref(generic=True)
    for name in NAMES:
        pl, hist = case_hists(name)
        img, size_wh = rc.case_image(name)
        budget = rc.budgets(name)[0][2]
        seen = {}

        def size(j):
            if j not in seen:
                seen[j] = len(ref.encode(img, size=size_wh if isinstance(img, list) else None, **rc.case_kwargs(name, rc.grid_qstep(j))))
            return seen[j]
        info, asked = search(pl, hist, budget, size)
        certify(info, size, budget)
        assert all(seen[j] == GOLD["cases"][name]["sizes"][j] for j in seen)


def test_hostile_inputs_stay_within_the_cap():
    pl, hist = case_hists("A")
    sizes = GOLD["cases"]["A"]["sizes"]
    rng = np.random.default_rng(5)
    hists = [None, np.zeros_like(hist), rng.integers(0, 2 ** 32, hist.shape, dtype=np.uint64).astype(np.uint32),
             np.full_like(hist, 0xFFFFFFFF), hist]
    dip = list(sizes)
    for j in range(100, 110):
        dip[j] = sizes[90]                                   # a table that is not monotone
    tables = [("golden", sizes), ("dip", dip)]
    for at in (0, 1, 57, 239, 240):
        tables.append(("step at %d" % at, [10 if j < at else 10 ** 9 for j in range(rc.GRID)]))
    tables.append(("flat", [1000] * rc.GRID))
    tables.append(("random", [int(v) for v in rng.integers(1, 10 ** 6, rc.GRID)]))
    worst = 0
    for h in hists:
        for label, tab in tables:
            for budget in (5, 1000, 37440, sizes[90], 10 ** 6, 10 ** 12):
                info, asked = search(pl, h, budget, lambda j: tab[j])
                worst = max(worst, info["passes"])
                if "error" in info:
                    assert info["error"] == capi.E_BUDGET and tab[0] > budget, (label, budget)
                else:
                    certify(info, lambda j: tab[j], budget)
    print("most passes over the hostile inputs:", worst)
    # a size function that fails: its value comes back as it is
    with pytest.raises(capi.OjphError) as e:
        planmod.rate_search(pl, hist, 1000, lambda j: capi.E_HIP)
    assert e.value.code == capi.E_HIP


def test_fewer_passes_than_bisection():
    total = bis = n = 0
    for name in NAMES:
        pl, hist = case_hists(name)
        sizes = GOLD["cases"][name]["sizes"]
        pred = planmod.rate_predict(pl, hist)
        for b in rc.budgets(name)[0]:
            info, asked = search(pl, hist, b, lambda j: sizes[j])
            jb, nb = rc.bisect_passes(lambda j: sizes[j], b)
            assert jb == info["grid_index"]
            total += info["passes"]; bis += nb; n += 1
            print("%s budget %7d: j* %3d first guess %3d passes %2d (bisection %2d), model / true at j* %.2f"
                  % (name, b, info["grid_index"], info["first_guess"], info["passes"], nb, pred[jb] / sizes[jb]))
    print("passes: %d over %d searches, mean %.2f; bisection %d, mean %.2f" % (total, n, total / n, bis, bis / n))
    assert total < bis


def test_search_refuses_what_has_no_base_step():
    for kw in (dict(reversible=True), dict(reversible=False, qfactor=85), dict(reversible=False, coc={1: dict(reversible=True)}),
               dict(reversible=False, qfactors={0: ("Y", 80)})):
        pl = Plan(make_params(64, 64, 3, bit_depth=8, **kw))
        with pytest.raises(capi.OjphError) as e:
            planmod.rate_search(pl, None, 1000, lambda j: 1)
        assert e.value.code == capi.E_INVALID, kw
