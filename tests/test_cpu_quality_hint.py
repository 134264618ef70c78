"""The search of a quality target started from a guess (ojphgpu_quality_search_hint, include/ojphgpu.h section 5c): what the
encoder pipe calls with the previous frame's answer.  Driven through the C ABI with a ctypes callback by the reference's
recorded error tables (tests/golden/quality_sse.json, total over components) and by hostile tables.  No GPU needed.

The hinted trials are the hint and up to two neighbours on the side its result points to; then the probe of the end that
is still unmeasured (240, then 0) and halving.  SSE is not monotone over the grid, so the only thing asserted about an answer
is the certificate, both sides of it measured."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd import plan as planmod
from tests import quality_cases as qc
from tests import rate_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "quality_sse.json")))
NAMES = sorted(rc.CASES)
CAP = 12                                                     # 3 hinted trials, 1 end probe, ceil(log2(238)) = 8 halvings


def table(name):
    return [sum(s) for s in GOLD["cases"][name]["sse"]]


def targets(name):
    """the four recorded targets, total[j] for every seventh j and total[j] - 1 for every eleventh"""
    tab = table(name)
    ts = [GOLD["cases"][name]["targets"][str(db)]["max_sse"] for db in qc.TARGETS_DB]
    ts += [tab[j] for j in range(0, rc.GRID, 7)]
    ts += [tab[j] - 1 for j in range(0, rc.GRID, 11) if tab[j] > 0]
    return sorted(set(ts))


def search(tab, T, hint):
    """-> (info, or None on E_QUALITY; indices asked); asserts what holds for every table, target and hint"""
    asked = []

    def fn(j):
        assert 0 <= j < rc.GRID
        asked.append(j)
        return tab[j]
    try:
        info = planmod.quality_search(T, fn, hint=hint)
    except capi.OjphError as e:
        assert e.code == capi.E_QUALITY, e
        info, left = None, e.info
    else:
        left = info
    assert len(set(asked)) == len(asked), "an index was asked twice: %s" % asked
    assert left["passes"] == len(asked) <= CAP, asked
    assert left["first_guess"] == asked[0] == (hint if hint >= 0 else rc.GRID - 1)
    if info is None:
        assert tab[-1] > T and (rc.GRID - 1) in asked        # only on a measured SSE(240) > T
        return None, asked
    j = info["grid_index"]
    assert j in qc.certified(tab, T), (j, T, hint)
    assert j in asked and info["sse"] == tab[j] <= T
    if j == 0:
        assert info["sse_coarser"] == 0
    else:
        assert (j - 1) in asked and info["sse_coarser"] == tab[j - 1] > T
    assert info["qstep"] == rc.grid_qstep(j)
    return info, asked


@pytest.mark.parametrize("name", NAMES)
def test_every_hint_over_the_reference_tables(name):
    tab = table(name)
    worst = 0
    for T in targets(name):
        unreachable = tab[-1] > T
        for hint in range(-1, rc.GRID):
            info, asked = search(tab, T, hint)
            assert (info is None) == unreachable, (T, hint)
            worst = max(worst, len(asked))
        for j in qc.certified(tab, T):                       # an unchanged answer: the two trials of its certificate
            info, asked = search(tab, T, j)
            assert info["grid_index"] == j and asked == ([j, j - 1] if j else [0]), (T, j, asked)
    print(name, "most passes over every hint and target:", worst)
    for db in qc.TARGETS_DB:                                 # the recorded answers, from a hint beside them too
        t = GOLD["cases"][name]["targets"][str(db)]
        j = t["certified"][0]
        for hint in (-1, j, j + 1, j - 1):
            if -1 <= hint < rc.GRID:
                info, asked = search(tab, t["max_sse"], hint)
                assert info["grid_index"] == j, (db, hint)   # (the recorded lists are singletons)
                if hint >= 0:
                    assert len(asked) <= 3, asked


def test_no_hint_asks_what_the_plain_search_asks():
    lib = capi.lib()
    for name in NAMES:
        tab = table(name)
        for T in targets(name):
            plain = []

            def fn(user, j, out, plain=plain):
                plain.append(int(j))
                out[0] = tab[j]
                return 0
            info = capi.QualityInfo()
            rc0 = lib.ojphgpu_quality_search(T, capi.SSE_FN(fn), None, C.byref(info))
            asked = []
            try:
                got = planmod.quality_search(T, lambda j: (asked.append(j), tab[j])[1], hint=-1)
                rc1 = capi.OK
            except capi.OjphError as e:
                got, rc1 = e.info, e.code
            assert rc1 == rc0 and asked == plain and asked[0] == rc.GRID - 1
            assert all(got[k] == getattr(info, k) for k, _ in capi.QualityInfo._fields_)
            assert got["first_guess"] == rc.GRID - 1


def hostile_tables():
    rng = np.random.default_rng(9)
    return [("constant", [1000] * rc.GRID), ("rising", [10 * j for j in range(rc.GRID)]),
            ("sawtooth", [(1000 if j % 2 else 10) for j in range(rc.GRID - 1)] + [10]),
            ("meets_only_at_240", [10 ** 9] * (rc.GRID - 1) + [5]), ("meets_nowhere", [10 ** 9] * rc.GRID),
            ("zero", [0] * rc.GRID), ("random", [int(v) for v in rng.integers(0, 10 ** 6, rc.GRID)]),
            ("huge", [2 ** 64 - 1 - j for j in range(rc.GRID)])]


@pytest.mark.parametrize("label,tab", hostile_tables(), ids=[t[0] for t in hostile_tables()])
def test_hostile_tables_stay_within_the_cap_with_every_hint(label, tab):
    worst = 0
    for T in (0, 5, 9, 10, 999, 1000, 1200, 10 ** 6, 10 ** 9 - 1, 10 ** 9, 2 ** 64 - 1):
        for hint in range(-1, rc.GRID):
            info, asked = search(tab, T, hint)
            worst = max(worst, len(asked))
            # (search() holds E_QUALITY to a measured SSE(240) > T; a table that is not monotone may certify an index
            # below a failing 240 when a hint leads there -- without one, 240 is asked first)
            if tab[-1] <= T or hint < 0:
                assert (info is None) == (tab[-1] > T), (label, T, hint)
    print("most passes over", label, "with every hint:", worst)
    if label == "meets_only_at_240":
        for hint in (-1, 0, 100, 238, 239, 240):
            assert search(tab, 5, hint)[0]["grid_index"] == rc.GRID - 1
    if label == "meets_nowhere":
        assert search(tab, 5, 240)[1] == [240] and search(tab, 5, 239)[1] == [239, 240]


def test_a_failing_sse_function_comes_back_as_it_is():
    for hint in (-1, 0, 17, 240):
        with pytest.raises(capi.OjphError) as e:
            planmod.quality_search(1000, lambda j: capi.E_HIP, hint=hint)
        assert e.value.code == capi.E_HIP and e.value.info["passes"] == 1
    asked = []
    with pytest.raises(capi.OjphError) as e:                 # ... from a later trial, too
        planmod.quality_search(1000, lambda j: (asked.append(j), 10 if len(asked) < 3 else capi.E_NOMEM)[1], hint=50)
    assert e.value.code == capi.E_NOMEM and asked == [50, 49, 48]


def test_bad_arguments_are_refused():
    lib = capi.lib()
    asked = []
    for hint in (-2, rc.GRID, rc.GRID + 1, 10 ** 6, -(2 ** 31), 2 ** 31 + 5, 2 ** 32 + 7, -(2 ** 32) + 3):
        with pytest.raises(capi.OjphError) as e:
            planmod.quality_search(1000, lambda j: (asked.append(j), 10)[1], hint=hint)
        assert e.value.code == capi.E_INVALID and not asked, hint
    cb = capi.SSE_FN(lambda user, j, out: (asked.append(int(j)), 0)[1])
    info, first = capi.QualityInfo(), C.c_uint32()
    null_fn = C.cast(None, capi.SSE_FN)
    assert lib.ojphgpu_quality_search_hint(1000, 5, null_fn, None, C.byref(info), C.byref(first)) == capi.E_INVALID
    assert lib.ojphgpu_quality_search_hint(1000, 5, cb, None, None, C.byref(first)) == capi.E_INVALID
    assert lib.ojphgpu_quality_search_hint(1000, 5, cb, None, C.byref(info), None) == capi.E_INVALID
    assert not asked
    assert lib.ojphgpu_quality_search_hint(1000, 5, cb, None, C.byref(info), C.byref(first)) == capi.OK
    assert asked[0] == 5 and first.value == 5
