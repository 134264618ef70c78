"""The budget stepper under a ceiling (ojphgpu_rate_stepper_create_under, include/ojphgpu.h section 5b): what the capped mode
of section 5c runs below the quality target's own index q once size(q) was measured above the cap.  Driven by the recorded
codestream lengths of the five frames (tests/golden/rate_sizes.json) and the hostile tables of tests/test_cpu_rate_hint.py.
No GPU needed."""
import ctypes as C

import pytest

from openjph_amd import capi
from tests import rate_cases as rc
from tests.test_cpu_rate_hint import GOLD, NAMES, case_hists, hostile_tables


def run_under(pl, hist, budget, hint, ceil, ceil_size, tab):
    """-> (rc of the last _next, info dict, indices asked in order)"""
    lib = capi.lib()
    st = C.c_void_p()
    hp = None if hist is None else hist.ctypes.data
    capi.check(lib.ojphgpu_rate_stepper_create_under(pl.handle, hp, budget, hint, ceil, ceil_size, C.byref(st)), "stepper_create_under")
    asked, j = [], C.c_uint32()
    try:
        while True:
            r = lib.ojphgpu_rate_stepper_next(st, C.byref(j))
            if r != 1:
                break
            asked.append(int(j.value))
            assert len(asked) <= 16, asked
            capi.check(lib.ojphgpu_rate_stepper_feed(st, tab[asked[-1]]), "stepper_feed")
        info = capi.RateInfo()
        capi.check(lib.ojphgpu_rate_stepper_info(st, C.byref(info)), "stepper_info")
    finally:
        lib.ojphgpu_rate_stepper_destroy(st)
    return r, {k: getattr(info, k) for k, _ in capi.RateInfo._fields_}, asked


def check_under(pl, hist, budget, hint, c, tab):
    r, info, asked = run_under(pl, hist, budget, hint, c, tab[c], tab)
    what = (budget, hint, c, asked)
    assert all(j < c for j in asked), what                   # never the ceiling or beyond it
    assert len(set(asked)) == len(asked), what
    assert info["passes"] == len(asked) <= 16, what
    if asked:
        assert info["first_guess"] == asked[0], what
        if hint >= 0:
            assert asked[0] == min(hint, c - 1), what
    if r == capi.E_BUDGET:
        assert tab[0] > budget and 0 in asked, what
        return None
    assert r == capi.OK, what
    j = info["grid_index"]
    assert j < c and j in asked, what
    assert info["bytes"] == tab[j] <= budget, what
    assert tab[j + 1] > budget, what                         # (j + 1 <= c <= 240: it exists; measured by the stepper, or the ceiling)
    assert j + 1 == c or j + 1 in asked, what
    assert info["bytes_finer"] == tab[j + 1], what
    assert info["qstep"] == rc.grid_qstep(j), what
    return j


def ceilings_of(tab, b):
    return [c for c in range(1, rc.GRID) if tab[c] > b]


def product(pl, h, b, tab, want=None):
    """every ceiling c with tab[c] > b under every hint -1 .. 240.  want: the answer every one of them must give (None:
    any index with the certificate) -> searches made"""
    n = 0
    for c in ceilings_of(tab, b):
        for hint in range(-1, rc.GRID):
            got = check_under(pl, h, b, hint, c, tab)
            assert want is None or got == want[0]
            n += 1
    return n


def cross(pl, h, b, tab, want=None):
    """The budgets beside the one of the whole product: every ceiling with the hints that take a different path each (none;
    the answer of the search without a ceiling, or index 0; one at or beyond the ceiling, which is moved below it), and
    every hint -1 .. 240 under the lowest and the highest ceiling there is."""
    ceilings = ceilings_of(tab, b)
    near = max([j for j in range(rc.GRID) if tab[j] <= b], default=0)
    for c in ceilings:
        for hint in (-1, near, rc.GRID - 1):
            got = check_under(pl, h, b, hint, c, tab)
            assert want is None or got == want[0]
    for c in sorted({ceilings[0], ceilings[-1]}) if ceilings else []:
        for hint in range(-1, rc.GRID):
            got = check_under(pl, h, b, hint, c, tab)
            assert want is None or got == want[0]


def answer(sizes, b):
    return [max([j for j in range(rc.GRID) if sizes[j] <= b], default=None)]


@pytest.mark.parametrize("with_hist", [True, False], ids=["model", "no_hist"])
@pytest.mark.parametrize("name", NAMES)
def test_every_ceiling_with_every_hint_over_the_recorded_tables(name, with_hist):
    """The whole product at 0.73 bytes per sample, the budget of the five whose answer lies nearest the middle of the grid:
    about a hundred ceilings above it and as many hints below.  The recorded tables are monotone, so the answer is the one of
    the search without a ceiling."""
    pl, hist = case_hists(name)
    sizes = GOLD["cases"][name]["sizes"]
    b = rc.budgets(name)[0][2]
    n = product(pl, hist if with_hist else None, b, sizes, want=answer(sizes, b))
    print(name, "budget", b, "ceilings", len(ceilings_of(sizes, b)), "searches", n)
    assert n >= 50 * (rc.GRID + 1)


@pytest.mark.parametrize("name", NAMES)
def test_the_other_budgets_of_the_recorded_tables(name):
    """the model's histograms on the other in-range budgets; plain halving on two of them and on the budget nothing fits"""
    pl, hist = case_hists(name)
    sizes = GOLD["cases"][name]["sizes"]
    inr, below, above = rc.budgets(name)
    for h, budgets in ((hist, [inr[0], inr[1], inr[3]]), (None, [inr[1], inr[3], below])):
        for b in budgets:
            cross(pl, h, b, sizes, want=answer(sizes, b))


HOSTILE = [t for t in hostile_tables() if t[0] != "golden"]      # (that one is frame A's recorded table: above)


@pytest.mark.parametrize("with_hist", [True, False], ids=["model", "no_hist"])
@pytest.mark.parametrize("label,tab", HOSTILE, ids=[t[0].replace(" ", "_") for t in HOSTILE])
def test_every_ceiling_with_every_hint_over_hostile_tables(label, tab, with_hist):
    """The whole product at the budget sizes[90] of frame A, the value the dipped table repeats at 100 .. 109: there a
    ceiling can stand inside the dip, at its far edge or beyond it, with the hint on either side of each."""
    pl, hist = case_hists("A")
    b = GOLD["cases"]["A"]["sizes"][90]
    n = product(pl, hist if with_hist else None, b, tab)
    print(label, "ceilings", len(ceilings_of(tab, b)), "searches", n)


@pytest.mark.parametrize("label,tab", hostile_tables(), ids=[t[0].replace(" ", "_") for t in hostile_tables()])
def test_the_other_budgets_of_the_hostile_tables(label, tab):
    pl, hist = case_hists("A")
    for h, budgets in ((None, (5, 1000)), (hist, (37440,))):
        for b in budgets:
            cross(pl, h, b, tab)


def test_no_ceiling_is_the_plain_stepper():
    """ceil_index == 241: the same indices in the same order, the same info and codes as ojphgpu_rate_stepper_create"""
    lib = capi.lib()
    for name in NAMES:
        pl, hist = case_hists(name)
        sizes = GOLD["cases"][name]["sizes"]
        inr, below, above = rc.budgets(name)
        for h in (hist, None):
            for b in inr + [below, above]:
                for hint in (-1, 0, 1, 57, 100, 239, 240):
                    st = C.c_void_p()
                    capi.check(lib.ojphgpu_rate_stepper_create(pl.handle, None if h is None else h.ctypes.data, b, hint, C.byref(st)))
                    plain, j = [], C.c_uint32()
                    while True:
                        r0 = lib.ojphgpu_rate_stepper_next(st, C.byref(j))
                        if r0 != 1:
                            break
                        plain.append(int(j.value))
                        capi.check(lib.ojphgpu_rate_stepper_feed(st, sizes[plain[-1]]))
                    i0 = capi.RateInfo()
                    capi.check(lib.ojphgpu_rate_stepper_info(st, C.byref(i0)))
                    lib.ojphgpu_rate_stepper_destroy(st)
                    r1, i1, asked = run_under(pl, h, b, hint, rc.GRID, 12345, sizes)
                    assert (r1, asked) == (r0, plain)
                    assert all(i1[k] == getattr(i0, k) for k, _ in capi.RateInfo._fields_)


def test_ceilings_that_are_none_are_refused():
    pl, hist = case_hists("B")
    lib = capi.lib()
    for ceil, size, budget in ((0, 10 ** 6, 1000), (rc.GRID + 1, 10 ** 6, 1000), (2 ** 32 - 1, 10 ** 6, 1000), (100, 1000, 1000), (100, 0, 1000),
                               (100, 2 ** 63, 1000)):
        st = C.c_void_p()
        assert lib.ojphgpu_rate_stepper_create_under(pl.handle, None, budget, -1, ceil, size, C.byref(st)) == capi.E_INVALID, (ceil, size)
        assert not st.value
    st = C.c_void_p()
    assert lib.ojphgpu_rate_stepper_create_under(pl.handle, None, 1000, 241, 100, 10 ** 6, C.byref(st)) == capi.E_INVALID
