"""The byte-budget search in steps (ojphgpu_rate_stepper_*, include/ojphgpu.h section 5b): what a batch encoder advances one
of per frame over shared launches.  ojphgpu_rate_search_hint is a loop over the same state machine, so a stepper driven by
hand against a size table must ask the indices the callback form asks, in their order, and end with the same info struct and
the same return code.  Driven by the reference's recorded codestream lengths (tests/golden/rate_sizes.json) and hostile
tables.  No GPU needed."""
import ctypes as C
import json
import os

import pytest

from openjph_amd import capi
from openjph_amd.plan import Plan, make_params
from tests import cpu_pipeline as cp
from tests import rate_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "rate_sizes.json")))
NAMES = sorted(rc.CASES)
FIELDS = [k for k, _ in capi.RateInfo._fields_]

_HISTS = {}


def case_hists(name):
    if name not in _HISTS:
        c = rc.CASES[name]
        pl = Plan(make_params(c["w"], c["h"], c["nc"], **rc.case_kwargs(name)))
        img, _ = rc.case_image(name)
        _HISTS[name] = (pl, rc.plan_hists(pl, cp.forward_stages(pl, img)))
    return _HISTS[name]


class Stepper:
    def __init__(self, pl, hist, budget, hint):
        self.lib = capi.lib()
        self.h = C.c_void_p()
        rc0 = self.lib.ojphgpu_rate_stepper_create(pl.handle, None if hist is None else hist.ctypes.data, budget, hint, C.byref(self.h))
        assert rc0 == capi.OK, rc0

    def next(self):
        j = C.c_uint32(0xFFFFFFFF)
        return self.lib.ojphgpu_rate_stepper_next(self.h, C.byref(j)), int(j.value)

    def feed(self, size):
        return self.lib.ojphgpu_rate_stepper_feed(self.h, size)

    def info(self):
        info = capi.RateInfo()
        assert self.lib.ojphgpu_rate_stepper_info(self.h, C.byref(info)) == capi.OK
        return {k: getattr(info, k) for k in FIELDS}

    def close(self):
        self.lib.ojphgpu_rate_stepper_destroy(self.h)
        self.h = None


def by_hand(pl, hist, budget, hint, size):
    """-> (indices asked, info, return code) of a stepper driven against size(j)"""
    st = Stepper(pl, hist, budget, hint)
    asked = []
    try:
        while True:
            code, j = st.next()
            if code != 1:
                return asked, st.info(), code
            assert 0 <= j < rc.GRID
            asked.append(j)
            code = st.feed(size(j))
            if code != capi.OK:
                return asked, st.info(), code
    finally:
        st.close()


def by_callback(pl, hist, budget, hint, size):
    asked = []
    cb = capi.SIZE_FN(lambda user, j: (asked.append(int(j)), size(int(j)))[1])
    info = capi.RateInfo()
    code = capi.lib().ojphgpu_rate_search_hint(pl.handle, None if hist is None else hist.ctypes.data, budget, hint, cb, None, C.byref(info))
    return asked, {k: getattr(info, k) for k in FIELDS}, code


def same(pl, hist, budget, hint, size):
    a = by_hand(pl, hist, budget, hint, size)
    b = by_callback(pl, hist, budget, hint, size)
    assert a == b, (budget, hint, a, b)
    asked, info, code = a
    assert info["passes"] == len(asked) <= 16 and len(set(asked)) == len(asked)
    if asked:
        assert info["first_guess"] == asked[0]
    return a


def answer(tab, budget):
    """the finest index that fits when the table is monotone (None: nothing fits)"""
    fits = [j for j in range(rc.GRID) if tab[j] <= budget]
    return fits[-1] if fits else None


def hints_for(js):
    out = [-1, 0, rc.GRID - 1]
    if js is not None:
        out += [js, js - 1, js + 1, js - 7, js + 7]
    return sorted({h for h in out if -1 <= h < rc.GRID})


@pytest.mark.parametrize("with_hist", [True, False], ids=["model", "no_hist"])
@pytest.mark.parametrize("name", NAMES)
def test_golden_sizes(name, with_hist):
    pl, hist = case_hists(name)
    if not with_hist:
        hist = None
    sizes = GOLD["cases"][name]["sizes"]
    inr, below, above = rc.budgets(name)
    for b in inr + [below, above]:
        js = answer(sizes, b)
        for hint in hints_for(js):
            asked, info, code = same(pl, hist, b, hint, lambda j: sizes[j])
            if b == below:
                assert code == capi.E_BUDGET and 0 in asked
            else:
                assert code == capi.OK and info["grid_index"] == js == GOLD["cases"][name]["budgets"][str(b)]["j"]
                assert info["bytes"] == sizes[js] and info["bytes_finer"] == (sizes[js + 1] if js + 1 < rc.GRID else 0)
                assert info["qstep"] == rc.grid_qstep(js)


def hostile_tables(name):
    sizes = GOLD["cases"][name]["sizes"]
    dip = list(sizes)
    for j in range(100, 110):
        dip[j] = sizes[90]                                   # a table that is not monotone
    tables = [("dip", dip)]
    for at in (0, 1, 57, 239, 240):
        tables.append(("step at %d" % at, [10 if j < at else 10 ** 9 for j in range(rc.GRID)]))
    tables.append(("flat", [1000] * rc.GRID))
    tables.append(("flat and large", [10 ** 9] * rc.GRID))
    return tables


@pytest.mark.parametrize("with_hist", [True, False], ids=["model", "no_hist"])
@pytest.mark.parametrize("name", NAMES)
def test_steps_dips_and_flat_tables(name, with_hist):
    pl, hist = case_hists(name)
    if not with_hist:
        hist = None
    inr, below, above = rc.budgets(name)
    for label, tab in hostile_tables(name):
        for b in inr + [below, above]:
            js = answer(tab, b)
            for hint in hints_for(js):
                asked, info, code = same(pl, hist, b, hint, lambda j: tab[j])
                if tab[0] > b:
                    assert code == capi.E_BUDGET, (label, b, hint)
                else:
                    j = info["grid_index"]                    # the certificate, whatever the table
                    assert code == capi.OK and tab[j] <= b and (j == rc.GRID - 1 or tab[j + 1] > b), (label, b, hint)
                    assert info["bytes"] == tab[j] and info["bytes_finer"] == (tab[j + 1] if j + 1 < rc.GRID else 0)


def test_a_negative_feed_ends_the_stepper_with_that_code():
    pl, hist = case_hists("A")
    sizes = GOLD["cases"]["A"]["sizes"]
    for h in (hist, None):
        for hint in (-1, 17):
            for after in (0, 1, 3):
                for err in (capi.E_HIP, capi.E_OVERFLOW, -(2 ** 40)):
                    seen = set()                              # the first `after` distinct indices answer, whoever asks

                    def size(j):
                        if j not in seen and len(seen) < after:
                            seen.add(j)
                        return sizes[j] if j in seen else err
                    asked, info, code = same(pl, h, 37440, hint, size)
                    assert code == (err if err >= -(2 ** 31) else capi.E_INVALID)
                    assert len(asked) == after + 1 == info["passes"]
    st = Stepper(pl, hist, 37440, -1)
    code, j = st.next()
    assert code == 1
    assert st.feed(capi.E_HIP) == capi.E_HIP
    assert st.next()[0] == capi.E_INVALID and st.feed(1000) == capi.E_INVALID
    st.close()


def test_calls_out_of_turn_are_refused():
    pl, hist = case_hists("B")
    sizes = GOLD["cases"]["B"]["sizes"]
    inr, below, above = rc.budgets("B")
    st = Stepper(pl, hist, inr[1], -1)
    assert st.feed(1000) == capi.E_INVALID                    # nothing handed out yet
    code, j = st.next()
    assert code == 1
    assert st.next()[0] == capi.E_INVALID                     # an index is still out ...
    assert st.feed(sizes[j]) == capi.OK                       # ... and stays out: the search goes on where it was
    assert st.feed(sizes[j]) == capi.E_INVALID
    asked = [j]
    while True:
        code, j = st.next()
        if code != 1:
            break
        asked.append(j)
        assert st.feed(sizes[j]) == capi.OK
    assert code == capi.OK
    want_asked, want_info, want_code = by_callback(pl, hist, inr[1], -1, lambda j: sizes[j])
    assert asked == want_asked and st.info() == want_info and want_code == capi.OK
    assert st.next()[0] == capi.E_INVALID and st.feed(5) == capi.E_INVALID      # after the end
    assert st.info() == want_info
    st.close()
    st = Stepper(pl, None, below, 100)                        # nothing fits: the end, too
    while True:
        code, j = st.next()
        if code != 1:
            break
        assert st.feed(sizes[j]) == capi.OK
    assert code == capi.E_BUDGET and st.next()[0] == capi.E_INVALID
    st.close()


def test_create_refuses_what_the_search_refuses():
    lib = capi.lib()
    pl, hist = case_hists("B")
    h = C.c_void_p()
    for hint in (rc.GRID, -2, 10 ** 6):
        assert lib.ojphgpu_rate_stepper_create(pl.handle, None, 1000, hint, C.byref(h)) == capi.E_INVALID and not h
    rev = Plan(make_params(64, 64, 3, bit_depth=8, reversible=True))
    assert lib.ojphgpu_rate_stepper_create(rev.handle, None, 1000, -1, C.byref(h)) == capi.E_INVALID and not h
    assert lib.ojphgpu_rate_stepper_create(None, None, 1000, -1, C.byref(h)) == capi.E_INVALID
    lib.ojphgpu_rate_stepper_destroy(None)
