"""A reversible frame under a byte cap, the host side (include/ojphgpu.h section 5f): the ladder of truncation tables in C
against its numpy restatement, the CPU statement of a truncated encode against the reference (its encode at level 0, its
decode at every level) and the recorded digests (tests/golden/trunc.json), and ojphgpu_trunc_search over recorded and
synthetic size functions.  No GPU needed."""
import json
import math
import os

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd import plan as planmod
from openjph_amd.plan import Plan, make_params
from oracle import refbind
from tests import cpu_pipeline as cp
from tests import trunc_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "trunc.json")))["cases"]
needs_ref = pytest.mark.skipif(not refbind.available(), reason="oracle/_ref has not been built")


# ---------------------------------------------------------------------------------------------
# the ladder
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_ladder_is_the_formula(name):
    plan = tc.case_plan(name)
    q, J, tie = tc.ladder_np(name, plan)
    assert tie > 0.01, "a 4 w_b of this plan sits on a rounding tie: C and numpy may disagree by an ulp"
    assert (plan.trunc_weights() == q).all() and plan.trunc_levels == J
    top = plan.bands["K_max"].astype(np.int64) - 1
    assert q.min() == 0 and J == int((4 * top + q).max()) - 2
    last = None
    for j in range(J):
        t = plan.trunc_table(j)
        assert (t == tc.ladder_np(name, plan, j)[3]).all(), j
        assert last is None or (t >= last).all(), j            # never fewer planes dropped at a higher level
        last = t
    assert not plan.trunc_table(0).any()
    assert plan.trunc_table(1).sum() >= 1 and set(np.flatnonzero(plan.trunc_table(1))) == set(np.flatnonzero((q == 0) & (top > 0)))
    assert (plan.trunc_table(J - 1) == top).all()
    assert J < 2 or not (plan.trunc_table(J - 2) == top).all()     # ... and no level is spare at the end
    with pytest.raises(capi.OjphError) as e:
        plan.trunc_table(J)
    assert e.value.code == capi.E_INVALID


def test_ladder_figures_of_the_issue():
    a, b = tc.case_plan("A"), tc.case_plan("B")
    assert a.num_bands == 48 and a.trunc_levels == 58
    assert sorted(set(a.trunc_weights().tolist())) == [0, 1, 2, 4, 5, 6, 8, 9, 12, 13, 16, 17, 20, 24]
    assert b.trunc_levels == 74 and sorted(set(b.trunc_weights().tolist())) == [0, 1, 2, 5, 8, 12]


def test_synthesis_norms():
    """the impulse through the lifting gives the 5/3 synthesis filters' energies: (1/2, 1, 1/2) and (-1/8, -1/4, 3/4, -1/4, -1/8)"""
    assert planmod.trunc_synth_norm(0, False) == 1.0 == planmod.trunc_synth_norm(0, True)
    assert abs(planmod.trunc_synth_norm(1, False) ** 2 - 1.5) < 1e-12
    assert abs(planmod.trunc_synth_norm(1, True) ** 2 - 0.71875) < 1e-12
    lo2 = np.convolve(np.repeat([0.5, 1.0, 0.5], 2) * np.tile([1.0, 0.0], 3), [0.5, 1.0, 0.5])    # low-pass twice, by hand
    assert abs(planmod.trunc_synth_norm(2, False) ** 2 - (lo2 ** 2).sum()) < 1e-12


@pytest.mark.parametrize("kw", [
    dict(reversible=False),                                                       # an irreversible component
    dict(reversible=True, coc={1: dict(reversible=False)}),                      # ... through a COC
    dict(reversible=True, coc={1: dict(num_decomps=2)}),                         # components that differ in decompositions
    dict(reversible=True, bit_depth=30),                                          # the 64-bit sample path
    dict(reversible=True, wavelet=2, atk={2: dict(steps=[(1, 2, 2), (-1, 1, 1)])}),                       # ATK
    dict(reversible=True, dfs={1: [1, 2, 3]}, coc={0: dict(dfs=1, num_decomps=3)}),                       # DFS
])
def test_ladder_refusals(kw):
    kw = dict(dict(bit_depth=8, num_decomps=3), **kw)
    plan = Plan(make_params(64, 48, 3, **kw))
    for f in (lambda: plan.trunc_levels, plan.trunc_weights, lambda: plan.trunc_table(0),
              lambda: planmod.trunc_search(plan, None, 1000, lambda j: 10)):
        with pytest.raises(capi.OjphError) as e:
            f()
        assert e.value.code == capi.E_INVALID


# ---------------------------------------------------------------------------------------------
# the CPU statement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.CODED)
def test_cpu_statement_is_the_golden(name):
    plan, img, _ = tc.case_state(name)
    g = GOLD[name]
    J = plan.trunc_levels
    assert g["levels"] == J
    sizes = [len(tc.cpu_codestream(name, j)) for j in range(J)]
    assert sizes == g["sizes"]
    assert all(a >= b for a, b in zip(sizes, sizes[1:])), "a size grows with the level"
    assert [tc.sha(tc.cpu_codestream(name, j)) for j in range(J)] == g["codestream_sha256"]
    for j in tc.distinct_levels(plan):                          # the oracle pipeline reads every one of them as recorded
        dec, _ = cp.decode(tc.cpu_codestream(name, j))
        assert tc.sha(np.ascontiguousarray(dec, dtype=np.int32).tobytes()) == g["decoded_sha256"][j], j
    dec0, _ = cp.decode(tc.cpu_codestream(name, 0))
    assert (np.asarray(dec0) == img).all()                      # level 0 is lossless
    assert tc.cpu_codestream(name, 0) == cp.encode(img, **tc.CASES[name]["kw"])[0]


def test_cpu_statement_figures_of_the_issue():
    a, b = GOLD["A"]["sizes"], GOLD["B"]["sizes"]
    assert (a[0], a[1], a[10], a[11], len(a)) == (55401, 53418, 31170, 23642, 58)
    assert (b[0], b[1], len(b)) == (15454, 15185, 74)


@needs_ref
@pytest.mark.parametrize("name", tc.CODED)
def test_cpu_statement_against_the_reference(name):
    ref = refbind.Ref()
    plan, img, _ = tc.case_state(name)
    assert ref.encode(img, **tc.CASES[name]["kw"]) == tc.cpu_codestream(name, 0)
    for j in tc.distinct_levels(plan):
        cs = tc.cpu_codestream(name, j)
        want, _ = ref.decode(cs)
        got, _ = cp.decode(cs)
        assert (np.asarray(want) == np.asarray(got)).all(), j
        assert tc.sha(np.ascontiguousarray(want, dtype=np.int32).tobytes()) == GOLD[name]["decoded_sha256"][j]


# ---------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------
def search(plan, hist, cap, size):
    asked = []

    def fn(j):
        asked.append(j)
        return size(j)
    try:
        info = planmod.trunc_search(plan, hist, cap, fn)
    except capi.OjphError as e:
        info = dict(e.info, error=e.code)
    J = plan.trunc_levels
    assert len(set(asked)) == len(asked), "a level was asked twice: %s" % asked
    assert set(asked) <= set(tc.distinct_levels(plan)), "a level that shares its table with the one before was measured"
    assert info["passes"] == len(asked) <= 2 + math.ceil(math.log2(J)), asked
    assert asked[0] == 0 and info["first_guess"] == asked[min(1, len(asked) - 1)]
    return info, asked


def certify(plan, info, size, cap):
    j = info["level"]
    assert "error" not in info
    assert size(j) <= cap and info["bytes"] == size(j)
    assert j == 0 or size(j - 1) > cap
    assert info["bytes_finer"] == (size(j - 1) if j else 0)
    assert info["lossless"] == (1 if j == 0 else 0)
    assert info["max_dropped"] == int(plan.trunc_table(j).max())


def caps_of(sizes):
    d = sorted(set(sizes))
    out = {d[0], d[0] + 1, d[-1], d[-1] - 1, d[-1] + 1, 10 ** 9}
    for a, b in zip(d, d[1:]):
        out |= {a, b - 1, (a + b) // 2}
    return sorted(out)


@pytest.mark.parametrize("name", tc.CODED)
@pytest.mark.parametrize("model", [False, True])
def test_search_over_recorded_sizes(name, model):
    plan, _, arena = tc.case_state(name)
    sizes = GOLD[name]["sizes"]
    hist = tc.int_hist(plan, arena) if model else None
    for cap in caps_of(sizes):
        info, asked = search(plan, hist, cap, lambda j: sizes[j])
        certify(plan, info, lambda j: sizes[j], cap)
        if cap >= sizes[0]:
            assert info["level"] == 0 and asked == [0]          # a frame that fits: lossless, in one pass
    info, asked = search(plan, hist, sizes[-1] - 1, lambda j: sizes[j])
    assert info["error"] == capi.E_BUDGET and asked[-1] == tc.distinct_levels(plan)[-1]


def by_table(plan, values):
    """a size function that is constant over the levels of one table: values[k] for the k-th distinct table"""
    d = tc.distinct_levels(plan)
    group = np.searchsorted(d, np.arange(plan.trunc_levels), side="right") - 1
    return lambda j: int(values[group[j]])


@pytest.mark.parametrize("model", [False, True])
def test_search_over_synthetic_sizes(model):
    plan, _, arena = tc.case_state("A")
    hist = tc.int_hist(plan, arena) if model else None
    U = len(tc.distinct_levels(plan))
    rng = np.random.default_rng(5)
    # plateaus: runs of tables with one size
    plateau = np.repeat(np.arange(U // 4 + 1, 0, -1) * 1000, 4)[:U]
    # a dip: not monotone -- sizes fall, rise again in the middle, and fall
    dip = np.concatenate([np.linspace(9000, 3000, U // 2), np.linspace(7000, 500, U - U // 2)]).astype(np.int64)
    noisy = np.sort(rng.integers(100, 50000, U))[::-1] + rng.integers(-300, 300, U)
    for values in (plateau, dip, noisy):
        size = by_table(plan, values)
        for cap in sorted({int(v) + d for v in values for d in (-1, 0, 1)} | {10 ** 9}):
            info, asked = search(plan, hist, cap, size)
            if "error" in info:
                assert info["error"] == capi.E_BUDGET and size(plan.trunc_levels - 1) > cap
                continue
            j = info["level"]                                   # the certificate, in measured sizes
            assert size(j) <= cap and (j == 0 or size(j - 1) > cap) and j in asked and (j == 0 or info["bytes_finer"] == size(j - 1))
    # all sizes equal
    for cap, level in ((4999, None), (5000, 0), (5001, 0)):
        info, asked = search(plan, hist, cap, lambda j: 5000)
        if level is None:
            assert info["error"] == capi.E_BUDGET
        else:
            assert info["level"] == level and info["lossless"] == 1 and asked == [0]
    # an error of the size function comes back as it is
    with pytest.raises(capi.OjphError) as e:
        planmod.trunc_search(plan, hist, 1000, lambda j: capi.E_HIP)
    assert e.value.code == capi.E_HIP
