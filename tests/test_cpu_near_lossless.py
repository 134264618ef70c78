"""Near-lossless coding of a reversible frame, the host side (include/ojphgpu.h section 5g): the truncation of the planes
followed by the oracle's synthesis against the reference's decode of every distinct level (tests/golden/near_lossless.json),
and ojphgpu_near_lossless_search over the recorded tables and over hostile ones.  No GPU needed."""
import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd import plan as planmod
from openjph_amd.plan import Plan, make_params
from tests import cpu_pipeline as cp
from tests import near_lossless_cases as nl
from tests import trunc_cases as tc


@pytest.mark.parametrize("name", tc.CODED)
def test_golden_table_is_the_ladder(name):
    plan, levels = nl.case_plan_levels(name)
    g_levels, sse, pae = nl.gold(name)
    assert g_levels == levels and levels[0] == 0
    assert len(sse) == len(pae) == len(levels) and all(len(s) == plan.params.num_comps for s in sse)
    assert not any(sse[0]) and not any(pae[0])


def test_figures_of_the_issue():
    """the peak errors over the first distinct levels, and the PSNR of the first of them"""
    want = {"A": [1, 2, 3, 5, 5, 7, 10], "B": [1, 2, 3, 4, 4, 5, 6], "T": [1, 2, 4, 4, 5, 6, 8]}
    db = {"A": 56.0, "B": 103.3, "T": 79.0}
    for name in tc.CODED:
        _, sse, pae = nl.totals(name)
        assert pae[1:8] == want[name]
        c = tc.CASES[name]
        psnr = 10 * np.log10(c["w"] * c["h"] * c["nc"] * float((1 << c["bd"]) - 1) ** 2 / sse[1])
        assert abs(psnr - db[name]) < 0.05


@pytest.mark.parametrize("name", tc.CODED)
def test_truncated_planes_through_the_synthesis_are_the_decode(name):
    """no block needs coding for a trial: every distinct level, per component"""
    plan, img, arena = tc.case_state(name)
    levels, sse, pae = nl.gold(name)
    for k, j in enumerate(levels):
        dec = cp.inverse_stages(plan, nl.truncated_arena(plan, arena, plan.trunc_table(j)))
        assert nl.errors(img, dec) == list(zip(sse[k], pae[k])), (name, j)


@pytest.mark.parametrize("name", tc.CODED)
def test_search_over_the_recorded_table(name):
    plan, _ = nl.case_plan_levels(name)
    levels, sse, pae = nl.totals(name)
    for T, E in nl.targets(sse, pae):
        nl.run_search(plan, levels, sse, pae, T, E)


def _hostile(U):
    rng = np.random.default_rng(17)
    rise = [0] + [100 * k for k in range(1, U)]
    saw = [0] + [1000 + 400 * (k % 3) - 10 * k for k in range(1, U)]
    rnd = [0] + rng.integers(1, 10 ** 6, U - 1).tolist()
    only0 = [0] + [10 ** 9] * (U - 1)
    const = [0] + [5000] * (U - 1)
    return dict(constant=const, rising=rise, sawtooth=saw, random=rnd, only_level_0=only0)


@pytest.mark.parametrize("kind", ["constant", "rising", "sawtooth", "random", "only_level_0"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_search_over_hostile_tables(name, kind):
    plan, levels = nl.case_plan_levels(name)
    U = len(levels)
    sse = _hostile(U)[kind]
    pae = [0] + [1 + (s * 7919) % 97 for s in sse[1:]]            # peaks that do not follow the sums
    for T, E in nl.targets(sse, pae):
        nl.run_search(plan, levels, sse, pae, T, E)


def test_zero_bounds_and_unbounded():
    plan, levels = nl.case_plan_levels("A")
    _, sse, pae = nl.totals("A")
    for T, E in ((0, None), (None, 0), (0, 5), (10 ** 9, 0)):
        info = nl.run_search(plan, levels, sse, pae, T, E)
        assert info["level"] == 0 and info["passes"] == 0 and info["lossless"] == 1
    info = nl.run_search(plan, levels, sse, pae, 2 ** 64 - 2, None)        # every level meets: the last one
    assert info["level"] == levels[-1] and info["level_coarser"] == 0
    with pytest.raises(capi.OjphError) as e:
        planmod.near_lossless_search(plan, None, None, lambda j: (0, 0))
    assert e.value.code == capi.E_INVALID


def test_an_error_of_the_trial_is_returned():
    plan, _ = nl.case_plan_levels("B")
    cb = capi.ERR_FN(lambda user, level, sse, pae: capi.E_HIP)
    info = capi.NearLosslessInfo()
    assert capi.lib().ojphgpu_near_lossless_search(plan.handle, 100, 2 ** 32 - 1, cb, None, info) == capi.E_HIP


@pytest.mark.parametrize("kw", [
    dict(reversible=False),                                                       # an irreversible component
    dict(reversible=True, coc={1: dict(reversible=False)}),                      # ... through a COC
    dict(reversible=True, coc={1: dict(num_decomps=2)}),                         # components that differ in decompositions
    dict(reversible=True, bit_depth=30),                                          # the 64-bit sample path
    dict(reversible=True, wavelet=2, atk={2: dict(steps=[(1, 2, 2), (-1, 1, 1)])}),                       # ATK
    dict(reversible=True, dfs={1: [1, 2, 3]}, coc={0: dict(dfs=1, num_decomps=3)}),                       # DFS
    dict(reversible=True, bit_depth=20),                                          # deeper than the error sums allow
])
def test_search_refusals(kw):
    kw = dict(dict(bit_depth=8, num_decomps=3), **kw)
    plan = Plan(make_params(64, 48, 3, **kw))
    with pytest.raises(capi.OjphError) as e:
        planmod.near_lossless_search(plan, 1000, None, lambda j: (0, 0))
    assert e.value.code == capi.E_INVALID
