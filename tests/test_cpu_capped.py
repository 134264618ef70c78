"""A quality target under a byte cap, host side (ojphgpu_capped_search, include/ojphgpu.h section 5c): the search over
table-backed callbacks -- SSE(j) from tests/golden/quality_sse.json, size(j) from tests/golden/rate_sizes.json, both measured
on the reference for the five frames of tests/rate_cases.py -- and over hostile tables.  What is checked is the predicate of
the contract (tests/capped_cases.py: answers, check_info), not one search order.  No GPU needed."""
import pytest

from openjph_amd import capi
from openjph_amd import plan as planmod
from tests import capped_cases as cc
from tests import quality_cases as qc
from tests import rate_cases as rc
from tests.test_cpu_rate_hint import NAMES, case_hists


def search(pl, hist, T, B, total, sizes, hint_q=-1, hint_b=-1):
    """-> (info dict, with "error" after a failure; indices asked of sse_fn; of size_fn; calls of hist_fn)"""
    asked_q, asked_b, hists = [], [], []

    def sse(j):
        asked_q.append(j)
        return total[j]

    def size(j):
        asked_b.append(j)
        return sizes[j]

    def hist_fn():
        hists.append(1)
        return hist
    try:
        info = planmod.capped_search(pl, T, B, sse, size, hist_fn, hint_q=hint_q, hint_b=hint_b)
    except capi.OjphError as e:
        info = dict(e.info, error=e.code)
    what = (T, B, hint_q, hint_b, asked_q, asked_b)
    assert len(set(asked_q)) == len(asked_q) and len(set(asked_b)) == len(asked_b), "an index was asked twice: %s" % (what,)
    assert info["quality_passes"] == len(asked_q) <= 12 + 1, what
    assert info["rate_passes"] == len(asked_b) <= 1 + 16, what
    assert len(hists) <= 1, what
    assert info.get("error") in (None, capi.E_BUDGET), what    # never E_QUALITY: the cap wins
    if asked_q:
        assert info["first_guess_q"] == asked_q[0] and (hint_q < 0 or asked_q[0] == hint_q), what
    if "error" not in info:
        if info["outcome"] == cc.MET:
            assert not hists and len(asked_b) == 1, what       # the statistics are for a cap that binds
        assert info["grid_index"] in asked_b and info["grid_index"] in asked_q, what
        cc.check_info(info, total, sizes, T, B)
    return info, asked_q, asked_b, len(hists)


def targets(name, total):
    beyond = total[rc.GRID - 1] - 1                            # out of reach for every step (where the finest step loses anything)
    return [qc.psnr_to_sse(name, db) for db in qc.TARGETS_DB] + [0] + ([beyond] if beyond > 0 else [])


@pytest.mark.parametrize("name", NAMES)
def test_recorded_tables_every_target_budget_and_hint(name):
    pl, hist = case_hists(name)
    total, sizes = cc.tables(name)
    inr, below, above = rc.budgets(name)
    seen = set()
    for T in targets(name, total):
        qs = qc.certified(total, T)
        q = qs[0] if qs else rc.GRID - 1
        for B in inr + [below, above]:
            allowed = cc.answers(total, sizes, T, B)
            jb = max([j for j in range(rc.GRID) if sizes[j] <= B], default=0)
            hq = sorted({-1, 0, 240} | {h for h in (q - 1, q, q + 1) if 0 <= h < rc.GRID})
            hb = sorted({-1, 0, 240} | {h for h in (jb - 1, jb, jb + 1) if 0 <= h < rc.GRID})
            for hint_q in hq:
                for hint_b in hb:
                    info, aq, ab, nh = search(pl, hist if (hint_q + hint_b) % 2 else None, T, B, total, sizes, hint_q, hint_b)
                    if sizes[0] > B:
                        assert info.get("error") == capi.E_BUDGET, (T, B, hint_q, hint_b)
                        continue
                    assert "error" not in info, (T, B, hint_q, hint_b, info)
                    assert (info["grid_index"], info["outcome"]) in allowed, (T, B, hint_q, hint_b, info, allowed)
                    seen.add(info["outcome"])
                    if info["outcome"] == cc.BY_BUDGET:
                        assert nh == 1
    assert seen == {cc.MET, cc.BY_BUDGET}


def test_the_crossings_of_frame_a():
    """50 dB on frame A is index 107 at 93 067 bytes, 40 dB index 85 at 49 757: the two larger in-range budgets meet both
    targets, the two smaller ones bind"""
    pl, hist = case_hists("A")
    total, sizes = cc.tables("A")
    inr, _, _ = rc.budgets("A")
    assert inr == [9360, 37440, 136656, 243360]
    for db, q, nbytes in ((50, 107, 93067), (40, 85, 49757)):
        T = qc.psnr_to_sse("A", db)
        assert qc.certified(total, T) == [q] and sizes[q] == nbytes
        for B in inr:
            info, aq, ab, nh = search(pl, hist, T, B, total, sizes)
            jb = max(j for j in range(rc.GRID) if sizes[j] <= B)
            assert cc.answers(total, sizes, T, B) == {(min(q, jb), cc.MET if q <= jb else cc.BY_BUDGET)}
            assert (info["grid_index"], info["outcome"]) == (min(q, jb), cc.MET if B >= nbytes else cc.BY_BUDGET)
            assert info["quality_index"] == q and info["quality_bytes"] == nbytes
            assert aq[:2] == [240, 0] and ab[0] == q                         # no hint: the plain quality search's indices
            assert all(j < q for j in ab[1:])                                # the stepper stays under its ceiling
            print("A %d dB, cap %d: j* %d %s, quality trials %s, size trials %s" % (db, B, info["grid_index"], ("MET", "BY_BUDGET")[info["outcome"]], aq, ab))


def test_steady_state_costs_with_the_hints_of_a_sequence():
    """an unchanged frame with hint_q = q and hint_b = the last bound j*: MET in two quality trials and one coding; BY_BUDGET
    in at most three and three (size(q) and the two of the certificate; two when j* == q - 1)"""
    for name in NAMES:
        pl, hist = case_hists(name)
        total, sizes = cc.tables(name)
        inr, _, _ = rc.budgets(name)
        for db in (40, 50):
            T = qc.psnr_to_sse(name, db)
            (q,) = qc.certified(total, T)
            for B in inr:
                jb = max(j for j in range(rc.GRID) if sizes[j] <= B)
                info, aq, ab, nh = search(pl, hist, T, B, total, sizes, q, jb)
                if q <= jb:
                    assert info["outcome"] == cc.MET and len(aq) <= 2 and len(ab) == 1, (name, db, B, aq, ab)
                else:
                    assert info["outcome"] == cc.BY_BUDGET and len(aq) <= 3 and len(ab) <= 3, (name, db, B, aq, ab)
                    assert len(ab) == (2 if jb == q - 1 else 3)


def hostile():
    total, sizes = cc.tables("A")
    saw = [total[j] * (3 if j % 7 == 3 else 1) // (2 if j % 5 == 0 else 1) for j in range(rc.GRID)]     # a sawtooth: rises again in places
    dip = list(sizes)
    for j in range(100, 110):
        dip[j] = sizes[90]
    return [("sawtooth", saw, sizes), ("dip", total, dip), ("both", saw, dip), ("flat sse", [total[120]] * rc.GRID, dip),
            ("rising sse", total[::-1], sizes), ("falling sizes", saw, sizes[::-1])]


@pytest.mark.parametrize("label,total,sizes", hostile(), ids=[h[0].replace(" ", "_") for h in hostile()])
def test_hostile_tables_satisfy_the_predicate_as_measured(label, total, sizes):
    pl, hist = case_hists("A")
    real_total, real_sizes = cc.tables("A")
    Ts = [qc.psnr_to_sse("A", db) for db in qc.TARGETS_DB] + [0, real_total[120], min(total) - 1 if min(total) else 0, max(total)]
    Bs = [9360, 37440, real_sizes[90], real_sizes[105], 136656, 10 ** 9, 64]
    for T in Ts:
        for B in Bs:
            for hint_q in (-1, 0, 57, 104, 240):
                for hint_b in (-1, 0, 99, 105, 240):
                    info, aq, ab, nh = search(pl, hist if hint_b % 2 else None, T, B, total, sizes, hint_q, hint_b)
                    if "error" in info:
                        assert 0 in ab and sizes[0] > B, (label, T, B, hint_q, hint_b)
                    else:
                        assert (info["grid_index"], info["outcome"]) in cc.answers(total, sizes, T, B)


def test_callback_errors_and_refusals():
    pl, hist = case_hists("B")
    total, sizes = cc.tables("B")
    T, B = qc.psnr_to_sse("B", 50), rc.budgets("B")[0][0]
    for kw in (dict(sse_fn=lambda j: capi.E_HIP), dict(size_fn=lambda j: capi.E_NOMEM if j < 100 else sizes[j])):
        args = dict(dict(sse_fn=lambda j: total[j], size_fn=lambda j: sizes[j]), **kw)
        with pytest.raises(capi.OjphError) as e:
            planmod.capped_search(pl, T, B, args["sse_fn"], args["size_fn"], lambda: hist, hint_b=args.get("hint_b", -1))
        assert e.value.code in (capi.E_HIP, capi.E_NOMEM)
    for bad in (dict(cap=0), dict(hint_q=241), dict(hint_q=-2), dict(hint_b=241), dict(hint_b=2 ** 32 + 5)):
        asked = []
        with pytest.raises(capi.OjphError) as e:
            planmod.capped_search(pl, T, bad.get("cap", B), lambda j: (asked.append(j), total[j])[1], lambda j: (asked.append(j), sizes[j])[1],
                                  None, hint_q=bad.get("hint_q", -1), hint_b=bad.get("hint_b", -1))
        assert e.value.code == capi.E_INVALID and not asked, bad
