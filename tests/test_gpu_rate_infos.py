"""What the budget search reports, pinned to a recording (tests/golden/rate_search_infos.json, tools/record_rate_infos.py).
The single encoder and the batch encoder run one loop, and the batch test's oracle is the single encoder: the bytes are
anchored by the reference's digests (tests/golden/rate_sizes.json), but passes, first_guess and rounds would follow any
change of the loop on both sides at once.  The recording was taken from the commit before the two loops became one."""
import json
import os

import numpy as np
import pytest

from tests import rate_cases as rc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "rate_search_infos.json")
BATCHES = ("A", "C", "E", "B")


def measure():
    """-> {"single": {case: {budget: {"info": rate_info(), "rounds": rate_rounds()}}}, "batch": {case: {"budgets", "infos",
    "rounds"}}}: cases A to E at every in-range budget and the one above, in the smallest container that holds the samples;
    the batches of tests/test_gpu_rate_batch.py at budgets_of(name)"""
    from openjph_amd import codec
    from openjph_amd.plan import Plan
    from tests import test_gpu_rate as single
    from tests import test_gpu_rate_batch as tb
    out = {"single": {}, "batch": {}}
    for name in sorted(rc.CASES):
        params = single.case_params(name)
        frame = single.case_frame(name, Plan(params)).astype(single.containers(name)[0])
        inr, _, above = rc.budgets(name)
        out["single"][name] = {}
        for budget in inr + [above]:
            enc = codec.Encoder(params, max_bytes=budget)
            enc.encode(frame)
            out["single"][name][str(budget)] = dict(info=enc.rate_info(), rounds=enc.rate_rounds())
    for name in BATCHES:
        budgets = tb.budgets_of(name)
        enc = codec.Encoder(tb.case_params(name), frames=tb.FRAMES[name], budgets=budgets)
        enc.encode(tb.batch(name))
        out["batch"][name] = dict(budgets=budgets, infos=enc.rate_info(), rounds=enc.rate_rounds())
    return json.loads(json.dumps(out))                       # (as the fixture reads back: a float's repr round-trips)


def test_infos_and_rounds_are_the_recorded_ones():
    want = json.load(open(FIXTURE))
    got = measure()
    for kind in ("single", "batch"):
        assert sorted(got[kind]) == sorted(want[kind])
        for name in sorted(want[kind]):
            print(kind, name, got[kind][name])
            assert got[kind][name] == want[kind][name], (kind, name)
    for name, by_budget in got["single"].items():            # all six fields were recorded, and a single frame's rounds are its passes
        for rec in by_budget.values():
            assert sorted(rec["info"]) == ["bytes", "bytes_finer", "first_guess", "grid_index", "passes", "qstep"]
            assert rec["rounds"] == rec["info"]["passes"]
