"""What the tests of a quality target under a byte cap share (tests/test_cpu_capped.py, tests/test_gpu_capped.py,
tests/test_gpu_capped_pipe.py): the recorded tables of the five frames of tests/rate_cases.py -- SSE(j) from
tests/golden/quality_sse.json, size(j) from tests/golden/rate_sizes.json -- and the set of answers the contract of
include/ojphgpu.h section 5c ("under a byte cap") allows over a pair of tables."""
import json
import os

from tests import quality_cases as qc
from tests import rate_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
QUAL = json.load(open(os.path.join(HERE, "golden", "quality_sse.json")))
RATE = json.load(open(os.path.join(HERE, "golden", "rate_sizes.json")))
MET, BY_BUDGET = 0, 1


def tables(name):
    """-> (total[j] = SSE(j) over all components, sizes[j]) of frame `name`, both measured on the reference"""
    return [sum(int(v) for v in row) for row in QUAL["cases"][name]["sse"]], [int(v) for v in RATE["cases"][name]["sizes"]]


def comp_figures(name, j):
    """-> [(sse, pae) per component] of frame `name` at grid index j"""
    c = QUAL["cases"][name]
    return [(int(s), int(p)) for s, p in zip(c["sse"][j], c["pae"][j])]


def budget_certified(sizes, B):
    """every index that carries the budget certificate of section 5b"""
    return [j for j in range(len(sizes)) if sizes[j] <= B and (j == len(sizes) - 1 or sizes[j + 1] > B)]


def answers(total, sizes, T, B):
    """the set of (j*, outcome) a capped encode may return for target T and cap B.  Empty: nothing is allowed but an error."""
    out = set()
    q_all = qc.certified(total, T)
    for q in q_all:
        if sizes[q] <= B:
            out.add((q, MET))
    none_meets = total[-1] > T
    for j in budget_certified(sizes, B):
        if none_meets or any(q > j and sizes[q] > B for q in q_all):
            out.add((j, BY_BUDGET))
    return out


def check_info(info, total, sizes, T, B):
    """the figures of a result against the tables: the predicate of its outcome, as measured"""
    j, q = info["grid_index"], info["quality_index"]
    assert info["qstep"] == rc.grid_qstep(j)
    assert info["bytes"] == sizes[j] <= B
    assert info["sse"] == total[j]
    if info["outcome"] == MET:
        assert q == j and total[j] <= T and (j == 0 or total[j - 1] > T)
        assert info["sse_coarser"] == (total[j - 1] if j else 0)
        assert info["quality_bytes"] == sizes[j]
    else:
        assert info["outcome"] == BY_BUDGET
        assert j == rc.GRID - 1 or sizes[j + 1] > B
        assert info["bytes_finer"] == (sizes[j + 1] if j + 1 < rc.GRID else 0)
        if q == rc.GRID:
            assert total[rc.GRID - 1] > T and info["quality_bytes"] == 0
        else:
            assert q > j and total[q] <= T and (q == 0 or total[q - 1] > T)
            assert info["quality_bytes"] == sizes[q] > B
