"""Near-lossless coding (include/ojphgpu.h section 5g): what tests/test_cpu_near_lossless.py builds on -- the recorded
figures of the reference (tests/golden/near_lossless.json), the truncation of a plane restated in numpy, and the certificate
every search result must carry."""
import json
import math
import os

import numpy as np

from openjph_amd import plan as planmod
from tests import cpu_pipeline as cp
from tests import trunc_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
_GOLD = {}


def gold(name):
    """(levels, sse [U][comps], pae [U][comps]) of a coded case: the reference's decode of every distinct level"""
    if not _GOLD:
        _GOLD.update(json.load(open(os.path.join(HERE, "golden", "near_lossless.json")))["cases"])
    g = _GOLD[name]
    return g["levels"], g["sse"], g["pae"]


def totals(name):
    """(levels, SSE [U], PAE [U]) over all components"""
    levels, sse, pae = gold(name)
    return levels, [sum(s) for s in sse], [max(p) for p in pae]


def truncate_rule(v, t):
    """the rule of the issue on samples that fit K_max bits: magnitude m -> 0 where m >> t == 0, else (m >> t << t) | 1 << (t - 1),
    sign kept"""
    v = np.asarray(v).astype(np.int64)
    if t == 0:
        return v.astype(np.int32)
    m = np.abs(v)
    out = np.where((m >> t) != 0, ((m >> t) << t) | (1 << (t - 1)), 0)
    return np.where(v < 0, -out, out).astype(np.int32)


def truncated_arena(plan, arena, table):
    """a copy of the arena with every band's plane truncated by its entry of the table"""
    out = arena.copy()
    for i, b in enumerate(plan.bands):
        w, h, t = int(b["w"]), int(b["h"]), int(table[i])
        if w and h and t:
            v = cp._view(out, int(b["plane_off"]), int(b["pitch"]), w, h, np.int32)
            v[:] = truncate_rule(v, t)
    return out


def errors(img, dec):
    """[(sse, pae) per component] between two frames [C, H, W]"""
    d = np.asarray(dec).astype(np.int64) - np.asarray(img).astype(np.int64)
    return [(int((d[c] * d[c]).sum()), int(np.abs(d[c]).max())) for c in range(len(d))]


def pass_cap(U):
    return math.ceil(math.log2(U)) if U > 1 else 0


def meets(sse, pae, k, T, E):
    return (T is None or sse[k] <= T) and (E is None or pae[k] <= E)


def check_certificate(info, levels, sse, pae, T, E, asked=None):
    """info = the dict of a search over the table (levels, sse, pae: totals per distinct level): the
    certificate, the pass cap and the reported figures.  asked: the levels err_fn was called with, in order."""
    U = len(levels)
    assert info["level"] in levels
    k = levels.index(info["level"])
    assert info["passes"] <= pass_cap(U)
    assert info["lossless"] == (k == 0)
    if T == 0 or E == 0:
        assert k == 0 and info["passes"] == 0
    if k == 0:
        assert info["sse"] == 0 and info["pae"] == 0                       # level 0 meets by contract, unmeasured
    else:
        assert meets(sse, pae, k, T, E), (k, T, E)
        assert (info["sse"], info["pae"]) == (sse[k], pae[k])
    if k == U - 1 or T == 0 or E == 0:
        assert (info["level_coarser"], info["sse_coarser"], info["pae_coarser"]) == (0, 0, 0)
    else:
        assert not meets(sse, pae, k + 1, T, E), (k, T, E)
        assert (info["level_coarser"], info["sse_coarser"], info["pae_coarser"]) == (levels[k + 1], sse[k + 1], pae[k + 1])
    if asked is not None:
        assert len(asked) == info["passes"] and len(set(asked)) == len(asked) and 0 not in asked
        assert k == 0 or levels[k] in asked
        assert k == U - 1 or T == 0 or E == 0 or levels[k + 1] in asked


def run_search(plan, levels, sse, pae, T, E):
    """ojphgpu_near_lossless_search over a table, with the certificate checked"""
    asked = []

    def fn(level):
        asked.append(level)
        k = levels.index(level)                                            # (a level that is not distinct is never asked)
        return sse[k], pae[k]

    info = planmod.near_lossless_search(plan, T, E, fn)
    check_certificate(info, levels, sse, pae, T, E, asked)
    assert info["max_dropped"] == int(plan.trunc_table(info["level"]).max()) and info["bytes"] == 0
    return info


def targets(sse, pae):
    """the targets of the issue over a table: every SSE value and its neighbours, max_pae 0 .. 3 and every PAE value, a dozen
    pairs"""
    out = []
    for s in sorted(set(sse)):
        out += [(max(s - 1, 0), None), (s, None), (s + 1, None)]
    for p in sorted(set(pae) | {0, 1, 2, 3}):
        out.append((None, p))
    U = len(sse)
    for i in range(12):
        a, b = (i * 5 + 1) % U, (i * 7 + 2) % U
        out.append((sse[a] + (i % 3) - 1 if sse[a] else 0, pae[b]))
    return out


def case_plan_levels(name):
    plan = tc.case_state(name)[0]
    return plan, tc.distinct_levels(plan)
