"""What a view decoder uploads (ojphgpu_plan_upload_runs, Plan.upload_runs): the runs of coded blocks a decoder pipe with a
reduced resolution or a window gathers out of the pinned codestream -- their order, their places in the staged bytes, and
that together they are exactly the bytes of the blocks the view decodes.  No GPU: host logic of the plan alone."""
import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd.plan import parse_codestream
from tests.region_cases import CASES, encode_case, planes_for, regions_for

SKIPS = [None, (1, 1), (2, 1)]
ORDERS = ["LRCP", "RLCP", "RPCL", "PCRL", "CPRL"]


def _align64(v):
    return (v + 63) & ~63


def _union(spans):
    """sorted, merged list of [a, b) intervals (touching ones merge)"""
    out = []
    for a, b in sorted(spans):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def check_runs(pl, skip_blocks=()):
    """the rules of ojphgpu.h for pl.upload_runs(); skip_blocks: plan indices that must not lie in a run (padded blocks).
    -> (runs, staged_len)"""
    runs, staged = pl.upload_runs()
    src, dst, n = (runs[k].astype(np.int64) for k in ("src", "dst", "n"))
    coded = pl.coded_blocks()
    sel = pl.region_blocks()
    padded = set(int(b) for b in skip_blocks)
    spans = [(int(c["offset"]), int(c["offset"]) + int(c["len1"]) + int(c["len2"]))
             for k, c in enumerate(coded) if sel[k] and int(c["len1"]) + int(c["len2"]) > 0 and k not in padded]
    if not spans:
        assert runs.size == 0 and staged == 0
        return runs, staged
    assert runs.size >= 1 and (n > 0).all()
    assert (src[1:] > src[:-1] + n[:-1]).all(), "runs are sorted by src and strictly apart"
    assert (dst % 64 == 0).all() and dst[0] == 64
    for i in range(1, runs.size):
        assert dst[i] >= _align64(dst[i - 1] + n[i - 1]) + 64
    assert staged == _align64(int(dst[-1] + n[-1])) + 64
    want = _union(spans)
    assert [[int(a), int(a + b)] for a, b in zip(src, n)] == want, "the runs are the union of the decoded blocks' bytes"
    assert int(n.sum()) == sum(b - a for a, b in want)
    return runs, staged


def _plan(cs, skip, region, resilient=False):
    pl = parse_codestream(cs, resilient)
    if skip:
        pl.restrict_resolution(*skip)
    if region is not None:
        pl.restrict_region(*region)
    return pl


@pytest.mark.parametrize("skip", SKIPS, ids=["full", "skip11", "skip21"])
@pytest.mark.parametrize("name,kw,size", CASES, ids=[c[0] for c in CASES])
def test_runs_of_every_case_region_and_skip(name, kw, size, skip):
    cs = encode_case(kw, size)
    if skip and kw["num_decomps"] < skip[0]:               # no such view: the restriction is refused and leaves the plan whole
        pl = parse_codestream(cs)
        whole = pl.upload_runs()
        with pytest.raises(capi.OjphError) as e:
            pl.restrict_resolution(*skip)
        assert e.value.code == capi.E_INVALID
        runs, staged = check_runs(pl)
        assert staged == whole[1] and np.array_equal(runs, whole[0])
        return
    check_runs(_plan(cs, skip, None))
    for r in regions_for(size):
        pl = _plan(cs, skip, r)
        runs, staged = check_runs(pl)
        assert runs.size <= int(pl.region_blocks().sum())


def _order_case(order):
    kw = dict(reversible=True, num_decomps=3, prog_order=order, precinct=(32, 32), tile=(64, 64))
    return kw, (128, 128)


@pytest.mark.parametrize("skip", SKIPS, ids=["full", "skip11", "skip21"])
@pytest.mark.parametrize("order", ORDERS)
def test_runs_in_every_progression_order(order, skip):
    kw, size = _order_case(order)
    cs = encode_case(kw, size)
    assert parse_codestream(cs).num_tiles == 4
    check_runs(_plan(cs, skip, None))
    for r in regions_for(size, seed=5):
        check_runs(_plan(cs, skip, r))


def test_no_coded_block_no_runs():
    kw, size = dict(reversible=True, num_decomps=3), (77, 61)
    from tests import cpu_pipeline as cp
    planes = [np.full_like(q, 128) for q in planes_for(kw, size)]       # every sample 0 after the level shift
    cs = cp.encode(planes, size=size, downsampling=[(1, 1)], **kw)[0]
    pl = parse_codestream(cs)
    coded = pl.coded_blocks()
    assert int((coded["len1"].astype(np.int64) + coded["len2"]).sum()) == 0, "the flat image codes no block"
    runs, staged = pl.upload_runs()
    assert runs.size == 0 and staged == 0
    pl.restrict_region(3, 4, 20, 20)
    runs, staged = check_runs(pl)
    assert runs.size == 0 and staged == 0


def _damaged(cs):
    """the codestream cut at 40 .. 80 % of its length, and with the Psot of every tile-part but the first lowered so that the
    tile-part ends inside its last block (the reference decodes such a block from the bytes there are: a padded block)"""
    for frac in (0.6, 0.5, 0.7, 0.4, 0.8):
        yield "cut%d" % int(frac * 100), cs[:int(len(cs) * frac)]
    sots, at = [], cs.find(b"\xff\x90\x00\x0a")
    while at >= 0:
        sots.append(at)
        at = cs.find(b"\xff\x90\x00\x0a", at + 12)
    for at in sots[1:]:
        for short in (1, 7, 40):
            b = bytearray(cs)
            psot = int.from_bytes(cs[at + 6:at + 10], "big") - short
            b[at + 6:at + 10] = psot.to_bytes(4, "big")
            yield "psot@%d-%d" % (at, short), bytes(b)


def test_padded_blocks_lie_in_no_run():
    _, kw, size = next(c for c in CASES if c[0] == "tiles-2x2")
    cs = encode_case(kw, size)
    found = 0
    for name, bad in _damaged(cs):
        for skip in SKIPS:
            for region in (None, (0, 0) + size, (size[0] // 2, size[1] // 3, 50, 70)):
                try:
                    pl = parse_codestream(bad, True)
                except capi.OjphError:
                    continue                                # (a cut the resilient parser gives up on)
                if skip:
                    pl.restrict_resolution(*skip)
                if region is not None:
                    pl.restrict_region(*region)
                pb = pl.padded_blocks()
                sel = pl.region_blocks()
                found += int(sum(bool(sel[int(b["block"])]) and int(b["got"]) > 0 for b in pb))
                runs, staged = check_runs(pl, skip_blocks=pb["block"])
                for b in pb:                                # ... and no run reaches into a padded block's bytes
                    a0, a1 = int(b["offset"]), int(b["offset"]) + int(b["got"])
                    for r in runs:
                        assert a0 == a1 or int(r["src"]) + int(r["n"]) <= a0 or int(r["src"]) >= a1, (name, skip, region)
    assert found, "no damaged codestream produced a padded block inside a view"


def test_resolution_only_view_under_pcrl_uploads_runs_not_a_range():
    kw, size = _order_case("PCRL")
    cs = encode_case(kw, size)
    pl = _plan(cs, (1, 1), None)
    runs, staged = check_runs(pl)
    coded, sel = pl.coded_blocks(), pl.region_blocks()
    ends = [(int(c["offset"]), int(c["offset"]) + int(c["len1"]) + int(c["len2"])) for k, c in enumerate(coded) if sel[k] and c["len1"] + c["len2"]]
    span = max(e for _, e in ends) - min(a for a, _ in ends)
    assert runs.size > 1 and staged < span
