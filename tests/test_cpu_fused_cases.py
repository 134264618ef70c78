"""The net of tests/test_gpu_fused_geometry.py is sound -- checked without a GPU, through the two host functions of the
fused launch's stage entry (ojphgpu_ht_decode_fused_shape, ojphgpu_ht_decode_fused_slices) and on the oracle's bytes:
the geometry table reaches every way the launch deals blocks out, under each of the three settings; the slice schedule of
every max_qh is a partition with the stated cuts and every launch has blocks ending in every slice and on every cut; the
pool holds the content that breaks decoders."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fused_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setting():
    shape = os.environ.get("OJPHGPU_FUSED_SHAPE")
    return "shape0" if shape is not None and int(shape) != 1 else "rings1" if os.environ.get("OJPHGPU_FUSED_RINGS") == "1" else "default"


def test_geometry_table_reaches_every_item():
    """under the setting this process runs with (the knobs are read once per process)"""
    setting = _setting()
    rows = [(n, cus, fc.shape_of(n, cus)) for n, cus in fc.GEOMETRY]
    able = [(n, cus, s) for n, cus, s in rows if s["able"]]
    assert {n for n, _, _ in able} >= {1, 7, 64, 65, 256, 257}
    assert any(not s["able"] for _, _, s in rows), "no refusal (n1 > cus)"
    for n, cus, s in rows:
        assert s["able"] == (1 if s["n1"] <= cus else 0)
        assert (s["shape"], s["ch"], s["wgw"]) == ((0, 2, 8) if setting == "shape0" else (1, 4, 12))
        # NR: a ring per block exactly for per_wave <= 5 under the default setting
        assert s["nr"] == (5 if setting == "default" and s["per_wave"] <= 5 else 1), (n, cus, s)
    # every per_wave the shape can reach with n1 <= cus: 1..8, and 1..6 for OJPHGPU_FUSED_SHAPE=0 (fused_cases.GEOMETRY)
    reach = range(1, 7) if setting == "shape0" else range(1, 9)
    assert {s["per_wave"] for _, _, s in able} >= set(reach)
    for pw in reach:
        if pw > 1:           # ... with a launch that leaves some wavefronts short of per_wave
            assert any(s["per_wave"] == pw and n % -(-n // pw) != 0 for n, _, s in able), "per_wave %d: every wavefront full" % pw
    assert {s["n1"] for _, _, s in able} >= {1, 2, 3}
    assert any(s["n1"] == cus for _, cus, s in able), "n1 == cus"
    # a last step-1 workgroup with one live lane; idle wavefronts in the last worker workgroup
    assert any(s["n1"] >= 2 and n % (64 * s["ch"]) == 1 for n, _, s in able)
    assert any(s["wwgs"] * s["wgw"] > -(-n // s["per_wave"]) for n, _, s in able)
    if setting != "shape0":  # per_wave capped (what the wavefront slots ask for is more than 8) on three worker workgroups or more
        assert any(s["per_wave"] == 8 and s["want"] > 8 and s["wwgs"] >= 3 for n, cus, s in able)
    assert all(s["per_wave"] == min(s["want"], 8) for _, _, s in rows)
    # the NR = 1 form with several blocks interleaved in one wavefront
    assert any(s["nr"] == 1 and s["per_wave"] >= 2 for _, _, s in able)
    # the sequences run under every setting, and change per_wave and NR from run to run under the default one
    seq = [fc.shape_of(L.n, L.cus) for L in fc.sequences()]
    assert all(s["able"] for s in seq)
    if setting == "default":
        assert {s["nr"] for s in seq} == {1, 5} and len({s["per_wave"] for s in seq}) >= 4


@pytest.mark.parametrize("name", [n for n in fc.SETTINGS if n != "default"])
def test_geometry_table_under_setting(name):
    """the same in a child process per setting"""
    env = {k: v for k, v in os.environ.items() if k not in ("OJPHGPU_FUSED_SHAPE", "OJPHGPU_FUSED_RINGS")}
    env.update(fc.SETTINGS[name])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", "test_geometry_table_reaches_every_item",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"1 passed" in r.stdout, "setting %s:\n%s" % (name, r.stdout[-3000:].decode(errors="replace"))


@pytest.mark.parametrize("max_qh", sorted(set(fc.SLICE_QH) | set(range(1, 140)) | {511, 512, 513}))
def test_slice_schedule_is_a_partition_with_the_stated_cuts(max_qh):
    """slices of 8 quad rows, the last one cut at max_qh - 4 and max_qh - 2 where those fall inside it; the same for both
    heights that give max_qh"""
    tail = 8 * ((max_qh - 1) // 8)
    cuts = sorted(set(range(8, max_qh, 8)) | {c for c in (max_qh - 4, max_qh - 2) if c > tail})
    want = list(zip([0] + cuts, cuts + [max_qh]))
    for max_h in (2 * max_qh - 1, 2 * max_qh):
        assert fc.slices_of(max_h) == want


@pytest.mark.parametrize("max_qh", fc.SLICE_QH)
def test_slice_launch_has_blocks_in_every_slice_and_on_every_cut(max_qh):
    L = fc.slice_launch(max_qh)
    qh = [(e.h + 1) // 2 for e in L.entries if e.coded and e.ok]          # blocks that are decoded to their last row
    assert max(qh) == max_qh and L.max_h in (2 * max_qh - 1, 2 * max_qh)
    e0 = max(L.entries, key=lambda e: e.h)
    assert e0.coded and e0.ok, "the tallest block is decoded"
    if max_qh == 512:
        assert (e0.w, e0.h) == (4, 1024)
    for lo, hi in L.bounds:
        assert hi in qh, "no block ends on the cut %d" % hi
        assert hi - lo == 1 or any(lo < q < hi for q in qh), "no block ends inside [%d, %d)" % (lo, hi)
    assert all(e.w * e.h <= 4096 and e.w <= 64 for e in L.entries)
    assert fc.shape_of(L.n, L.cus)["able"]
    assert 15 <= L.n and (L.n <= 24 or max_qh >= 64)
    # two refused by the first test, two uncoded, two refused late: whatever per_wave the setting gives the launch
    assert sum(1 for e in L.entries if e.early_refused) >= 2
    assert sum(1 for e in L.entries if not e.coded and e.w and e.h) >= 2
    assert sum(1 for e in L.entries if e.late_refused) >= 2
    assert {e.h % 2 for e in L.entries if e.coded and e.ok} == ({0, 1} if max_qh > 1 else {1})


def test_pool_holds_what_breaks_decoders():
    P = fc.pool()
    assert {e.w for e in P} >= set(fc.WIDTHS) and {e.h for e in P} >= {1, 2, 3, 63, 64}
    plain = [e for e in P if e.kind in ("plain", "big") and e.mm == e.kmax - 1]
    assert {e.kmax for e in plain} == set(range(1, 31))
    assert {e.mm for e in P if e.kind == "mm"} == {28, 29, 30}
    assert all((e.mm == 30) == (not e.ok) for e in P if e.kind == "mm")
    assert sum(1 for e in P if len(e.magsgn) > 4096) >= 32
    assert fc.boundary_ff(P) >= 16
    intact = [e for e in P if e.damaged and e.passes_first_test]
    assert sum(1 for e in intact if not e.ok) >= 16 and sum(1 for e in intact if e.ok) >= 16
    assert sum(1 for e in P if e.kind == "cut") >= 16 and sum(1 for e in P if e.early_refused) >= 8
    assert sum(1 for e in P if e.kind == "short-mm" and e.late_refused) >= 8
    assert sum(1 for e in P if not e.coded and e.len1 == 0 and e.w and e.h) >= 4
    assert sum(1 for e in P if not e.coded and e.num_passes == 0 and e.len1) >= 4
    assert any(e.w == 0 for e in P) and any(e.h == 0 for e in P)
    # the sentinel occurs in no expected sample, of either transfer
    for e in P:
        for rev in (True, False):
            assert not (e.expect(rev) == fc.SENTINEL).any()
    # a refused block that is not zero where it was accepted before would not be noticed: the accepted ones are not all zero
    assert sum(1 for e in P if e.ok and e.coded and e.expect(True).any()) > len(P) // 3


def test_every_launch_holds_the_block_kinds():
    used = set()
    for L in [fc.slice_launch(q) for q in fc.SLICE_QH]:      # every launch with per_wave > 1, the slice launches included
        assert sum(1 for e in L.entries if e.early_refused) >= 2 and sum(1 for e in L.entries if e.late_refused) >= 2, L.tag
        assert sum(1 for e in L.entries if not e.coded and e.w and e.h) >= 2, L.tag
    for L in fc.geometry_launches() + fc.sequences():
        used |= {id(e) for e in L.entries}
        e0 = L.entries[0]
        assert e0.coded and e0.ok and 2 <= e0.len1 < 34 and L.descs[0]["data_off"] == 0
        assert all(d["data_off"] == sum(len(e.data) for e in L.entries[:i]) for i, d in enumerate(L.descs)), "no padding"
        s = fc.shape_of(L.n, L.cus)
        if s["per_wave"] > 1 or L.n >= 12:
            assert sum(1 for e in L.entries if e.early_refused) >= 2, L.tag
            assert sum(1 for e in L.entries if not e.coded and e.w and e.h) >= 2, L.tag
            assert sum(1 for e in L.entries if e.late_refused) >= 2, L.tag
            assert sum(1 for e in L.entries if len(e.magsgn) > 4096) >= 2, L.tag
        assert s["per_wave"] == 1 or L.n >= 12
    assert used >= {id(e) for e in fc.pool()}, "a pool block that no launch decodes"
    assert len({L.descs[i]["data_off"] % 4 for L in fc.geometry_launches() for i in range(L.n)}) == 4
    # sequences: positions that change between coded and not from one run to the next
    q = fc.sequences()
    a, b = q[0].entries, q[1].entries
    assert sum(1 for x, y in zip(a, b) if x.coded and x.ok and (not y.coded or not y.ok)) >= 20
    assert sum(1 for x, y in zip(a, b) if (not x.coded or not x.ok) and y.coded and y.ok) >= 20
    assert {L.rev for L in q} == {True, False} and q[0].n > q[2].n > q[4].n


def test_verify_notices_what_it_should():
    """the comparison itself: one wrong word inside a rectangle, one outside, one verdict"""
    L = fc.geometry_launches()[6]
    want = L.expected()
    assert not L.problems(L.status, want)
    i = next(i for i, e in enumerate(L.entries) if e.w >= 2 and e.h >= 2)
    for ix in (L.rects[i][0] + 1, L.rects[i][0] + L.entries[i].w, L.size - 1, 0):
        got = want.copy()
        got[ix] ^= 1
        assert L.problems(L.status, got)
    st = L.status.copy()
    st[3] ^= 1
    assert L.problems(st, want)
