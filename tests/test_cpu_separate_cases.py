"""The net of tests/test_gpu_separate_launches.py is sound -- checked without a GPU, through the two host functions of the
separate launches' stage entry (ojphgpu_ht_decode_kinds, ojphgpu_ht_decode_launches) and on the oracle's bytes: the launches
of tests/separate_cases.py reach every one of the ten step-2 instantiations, under each of them every grid (1, 7, 8, 9, 16, 17
workgroups) and every partial last wavefront, and every step-1 size; the kinds a launch is given are what the library says of
its descriptors or a valid coarsening of that; the hand-ordered wavefronts hold what they are there for; the pools hold the
content that breaks decoders."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import separate_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEN = {(0, tx, wd, 1) for tx in (0, 1, 2) for wd in (0, 1)} | {(1, tx, 1, nb) for tx in (1, 2) for nb in (2, 4)}


def _setting():
    e = os.environ
    ch, dual = e.get("OJPHGPU_S1_CH"), e.get("OJPHGPU_DEC_DUAL")
    prep = e.get("OJPHGPU_DEC_PREP")
    return dict(ch=int(ch) if ch in ("1", "2", "4") else 4, prep=1 if prep is not None and int(prep) != 0 else 0, dual=4 if dual is None else int(dual))


def _inst(s):
    return (s["multi"], s["tx"], s["wd"], s["nb"])


def _runs():
    """(launch, variant, what ojphgpu_ht_decode_launches says) of every geometry test of the GPU file"""
    for L in sc.launches():
        for v in sc.variants_of(L.cls):
            yield L, v, sc.launches_of(L.n, sc.VARIANTS[v][0](L.truth))


def test_kinds_are_what_the_library_says_of_the_descriptors():
    from openjph_amd import codec
    assert codec.ht_decode_kinds(np.zeros(0, codec.cb_desc_dtype)) == 0
    for L in sc.launches() + [L for L, _ in sc.sequences()]:
        assert codec.ht_decode_kinds(L.desc_array(codec.cb_desc_dtype)) == L.truth, L.tag
        want = {"w16": 1 | 256, "w32": 1 | 128 | 256, "wide": 2 | 64 | 128 | 256}[L.cls] | (4 if L.rev else 8)
        # (a launch of wide blocks with an empty descriptor of 127 x 0 or 0 x 11 in it also holds a "block of at most 64 columns")
        assert L.truth | 1 == want | 1 and L.truth & 3 in ((1,) if L.cls != "wide" else (2, 3)), L.tag
    # blocks with refinement passes, and blocks on the 64-bit sample path
    d = np.zeros(3, codec.cb_desc_dtype)
    d["w"], d["h"], d["reversible"], d["num_passes"], d["len1"], d["len2"] = (8, 40, 8), 4, (1, 0, 5), (1, 3, 1), 9, (0, 5, 0)
    assert codec.ht_decode_kinds(d[:1]) == 1 | 4 | 256
    assert codec.ht_decode_kinds(d[1:2]) == 1 | 8 | 16 | 64 | 128 | 256
    assert codec.ht_decode_kinds(d[2:]) == 32
    d["len2"][1] = 0
    assert codec.ht_decode_kinds(d[:2]) == 1 | 4 | 8 | 64 | 128 | 256


def test_every_coarsening_is_a_valid_one():
    """set bit 6 / 7, clear bit 8, set both of bits 2 and 3, set bit 1 -- nothing else: a caller may know less, never more"""
    for L in sc.launches():
        for v, (f, _) in sc.VARIANTS.items():
            k, t = f(L.truth), L.truth
            lost, gained = t & ~k, k & ~t
            assert lost & ~256 == 0, (v, "a bit of the truth other than bit 8 was cleared")
            assert gained & ~(2 | 4 | 8 | 64 | 128) == 0, v
            assert not (gained & 12) or (k & 12) == 12, v
    assert sc.VARIANTS["truth"][0](0x1A5) == 0x1A5


def test_launches_reach_every_instantiation_grid_and_partial_wavefront():
    """under the setting this process runs with (the knobs are read once per process)"""
    st = _setting()
    runs = list(_runs())
    for L, v, s in runs:
        assert (s["ch"], s["prep"]) == (st["ch"], st["prep"])
        assert s["wgs1"] == -(-L.n // (64 * s["ch"])) and s["per_wg"] == 4 * s["nb"] and s["wgs2"] == -(-L.n // s["per_wg"])
        multi, tx, wd, nb = sc.VARIANTS[v][1][L.cls]
        tx = (1 if L.rev else 2) if tx is None else tx
        if st["dual"] == 0:
            multi, nb = 0, 1
        elif st["dual"] < 4 and nb == 4:
            nb = 2
        assert _inst(s) == (multi, tx, wd, nb), (L.tag, v, s)
    reach = TEN if st["dual"] >= 4 else {i for i in TEN if i[3] != 4} if st["dual"] else {i for i in TEN if not i[0]}
    assert {_inst(s) for _, _, s in runs} == reach
    for inst in reach:
        mine = [(L, s) for L, _, s in runs if _inst(s) == inst and L.n != len([e for _, g in getattr(L, "groups", []) for e in g])]
        assert {s["wgs2"] for _, s in mine} >= set(sc.GRIDS), (inst, sorted({s["wgs2"] for _, s in mine}))
        # the XCD re-ordering of the workgroups: r8 = grid % 8 in {0, 1, 7}, q8 = grid // 8 in {0, 1, 2}
        assert {s["wgs2"] & 7 for _, s in mine} >= {0, 1, 7} and {s["wgs2"] >> 3 for _, s in mine} >= {0, 1, 2}
        assert {L.n % inst[3] for L, _ in mine} >= set(range(inst[3])), "a last wavefront with every count of blocks"
        if inst[1]:
            assert {L.rev for L, _ in mine} == {inst[1] == 1}
        else:
            assert {L.rev for L, _ in mine} == {True, False}, "the per-block transfer, both"
    # the classes under their instantiations: six, five and two per transfer
    if st["dual"] >= 4:
        for cls, count in (("w16", 6), ("w32", 5), ("wide", 2)):
            for rev in (True, False):
                assert len({_inst(s) for L, _, s in runs if L.cls == cls and L.rev == rev}) == count
    # step 1: 1, 63, 64, 65, 256, 257 blocks, and a last workgroup with one live lane
    ns = {L.n for L, _, _ in runs}
    assert ns >= set(sc.STEP1_N) and max(ns) == 257
    assert any(s["wgs1"] >= 2 and L.n % (64 * s["ch"]) == 1 for L, _, s in runs)
    assert {s["wgs1"] for _, _, s in runs} >= {1, 2}
    # the sequences: four blocks to a wavefront, one, two, one per wide block; single between multi launches
    seq = [_inst(sc.launches_of(L.n, sc.VARIANTS[v][0](L.truth))) for L, v in sc.sequences()]
    if st["dual"] >= 4:
        assert seq == [(1, 1, 1, 4), (0, 2, 1, 1), (1, 2, 1, 2), (1, 1, 1, 4), (0, 1, 0, 1), (1, 1, 1, 2)]


@pytest.mark.parametrize("name", [n for n in sc.SETTINGS if n != "default"])
def test_launches_under_setting(name):
    """the same in a child process per setting"""
    env = {k: v for k, v in os.environ.items() if k not in sc.KNOBS}
    env.update(sc.SETTINGS[name])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", "test_launches_reach_every_instantiation",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"1 passed" in r.stdout, "setting %s:\n%s" % (name, r.stdout[-3000:].decode(errors="replace"))


def test_launches_function_for_other_kinds():
    """what the decoder objects pass: refinement passes, both transfers, nothing known"""
    st = _setting()
    assert _inst(sc.launches_of(100, 0)) == (0, 0, 0, 1)
    assert _inst(sc.launches_of(100, 1 | 4 | 16 | 256)) == (0, 0, 1, 1)
    assert _inst(sc.launches_of(100, 1 | 4 | 8 | 256)) == (0, 0, 1, 1)
    assert _inst(sc.launches_of(100, 1 | 2 | 8 | 64 | 128 | 256)) == (0, 2, 0, 1)
    assert _inst(sc.launches_of(100, 1 | 4)) == (0, 1, 1, 1), "bits 6 and 7 clear without bit 8: one block to a wavefront"
    s = sc.launches_of(0, 1 | 4 | 256)
    assert (s["wgs1"], s["wgs2"]) == (0, 0)
    s = sc.launches_of(100000, 1 | 8 | 256)
    assert s["wgs1"] == -(-100000 // (64 * st["ch"])) and s["wgs2"] == -(-100000 // s["per_wg"])


@pytest.mark.parametrize("cls", list(sc.CLASSES))
def test_pool_holds_what_breaks_decoders(cls):
    P = sc.pool(cls)
    W = sc.CLASSES[cls]
    assert {e.w for e in P if e.w} >= set(W) and max(e.w for e in P) == max(W) and all(e.w * e.h <= 4096 for e in P)
    if cls == "wide":
        assert all(e.w >= 65 or not (e.w and e.h) for e in P)
    assert {e.h for e in P} >= {1, 2, 3} and max(e.h for e in P) == (63 if cls == "wide" else 64)
    plain = [e for e in P if e.kind in ("plain", "big") and e.mm == e.kmax - 1]
    assert {e.kmax for e in plain} == set(range(1, 31))
    assert {e.mm for e in P if e.kind == "mm"} == {28, 29, 30}
    assert all((e.mm == 30) == (not e.ok) for e in P if e.kind == "mm")
    assert sum(1 for e in P if e.kind == "tiny" and e.ok and 2 <= e.len1 < 34 and e.w in W) >= 8
    assert sum(1 for e in P if e.coded and e.ok and not e.expect(True).any()) >= 6, "density 0"
    intact = [e for e in P if e.damaged and e.passes_first_test]
    assert sum(1 for e in intact if not e.ok) >= 16 and sum(1 for e in intact if e.ok) >= 16
    assert sum(1 for e in P if e.kind == "cut") >= 16 and sum(1 for e in P if e.early_refused) >= 8
    assert sum(1 for e in P if e.kind == "short-mm" and e.late_refused) >= 8
    assert sum(1 for e in P if e.coded and e.ok) >= 150
    assert sum(1 for e in P if not e.coded and e.len1 == 0 and e.w and e.h) >= 4
    assert sum(1 for e in P if not e.coded and e.num_passes == 0 and e.len1) >= 4
    assert any(e.w == 0 for e in P) and any(e.h == 0 for e in P)
    if cls in sc.FULL:
        big = [e for e in P if e.kind == "big" and e.w in sc.FULL[cls]]
        assert len(big) >= 12 and {e.w for e in big} == set(sc.FULL[cls]) and all(e.ok for e in big)
        assert sc.ff_blocks(P, sc.CHUNK[cls]) >= sc.FF_BLOCKS
        # ... of which blocks as wide as the segment: every lane of it holds a column
        assert sc.ff_blocks([e for e in P if e.w == max(W)], sc.CHUNK[cls]) >= 2
    for e in P:
        for rev in (True, False):
            assert not (e.expect(rev) == sc.fc.SENTINEL).any()
    assert sum(1 for e in P if e.ok and e.coded and e.expect(True).any()) > len(P) // 3


def test_chunk_ff_counts_what_it_says():
    for m, want in ((b"\x00" * 63 + b"\xff" + b"\x01", 1), (b"\x00" * 63 + b"\xff", 0), (b"\xff" * 62 + b"\x00\x00", 0),
                    (b"\x00" * 126 + b"\xff\x00\x00", 0), (b"\x00" * 63 + b"\xff" + b"\x00" * 63 + b"\xff\x7f", 2)):
        assert sc.ff_places(m, 64) == want
    assert sc.ff_places(b"\x00" * 127 + b"\xff\x00", 128) == 1


@pytest.mark.parametrize("cls", list(sc.CLASSES))
def test_each_class_decodes_with_the_oracle(cls):
    """the expectations are the oracle's answer on the very bytes: decoded again here, independently of what Entry stored"""
    ob = sc.fc._ob()
    for e in sc.pool(cls)[::7]:
        if e.coded:
            ok, dec = ob.ht_decode(e.data, e.w, e.h, e.w, e.mm)
            assert bool(ok) == bool(e.ok)
            want = ob.dequant_rev(dec, e.kmax) if ok else np.zeros((e.h, e.w), np.int32)
            assert np.array_equal(e.expect(True), want)
        else:
            assert e.ok and not e.expect(False).any()


def test_every_launch_holds_the_block_kinds():
    used = {c: set() for c in sc.CLASSES}
    for L in sc.launches() + [L for L, _ in sc.sequences()]:
        used[L.cls] |= {id(e) for e in L.entries}
        W = sc.CLASSES[L.cls]
        assert all(e.w <= max(W) for e in L.entries) and {d["reversible"] for d in L.descs} == {1 if L.rev else 0}
        e0 = L.entries[0]
        assert e0.coded and e0.ok and 2 <= e0.len1 < 34 and L.descs[0]["data_off"] == 0
        assert all(d["data_off"] == sum(len(e.data) for e in L.entries[:i]) for i, d in enumerate(L.descs)), "no padding"
        if L.n >= 12:
            assert sum(1 for e in L.entries if e.early_refused) >= 2, L.tag
            assert sum(1 for e in L.entries if not e.coded and e.w and e.h) >= 2, L.tag
            assert sum(1 for e in L.entries if e.late_refused) >= 2, L.tag
            assert sum(1 for e in L.entries if e.ok and (e.kind == "big" or len(e.magsgn) > 2048)) >= 2, L.tag
    for c in sc.CLASSES:
        assert used[c] >= {id(e) for e in sc.pool(c)}, "a pool block of class %s that no launch decodes" % c
    # sequences: positions that change between coded and not from one run to the next
    q = [L for L, _ in sc.sequences()]
    a, b = q[0].entries, q[1].entries
    assert sum(1 for x, y in zip(a, b) if x.coded and x.ok and (not y.coded or not y.ok)) >= 20
    assert sum(1 for x, y in zip(a, b) if (not x.coded or not x.ok) and y.coded and y.ok) >= 20
    assert {L.rev for L in q} == {True, False} and q[0].n > q[2].n > q[4].n and len(q) == 6


@pytest.mark.parametrize("cls", ["w16", "w32"])
def test_mixed_wavefronts_hold_what_they_are_there_for(cls):
    L = next(L for L in sc.launches() if L.cls == cls and hasattr(L, "groups"))
    G = dict(L.groups)
    at = 0
    for name, g in L.groups:                                 # every group starts a wavefront of four (and one of two)
        assert at % 4 == 0 and L.entries[at:at + len(g)] == g
        at += len(g)
    assert at == L.n and L.n % 4 == 3
    acc = lambda e: e.coded and e.ok
    pairs = lambda g: [g[:2], g[2:]]
    for part in (lambda g: [g], pairs):                      # ... as one wavefront of four, and as two of two
        assert all({e.h for e in p} == {1, 64} for p in part(G["heights 1 and 64"]))
        assert all({e.kmax for e in p} == {1, 30} and all(acc(e) for e in p) for p in part(G["K_max 1 and 30"]))
        assert all({(e.w, e.h) for e in p if e.kind != "big"} == {(1, 1)} and {e.kmax for e in p if e.kind == "big"} == {30} and
                   len([e for e in p if e.kind == "big"]) == len(p) // 2 for p in part(G["K_max 30 full amplitude beside 1 x 1"]))
    for name in ("early, late, uncoded, accepted", "accepted, uncoded, late, early"):
        g = G[name]
        assert sum(e.early_refused for e in g) == sum(e.late_refused for e in g) == sum(acc(e) for e in g) == sum(not e.coded for e in g) == 1
    assert all(e.kind == "big" and acc(e) and e.w in sc.FULL[cls] and len(e.magsgn) > 3000 for e in G["four big"])
    assert not any(acc(e) for e in G["nothing decodes"]) and all(e.late_refused for e in G["all refused late"])
    assert sum(1 for e in G["0xFF at a chunk end beside short blocks"] if sc.chunk_ff(e, sc.CHUNK[cls])) == 2
    for pos in range(4):
        for kind in ("early", "late"):
            g = G["%s-refused at position %d" % (kind, pos)]
            assert [getattr(e, kind + "_refused") for e in g] == [j == pos for j in range(4)]
            assert all(acc(e) and e.expect(True).any() for j, e in enumerate(g) if j != pos)
    # the widest blocks of the class are among the accepted neighbours: every lane of a segment is live somewhere
    assert sum(1 for e in L.entries if acc(e) and e.w == max(sc.CLASSES[cls])) >= 12


def test_verify_notices_what_it_should():
    """the comparison itself (fused_cases.Launch.problems on a launch of this file): a wrong word inside a rectangle, one
    outside, one verdict"""
    L = sc.launches()[8]
    want = sc.expected(L)
    assert not L.problems(L.status, want)
    i = next(i for i, e in enumerate(L.entries) if e.w >= 2 and e.h >= 2)
    for ix in (L.rects[i][0] + 1, L.rects[i][0] + L.entries[i].w, L.size - 1, 0):
        got = want.copy()
        got[ix] ^= 1
        assert L.problems(L.status, got)
    st = L.status.copy()
    st[3] ^= 1
    assert L.problems(st, want)
