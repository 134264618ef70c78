"""The net of tests/test_gpu_enc_forms.py is sound, without a GPU: the launches of tests/enc_cases.py state what
ojphgpu_ht_encode_kinds states, run under valid coarsenings only, reach every instantiation of the block encoder at every
grid (asked of ojphgpu_ht_encode_launches: nothing about grids is restated here), and the pools hold the content they are
there for -- each condition read from the oracle's bytes."""
import numpy as np
import pytest

from tests import enc_cases as ec


def _codec():
    from openjph_amd import codec
    return codec


def _every_launch():
    return (ec.all_launches() + [l for l, _ in ec.short_region_launches()] + [ec.scratch_launch(c) for c in ec.NARROW]
            + [ec.Launch("cut, whole", ec.cut_blocks(), nreg=16)])


def test_kinds_of_every_launch_are_the_class_statement_and_every_variant_is_a_valid_coarsening():
    codec = _codec()
    for L in _every_launch():
        truth = codec.ht_encode_kinds(L.desc_array(codec.cb_desc_dtype))
        assert truth == L.truth, (L.tag, truth, L.truth)
        assert ec.valid_coarsening(truth, L.widths), (L.tag, truth, L.widths)
        launches = ec.launches_of(L.n, L.widths)
        assert all(ec.owner(b, launches) is not None for b in L.blocks), L.tag
    for c in ec.CUTS:
        blocks = ec.cut_blocks()
        for part in (blocks[:c], blocks[c:]):
            d = ec.Launch("part", part).desc_array(codec.cb_desc_dtype)
            assert codec.ht_encode_kinds(d) == ec.stated_widths(part)
    assert codec.ht_encode_kinds(np.zeros(0, codec.cb_desc_dtype)) == 16 | 64


def test_the_ranges_of_the_cuts_state_different_things():
    blocks = ec.cut_blocks()
    assert len(blocks) == 41
    said = {ec.stated_widths(blocks)} | {ec.stated_widths(p) for c in ec.CUTS for p in (blocks[:c], blocks[c:])}
    assert len(said) >= 4
    assert {(0, 0, 5)} == set(ec.kernels_of(1, ec.stated_widths(blocks[:1])))          # the 128-column 9/7 block alone
    # with 5/3 blocks of at most 32 columns behind it: the bits do not pair widths with wavelets, four kernels
    assert [(0, 1, 3), (0, 0, 3), (0, 1, 5), (0, 0, 5)] == ec.kernels_of(4, ec.stated_widths(blocks[:4]))


def _owned(blocks, launches):
    return all(ec.owner(b, launches) is not None for b in blocks)


def _omitted_wavelet(truth, v):
    """the wavelet bit (4: 5/3, 8: 9/7) that occurs by `truth` and that `v`, stating the other one alone, leaves out; 0: none"""
    return (truth & 12) & ~v if (v & 12) in (4, 8) else 0


def _all_taken_by_the_wide_kernel(blocks, bit, launches):
    """every block of the wavelet `bit` is owned by ht_encode_wide_kernel<false>, which reads each block's transfer from its
    descriptor and so codes it whatever `widths` says of the wavelets"""
    mine = [b for b in blocks if b.kind != "s64" and (4 if b.kind == "rev" else 8) == bit]
    return all(ec.owner(b, launches) is not None and launches[ec.owner(b, launches)]["wide"] for b in mine)


def _valid_or_unnoticed(truth, v, blocks, launches):
    """valid by the header -- or invalid in the ONE way that leaves no block without a kernel: a single wavelet stated where
    the other occurs too, everything else about v valid, and the omitted wavelet's blocks all taken by the wide kernel"""
    if ec.valid_coarsening(truth, v):
        return True
    bit = _omitted_wavelet(truth, v)
    return bool(bit) and ec.valid_coarsening(truth, v | 12) and _all_taken_by_the_wide_kernel(blocks, bit, launches)


@pytest.mark.parametrize("cls", ec.NARROW + ("over128", "s64"))
def test_valid_by_the_header_is_every_block_owned(cls):
    """all 128 values of `widths` over a launch of 33 blocks of a class (both wavelets where it has two, and with blocks of the
    64-bit path): what the header's rules allow is exactly what leaves no block without a kernel"""
    blocks = []
    for kind in ec.class_kinds(cls):
        blocks += ec.pool(cls, kind)[:14]
    blocks = (blocks + ec.pool("s64", "rev")[:5])[:33]
    truth = ec.stated_widths(blocks)
    for v in range(128):
        launches = ec.launches_of(len(blocks), v)
        assert _owned(blocks, launches) == _valid_or_unnoticed(truth, v, blocks, launches), (cls, truth, v)
    # each wavelet alone as well: stating the other one is invalid
    for kind in ec.class_kinds(cls):
        blocks = ec.pool(cls, kind)[:33]
        truth = ec.stated_widths(blocks)
        for v in range(128):
            launches = ec.launches_of(len(blocks), v)
            assert _owned(blocks, launches) == _valid_or_unnoticed(truth, v, blocks, launches), (cls, kind, truth, v)


def test_the_headers_example_of_an_invalid_value():
    """bit 4 set with a 40-column block present: no instantiation owns the block"""
    b = ec.Blk("w64", "x", (40, 8, 9, "rev", np.zeros(0, np.int32), 64, 0.0, b""))
    truth = ec.stated_widths([b])
    assert not truth & 16 and not ec.valid_coarsening(truth, truth | 16)
    assert ec.owner(b, ec.launches_of(1, truth | 16)) is None and ec.owner(b, ec.launches_of(1, truth)) == 0


INSTANTIATIONS = [(0, 1, 3), (0, 0, 3), (0, 1, 4), (0, 0, 4), (0, 1, 5), (0, 0, 5), (1, 0, 0), (1, 1, 0)]


def test_every_instantiation_at_every_grid():
    """narrow {rev, irv} x {3, 4, 5}, wide<false>, wide<true>: each codes blocks in launches of 1, 2, 8 and 9 workgroups and with
    every number of wavefronts in the last workgroup"""
    wgs = {k: set() for k in INSTANTIATIONS}
    last = {k: set() for k in INSTANTIATIONS}
    per = {}
    for L in ec.all_launches():
        launches = ec.launches_of(L.n, L.widths)
        for i, l in enumerate(launches):
            if any(ec.owner(b, launches) == i and b.want for b in L.blocks):
                k = (l["wide"], l["flag"], l["logp"])
                wgs[k].add(l["wgs"]); last[k].add(L.n - (l["wgs"] - 1) * l["per_wg"]); per[k] = l["per_wg"]
                assert (l["wgs"] - 1) * l["per_wg"] < L.n <= l["wgs"] * l["per_wg"]
    for k in INSTANTIATIONS:
        assert {1, 2, 8, 9} <= wgs[k], (k, sorted(wgs[k]))
        assert set(range(1, per[k] + 1)) <= last[k], (k, sorted(last[k]))


def test_the_stage_entry_alone_never_runs_the_8_by_8_or_the_32_by_2_layout():
    for n in ec.N_LIST:
        assert ec.kernels_of(n, 3 | 32) == [(0, 1, 4), (0, 0, 4), (1, 0, 0), (1, 1, 0)]


def test_mixed_launches_issue_the_stated_kernels_and_every_workgroup_codes_and_skips():
    for L in ec.mixed_launches():
        launches = ec.launches_of(L.n, L.widths)
        assert ec.kernels_of(L.n, L.widths) == L.kernels, L.tag
        own = [ec.owner(b, launches) for b in L.blocks]
        assert all(b.want for b in L.blocks)
        for i, l in enumerate(launches):
            places = set()
            for g in range(l["wgs"]):
                mine = [own[j] == i for j in range(g * l["per_wg"], min((g + 1) * l["per_wg"], L.n))]
                assert not all(mine) or len(mine) == 1, (L.tag, i, g)                  # a wavefront that skips
                # (five kernels cannot all code in a workgroup of four wavefronts: there, in four workgroups out of five)
                assert any(mine) or len(launches) > 4 or len(mine) < l["per_wg"], (L.tag, i, g)
                places |= {j for j, m in enumerate(mine) if m}
            assert places == set(range(l["per_wg"])), (L.tag, i, places)              # it codes at every wavefront position


# ---- the pools hold what they are there for -----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("cls", ec.NARROW)
def test_narrow_pools(cls, kind):
    P = ec.pool(cls, kind)
    coded = [b for b in P if b.want]
    for b in coded:
        assert 2 <= b.scup <= len(b.want)
    assert sum(1 for b in coded if len(b.want) > ec.OUT_STAGE + 2048) >= 4
    over = [b for b in coded if b.tag == "overflow"]
    assert all(len(b.want) > ec.OUT_STAGE + 2048 for b in over)
    assert any(b.w % 4 for b in over) and any((b.h % ec.ROWS_PER_STEP[cls]) for b in over)
    ff = [b for b in coded if len(b.magsgn) >= 1024 and 4 * b.magsgn.count(0xFF) >= len(b.magsgn)]
    assert len(ff) >= 2 and {int(np.sign(b.words[0])) for b in ff if b.tag == "ff"} == {1, -1}   # (both signs: int32 or float bits)
    mel = [b for b in coded if b"\xff\x7f" in b.tail]
    assert len(mel) >= 3
    for b in coded:
        if b.tag == "one sample: last":
            assert len(b.want) == 10 and b.scup == 9 and b.tail.startswith(b"\xff\x7f\xff\x7f\xff"), (b.w, b.h, b.want.hex())
    assert {b.kmax for b in coded if b.tag == "plain"} == set(range(1, 31))
    shapes = {(b.w, b.h) for b in P}
    assert set(ec._shapes(cls)) <= shapes
    for t in ec.FIRST_ROW_KINDS:
        assert any(b.tag == t and b.want and b.w == ec.FULL_W[cls] for b in P), t
    rps = ec.ROWS_PER_STEP[cls]
    banded = [b for b in P if b.tag == "banded"]
    assert {b.empty for b in banded} == set(ec.EMPTY_BANDS) | {tuple(range(8)), ()} and {b.w for b in banded} == {ec.FULL_W[cls], ec.FULL_W[cls] - 1}
    for b in banded:
        assert b.h == 8 * rps
        for s in range(8):
            assert b.rowsig[s * rps:(s + 1) * rps].any() == (s not in b.empty), (b.empty, s)
        assert bool(b.want) == (len(b.empty) < 8)
    assert {(b.w == 0, b.h == 0) for b in P if b.tag == "empty"} == {(False, True), (True, False), (True, True)}
    nothing = [b for b in P if b.tag == "nothing"]
    assert len(nothing) >= 2 and all(not b.want and b.w and b.h for b in nothing)
    assert kind == "rev" or any(np.any(b.words) for b in nothing)
    assert all(b.w * b.h <= 4096 for b in P)
    if cls == "w32":
        assert all(b.w <= 32 for b in P)
    elif cls == "w64":
        assert all(b.w <= 64 for b in P) and any(32 < b.w for b in P)
    else:
        assert all(b.w == 0 or 64 < b.w <= 128 for b in P)


def test_wide_pools():
    for kind in ec.KINDS:
        P = ec.pool("over128", kind)
        assert {b.w for b in P if b.want} == {129, 256, 1000, 1024} and all(b.w > 128 and b.w * b.h <= 4096 for b in P)
    P = ec.pool("s64", "rev")
    assert {(b.w, b.h) for b in P} >= set(ec.s64_shapes()) and all(b.kind == "s64" for b in P)
    assert sum(1 for b in P if b.want) >= 12


# ---- regions ------------------------------------------------------------------------------------------------------------

def test_region_arithmetic():
    seen = set()
    for L in ec.region_launches() + [l for l, _ in ec.short_region_launches()]:
        seen.add((L.nreg, L.first))
        per = [0] * max(L.nreg, 1)
        for i, b in enumerate(L.blocks):
            r = (L.first + i) & (L.nreg - 1) if L.nreg else 0
            assert ec.Launch.region_of(i, L.nreg, L.first) == r
            per[r] += (len(b.want) + 3) & ~3
        assert per == L.sums
        short = {7: 4} if "region 7" in L.tag else {1: 4} if "region 1" in L.tag else {}
        for r in range(max(L.nreg, 1)):
            base, cap = L.region_span(r)
            assert cap == per[r] - short.get(r, 0) and base % 4 == 0
        if L.nreg:                                             # regions do not overlap
            spans = sorted(L.region_span(r) for r in range(L.nreg))
            assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= L.out_cap
    assert seen >= {(n, f) for n in (0, 1, 2, 16) for f in (0, 3, 37)}
    (a, fa), (b, fb) = ec.short_region_launches()
    assert [i for i in range(20) if ec.Launch.region_of(i, 16, 0) == 7] == list(fa) == [7] and a.blocks[7].want
    assert [i for i in range(20) if ec.Launch.region_of(i, 16, 0) == 1] == list(fb) == [1, 17] and all(b.blocks[i].slot > 4 for i in fb)


def test_region_sums_do_not_depend_on_the_cut():
    blocks = ec.cut_blocks()
    whole = ec.Launch.region_sums(blocks, 16, 0)
    for c in ec.CUTS:
        a, b = ec.Launch.region_sums(blocks[:c], 16, 0), ec.Launch.region_sums(blocks[c:], 16, c)
        assert [x + y for x, y in zip(a, b)] == whole
    assert sum(1 for s in whole if s) == 16


def test_scratch_launches():
    for cls in ec.NARROW:
        L = ec.scratch_launch(cls)
        assert L.n == 4 and not L.fails
        big = L.blocks[1]
        assert len(big.want) > ec.OUT_STAGE + 2048 and len(big.magsgn) > ec.OUT_STAGE
        assert all(len(L.blocks[i].want) + ec.VLC_CAP < ec.OUT_STAGE for i in (0, 2, 3))   # these never flush
        assert len({ec.owner(b, ec.launches_of(4, L.widths)) for b in L.blocks}) == 1      # one kernel, one workgroup
        T = ec.scratch_launch(cls, ec.VLC_CAP + 2052, fails=(1,))
        assert T.slots[1] == (L.slots[1][0], ec.VLC_CAP + 2052) and all(so % 64 == 0 for so, _ in T.slots)
