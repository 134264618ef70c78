"""The block encoder's kernels, launch form by launch form (ojphgpu_ht_encode_ex: what the encoder objects launch): every
launch of tests/enc_cases.py -- each width class under its truthful `widths` and under every valid coarsening that changes the
kernels, launches of mixed classes, output regions that fit exactly, that are 4 bytes short and that are chosen by `first`,
one array coded in two launches, a scratch slot that is too small -- every block's bytes against the oracle's, and every
byte of the output and the scratch that nobody should have written against the sentinel it was filled with.
tests/test_cpu_enc_cases.py shows that these launches reach what they claim."""
import numpy as np
import pytest

from tests import enc_cases as ec

pytestmark = pytest.mark.gpu


def _stage(L):
    import torch
    from openjph_amd import codec
    return codec.EncodeStage(L.desc_array(codec.cb_desc_dtype), torch.from_numpy(L.coef).cuda(), L.scratch_bytes, L.out_cap, L.regions)


def _run(L):
    import torch
    from openjph_amd import codec
    return codec.ht_encode(L.desc_array(codec.cb_desc_dtype), torch.from_numpy(L.coef).cuda(), L.scratch_bytes, L.out_cap,
                           widths=L.widths, regions=L.regions, first=L.first)


def problems(L, got, may_fail=(), no_request=()):
    """what differs from the oracle and from the contract, as text (empty: nothing).  L.fails: blocks that must report (0, 0);
    may_fail: blocks that are right or (0, 0); no_request: failing blocks that never asked for a slot"""
    from openjph_amd import codec
    res, out, status, scratch, cursor = got
    S = codec.EncodeStage.SENTINEL
    bad = []
    if (status != 0) != bool(L.fails or may_fail):
        bad.append("status %d" % status)
    claimed = np.zeros(len(out), bool)
    slots, asked = [], [0] * max(L.nreg, 1)
    for i, b in enumerate(L.blocks):
        o, n = int(res[i, 0]), int(res[i, 1])
        r = ec.Launch.region_of(i, L.nreg, L.first)
        if b.want and i not in no_request:
            asked[r] += b.slot
        if (o, n) == (0xFFFFFFFF, 0xFFFFFFFF):
            bad.append("block %d (%s %dx%d %s): result never written" % (i, b.cls, b.w, b.h, b.tag))
            continue
        if i in L.fails or not b.want or (i in may_fail and (o, n) == (0, 0)):
            if (o, n) != (0, 0):
                bad.append("block %d (%s %dx%d %s): (%d, %d), expected (0, 0)" % (i, b.cls, b.w, b.h, b.tag, o, n))
            continue
        base, cap = L.region_span(r)
        if o % 4 or o < base or o + b.slot > base + cap or n != len(b.want):
            bad.append("block %d (%s %dx%d K %d %s): offset %d length %d, expected %d bytes inside region %d = [%d, %d)" % (
                i, b.cls, b.w, b.h, b.kmax, b.tag, o, n, len(b.want), r, base, base + cap))
            continue
        if out[o:o + n].tobytes() != b.want:
            g = np.frombuffer(out[o:o + n].tobytes(), np.uint8); w = np.frombuffer(b.want, np.uint8)
            k = int(np.nonzero(g != w)[0][0])
            bad.append("block %d (%s %s %dx%d K %d %s): bytes differ from byte %d of %d (MagSgn %d, Scup %d)" % (
                i, b.cls, b.kind, b.w, b.h, b.kmax, b.tag, k, n, len(b.magsgn), b.scup))
        if claimed[o:o + b.slot].any():
            bad.append("block %d: its slot [%d, %d) overlaps another" % (i, o, o + b.slot))
        claimed[o:o + b.slot] = True
        slots.append((o, b.slot))
    if not bad:
        if [int(c) for c in cursor] != asked:
            bad.append("cursors %s, the regions' slot sizes are %s" % ([int(c) for c in cursor], asked))
    stray = np.nonzero((out != S) & ~claimed)[0]
    if len(stray):
        bad.append("%d output bytes outside the claimed slots were written, first at %d" % (len(stray), int(stray[0])))
    mine = np.zeros(len(scratch), bool)
    for (so, cap) in L.slots:
        mine[so:so + cap] = True
    stray = np.nonzero((scratch != S) & ~mine)[0]
    if len(stray):
        bad.append("%d scratch bytes outside the blocks' slots were written, first at %d" % (len(stray), int(stray[0])))
    return bad


def _check_all(launches):
    bad = []
    for L in launches:
        bad += ["%s (widths %d): %s" % (L.tag, L.widths, p) for p in problems(L, _run(L))[:4]]
    assert not bad, "\n".join(bad[:24])


CLASSES = [(c, k) for c in ec.NARROW + ("over128", "s64") for k in ec.class_kinds(c)]


@pytest.mark.parametrize("cls,kind", CLASSES, ids=["%s-%s" % ck for ck in CLASSES])
def test_class_launches(cls, kind):
    """1 .. 33 blocks of one class and wavelet under the truthful widths and under each coarsening that changes the kernels"""
    _check_all(ec.class_launches(cls, kind))


def test_mixed_launches():
    """the instantiations skip each other's blocks in one launch: w32 + w128 in both wavelets, the same with blocks of the
    64-bit path, w64 + blocks of more than 128 columns"""
    _check_all(ec.mixed_launches())


def test_regions_that_fit_exactly():
    """20 blocks in 0, 1, 2 and 16 regions, each exactly as large as its blocks, with first = 0, 3 and 37"""
    _check_all(ec.region_launches())


def test_regions_4_bytes_short():
    (a, fa), (b, fb) = ec.short_region_launches()
    bad = problems(a, _run(a))
    assert not bad, "\n".join(bad)
    got = _run(b)
    bad = problems(b, got, may_fail=fb)
    assert not bad, "\n".join(bad)
    assert any(tuple(got[0][i]) == (0, 0) for i in fb)


@pytest.mark.parametrize("cls", ec.NARROW)
def test_scratch_slot_to_the_dword(cls):
    """A block that outgrows the stage flushes whole dwords of MagSgn bytes to its scratch slot.  How far is read, not restated:
    with a roomy slot over the sentinel the written prefix of the slot is F bytes, a multiple of 4 and the oracle's first F MagSgn
    bytes.  A slot of VLC_CAP + F bytes then suffices, byte-right; one of VLC_CAP + F - 4 does not: the block reports (0, 0),
    asks for no output slot and sets the status, its neighbours in the workgroup are right."""
    from openjph_amd import codec
    S = codec.EncodeStage.SENTINEL
    L = ec.scratch_launch(cls)
    got = _run(L)
    bad = problems(L, got)
    assert not bad, "\n".join(bad)
    so, cap = L.slots[1]
    slot = got[3][so:so + cap]
    written = np.nonzero(slot != S)[0]
    F = (int(written[-1]) + 4) & ~3 if len(written) else 0
    big = L.blocks[1]
    print("%s: block of %d bytes (MagSgn %d), flushed extent %d" % (cls, len(big.want), len(big.magsgn), F))
    assert ec.OUT_STAGE - ec.VLC_CAP - 512 < F <= len(big.magsgn) and len(big.magsgn) - F < ec.OUT_STAGE
    assert slot[:F].tobytes() == big.magsgn[:F]
    for k in (0, 2, 3):                                          # the normal blocks never flush
        assert (got[3][L.slots[k][0]:L.slots[k][0] + L.slots[k][1]] == S).all()
    fits = ec.scratch_launch(cls, ec.VLC_CAP + F)
    bad = problems(fits, _run(fits))
    assert not bad, "a slot of VLC_CAP + %d bytes must suffice: %s" % (F, "\n".join(bad))
    short = ec.scratch_launch(cls, ec.VLC_CAP + F - 4, fails=(1,))
    bad = problems(short, _run(short), no_request=(1,))
    assert not bad, "a slot of VLC_CAP + %d - 4 bytes must not suffice: %s" % (F, "\n".join(bad))


def test_scratch_slots_laid_out_by_the_call():
    """scratch_caps_as_given=False: the call lays the slots out itself, roomy ones one behind the other from byte 0"""
    import torch
    from openjph_amd import codec
    from openjph_amd.csrc_consts import block_scratch_bytes
    L = ec.mixed_launches()[0]
    got = codec.ht_encode(L.desc_array(codec.cb_desc_dtype), torch.from_numpy(L.coef).cuda(), 0, L.out_cap,
                          widths=L.widths, scratch_caps_as_given=False)
    given, L.slots = L.slots, []
    try:
        off = 0
        for b in L.blocks:
            L.slots.append((off, block_scratch_bytes(b.w, b.h, 30)))
            off += L.slots[-1][1]
        assert len(got[3]) == off
        bad = problems(L, got)
    finally:
        L.slots = given
    assert not bad, "\n".join(bad)


def test_one_array_in_two_launches():
    """41 blocks in one launch, and in two at 1, 4, 5 and 40 -- each range under its own truthful widths, the second with first =
    the cut, both into the same regions, cursors and output"""
    blocks = ec.cut_blocks()
    L = ec.Launch("41 blocks, 16 regions", blocks, nreg=16)
    st = _stage(L)
    st.launch()
    whole = st.read()
    bad = problems(L, whole)
    assert not bad, "\n".join(bad)
    data = lambda got, i: got[1][int(got[0][i, 0]):int(got[0][i, 0]) + int(got[0][i, 1])].tobytes()
    for c in ec.CUTS:
        st = _stage(L)
        st.launch(0, c)
        st.launch(c, L.n - c)                                    # (first = c)
        got = st.read()
        bad = problems(L, got)                                   # (slots disjoint across both launches, cursors, sentinels)
        assert not bad, "cut at %d: %s" % (c, "\n".join(bad))
        assert all(data(got, i) == data(whole, i) == blocks[i].want for i in range(L.n)), c
        assert np.array_equal(got[4], whole[4]), c


@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irv"])
@pytest.mark.parametrize("frame", ec.FRAMES, ids=lambda f: "%dx%d-%dx%d" % (f["w"], f["h"], f["block"][0], f["block"][1]))
def test_objects_state_their_blocks_with_the_same_helper(frame, rev):
    """encoder_cut takes its bits from the helper behind ojphgpu_ht_encode_kinds: the codestream of small frames is still the
    oracle pipeline's, and the kinds of the frame's planned blocks -- per range, in the object's order (the top resolution's
    blocks first) and split at the object's cut, as encoder_cut states them -- select the layouts the frame is there for.  (What
    an object passes as `widths` cannot be read from outside; this mirrors it.)  The 256 x 96 frame's bands are 128 and 64
    columns wide: LOGP 5 and 4, each in a launch of its own; the 288 x 96 frame runs LOGP 3 and 5 in one launch."""
    from openjph_amd import codec
    from openjph_amd.plan import Plan, make_params
    from tests import cpu_pipeline as cp
    w, h = frame["w"], frame["h"]
    rng = np.random.default_rng(w + h)
    img = np.where(rng.random((1, h, w)) < 0.3, 2048, rng.integers(0, 4096, (1, h, w))).astype(np.int64)
    kw = dict(bit_depth=12, num_decomps=frame["num_decomps"], block=frame["block"], reversible=rev)
    if not rev:
        kw["qstep"] = 0.002
    enc = codec.Encoder(make_params(w, h, 1, **kw))
    assert enc.encode(img) == cp.encode(img, **kw)[0]
    n_top = enc.top_blocks()
    P = Plan(make_params(w, h, 1, **kw))
    top = P.bands["res"][P.blocks["band"]] == frame["num_decomps"]
    order = np.concatenate([np.nonzero(top)[0], np.nonzero(~top)[0]])
    assert 0 <= n_top <= int(top.sum())
    descs = np.zeros(P.num_blocks, codec.cb_desc_dtype)
    descs["w"], descs["h"], descs["reversible"] = P.blocks["w"][order], P.blocks["h"][order], 1 if rev else 0

    def stated(ws):
        return (1 if any(x <= 64 for x in ws) else 0) | (2 if any(x > 64 for x in ws) else 0) | ((4 if rev else 8) if len(ws) else 0) \
            | (0 if any(32 < x <= 64 for x in ws) else 16) | (0 if any(x > 128 for x in ws) else 64)

    logps = set()
    for part in (descs[:n_top], descs[n_top:]):
        kinds = codec.ht_encode_kinds(part)
        assert kinds == stated([int(x) for x in part["w"]])
        per_launch = [l["logp"] for l in codec.ht_encode_launches(len(part), kinds)]
        logps |= set(per_launch)
        if frame["num_decomps"] == 1:
            assert n_top == 0 and (len(part) == 0 or per_launch == [3, 5])   # both layouts over ONE range
    assert sorted(logps) == frame["logps"]
