"""A quality target in the encoder pipe (ojphgpu_enc_pipe_set_quality, include/ojphgpu.h section 6): every frame of a
sequence against the certificate of section 5c, measured with the project's own plain encoder and decoder at qstep(j), and
-- for the frames as the reference coded them -- against its recorded indices, figures and digests
(tests/golden/quality_sse.json).  Frames are the small cases of tests/rate_cases.py, rolled by k columns as in
tests/test_gpu_rate_pipe.py; every sequence is longer than depth + 2, so the slots wrap."""
import hashlib
import json
import os

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd import plan as planmod
from tests import quality_cases as qc
from tests import rate_cases as rc
from tests import test_gpu_quality as tq
from tests.test_gpu_rate_pipe import case_plan, rolled

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "quality_sse.json")))
NAMES = sorted(rc.CASES)
CAP = 12                                                     # ojphgpu_quality_search_hint: 3 + 1 + ceil(log2(238))


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def target(name, db):
    return GOLD["cases"][name]["targets"][str(db)]["max_sse"]


_ENC, _PLAIN = {}, {}


def plain(name, j, key, frame):
    """the plain encode of a frame of a case at grid index j and the int64 error sums of its int32 decode, computed once
    per (case, index, frame key); the frame as the reference coded it (key 0) is tests/test_gpu_quality.py's plain_encode"""
    from openjph_amd import codec
    if key == 0:
        return tq.plain_encode(name, j, frame)
    if (name, j, key) not in _PLAIN:
        if (name, j) not in _ENC:
            _ENC[(name, j)] = codec.Encoder(tq.case_params(name, planmod.rate_grid_qstep(j)))
        cs = _ENC[(name, j)].encode(frame)
        dec = codec.Decoder(cs)
        got = dec.plan.unpack_frame(dec.decode())
        _PLAIN[(name, j, key)] = (cs, qc.frame_error(dec.plan.unpack_frame(frame), got))
    return _PLAIN[(name, j, key)]


def run_pipe(pipe, frames, targets):
    """frames through the pipe, frame k at targets[k] (None: the one in force) -> [(codestream or OjphError, quality_info
    or None)] in order"""
    out = []

    def collect():
        try:
            cs = pipe.collect()
        except capi.OjphError as e:
            cs = e
        try:
            info = pipe.quality_info()
        except capi.OjphError:
            info = None
        out.append((cs, info))
    for f, t in zip(frames, targets):
        if t is not None:
            pipe.set_quality(max_sse=t)
        buf = pipe.acquire()
        while buf is None:
            collect()
            buf = pipe.acquire()
        np.copyto(buf, np.asarray(f).astype(buf.dtype, copy=False).reshape(buf.shape), casting="unsafe")
        pipe.submit()
    while pipe.in_flight:
        collect()
    return out


def certify(name, key, frame, cs, info, T):
    """the contract of section 5c for one frame: both sides of the certificate against the decode of a plain encode"""
    assert not isinstance(cs, Exception), cs
    j = info["grid_index"]
    assert info["qstep"] == planmod.rate_grid_qstep(j) == rc.grid_qstep(j)
    want_cs, (sse, pae) = plain(name, j, key, frame)
    assert cs == want_cs and info["bytes"] == len(cs)
    assert [c[0] for c in info["comps"]] == sse and [c[1] for c in info["comps"]] == pae
    assert info["sse"] == sum(sse) <= T and info["pae"] == max(pae)
    if j == 0:
        assert info["sse_coarser"] == 0
    else:
        _, (sse_c, _) = plain(name, j - 1, key, frame)
        assert info["sse_coarser"] == sum(sse_c) > T
    assert 1 <= info["passes"] <= CAP


def check_golden(name, cs, info, db):
    """a frame as the reference coded it: its recorded index (the recorded lists are singletons), figures and digest"""
    gold = GOLD["cases"][name]
    t = gold["targets"][str(db)]
    assert t["certified"] == [info["grid_index"]] and sha(cs) == t["sha256"]
    j = info["grid_index"]
    assert [c[0] for c in info["comps"]] == gold["sse"][j] and [c[1] for c in info["comps"]] == gold["pae"][j]


@pytest.mark.parametrize("cycle", [False, True], ids=["one_target", "target_per_frame"])
@pytest.mark.parametrize("name", NAMES)
def test_certificate_per_frame(name, cycle):
    from openjph_amd.pipeline import EncoderPipe
    n = 7
    frames = [rolled(name, k) for k in range(n)]
    dbs = [qc.TARGETS_DB[k % 4] for k in range(n)] if cycle else [40] * n
    targets = [target(name, db) for db in dbs]
    if cycle:
        pipe = EncoderPipe(case_plan(name), depth=3, max_sse=targets[0])
    else:
        pipe = EncoderPipe(case_plan(name), depth=2, min_psnr=40)
    got = run_pipe(pipe, frames, targets if cycle else [None] * n)
    pipe.close()
    assert len(got) == n
    for k, (cs, info) in enumerate(got):
        print(name, "frame", k, "target", targets[k], {a: b for a, b in info.items() if a != "comps"})
        certify(name, k, frames[k], cs, info, targets[k])
    check_golden(name, got[0][0], got[0][1], dbs[0])           # the frame as the reference coded it, no hint yet
    assert got[0][1]["first_guess"] == rc.GRID - 1
    if not cycle:                                              # one target: the search starts at the last answer
        for k in range(1, n):
            assert got[k][1]["first_guess"] == got[k - 1][1]["grid_index"]


@pytest.mark.parametrize("name,db", [("A", 40), ("C", 50), ("B", 30)])
def test_steady_state_takes_the_trials_of_the_certificate(name, db):
    from openjph_amd.pipeline import EncoderPipe
    frame = rolled(name, 0)
    T = target(name, db)
    pipe = EncoderPipe(case_plan(name), depth=2, max_sse=T)
    got = run_pipe(pipe, [frame] * 6, [None] * 6)
    pipe.close()
    certify(name, 0, frame, got[0][0], got[0][1], T)
    check_golden(name, got[0][0], got[0][1], db)
    js = got[0][1]["grid_index"]
    assert (js == 0) == (name == "B")                          # B's recorded answer at 30 dB is index 0
    for k in range(1, 6):
        cs, info = got[k]
        print(name, "frame", k, {a: b for a, b in info.items() if a != "comps"})
        assert cs == got[0][0]
        assert info["grid_index"] == js and info["first_guess"] == js
        assert info["passes"] == (1 if js == 0 else 2)          # j* and j* - 1
        assert all(info[a] == got[0][1][a] for a in ("sse", "sse_coarser", "pae", "bytes", "comps"))


@pytest.mark.parametrize("name", ["B", "E"])
def test_8_bit_containers_compare_against_int32(name):
    """B and E at 30 dB (both answer with index 0) through 8-bit containers: the figures are the reference's, from the int32
    decode.  B's decode at index 0 holds samples one past the 8-bit range (256), which a comparison in the pipe's container
    would saturate; E's does not at this index (its int32 decode spans 74 .. 253), so there the two comparisons agree and
    only the recorded figures tell."""
    from openjph_amd import codec
    from openjph_amd.pipeline import EncoderPipe
    pl = case_plan(name)
    frame = rolled(name, 0)
    T = target(name, 30)
    pipe = EncoderPipe(pl, depth=2, container=8, max_sse=T)
    got = run_pipe(pipe, [frame] * 5, [None] * 5)
    pipe.close()
    cs0, (sse, pae) = plain(name, 0, 0, frame)
    dec = codec.Decoder(cs0)
    planes = dec.plan.unpack_frame(dec.decode())
    lo, hi = min(int(np.asarray(q).min()) for q in planes), max(int(np.asarray(q).max()) for q in planes)
    print(name, "decoded range at index 0:", lo, hi)
    if name == "B":
        assert hi == 256                                       # one past the range
    sat_sse, _ = qc.frame_error(dec.plan.unpack_frame(frame), [np.clip(q, 0, 255) for q in planes])
    assert (sat_sse != sse) == (lo < 0 or hi > 255)            # (what a saturated comparison would have reported)
    for k, (cs, info) in enumerate(got):
        print(name, "frame", k, {a: b for a, b in info.items() if a != "comps"}, "saturated:", sum(sat_sse))
        certify(name, 0, frame, cs, info, T)
        check_golden(name, cs, info, 30)
        assert info["grid_index"] == 0 and [c[0] for c in info["comps"]] == sse
        assert name != "B" or [c[0] for c in info["comps"]] != sat_sse
        assert info["passes"] == (2 if k == 0 else 1)           # 240 and 0 without a hint; then index 0 alone


def test_an_unreachable_target_inside_a_sequence():
    from openjph_amd.pipeline import EncoderPipe
    name = "D"
    frame = rolled(name, 0)
    T40 = target(name, 40)
    total = [sum(s) for s in GOLD["cases"][name]["sse"]]
    assert total[-1] == 3284
    targets = [T40, 3283, 3284, T40, T40, T40]
    pipe = EncoderPipe(case_plan(name), depth=2, max_sse=targets[0])
    got = run_pipe(pipe, [frame] * len(targets), targets)
    pipe.close()
    for k, (cs, info) in enumerate(got):
        print("frame", k, cs if isinstance(cs, Exception) else len(cs), info and {a: b for a, b in info.items() if a != "comps"})
    certify(name, 0, frame, got[0][0], got[0][1], T40)
    check_golden(name, got[0][0], got[0][1], 40)
    j0 = got[0][1]["grid_index"]
    err, info = got[1]
    assert isinstance(err, capi.OjphError) and err.code == capi.E_QUALITY
    assert info is not None and 1 <= info["passes"] <= CAP and info["comps"] == []
    assert info["first_guess"] == j0                            # the hint: the last frame that was certified
    certify(name, 0, frame, got[2][0], got[2][1], 3284)
    assert got[2][1]["grid_index"] in qc.certified(total, 3284)
    assert got[2][1]["first_guess"] == j0                       # ... which the failed frame has not moved
    for k in (3, 4, 5):
        certify(name, 0, frame, got[k][0], got[k][1], T40)
        check_golden(name, got[k][0], got[k][1], 40)
    assert got[3][1]["first_guess"] == got[2][1]["grid_index"]
    assert got[5][1]["passes"] == 2 and got[5][1]["first_guess"] == j0


def test_scene_cut():
    from openjph_amd.pipeline import EncoderPipe
    from tests.synth import synth_image
    name = "A"
    c = rc.CASES[name]
    img = rolled(name, 0)
    frames = [img, np.full_like(img, 1000), synth_image(c["nc"], c["h"], c["w"], c["bd"], seed=12), img, img, img]
    keys = [0, "constant", "seed12", 0, 0, 0]
    T = target(name, 40)
    pipe = EncoderPipe(case_plan(name), depth=3, max_sse=T)
    got = run_pipe(pipe, frames, [None] * len(frames))
    pipe.close()
    for k, (cs, info) in enumerate(got):
        print("frame", k, {a: b for a, b in info.items() if a != "comps"})
        certify(name, keys[k], frames[k], cs, info, T)
        if k:
            assert info["first_guess"] == got[k - 1][1]["grid_index"]
    for k in (0, 3, 4, 5):
        check_golden(name, got[k][0], got[k][1], 40)
    assert got[5][1]["passes"] == 2


def test_hand_over_forms():
    from openjph_amd.pipeline import EncoderPipe, pack_bits
    n = 6
    for name, forms in (("A", [dict(pixels=(16, True)), dict(packed=12)]), ("B", [dict(pixels=(8, False))])):
        targets = [target(name, (30, 40, 50)[k % 3]) for k in range(n)]
        frames = [rolled(name, 3 * k) for k in range(n)]
        planar = EncoderPipe(case_plan(name), depth=2, max_sse=targets[0])
        want = run_pipe(planar, frames, targets)
        planar.close()
        check_golden(name, want[0][0], want[0][1], 30)
        for form in forms:
            pipe = EncoderPipe(case_plan(name), depth=3, max_sse=targets[0], **form)
            handed = [pack_bits(f, form["packed"]) if "packed" in form else f.transpose(1, 2, 0) for f in frames]
            got = run_pipe(pipe, handed, targets)
            pipe.close()
            for k in range(n):
                assert got[k][0] == want[k][0], (name, form, k)
                assert got[k][1] == want[k][1] and got[k][1]["bytes"] == len(got[k][0]), (name, form, k)
                assert got[k][1]["sse"] <= targets[k]


def test_encode_sequence_with_targets():
    from openjph_amd.pipeline import EncoderPipe
    name = "D"
    frames = [rolled(name, k) for k in range(6)]
    targets = [target(name, (40, 50, 30)[k % 3]) for k in range(6)]
    pipe = EncoderPipe(case_plan(name), depth=2)
    got = list(pipe.encode_sequence(frames, targets=iter(targets)))     # (the first target switches the mode on)
    check = EncoderPipe(case_plan(name), depth=2, max_sse=targets[1])
    want = run_pipe(check, frames, targets)
    check.close()
    assert got == [cs for cs, _ in want]
    for k, (cs, info) in enumerate(want):
        certify(name, k, frames[k], cs, info, targets[k])
    check_golden(name, want[0][0], want[0][1], 40)
    one = list(pipe.encode_sequence(frames, targets=targets[1]))         # a scalar: one target for every frame
    check = EncoderPipe(case_plan(name), depth=2, max_sse=targets[1])
    assert one == [cs for cs, _ in run_pipe(check, frames, [None] * 6)]
    check.close()
    assert sha(one[0]) == GOLD["cases"][name]["targets"]["50"]["sha256"]
    with pytest.raises(ValueError):
        list(pipe.encode_sequence(frames[:4], targets=targets[:2]))
    while pipe.in_flight:                                      # what was submitted before the targets ended
        pipe.collect()
    with pytest.raises(ValueError):
        list(pipe.encode_sequence(frames, budgets=100000, targets=targets[1]))
    with pytest.raises(capi.OjphError) as e:
        list(pipe.encode_sequence([frames[0]] * 3, targets=[targets[0], 3283, targets[0]]))
    assert e.value.code == capi.E_QUALITY
    while pipe.in_flight:                                      # what was behind the frame that raised
        pipe.collect()
    pipe.close()


def test_refusals():
    from openjph_amd.pipeline import EncoderPipe
    from openjph_amd.plan import make_params
    ok = dict(bit_depth=8, reversible=False)
    for kw in (dict(bit_depth=8, reversible=True), dict(ok, qfactor=85), dict(ok, coc={1: dict(reversible=True)}),
               dict(ok, qfactors={0: ("Y", 80)}),
               dict(ok, atk={2: dict(steps=[-0.443506852, -0.882911075, 0.052980118, 1.586134342], K=1.230174105)}, wavelet=2),
               dict(ok, dfs={1: [1, 2, 3]}, coc={0: dict(dfs=1, num_decomps=3)}, num_decomps=3),
               dict(bit_depth=17, reversible=False), dict(ok, bit_depths=[8, 17, 8])):
        deep = kw.get("bit_depth") == 17 or "bit_depths" in kw
        pipe = EncoderPipe(params=make_params(128, 128, 3, **kw), depth=2, container=32 if deep else 16)
        with pytest.raises(capi.OjphError) as e:
            pipe.set_quality(max_sse=10000)
        assert e.value.code == capi.E_INVALID, kw
        with pytest.raises(capi.OjphError) as e:
            EncoderPipe(params=make_params(128, 128, 3, **kw), depth=2, container=32 if deep else 16, max_sse=10000)
        assert e.value.code == capi.E_INVALID, kw
        pipe.close()
    name = "B"
    frame = rolled(name, 0)
    T = target(name, 40)
    inr, below, above = rc.budgets(name)
    pipe = EncoderPipe(case_plan(name), depth=2)                  # a plain pipe: no target once frames are handed out
    pipe.acquire()
    with pytest.raises(capi.OjphError) as e:
        pipe.set_quality(max_sse=T)
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.OjphError):
        pipe.quality_info()
    pipe.close()
    pipe = EncoderPipe(case_plan(name), depth=2, max_bytes=inr[1])   # a byte budget and a target do not combine
    with pytest.raises(capi.OjphError) as e:
        pipe.set_quality(max_sse=T)
    assert e.value.code == capi.E_INVALID
    pipe.close()
    with pytest.raises(capi.OjphError) as e:
        EncoderPipe(case_plan(name), depth=2, max_bytes=inr[1], max_sse=T)
    assert e.value.code == capi.E_INVALID
    pipe = EncoderPipe(case_plan(name), depth=2, max_sse=T)
    for b in (inr[1], 0):
        with pytest.raises(capi.OjphError) as e:
            pipe.set_budget(b)
        assert e.value.code == capi.E_INVALID
    with pytest.raises(ValueError):
        pipe.set_quality(max_sse=1, min_psnr=40)
    with pytest.raises(ValueError):
        pipe.set_quality()
    with pytest.raises(capi.OjphError):
        pipe.quality_info()                                       # nothing collected yet
    with pytest.raises(capi.OjphError):
        pipe.rate_info()
    got = run_pipe(pipe, [frame] * 3, [None, 0, None])            # 0 is a target: B loses nothing from index 134 on
    pipe.set_quality(min_psnr=50)
    got += run_pipe(pipe, [frame], [None])
    check_golden(name, got[0][0], got[0][1], 40)
    for k in (1, 2):
        certify(name, 0, frame, got[k][0], got[k][1], 0)
        assert got[k][1]["sse"] == 0 and got[k][1]["pae"] == 0 and got[k][1]["grid_index"] <= 134
    check_golden(name, got[3][0], got[3][1], 50)
    pipe.close()
    pipe = EncoderPipe(case_plan(name), depth=3, max_sse=T)       # close() with frames still in flight returns
    for k in range(3):
        buf = pipe.acquire()
        np.copyto(buf, frame.astype(buf.dtype).reshape(buf.shape))
        pipe.submit()
    assert pipe.acquire() is None and pipe.in_flight == 3
    pipe.close()
