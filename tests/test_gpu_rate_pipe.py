"""A byte budget in the encoder pipe (ojphgpu_enc_pipe_set_budget, include/ojphgpu.h section 6): every frame of a sequence
against the certificate of the rate grid, measured with the project's own plain encoder, and against the reference's
recorded indices and digests (tests/golden/rate_sizes.json).  Frames are the small cases of tests/rate_cases.py; every
sequence is longer than depth + 2, so the slots and the spare output buffer wrap."""
import hashlib
import json
import os

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd import plan as planmod
from openjph_amd.plan import Plan, make_params
from tests import rate_cases as rc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "rate_sizes.json")))
NAMES = sorted(rc.CASES)


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def case_params(name, qstep=-1.0):
    c = rc.CASES[name]
    return make_params(c["w"], c["h"], c["nc"], **rc.case_kwargs(name, qstep))


_PLANS, _PLAIN = {}, {}


def case_plan(name):
    if name not in _PLANS:
        _PLANS[name] = Plan(case_params(name))
    return _PLANS[name]


def rolled(name, k):
    """the frame of a case rolled by k columns, in the layout the codec calls take (flat for the 4:2:0 case), int32"""
    img, _ = rc.case_image(name)
    if isinstance(img, list):
        return case_plan(name).pack_frame([np.roll(q, k, axis=-1) for q in img])
    return np.ascontiguousarray(np.roll(img, k, axis=-1))


def plain(name, j, frame):
    """the plain encode of a frame at qstep(j): one encoder per (case, step), shared by the tests"""
    from openjph_amd import codec
    if (name, j) not in _PLAIN:
        _PLAIN[(name, j)] = codec.Encoder(case_params(name, planmod.rate_grid_qstep(j)))
    return _PLAIN[(name, j)].encode(frame)


def run_pipe(pipe, frames, budgets):
    """frames through the pipe, frame k at budgets[k] -> [(codestream or OjphError, rate_info or None)] in order"""
    out = []

    def collect():
        try:
            cs = pipe.collect()
        except capi.OjphError as e:
            cs = e
        try:
            info = pipe.rate_info()
        except capi.OjphError:
            info = None
        out.append((cs, info))
    for f, b in zip(frames, budgets):
        if b is not None:
            pipe.set_budget(b)
        buf = pipe.acquire()
        while buf is None:
            collect()
            buf = pipe.acquire()
        np.copyto(buf, np.asarray(f).astype(buf.dtype, copy=False).reshape(buf.shape), casting="unsafe")
        pipe.submit()
    while pipe.in_flight:
        collect()
    return out


def certify(name, frame, cs, info, budget):
    """the contract of section 5b for one frame, measured with plain encodes"""
    assert not isinstance(cs, Exception), cs
    j = info["grid_index"]
    assert len(cs) == info["bytes"] <= budget
    assert info["qstep"] == planmod.rate_grid_qstep(j) == rc.grid_qstep(j)
    assert cs == plain(name, j, frame)
    if j == rc.GRID - 1:
        assert info["bytes_finer"] == 0
    else:
        assert len(plain(name, j + 1, frame)) == info["bytes_finer"] > budget
    assert 1 <= info["passes"] <= 16


def check_golden(name, cs, info, budget):
    gold = GOLD["cases"][name]["budgets"][str(budget)]
    assert info["grid_index"] == gold["j"] and sha(cs) == gold["sha256"]


@pytest.mark.parametrize("cycle", [False, True], ids=["one_budget", "budget_per_frame"])
@pytest.mark.parametrize("name", NAMES)
def test_certificate_per_frame(name, cycle):
    from openjph_amd.pipeline import EncoderPipe
    inr, below, above = rc.budgets(name)
    n = 7
    frames = [rolled(name, k) for k in range(n)]
    budgets = [inr[k % len(inr)] for k in range(n)] if cycle else [inr[1]] * n
    depth = 3 if cycle else 2
    pipe = EncoderPipe(case_plan(name), depth=depth, max_bytes=budgets[0])
    got = run_pipe(pipe, frames, budgets if cycle else [None] * n)
    pipe.close()
    assert len(got) == n
    for k, (cs, info) in enumerate(got):
        print(name, "frame", k, "budget", budgets[k], info)
        certify(name, frames[k], cs, info, budgets[k])
    check_golden(name, got[0][0], got[0][1], budgets[0])       # the frame as the reference coded it
    if not cycle:                                              # similar frames, one budget: the search starts at the last answer
        for k in range(1, n):
            assert got[k][1]["first_guess"] == got[k - 1][1]["grid_index"]


@pytest.mark.parametrize("name,which", [("A", 1), ("C", 0), ("B", "above")])
def test_steady_state_takes_the_two_trials_of_the_certificate(name, which):
    from openjph_amd.pipeline import EncoderPipe
    inr, below, above = rc.budgets(name)
    budget = above if which == "above" else inr[which]
    frame = rolled(name, 0)
    pipe = EncoderPipe(case_plan(name), depth=2, max_bytes=budget)
    got = run_pipe(pipe, [frame] * 6, [None] * 6)
    pipe.close()
    certify(name, frame, got[0][0], got[0][1], budget)
    check_golden(name, got[0][0], got[0][1], budget)
    js = got[0][1]["grid_index"]
    for k in range(1, 6):
        cs, info = got[k]
        print(name, "frame", k, info)
        assert cs == got[0][0]
        assert info["grid_index"] == js and info["first_guess"] == js
        assert info["passes"] == (1 if js == rc.GRID - 1 else 2)       # j* and j* + 1, neither coded again
        assert info["bytes"] == got[0][1]["bytes"] and info["bytes_finer"] == got[0][1]["bytes_finer"]
    assert (js == rc.GRID - 1) == (which == "above")


def test_scene_cut_and_a_frame_that_cannot_fit():
    from openjph_amd.pipeline import EncoderPipe
    from tests.synth import synth_image
    name = "A"
    c = rc.CASES[name]
    inr, below, above = rc.budgets(name)
    img = rolled(name, 0)
    frames = [img, np.full_like(img, 1000), synth_image(c["nc"], c["h"], c["w"], c["bd"], seed=12), img, img, img]
    budgets = [inr[2], above, below, inr[0], inr[0], inr[3]]
    pipe = EncoderPipe(case_plan(name), depth=3, max_bytes=budgets[0])
    got = run_pipe(pipe, frames, budgets)
    pipe.close()
    for k in (0, 1, 3, 4, 5):
        print("frame", k, got[k][1])
        certify(name, frames[k], got[k][0], got[k][1], budgets[k])
    check_golden(name, got[0][0], got[0][1], inr[2])
    assert got[1][1]["grid_index"] == rc.GRID - 1
    err, info = got[2]
    assert isinstance(err, capi.OjphError) and err.code == capi.E_BUDGET
    assert info is not None and 1 <= info["passes"] <= 16
    assert info["first_guess"] == got[1][1]["grid_index"]       # the hint: the last frame that was certified
    check_golden(name, got[3][0], got[3][1], inr[0])
    assert got[3][1]["first_guess"] == got[1][1]["grid_index"]   # ... which the failed frame has not moved
    check_golden(name, got[4][0], got[4][1], inr[0])
    assert got[4][1]["passes"] == 2
    check_golden(name, got[5][0], got[5][1], inr[3])


def test_encode_sequence_with_budgets():
    from openjph_amd.pipeline import EncoderPipe
    name = "D"
    inr, below, above = rc.budgets(name)
    frames = [rolled(name, k) for k in range(6)]
    pipe = EncoderPipe(case_plan(name), depth=2)
    budgets = [inr[k % 3] for k in range(6)]
    got = list(pipe.encode_sequence(frames, budgets=iter(budgets)))    # (the first budget switches the mode on)
    check = EncoderPipe(case_plan(name), depth=2, max_bytes=inr[1])
    want = run_pipe(check, frames, budgets)
    check.close()
    assert got == [cs for cs, _ in want]
    for k, (cs, info) in enumerate(want):
        certify(name, frames[k], cs, info, budgets[k])
    check_golden(name, want[0][0], want[0][1], budgets[0])
    one = list(pipe.encode_sequence(frames, budgets=inr[1]))
    assert sha(one[0]) == GOLD["cases"][name]["budgets"][str(inr[1])]["sha256"]
    assert all(len(cs) <= inr[1] for cs in one)
    with pytest.raises(capi.OjphError) as e:
        list(pipe.encode_sequence(frames[:3], budgets=[inr[0], below, inr[0]]))
    assert e.value.code == capi.E_BUDGET
    while pipe.in_flight:                                      # what was behind the frame that raised
        pipe.collect()
    pipe.close()


def test_hand_over_forms():
    from openjph_amd.pipeline import EncoderPipe, pack_bits
    n = 6
    for name, forms in (("A", [dict(pixels=(16, True)), dict(packed=12)]), ("B", [dict(pixels=(8, False))])):
        inr, below, above = rc.budgets(name)
        budgets = [inr[k % 3] for k in range(n)]
        frames = [rolled(name, 3 * k) for k in range(n)]
        planar = EncoderPipe(case_plan(name), depth=2, max_bytes=budgets[0])
        want = run_pipe(planar, frames, budgets)
        planar.close()
        check_golden(name, want[0][0], want[0][1], budgets[0])
        for form in forms:
            pipe = EncoderPipe(case_plan(name), depth=3, max_bytes=budgets[0], **form)
            handed = [pack_bits(f, form["packed"]) if "packed" in form else f.transpose(1, 2, 0) for f in frames]
            got = run_pipe(pipe, handed, budgets)
            pipe.close()
            for k in range(n):
                assert got[k][0] == want[k][0], (name, form, k)
                assert got[k][1]["grid_index"] == want[k][1]["grid_index"] and got[k][1]["bytes"] == len(got[k][0])


def test_refusals():
    from openjph_amd.pipeline import EncoderPipe
    ok = dict(bit_depth=8, reversible=False)
    for kw in (dict(bit_depth=8, reversible=True), dict(ok, qfactor=85), dict(ok, coc={1: dict(reversible=True)}),
               dict(ok, qfactors={0: ("Y", 80)}),
               dict(ok, atk={2: dict(steps=[-0.443506852, -0.882911075, 0.052980118, 1.586134342], K=1.230174105)}, wavelet=2),
               dict(ok, dfs={1: [1, 2, 3]}, coc={0: dict(dfs=1, num_decomps=3)}, num_decomps=3)):
        pipe = EncoderPipe(params=make_params(128, 128, 3, **kw), depth=2)
        with pytest.raises(capi.OjphError) as e:
            pipe.set_budget(10000)
        assert e.value.code == capi.E_INVALID, kw
        with pytest.raises(capi.OjphError) as e:
            EncoderPipe(params=make_params(128, 128, 3, **kw), depth=2, max_bytes=10000)
        assert e.value.code == capi.E_INVALID, kw
        pipe.close()
    name = "B"
    inr, below, above = rc.budgets(name)
    frame = rolled(name, 0)
    pipe = EncoderPipe(case_plan(name), depth=2)                  # a plain pipe: no budget once frames are handed out
    pipe.acquire()
    with pytest.raises(capi.OjphError) as e:
        pipe.set_budget(inr[1])
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.OjphError):
        pipe.rate_info()
    pipe.close()
    pipe = EncoderPipe(case_plan(name), depth=2, max_bytes=inr[1])
    with pytest.raises(capi.OjphError):
        pipe.rate_info()                                          # nothing collected yet
    got = run_pipe(pipe, [frame] * 3, [None, inr[2], None])
    with pytest.raises(capi.OjphError) as e:
        pipe.set_budget(0)                                        # ... and no way back
    assert e.value.code == capi.E_INVALID
    pipe.set_budget(inr[0])
    got += run_pipe(pipe, [frame], [None])
    pipe.close()
    for (cs, info), b in zip(got, (inr[1], inr[2], inr[2], inr[0])):
        check_golden(name, cs, info, b)


def test_plain_pipe_is_unchanged():
    from openjph_amd import codec
    from openjph_amd.pipeline import EncoderPipe
    name = "A"
    frames = [rolled(name, k) for k in range(5)]
    kw = rc.case_kwargs(name, 0.004)
    c = rc.CASES[name]
    pipe = EncoderPipe(params=make_params(c["w"], c["h"], c["nc"], **kw), depth=2)
    pipe.set_budget(0)                                            # before the first acquire: a plain pipe
    got = list(pipe.encode_sequence(frames))
    with pytest.raises(capi.OjphError):
        pipe.rate_info()
    pipe.close()
    for f, cs in zip(frames, got):
        assert cs == codec.encode(f, **kw)
