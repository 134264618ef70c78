"""A batch encoder with a byte budget per frame (ojphgpu_encoder_set_budgets, include/ojphgpu.h section 5b).  The oracle is
the single-frame budgeted encoder, which tests/test_gpu_rate.py ties to the reference's digests: every codestream of a
batch is, byte for byte, what that encoder writes for the frame and its budget, and rate_info()[f] is what it reports."""
import hashlib
import json
import os

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd import plan as planmod
from openjph_amd.plan import Plan, make_params
from tests import cpu_pipeline as cp
from tests import rate_cases as rc
from tests.synth import synth_image

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "rate_sizes.json")))
# frames per batch: A three frames at three budgets; C tiled, 32 x 32 blocks (enough of them for the 16 output regions); E
# 4:2:0; B odd sizes, one component (the statistics' scalar path at a non-zero frame offset)
FRAMES = {"A": 3, "C": 3, "E": 2, "B": 4}


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def case_params(name, qstep=-1.0):
    c = rc.CASES[name]
    return make_params(c["w"], c["h"], c["nc"], **rc.case_kwargs(name, qstep))


_FRAMES, _ORACLE = {}, {}


def frame(name, seed):
    """frame `seed` of a case in the layout the codec calls take (flat for the 4:2:0 case), int32; read-only"""
    if (name, seed) not in _FRAMES:
        c = rc.CASES[name]
        img = synth_image(c["nc"], c["h"], c["w"], c["bd"], seed=seed)
        if c.get("sub"):
            img = Plan(case_params(name)).pack_frame([np.ascontiguousarray(img[0]), np.ascontiguousarray(img[1][::2, ::2]),
                                                      np.ascontiguousarray(img[2][::2, ::2])])
        img = np.ascontiguousarray(img, dtype=np.int32)
        img.setflags(write=False)
        _FRAMES[name, seed] = img
    return _FRAMES[name, seed]


def batch(name, n=None):
    return np.stack([frame(name, 11 + f) for f in range(n or FRAMES[name])])


def oracle(name, seed, budget):
    """-> (codestream, rate_info) of the single-frame encoder with that budget; (None, None) when nothing fits.  Once."""
    from openjph_amd import codec
    key = (name, seed, budget)
    if key not in _ORACLE:
        enc = codec.Encoder(case_params(name), max_bytes=budget)
        try:
            cs = enc.encode(frame(name, seed).copy())
            _ORACLE[key] = (cs, enc.rate_info())
        except capi.OjphError as e:
            assert e.code == capi.E_BUDGET
            _ORACLE[key] = (None, None)
    return _ORACLE[key]


def budgets_of(name, shift=0):
    """case A: the triple of test_one_encoder_three_frames_three_budgets_then_none; else the per-sample budgets of the cases
    rotated over the frames, so that the frames end at different indices"""
    if name == "A" and shift == 0:
        return [37440, 150000, 9000]
    n = rc.case_samples(name)
    return [int(n * rc.BPS[(f + shift) % len(rc.BPS)]) for f in range(FRAMES[name])]


def check_against_singles(name, enc, got, budgets):
    infos = enc.rate_info()
    print(name, "budgets", budgets, "rounds", enc.rate_rounds(), "infos", infos)
    assert len(got) == len(budgets) == len(infos)
    for f, b in enumerate(budgets):
        want, info = oracle(name, 11 + f, b)
        assert want is not None and got[f] == want, (name, f, b)
        assert len(got[f]) == info["bytes"] <= b
        assert infos[f] == info, (name, f, infos[f], info)
        assert enc.rate_info(frame=f) == info
    assert 1 <= enc.rate_rounds() <= 17
    assert enc.rate_rounds() >= max(i["passes"] for i in infos)


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_batch_is_the_single_encoders(name):
    from openjph_amd import codec
    budgets = budgets_of(name)
    enc = codec.Encoder(case_params(name), frames=FRAMES[name], budgets=budgets)
    got = enc.encode(batch(name))
    check_against_singles(name, enc, got, budgets)
    assert len({i["grid_index"] for i in enc.rate_info()}) > 1            # the frames of one launch at steps of their own
    if name == "A":
        assert sha(got[0]) == GOLD["cases"]["A"]["budgets"]["37440"]["sha256"]
    for f, cs in enumerate(got):
        j = enc.rate_info()[f]["grid_index"]
        assert cs == codec.Encoder(case_params(name, planmod.rate_grid_qstep(j))).encode(frame(name, 11 + f).copy())
        dec = codec.Decoder(cs)
        out = dec.decode()
        want, _ = cp.decode(cs)
        if isinstance(want, list):
            assert all(np.array_equal(a, b) for a, b in zip(dec.plan.unpack_frame(out), want))
        else:
            assert np.array_equal(out, want)


def test_mixed_outcomes_in_one_batch():
    """a frame nothing fits fails alone, a frame everything fits ends at the finest step, and the encoder codes on"""
    from openjph_amd import codec
    name = "A"
    n = rc.case_samples(name)
    budgets = [37440, 64, 8 * n + (1 << 20)]
    enc = codec.Encoder(case_params(name), frames=3, budgets=budgets)
    enc.run_device(_to_device(batch(name)))
    with pytest.raises(capi.OjphError) as e:
        enc.finish(1)
    assert e.value.code == capi.E_BUDGET
    infos = enc.rate_info()
    print("mixed", infos, enc.rate_rounds())
    assert infos[1] is None and enc.rate_info(frame=1) is None
    for f in (0, 2):
        want, info = oracle(name, 11 + f, budgets[f])
        assert enc.finish(f) == want and infos[f] == info
    assert infos[2]["grid_index"] == rc.GRID - 1 and infos[2]["bytes_finer"] == 0
    assert oracle(name, 12, 64) == (None, None)
    assert enc.rate_rounds() <= 17
    with pytest.raises(capi.OjphError) as e:                       # all frames: the first such frame raises
        enc.encode(batch(name))
    assert e.value.code == capi.E_BUDGET
    assert enc.finish(2) == oracle(name, 13, budgets[2])[0] and enc.finish(0) == oracle(name, 11, budgets[0])[0]
    budgets = budgets_of(name)
    enc.set_budgets(budgets)                                       # ... and the encoder codes the next batch
    check_against_singles(name, enc, enc.encode(batch(name)), budgets)


def _to_device(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


@pytest.mark.parametrize("name", ["A", "B"])
def test_containers_give_the_same_bytes(name):
    from openjph_amd import codec
    budgets = budgets_of(name)
    bd = rc.CASES[name]["bd"]
    enc = codec.Encoder(case_params(name), frames=FRAMES[name], budgets=budgets)
    for dt, bits in ((np.uint8, 8), (np.uint16, 16), (np.int32, 32)):
        if bd > bits:
            continue
        got = enc.encode(batch(name).astype(dt))
        for f, b in enumerate(budgets):
            assert got[f] == oracle(name, 11 + f, b)[0], (name, np.dtype(dt).name, f)


def test_two_budget_vectors_then_none():
    from openjph_amd import codec
    name = "A"
    params = case_params(name, 0.003)
    enc = codec.Encoder(params, frames=3)
    plain = enc.encode(batch(name))
    for shift in (0, 1):
        budgets = budgets_of(name, shift)
        enc.set_budgets(budgets)
        check_against_singles(name, enc, enc.encode(batch(name)), budgets)
    enc.set_budgets([0] * 3)
    assert enc.encode(batch(name)) == plain                        # the plan's own step again
    assert plain[2] == codec.Encoder(params).encode(frame(name, 13).copy())
    with pytest.raises(capi.OjphError):
        enc.rate_info()                                            # no budgets: nothing to report


def test_refusals():
    from openjph_amd import codec
    ok = dict(bit_depth=8, reversible=False)
    params = make_params(128, 128, 3, **ok)

    def refused(enc, seq):
        with pytest.raises(capi.OjphError) as e:
            enc.set_budgets(seq)
        assert e.value.code == capi.E_INVALID, seq

    enc = codec.Encoder(params, frames=3)
    for seq in ([10000, 10000], [10000] * 4, [], [10000, 0, 10000], [0, 10000, 10000]):
        refused(enc, seq)
    refused(codec.Encoder(make_params(128, 128, 3, bit_depth=8, reversible=True), frames=2), [10000, 10000])
    refused(codec.Encoder(make_params(128, 128, 3, **dict(ok, qfactor=85)), frames=2), [10000, 10000])
    tiled = make_params(256, 256, 1, tile=(128, 128), **ok)
    refused(codec.Encoder(tiled, tiles=(0, 2)), [10000])
    with pytest.raises(capi.OjphError) as e:                       # the scalar call stays refused on a batch, also with budgets on
        enc.set_budget(10000)
    assert e.value.code == capi.E_INVALID
    enc.set_budgets([10000] * 3)
    with pytest.raises(capi.OjphError) as e:
        enc.set_budget(10000)
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.OjphError) as e:                       # a quality target is a single encoder's
        enc.set_quality(max_sse=1000)
    assert e.value.code == capi.E_INVALID
    single = codec.Encoder(params, max_sse=10 ** 6)                # a quality target set: no budgets, whichever call
    refused(single, [10000])
    with pytest.raises(capi.OjphError):
        enc.rate_info()                                            # nothing coded yet
    with pytest.raises(capi.OjphError):
        enc.rate_rounds()
    enc.run_device(_to_device(np.stack([synth_image(3, 128, 128, 8, seed=5 + f) for f in range(3)]).astype(np.int32)))
    with pytest.raises(capi.OjphError) as e:
        enc.finish_tiles()                                         # a budget is a property of the whole codestream
    assert e.value.code == capi.E_INVALID
    assert len(enc.finish(1)) <= 10000


def test_one_budget_on_a_single_frame_encoder_is_set_budget():
    from openjph_amd import codec
    name = "A"
    enc = codec.Encoder(case_params(name))
    enc.set_budgets([37440])
    assert enc.max_bytes == 37440
    cs = enc.encode(frame(name, 11).copy())
    want, info = oracle(name, 11, 37440)
    assert cs == want and enc.rate_info() == info and sha(cs) == GOLD["cases"][name]["budgets"]["37440"]["sha256"]
    assert enc.rate_rounds() == info["passes"]
    enc.set_budgets([0])
    assert enc.max_bytes == 0
    assert enc.encode(frame(name, 11)) == codec.Encoder(case_params(name)).encode(frame(name, 11).copy())
