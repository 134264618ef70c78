"""Two product sets, a cut per schedule and the counter clear on the side stream (include/ojphgpu.h, "what a run leaves";
ojphgpu_objects.h): an encoder whose runs are released holds arena, output, results and counters twice, every released run
takes the set the run before it did not use and waits only for the run two back, a released run cuts the top resolution's
blocks where OJPHGPU_ENC_TOP_SHARE_RELEASED says and a joined one where the model does, and a block's output region goes by
its index among all blocks.  What can go wrong: a run that starts on a set still being coded into, an accessor that reads
the other set or waits for one set only, a region whose capacity was summed by another index than the kernel uses, a
counter clear that overtakes a launch still counting.  Every codestream is compared byte for byte with the oracle
pipeline's.

Frames: 192 x 160 x 3 (three decompositions, 64 x 64 blocks, 36 blocks of the top resolution: the smallest frame that forks;
its 63 blocks share one output cursor) and 320 x 256 x 3 with the same parameters (84 blocks, 54 of the top resolution: the
smallest with all 16 output regions in use)."""
import contextlib
import gc
import hashlib
import json
import os

import numpy as np
import pytest

from tests.synth import synth_image

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NC = 3
SIZES = {"small": (192, 160, 36), "big": (320, 256, 54)}   # width, height, blocks of the top resolution
KINDS = {
    "irv97_12b": dict(bit_depth=12, reversible=False, qstep=0.002, num_decomps=3, block=(64, 64)),
    "rev53_8b_rct": dict(bit_depth=8, reversible=True, color_transform=True, num_decomps=3, block=(64, 64)),
}
CASES = [(k, s) for k in sorted(KINDS) for s in sorted(SIZES)]
_REF = {}


def _params(kind, size):
    from openjph_amd.plan import make_params
    w, h, _ = SIZES[size]
    return make_params(w, h, NC, **KINDS[kind])


def ref(kind, size):
    """computed once and shared: three different frames and the oracle's codestream of each"""
    if (kind, size) not in _REF:
        from tests import cpu_pipeline as cp
        w, h, _ = SIZES[size]
        frames = [synth_image(NC, h, w, KINDS[kind]["bit_depth"], seed=s) for s in (5, 6, 7)]
        want = [cp.encode(f, **KINDS[kind])[0] for f in frames]
        assert len(set(want)) == 3
        _REF[(kind, size)] = dict(frames=frames, want=want)
    return _REF[(kind, size)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def released(kind, size, **knobs):
    """an encoder whose plain runs are released, created under the given knobs (they are read at creation)"""
    from openjph_amd import codec
    with env(**knobs):
        enc = codec.Encoder(_params(kind, size))
    enc.set_timing(False)
    return enc


def run_over(enc, d, frame, junk):
    """one released run from the staging tensor d, which is overwritten behind the run"""
    d.copy_(frame)
    enc.run_device(d)
    d.fill_(junk)
    assert enc.pending()


@pytest.mark.parametrize("kind,size", CASES)
@pytest.mark.parametrize("every", [0, 1, 2], ids=["finish_last", "finish_every", "finish_every_second"])
def test_runs_back_to_back(kind, size, every):
    """a b c a b with no accessor between the runs, with finish() after every run, after every second one"""
    r = ref(kind, size)
    frames = [dev(f) for f in r["frames"]]
    enc = released(kind, size)
    d = frames[0].clone()
    order = [0, 1, 2, 0, 1]
    for k, i in enumerate(order):
        run_over(enc, d, frames[i], k - 3)
        if every and (k + 1) % every == 0:
            assert enc.finish() == r["want"][i], "run %d" % k
            assert not enc.pending()
    assert enc.finish() == r["want"][order[-1]]
    assert not enc.pending()


@pytest.mark.parametrize("in_flight", [2, 3])
def test_destroyed_with_runs_in_flight(in_flight):
    kind, size = "irv97_12b", "big"
    r = ref(kind, size)
    frames = [dev(f) for f in r["frames"]]
    enc = released(kind, size)
    for k in range(in_flight):
        enc.run_device(frames[k])
    assert enc.pending()
    del enc                                                # no accessor call: destroy waits for the object's streams itself
    gc.collect()
    fresh = released(kind, size)
    fresh.run_device(frames[1])
    assert fresh.finish() == r["want"][1]


@pytest.mark.parametrize("kind,size", CASES)
def test_one_object_alternating_schedules(kind, size):
    """released a, joined b, released a, released b, joined a: every codestream, the cut of each run, nothing pending behind
    a joined run or an accessor"""
    r = ref(kind, size)
    a, b = dev(r["frames"][0]), dev(r["frames"][1])
    ntop = SIZES[size][2]
    enc = released(kind, size, OJPHGPU_ENC_TOP_SHARE_RELEASED=30, OJPHGPU_ENC_TOP_SHARE=None)
    cut_released = ntop * 30 // 100
    cut_joined = None
    for k, (frame, want, joined) in enumerate([(a, 0, False), (b, 1, True), (a, 0, False), (b, 1, False), (a, 0, True)]):
        enc.set_timing(joined)
        enc.run_device(frame)
        assert enc.pending() == (not joined), "run %d" % k
        assert enc.finish() == r["want"][want], "run %d" % k
        assert not enc.pending()
        if joined:
            cut_joined = cut_joined or enc.top_blocks()
            assert enc.top_blocks() == cut_joined and cut_joined != cut_released and 0 < cut_joined <= ntop
        else:
            assert enc.top_blocks() == cut_released
    # released, released, then a joined run while both are in flight: it waits for both sets
    enc.set_timing(False)
    enc.run_device(a)
    enc.run_device(b)
    enc.set_timing(True)
    enc.run_device(dev(r["frames"][2]))
    assert not enc.pending()
    assert enc.finish() == r["want"][2]


@pytest.mark.parametrize("kind,size", CASES)
def test_released_shares(kind, size):
    """encoders created under four released cuts in one process: the same bytes, the oracle's (100: the second launch holds
    no block of the top resolution)"""
    r = ref(kind, size)
    a, b = dev(r["frames"][0]), dev(r["frames"][1])
    ntop = SIZES[size][2]
    encs = [(s, released(kind, size, OJPHGPU_ENC_TOP_SHARE_RELEASED=s)) for s in (10, 50, 90, 100)]
    for _, enc in encs:
        enc.run_device(a)
        enc.run_device(b)
        enc.run_device(a)
    for s, enc in encs:
        assert enc.pending()
        assert enc.top_blocks() == ntop * s // 100, "share %d" % s
        assert enc.finish() == r["want"][0], "share %d" % s


@pytest.mark.parametrize("kind,size", CASES)
def test_one_set_against_two(kind, size):
    r = ref(kind, size)
    frames = [dev(f) for f in r["frames"]]
    one = released(kind, size, OJPHGPU_ENC_SETS=1)
    two = released(kind, size, OJPHGPU_ENC_SETS=2)
    eager = released(kind, size, OJPHGPU_ENC_SETS=1, OJPHGPU_ENC_SIDE_CLEAR=0)
    for k in (0, 1, 2, 1):
        for enc in (one, two, eager):
            enc.run_device(frames[k])
    n = [enc.coded_bytes() for enc in (one, two, eager)]
    assert n[0] == n[1] == n[2] > 0
    assert one.finish() == two.finish() == eager.finish() == r["want"][1]


def test_budget_on_and_off_an_object_with_two_sets():
    """set_budget(B), run, set_budget(0), two released runs, set_budget(B) while both are in flight: the budgeted results are
    the committed ones, the plain ones the oracle's"""
    from openjph_amd import codec
    from openjph_amd.plan import make_params
    from tests import rate_cases as rc
    gold = json.load(open(os.path.join(HERE, "golden", "rate_sizes.json")))["cases"]["A"]
    c = rc.CASES["A"]
    params = make_params(c["w"], c["h"], c["nc"], **rc.case_kwargs("A"))
    frame, _ = rc.case_image("A")
    other = np.roll(frame, 5, axis=-1)
    budget = rc.budgets("A")[0][1]
    g = gold["budgets"][str(budget)]
    with env(OJPHGPU_ENC_SETS=None):
        enc = codec.Encoder(params, max_bytes=budget)
    enc.set_timing(False)
    enc.run_device(dev(frame))
    assert not enc.pending()
    assert hashlib.sha256(enc.finish()).hexdigest() == g["sha256"] and enc.rate_info()["grid_index"] == g["j"]
    enc.set_budget(0)
    plain = codec.Encoder(params)
    want = [plain.encode(frame), plain.encode(other)]
    assert want[0] != want[1]
    enc.run_device(dev(frame))
    enc.run_device(dev(other))
    assert enc.pending()
    enc.set_budget(budget)
    assert not enc.pending()
    enc.run_device(dev(frame))
    assert not enc.pending()
    assert hashlib.sha256(enc.finish()).hexdigest() == g["sha256"]
    enc.set_budget(0)
    enc.run_device(dev(frame))
    enc.run_device(dev(other))
    enc.run_device(dev(frame))
    assert enc.pending()
    assert enc.finish() == want[0]
    enc.run_device(dev(other))
    assert enc.finish() == want[1]


@pytest.mark.parametrize("size", sorted(SIZES))
def test_step_shape_thirty_times(size):
    """the benchmark's step: a released encode, then the decode of a fixed codestream on the same stream, which runs beside
    the coder of this run and of the one before it; the encoder's frames alternate"""
    import torch
    from openjph_amd import codec
    from tests import cpu_pipeline as cp
    kind = "irv97_12b"
    r = ref(kind, size)
    cs = r["want"][2]
    samples, _ = cp.decode(cs)
    want = dev(samples)
    enc = released(kind, size)
    dec = codec.Decoder(cs)
    dec.set_timing(False)
    frames = [dev(r["frames"][0]), dev(r["frames"][1])]
    d_out = torch.zeros_like(frames[0])
    for k in range(30):
        enc.run_device(frames[k & 1])
        dec.run_device(d_out)
        assert enc.pending()
        assert dec.failed_blocks() == 0, "step %d" % k
        assert torch.equal(d_out, want), "step %d" % k
        d_out.zero_()
        if k % 5 == 4:
            assert enc.finish() == r["want"][k & 1], "step %d" % k
    assert dec.fused_retries() == 0


def test_c_abi_block_encoder_is_unchanged():
    """ojphgpu_ht_encode passes 0 for the index of its first descriptor and has one cursor: every block's bytes are the
    oracle's, and the slots are what a single cursor hands out -- 4-byte aligned, disjoint, together the whole output"""
    from tests.test_gpu_enc_startup import _block, _check, _launch
    rng = np.random.default_rng(21)
    spec = [(64, 64, "rev"), (32, 32, "irv"), (128, 32, "rev"), (64, 64, "s64"), (0, 16, "rev"), (64, 64, "irv"),
            (20, 20, "rev"), (100, 16, "irv"), (64, 33, "irv"), (31, 64, "rev"), (48, 48, "s64"), (96, 8, "rev")] * 2
    blocks = [_block(rng, w, h, 20 if kind == "s64" else 10, kind, 0.6, 500) for (w, h, kind) in spec]
    res, out, status = _launch(blocks)
    assert status == 0
    _check(blocks, res, out)
    slots = sorted((int(o), (int(n) + 3) & ~3) for o, n in res if n)
    assert all(o % 4 == 0 for o, _ in slots)
    assert slots[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(slots, slots[1:]))
    assert slots[-1][0] + slots[-1][1] == len(out) == sum((len(b[-1]) + 3) & ~3 for b in blocks)
