"""Released encoder runs (include/ojphgpu.h, ojphgpu_encoder_run_device): with per-launch timing off a plain single-frame run
leaves the caller's stream behind the last launch that reads the frame; the block coder and the lower transform levels go
on on two streams of the object's own, and whoever reads or overwrites the products waits for them first (encoder_settle).
What can go wrong is a consumer that does not wait, a run that starts on buffers the one before is still coding into, and a
path that must stay joined and is not.  Every codestream is compared byte for byte with the oracle pipeline's and with that
of an encoder created under OJPHGPU_NO_OVERLAP=1 (one stream, no fork).

Frames: 192 x 160, three components, three decompositions, 64 x 64 code-blocks -- 36 blocks of the top resolution (18 of
them on the side stream) and a non-empty set below: the smallest frame on which the run forks as the 8K one does."""
import gc
import hashlib
import json
import os

import numpy as np
import pytest

from tests.synth import synth_image

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, NC = 192, 160, 3
KINDS = {
    "irv97_12b": dict(bit_depth=12, reversible=False, qstep=0.002, num_decomps=3, block=(64, 64)),
    "rev53_8b_rct": dict(bit_depth=8, reversible=True, color_transform=True, num_decomps=3, block=(64, 64)),
}
NAMES = sorted(KINDS)
TILED = dict(KINDS["irv97_12b"], tile=(96, 80))            # 2 x 2 tiles; 36 top-resolution blocks again
_REF = {}


def _params(kw):
    from openjph_amd.plan import make_params
    return make_params(W, H, NC, **kw)


def ref(name):
    """computed once and shared: two frames of the kind, the oracle's codestream of each, and what an encoder that never
    forks (OJPHGPU_NO_OVERLAP=1 at creation) writes for them"""
    if name not in _REF:
        from openjph_amd import codec
        from tests import cpu_pipeline as cp
        kw = KINDS[name]
        frames = [synth_image(NC, H, W, kw["bit_depth"], seed=s) for s in (5, 6)]
        want = [cp.encode(f, **kw)[0] for f in frames]
        assert want[0] != want[1]
        old = os.environ.get("OJPHGPU_NO_OVERLAP")
        os.environ["OJPHGPU_NO_OVERLAP"] = "1"
        try:
            plain = codec.Encoder(_params(kw))
        finally:
            if old is None:
                del os.environ["OJPHGPU_NO_OVERLAP"]
            else:
                os.environ["OJPHGPU_NO_OVERLAP"] = old
        plain.set_timing(False)
        eager, nbytes = [], []
        for f in frames:
            plain.run_device(dev(f))
            assert not plain.pending()
            nbytes.append(plain.coded_bytes())
            eager.append(plain.finish())
        assert eager == want
        _REF[name] = dict(frames=frames, want=want, coded_bytes=nbytes)
    return _REF[name]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def released(kw):
    """an encoder whose plain runs are released"""
    from openjph_amd import codec
    enc = codec.Encoder(_params(kw))
    enc.set_timing(False)
    return enc


@pytest.mark.parametrize("name", NAMES)
def test_frame_overwritten_behind_the_run(name):
    r = ref(name)
    enc = released(KINDS[name])
    d = dev(r["frames"][0])
    enc.run_device(d)
    d.fill_(0)                                             # in stream order behind the run: the frame has been consumed
    assert enc.pending()                                   # (the run was released, and nothing has waited for it yet)
    assert enc.finish() == r["want"][0]
    assert not enc.pending()
    assert 0 < enc.top_blocks() < enc.plan.num_blocks      # both branches have blocks to code
    d.copy_(dev(r["frames"][1]))
    enc.run_device(d)
    d.fill_(-1 if KINDS[name]["bit_depth"] > 8 else 255)
    assert enc.finish() == r["want"][1]


@pytest.mark.parametrize("name", NAMES)
def test_runs_back_to_back(name):
    r = ref(name)
    a, b = dev(r["frames"][0]), dev(r["frames"][1])
    enc = released(KINDS[name])
    enc.run_device(a)
    enc.run_device(b)                                      # joins the first run before it clears the cursors
    assert enc.pending()
    assert enc.finish() == r["want"][1]
    one, two = released(KINDS[name]), released(KINDS[name])  # two objects taking turns on one stream
    for k in range(3):
        one.run_device(a if k % 2 == 0 else b)
        two.run_device(b if k % 2 == 0 else a)
    assert one.pending() and two.pending()
    assert one.finish() == r["want"][0] and two.finish() == r["want"][1]


@pytest.mark.parametrize("name", NAMES)
def test_caller_synchronises_its_own_stream_only(name):
    import torch
    r = ref(name)
    enc = released(KINDS[name])
    enc.run_device(dev(r["frames"][0]))
    torch.cuda.current_stream().synchronize()              # not the device: the object's streams may still be coding
    assert enc.pending()
    assert enc.coded_bytes() == r["coded_bytes"][0]
    assert not enc.pending()
    assert enc.finish() == r["want"][0]


def test_encoder_on_a_non_default_stream():
    import torch
    name = "irv97_12b"
    r = ref(name)
    d = dev(r["frames"][0])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        enc = released(KINDS[name])
        enc.run_device(d)
        d.zero_()
        assert enc.pending()
        assert enc.finish() == r["want"][0]
    s.synchronize()


@pytest.mark.parametrize("name", NAMES)
def test_step_shape_encode_then_decode_on_one_stream(name):
    """the benchmark's step at small size: the decode of a fixed codestream is enqueued behind a released encode and runs
    beside its block coder; every decode against the oracle's samples"""
    import torch
    from openjph_amd import codec
    from tests import cpu_pipeline as cp
    r = ref(name)
    cs = r["want"][1]
    samples, _ = cp.decode(cs)
    want = dev(samples)
    enc = released(KINDS[name])
    dec = codec.Decoder(cs)
    dec.set_timing(False)
    d_img = dev(r["frames"][0])
    d_out = torch.zeros_like(d_img)
    for k in range(20):
        enc.run_device(d_img)
        dec.run_device(d_out)
        assert enc.pending()
        assert dec.failed_blocks() == 0, "step %d" % k
        assert torch.equal(d_out, want), "step %d" % k
        d_out.zero_()
    assert dec.fused_retries() == 0
    assert enc.finish() == r["want"][0]


def test_tile_parts_right_after_the_run():
    from openjph_amd import codec
    from tests import cpu_pipeline as cp
    r = ref("irv97_12b")
    img = r["frames"][0]
    want = cp.encode(img, **TILED)[0]
    plan = codec.Encoder(_params(TILED)).plan
    parts, lens = cp.encode_tiles(plan, img, 0, plan.num_tiles)
    enc = released(TILED)
    d = dev(img)
    enc.run_device(d)
    assert enc.pending()
    hpart, hlens = enc.finish_tiles()
    assert bytes(hpart) == bytes(parts) and np.array_equal(hlens, np.asarray(lens, dtype=hlens.dtype))
    enc.run_device(d)
    assert enc.pending()
    dpart, dlens = enc.finish_tiles_device()
    assert dpart.cpu().numpy().tobytes() == bytes(parts) and np.array_equal(dlens, hlens)
    enc.run_device(d)
    assert enc.finish() == want


def test_destroyed_right_after_the_run():
    r = ref("irv97_12b")
    d = dev(r["frames"][0])
    for _ in range(3):
        enc = released(KINDS["irv97_12b"])
        enc.run_device(d)
        assert enc.pending()
        del enc                                            # no accessor call: destroy waits for the object's streams itself
        gc.collect()
    fresh = released(KINDS["irv97_12b"])
    fresh.run_device(d)
    assert fresh.finish() == r["want"][0]


@pytest.mark.parametrize("name", NAMES)
def test_per_launch_timing_keeps_the_join(name):
    from openjph_amd import codec
    r = ref(name)
    enc = codec.Encoder(_params(KINDS[name]))              # per-launch timing is the default
    d = dev(r["frames"][0])
    enc.run_device(d)
    assert not enc.pending()
    t = enc.timing()
    spans = t["dwt_levels_ms"] + t["ht_launches_ms"] + [t["dwt_ms"], t["ht_ms"], t["total_ms"]]
    assert len(t["dwt_levels_ms"]) >= 3 and len(t["ht_launches_ms"]) == 2
    assert all(np.isfinite(x) and x > 0 for x in spans), t
    assert t["total_ms"] >= max(t["dwt_levels_ms"][0], max(t["ht_launches_ms"]))
    assert enc.finish() == r["want"][0]
    enc.set_timing(False)                                  # the same object, released: one total, ending with the later branch
    enc.run_device(d)
    assert enc.pending()
    t = enc.timing()
    assert not enc.pending()
    assert np.isfinite(t["total_ms"]) and t["total_ms"] > 0
    assert enc.finish() == r["want"][0]
    enc.set_timing(True)
    enc.run_device(d)
    assert not enc.pending()
    assert enc.finish() == r["want"][0]


def test_searching_encoders_and_frame_pipes_stay_joined():
    """a byte budget (the search reads the planes on the caller's stream) and the encoder behind a frame pipe (its slots'
    hand-over events) produce their committed results; neither run is ever released"""
    from openjph_amd import codec
    from openjph_amd.pipeline import EncoderPipe
    from openjph_amd.plan import Plan, make_params
    from tests import rate_cases as rc
    gold = json.load(open(os.path.join(HERE, "golden", "rate_sizes.json")))["cases"]["A"]
    c = rc.CASES["A"]
    params = make_params(c["w"], c["h"], c["nc"], **rc.case_kwargs("A"))
    frame, _ = rc.case_image("A")
    budget = rc.budgets("A")[0][1]
    g = gold["budgets"][str(budget)]
    enc = codec.Encoder(params, max_bytes=budget)
    enc.set_timing(False)
    enc.run_device(dev(frame))
    assert not enc.pending()
    cs = enc.finish()
    assert enc.rate_info()["grid_index"] == g["j"] and hashlib.sha256(cs).hexdigest() == g["sha256"]
    enc.set_budget(0)                                      # the same object without the budget: a plain run, released
    enc.run_device(dev(frame))
    assert enc.pending()
    enc.set_budget(budget)                                 # ... and the budget again while that run is still coding:
    enc.run_device(dev(frame))                             # the searching run joins it before it touches a buffer
    assert not enc.pending() and hashlib.sha256(enc.finish()).hexdigest() == g["sha256"]
    plain = make_params(c["w"], c["h"], c["nc"], **rc.case_kwargs("A", 0.004))
    want = codec.Encoder(plain).encode(frame)
    pipe = EncoderPipe(Plan(params), depth=2, max_bytes=budget)
    got = list(pipe.encode_sequence([frame, frame]))
    pipe.close()
    assert all(hashlib.sha256(x).hexdigest() == g["sha256"] for x in got)
    pipe = EncoderPipe(params=plain, depth=2)
    got = list(pipe.encode_sequence([frame, np.roll(frame, 3, axis=-1)]))
    pipe.close()
    assert got[0] == want and got[1] == codec.encode(np.roll(frame, 3, axis=-1), **rc.case_kwargs("A", 0.004))
