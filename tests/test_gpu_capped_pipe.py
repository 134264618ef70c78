"""A quality target under a byte cap in the encoder pipe (ojphgpu_enc_pipe_set_quality_capped, include/ojphgpu.h section 6):
every frame of a sequence whose targets and caps move against what the single encoder writes for that frame and pair, the
frames the reference coded also against the answers the contract allows over its recorded tables (tests/capped_cases.py),
and the steady-state costs of an unchanged frame.  Frames are the small cases of tests/rate_cases.py."""
import numpy as np
import pytest

from openjph_amd import capi
from tests import capped_cases as cc
from tests import rate_cases as rc
from tests.test_gpu_capped import case_params, sha
from tests.test_gpu_rate_pipe import case_plan, rolled

pytestmark = pytest.mark.gpu


def run_pipe(pipe, frames, pairs):
    """frames through the pipe, frame k at pairs[k] = (max_sse, cap_bytes) -> [(codestream or OjphError, capped_info or None)]"""
    out = []

    def collect():
        try:
            cs = pipe.collect()
        except capi.OjphError as e:
            cs = e
        try:
            info = pipe.capped_info()
        except capi.OjphError:
            info = None
        out.append((cs, info))
    for f, (t, b) in zip(frames, pairs):
        pipe.set_quality(max_sse=t, cap_bytes=b)
        buf = pipe.acquire()
        while buf is None:
            collect()
            buf = pipe.acquire()
        np.copyto(buf, np.asarray(f).astype(buf.dtype, copy=False).reshape(buf.shape), casting="unsafe")
        pipe.submit()
    while pipe.in_flight:
        collect()
    return out


@pytest.mark.parametrize("depth,name", [(2, "A"), (4, "E")])
def test_targets_and_caps_move_from_frame_to_frame(depth, name):
    from openjph_amd import codec
    from openjph_amd.pipeline import EncoderPipe
    gold = cc.QUAL["cases"][name]["targets"]
    T40, T50 = gold["40"]["max_sse"], gold["50"]["max_sse"]
    inr, below, _ = rc.budgets(name)
    total, sizes = cc.tables(name)
    same, other = rolled(name, 0), rolled(name, 3)
    #        frame  pair               what it is
    seq = [(same, (T40, inr[2])),    # MET
           (same, (T40, inr[2])),    # MET, steady
           (same, (T50, inr[1])),    # BY_BUDGET
           (same, (T50, inr[1])),    # BY_BUDGET, steady
           (same, (T50, below)),     # nothing fits: this frame's collect alone
           (same, (T50, inr[1])),    # BY_BUDGET, steady: the hints stayed where they were
           (other, (T40, inr[3])),   # MET, another frame
           (same, (T40, inr[0]))]    # BY_BUDGET
    pipe = EncoderPipe(case_plan(name), depth=depth, max_sse=seq[0][1][0], cap_bytes=seq[0][1][1])
    got = run_pipe(pipe, [f for f, _ in seq], [p for _, p in seq])
    pipe.close()
    single = codec.Encoder(case_params(name))
    outcomes = []
    for k, ((frame, (T, B)), (cs, info)) in enumerate(zip(seq, got)):
        single.set_quality(max_sse=T, cap_bytes=B)
        if B == below:
            with pytest.raises(capi.OjphError) as e:
                single.encode(frame)
            assert e.value.code == capi.E_BUDGET
            assert isinstance(cs, capi.OjphError) and cs.code == capi.E_BUDGET, (k, cs)
            assert info is not None and info["comps"] == [] and info["rate_passes"] >= 1
            outcomes.append(None)
            continue
        want = single.encode(frame)
        winfo = single.capped_info()
        assert not isinstance(cs, capi.OjphError), (k, cs)
        print(name, k, {x: v for x, v in info.items() if x != "comps"})
        assert cs == want, (k, len(cs), len(want))
        for key in ("grid_index", "qstep", "outcome", "quality_index", "quality_bytes", "bytes", "bytes_finer", "sse", "sse_coarser", "pae", "comps"):
            assert info[key] == winfo[key], (k, key, info[key], winfo[key])
        assert info["quality_passes"] <= 13 and info["rate_passes"] <= 17
        if frame is same:                                        # the frame the reference coded: its tables, its digests
            assert (info["grid_index"], info["outcome"]) in cc.answers(total, sizes, T, B)
            cc.check_info(info, total, sizes, T, B)
            assert info["comps"] == cc.comp_figures(name, info["grid_index"])
            if info["outcome"] == cc.MET:
                assert sha(cs) == gold["40" if T == T40 else "50"]["sha256"]
        outcomes.append(info["outcome"])
    assert outcomes == [cc.MET, cc.MET, cc.BY_BUDGET, cc.BY_BUDGET, None, cc.BY_BUDGET, cc.MET, cc.BY_BUDGET]
    # an unchanged frame and pair: the trials of the certificates and no more
    i1, i3, i5 = got[1][1], got[3][1], got[5][1]
    assert i1["quality_passes"] <= 2 and i1["rate_passes"] == 1, i1
    for i in (i3, i5):
        assert i["quality_passes"] <= 3 and i["rate_passes"] <= 3, i
        assert i["rate_passes"] == (2 if i["grid_index"] == i["quality_index"] - 1 else 3), i
        assert i["first_guess_q"] == i["quality_index"] and i["first_guess_b"] == i["grid_index"]


def test_v210_frames():
    from openjph_amd import codec
    from openjph_amd.pipeline import EncoderPipe, pack_video
    from tests.synth import synth_image
    from tests.video_cases import C422, feed_planes, make_plan
    w, h, depth = 98, 34, 10
    img = synth_image(3, h, w, depth, seed=3)
    planes = [img[0], img[1][:, : (w + 1) // 2], img[2][:, : (w + 1) // 2]]
    plain = len(codec.Encoder(plan=make_plan(w, h, depth, False, C422), min_psnr=38.0).encode(planes))     # the target's own size
    seen = set()
    for cap in (plain * 2 // 3, plain * 2):
        kw = dict(min_psnr=38.0, cap_bytes=cap)
        a = EncoderPipe(plan=make_plan(w, h, depth, False, C422), depth=2, video="v210", **kw)
        got = list(a.encode_sequence([pack_video(planes, "v210", depth)]))
        ia = a.capped_info()
        a.close()
        b = EncoderPipe(plan=make_plan(w, h, depth, False, C422), depth=2, **kw)
        feed_planes(b, planes)
        want = b.collect()
        b.close()
        enc = codec.Encoder(plan=make_plan(w, h, depth, False, C422), **kw)
        assert got == [want] and want == enc.encode(planes) and len(want) <= cap
        assert ia["outcome"] == enc.capped_info()["outcome"] and ia["grid_index"] == enc.capped_info()["grid_index"]
        seen.add(ia["outcome"])
    assert seen == {cc.MET, cc.BY_BUDGET}


def test_pipes_without_a_cap_beside_a_capped_one():
    """a quality pipe made without a cap and a budget pipe, fed in turn with a capped pipe: the bytes they write alone"""
    from openjph_amd.pipeline import EncoderPipe
    from tests.test_gpu_rate_pipe import plain
    name = "A"
    t40 = cc.QUAL["cases"][name]["targets"]["40"]
    inr, _, _ = rc.budgets(name)
    jb = cc.RATE["cases"][name]["budgets"][str(inr[1])]["j"]
    frame = rolled(name, 0)
    pipes = [EncoderPipe(case_plan(name), depth=2, max_sse=t40["max_sse"]), EncoderPipe(case_plan(name), depth=2, max_bytes=inr[1]),
             EncoderPipe(case_plan(name), depth=2, max_sse=t40["max_sse"], cap_bytes=inr[1])]
    outs = [[], [], []]
    for _ in range(3):
        for p in pipes:
            buf = p.acquire()
            while buf is None:
                outs[pipes.index(p)].append(p.collect())
                buf = p.acquire()
            np.copyto(buf, frame.astype(buf.dtype).reshape(buf.shape), casting="unsafe")
            p.submit()
    for k, p in enumerate(pipes):
        while p.in_flight:
            outs[k].append(p.collect())
    assert pipes[0].quality_info()["grid_index"] == t40["certified"][0] and pipes[1].rate_info()["grid_index"] == jb
    with pytest.raises(capi.OjphError):
        pipes[0].capped_info()
    with pytest.raises(capi.OjphError):
        pipes[2].quality_info()
    for p in pipes:
        p.close()
    assert [sha(cs) for cs in outs[0]] == [t40["sha256"]] * 3
    assert outs[1] == [plain(name, jb, frame)] * 3
    assert outs[2] == outs[1]                                    # (the cap binds below 40 dB's step: the budget's own answer)


def test_encode_sequence_with_targets_and_caps():
    from openjph_amd import codec
    from openjph_amd.pipeline import EncoderPipe
    name = "B"
    gold = cc.QUAL["cases"][name]["targets"]
    inr, _, _ = rc.budgets(name)
    frames = [rolled(name, k) for k in (0, 1, 2)]
    targets = [gold["40"]["max_sse"], gold["50"]["max_sse"], gold["40"]["max_sse"]]
    caps = [inr[2], inr[1], inr[0]]
    pipe = EncoderPipe(case_plan(name), depth=2)
    got = list(pipe.encode_sequence(frames, targets=targets, caps=caps))
    pipe.close()
    enc = codec.Encoder(case_params(name))
    for f, t, b, cs in zip(frames, targets, caps, got):
        enc.set_quality(max_sse=t, cap_bytes=b)
        assert cs == enc.encode(f)
    pipe = EncoderPipe(case_plan(name), depth=2)
    assert list(pipe.encode_sequence(frames[:1], targets=targets[0], caps=caps[0])) == got[:1]
    pipe.close()
    pipe = EncoderPipe(case_plan(name), depth=2)
    with pytest.raises(ValueError):
        list(pipe.encode_sequence(frames, caps=caps))
    with pytest.raises(ValueError):
        list(pipe.encode_sequence(frames, budgets=caps, caps=caps))
    pipe.close()
    with pytest.raises(ValueError):
        EncoderPipe(case_plan(name), depth=2, cap_bytes=1000)


def test_refusals():
    from openjph_amd.pipeline import EncoderPipe
    name = "B"
    T = cc.QUAL["cases"][name]["targets"]["40"]["max_sse"]
    inr, _, _ = rc.budgets(name)

    def refused(call):
        with pytest.raises(capi.OjphError) as e:
            call()
        return e.value.code == capi.E_INVALID
    pipe = EncoderPipe(case_plan(name), depth=2, max_sse=T)          # a quality pipe made without a cap cannot gain one
    assert refused(lambda: pipe.set_quality(max_sse=T, cap_bytes=inr[1]))
    pipe.set_quality(max_sse=T, cap_bytes=0)                         # (cap 0 there is set_quality)
    pipe.close()
    pipe = EncoderPipe(case_plan(name), depth=2, max_bytes=inr[1])   # nor a budget pipe
    assert refused(lambda: pipe.set_quality(max_sse=T, cap_bytes=inr[1]))
    pipe.close()
    pipe = EncoderPipe(case_plan(name), depth=2, max_sse=T, cap_bytes=inr[1])
    assert refused(lambda: pipe.set_quality(max_sse=T, cap_bytes=0))  # the cap does not go back to 0
    assert refused(lambda: pipe.set_budget(inr[1]))
    assert refused(pipe.capped_info)                                 # nothing collected yet
    pipe.set_quality(max_sse=T + 1)                                  # the target alone may move; the cap stays
    buf = pipe.acquire()
    buf[...] = rolled(name, 0).astype(buf.dtype).reshape(buf.shape)
    pipe.submit()
    pipe.set_quality(max_sse=T, cap_bytes=inr[2])                    # both may move between frames
    assert refused(lambda: pipe.set_quality(max_sse=T, cap_bytes=0))
    assert len(pipe.collect()) <= inr[1] and pipe.capped_info()["outcome"] == cc.BY_BUDGET
    pipe.close()
    pipe = EncoderPipe(case_plan(name), depth=2)                     # a plain pipe: no cap once frames are handed out
    pipe.acquire()
    assert refused(lambda: pipe.set_quality(max_sse=T, cap_bytes=inr[1]))
    pipe.close()
