"""The hand-over of the frame pipelines (planes, pixel-interleaved, bit-packed, 4:2:2 video buffers) set more than once before
the first frame, and the three setters excluding each other: whatever was set last is what the pipe runs with -- sizes,
buffers and launches -- and a refused call changes nothing.  Tiny frames (3 components, 37 x 21: 2331 samples, 1575 as
4:2:2, neither a multiple of 32, so the packed tail is exercised), pipes of depth 2 coding 3 frames, so the slots recycle."""
import functools

import numpy as np
import pytest

from tests.video_cases import C422, make_plan

pytestmark = pytest.mark.gpu

W, H = 37, 21
# name -> (bit depth of the plan, 4:2:2?, the setters called in turn before the first frame: the last one is what counts)
SEQUENCES = {
    "pixels 8 then 16 big endian": (8, False, [("pixels", (8, False)), ("pixels", (16, True))]),
    "pixels 16 then 8": (8, False, [("pixels", (16, False)), ("pixels", (8, False))]),
    "packed 10 then 14": (10, False, [("packed", 10), ("packed", 14)]),
    "video uyvy, planes, packed 14": (8, True, [("video", "uyvy"), ("video", None), ("packed", 14)]),
}


def new_plan(depth, sub):
    from openjph_amd.plan import Plan, make_params
    return make_plan(W, H, depth, True, C422) if sub else Plan(make_params(W, H, 3, bit_depth=depth))


def setter(pipe, kind, arg):
    {"pixels": lambda: pipe.set_pixels(*arg), "packed": lambda: pipe.set_packed(arg), "video": lambda: pipe.set_video(arg)}[kind]()


def handed_over(plan, planes, kind, arg):
    """the planes of a frame -> what the caller writes into the memory an encoder pipe hands out"""
    from openjph_amd.pipeline import pack_bits, pack_video
    if kind == "pixels":
        return np.stack(planes, axis=2).astype(np.uint8 if arg[0] == 8 else np.dtype(">u2" if arg[1] else "<u2"))
    if kind == "packed":
        return pack_bits(plan.pack_frame(planes), arg)
    if kind == "video":
        return pack_video(planes, arg, plan.comp_format(0)[0])
    return plan.pack_frame(planes)


def planes_of(plan, frame, kind, arg):
    """the inverse, on what a decoder pipe hands back"""
    from openjph_amd.pipeline import unpack_bits, unpack_video
    if kind == "pixels":
        return [frame[:, :, c] for c in range(frame.shape[2])]
    if kind == "packed":
        return plan.unpack_frame(unpack_bits(frame, arg, plan.frame_elems))
    if kind == "video":
        return unpack_video(frame, arg, W, H, plan.comp_format(0)[0])
    return plan.unpack_frame(frame)


def frame_bytes(plan, kind, arg, container=16):
    from openjph_amd.pipeline import video_layout
    n = plan.frame_elems
    return {"pixels": lambda: n * arg[0] // 8, "packed": lambda: (n + 31) // 32 * 4 * arg, "video": lambda: video_layout(arg, W, H)[1],
            "planes": lambda: n * container // 8}[kind]()


@functools.lru_cache(maxsize=None)
def reference(depth, sub):
    """three random frames of such a plan and the codestreams the single encoder writes for them"""
    from openjph_amd import codec
    rng = np.random.default_rng(depth + sub)
    enc = codec.Encoder(plan=new_plan(depth, sub))
    frames = [[rng.integers(0, 1 << depth, (H, (W + 1) // 2 if sub and c else W)).astype(np.int32) for c in range(3)] for _ in range(3)]
    return frames, [enc.encode(enc.plan.pack_frame(p)) for p in frames]


def encode_frames(pipe, frames, kind, arg):
    want_bytes = frame_bytes(pipe.plan, kind, arg, pipe.container)
    out = []
    for planes in frames:
        buf = pipe.acquire()
        while buf is None:
            out.append(pipe.collect())
            buf = pipe.acquire()
        assert buf.nbytes == want_bytes, (kind, arg, buf.nbytes, want_bytes)
        buf[...] = handed_over(pipe.plan, planes, kind, arg).reshape(buf.shape)
        pipe.submit()
    while pipe.in_flight:
        out.append(pipe.collect())
    return out


def decode_frames(pipe, streams, kind, arg):
    want_bytes = frame_bytes(pipe.plan, kind, arg, pipe.container)
    out = []
    for frame in pipe.decode_sequence(streams):
        assert frame.nbytes == want_bytes, (kind, arg, frame.nbytes, want_bytes)
        out.append(planes_of(pipe.plan, frame, kind, arg))
    return out


def same_planes(got, want):
    return len(got) == len(want) and all(np.array_equal(np.asarray(g).astype(np.int64), w) for g, w in zip(got, want))


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_encoder_pipe_hand_over_set_again_before_the_first_frame(name):
    from openjph_amd.pipeline import EncoderPipe
    depth, sub, steps = SEQUENCES[name]
    frames, want = reference(depth, sub)
    kind, arg = steps[-1]
    pipe = EncoderPipe(plan=new_plan(depth, sub), depth=2, container=16)
    for k, a in steps:
        setter(pipe, k, a)
    got = encode_frames(pipe, frames, kind, arg)
    pipe.close()
    fresh = EncoderPipe(plan=new_plan(depth, sub), depth=2, container=16, **{kind: arg})       # created with the final hand-over
    direct = encode_frames(fresh, frames, kind, arg)
    fresh.close()
    assert got == want and got == direct


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_decoder_pipe_hand_over_set_again_before_the_first_frame(name):
    from openjph_amd.pipeline import DecoderPipe
    depth, sub, steps = SEQUENCES[name]
    frames, streams = reference(depth, sub)
    pipe = DecoderPipe(streams[0], depth=2, container=16)
    for k, a in steps:
        setter(pipe, k, a)
    got = decode_frames(pipe, streams, *steps[-1])
    pipe.close()
    assert len(got) == 3 and all(same_planes(g, f) for g, f in zip(got, frames))


# ---- the setters exclude each other
ON = {"pixels": (8, False), "packed": 10, "video": "uyvy"}                  # a valid argument of each kind (8-bit plans) ...
RAW = {"pixels": ((8, 0), (0, 0)), "packed": ((10,), (0,)), "video": ((1,), (0,))}   # ... as the C call takes it, and the kind's 0
PAIRS = [(a, b) for a in ON for b in ON if a != b]


def raw_call(pipe, side, kind, args):
    return getattr(pipe._lib, "ojphgpu_%s_pipe_set_%s" % (side, kind))(pipe._h, *args)


def pair_is_422(a, b):
    """the plan of a pair: one the hand-over that is on is valid for, and the refused setter's argument too where a plan can
    be both (pixels ask for planes of one size, video for 4:2:2: under the one, the other is refused twice over)"""
    return a == "video" or (a == "packed" and b == "video")


@pytest.mark.parametrize("a,b", PAIRS)
def test_encoder_pipe_one_kind_on_refuses_the_setters_of_the_others(a, b):
    from openjph_amd import capi
    from openjph_amd.pipeline import EncoderPipe
    sub = pair_is_422(a, b)
    frames, want = reference(8, sub)
    pipe = EncoderPipe(plan=new_plan(8, sub), depth=2, container=16, **{a: ON[a]})
    assert [raw_call(pipe, "enc", b, args) for args in RAW[b]] == [capi.E_INVALID, capi.E_INVALID]
    got = encode_frames(pipe, frames[:1], a, ON[a])
    pipe.close()
    assert got == want[:1]


@pytest.mark.parametrize("a,b", PAIRS)
def test_decoder_pipe_one_kind_on_refuses_the_setters_of_the_others(a, b):
    from openjph_amd import capi
    from openjph_amd.pipeline import DecoderPipe
    sub = pair_is_422(a, b)
    frames, streams = reference(8, sub)
    pipe = DecoderPipe(streams[0], depth=2, container=16, **{a: ON[a]})
    assert [raw_call(pipe, "dec", b, args) for args in RAW[b]] == [capi.E_INVALID, capi.E_INVALID]
    got = decode_frames(pipe, streams[:1], a, ON[a])
    pipe.close()
    assert len(got) == 1 and same_planes(got[0], frames[0])


@pytest.mark.parametrize("sub", [False, True])
def test_every_setter_is_refused_once_frames_flow(sub):
    """after the first acquire() of an encoder pipe / submit() of a decoder pipe: every setter, with a valid argument and with
    0, and the frame under way is not disturbed (4:4:4: pixels and packed would fit; 4:2:2: packed and video)"""
    from openjph_amd import capi
    from openjph_amd.pipeline import DecoderPipe, EncoderPipe
    frames, streams = reference(8, sub)
    calls = [(kind, args) for kind in RAW for args in RAW[kind]]
    pipe = EncoderPipe(plan=new_plan(8, sub), depth=2, container=16)
    assert pipe.acquire() is not None
    assert [raw_call(pipe, "enc", kind, args) for kind, args in calls] == [capi.E_INVALID] * 6
    got = encode_frames(pipe, frames[:1], "planes", None)
    pipe.close()
    assert got == streams[:1]
    pipe = DecoderPipe(streams[0], depth=2, container=16)
    pipe.acquire(len(streams[0]))[:] = np.frombuffer(streams[0], np.uint8)
    pipe.submit()
    assert [raw_call(pipe, "dec", kind, args) for kind, args in calls] == [capi.E_INVALID] * 6
    frame = pipe.collect()
    ok = frame.nbytes == frame_bytes(pipe.plan, "planes", None) and same_planes(pipe.plan.unpack_frame(frame), frames[0])
    pipe.close()
    assert ok


# ---- the refusal matrix of _set_video, against the literal table of tests/test_cpu_video_formats.py
def set_video_answers(pipe, cell, depth, container):
    """every name on a pipe that has no video hand-over on, planes again between names -> the names accepted; each answer
    checked against the table, a refusal E_INVALID that leaves the pipe as it was"""
    from openjph_amd import capi
    from tests.test_cpu_video_formats import TABLE, accepts
    taken = []
    for name in TABLE:
        want = accepts(name, cell, depth, container)
        try:
            pipe.set_video(name)
            got = True
        except capi.OjphError as e:
            assert e.code == capi.E_INVALID, (name, e.code)
            got = False
        assert got == want, (name, cell, depth, container, got)
        assert pipe.video == (name if got else None)
        pipe.set_video(None)
        assert pipe.video is None
        if got:
            taken.append(name)
    return taken


def replaced_and_refused(pipe, taken, cell, depth, container):
    """the accepted names one after the other without planes between them, a refused name after each: what was accepted last
    stays on -> it (None: nothing is accepted on this pipe)"""
    from openjph_amd import capi
    from tests.test_cpu_video_formats import TABLE, accepts
    refused = [n for n in TABLE if not accepts(n, cell, depth, container)]
    for i, name in enumerate(taken):
        pipe.set_video(name)
        with pytest.raises(capi.OjphError):
            pipe.set_video(refused[i % len(refused)])
        assert pipe.video == name
    return taken[-1] if taken else None


def test_set_video_accepts_exactly_what_the_format_table_says():
    """Encoder pipes of 3 components of 6 x 4 luma (chroma 6 x 4, 3 x 4, 3 x 2; depths 8, 10, 12, 16; containers 8, 16, 32: the 27 of
    the 36 whose container holds the depth exist) x every name, and two decoder pipes on a 4:4:4 stream, one of them a window
    with odd x0 and odd y0: there is no chroma cell, so it takes what the full frame takes."""
    from openjph_amd import capi, codec
    from openjph_amd.pipeline import DecoderPipe, EncoderPipe, pack_video444
    from openjph_amd.plan import Plan, make_params
    from tests.test_cpu_video_formats import table_layout
    pipes = 0
    for cell in ((1, 1), (2, 1), (2, 2)):
        for depth in (8, 10, 12, 16):
            for container in (8, 16, 32):
                plan = Plan(make_params(6, 4, 3, bit_depth=depth, downsampling=[(1, 1), cell, cell]))
                assert [(plan.comp_info(c)["w"], plan.comp_info(c)["h"]) for c in (1, 2)] == [(-(-6 // cell[0]), -(-4 // cell[1]))] * 2
                try:
                    pipe = EncoderPipe(plan=plan, depth=2, container=container)
                except capi.OjphError:
                    assert container < depth, (cell, depth, container)
                    continue
                assert container >= depth
                pipes += 1
                last = replaced_and_refused(pipe, set_video_answers(pipe, cell, depth, container), cell, depth, container)
                buf = pipe.acquire()                               # the frame is the one of what was accepted last
                assert buf.nbytes == (table_layout(last, 6, 4)[2] if last else plan.frame_elems * container // 8), (cell, depth, container, last)
                pipe.close()
    assert pipes == 3 * (3 + 2 + 2 + 2)
    w, h, depth, container = 22, 10, 8, 16
    rng = np.random.default_rng(22)
    cs = codec.Encoder(plan=Plan(make_params(w, h, 3, bit_depth=depth))).encode([rng.integers(0, 1 << depth, (h, w)).astype(np.int32) for _ in range(3)])
    for view in ({}, dict(region=(3, 1, 9, 5))):
        pipe = DecoderPipe(cs, depth=2, container=container, **view)
        last = replaced_and_refused(pipe, set_video_answers(pipe, (1, 1), depth, container), (1, 1), depth, container)
        assert last is not None
        dec = codec.Decoder(cs, **view)
        want = pack_video444(dec.plan.unpack_frame(dec.decode()), last, depth)
        (got,) = list(pipe.decode_sequence([cs]))
        pipe.close()
        assert got.dtype == np.uint8 and got.shape == want.shape and got.tobytes() == want.tobytes(), (view, last)


# ---- the clamp of the hand-over kernels inside decoder pipes: lossy frames whose plain decode leaves the range
OVERSHOOT = {8: 0.05, 10: 0.05, 12: 0.03}                    # bit depth -> the 9/7 step at which samples decode to 2^depth


@functools.lru_cache(maxsize=None)
def overshooting(depth):
    """80 x 48, 3 components, 3 decompositions, 9/7: a 4 x 4 checkerboard of 0 and 2^depth - 1, its inverse and a random plane of
    those two values -> (codestream, the single decoder's frame [3, 48, 80], which holds 2^depth: one past the range)"""
    from openjph_amd import codec
    from tests import cpu_pipeline as cp
    w, h, top = 80, 48, (1 << depth) - 1
    board = ((np.arange(h)[:, None] // 4 + np.arange(w)[None, :] // 4) & 1) * top
    rnd = np.random.default_rng(depth).integers(0, 2, (h, w)) * top
    img = np.stack([board, top - board, rnd]).astype(np.int32)
    cs = cp.encode(img, bit_depth=depth, reversible=False, qstep=OVERSHOOT[depth], num_decomps=3)[0]
    frame = codec.Decoder(cs).decode().astype(np.int64).reshape(3, h, w)
    assert (frame == top + 1).sum() >= 1, "depth %d: the plain decode stays in range, the test proves nothing" % depth
    assert frame.max() == top + 1 and frame.min() >= 0
    return cs, frame


def one_frame(cs, **kw):
    from openjph_amd.pipeline import DecoderPipe
    pipe = DecoderPipe(cs, depth=2, **kw)
    try:
        (got,) = list(pipe.decode_sequence([cs]))
        return np.array(got)
    finally:
        pipe.close()


@pytest.mark.parametrize("container", [16, 32])
@pytest.mark.parametrize("depth,bits", [(10, 10), (12, 12), (8, 10), (10, 12)])
def test_decoder_pipe_packed_clamps_to_the_bit_string_not_to_the_depth(depth, bits, container):
    """depth == bits: a decoded 2^bits must not wrap to 0 in the bit string; depth < bits: 2^depth comes through, as the header
    says ("clamped to [0, 2^bits - 1]")"""
    from openjph_amd.pipeline import pack_bits, unpack_bits
    cs, frame = overshooting(depth)
    got = one_frame(cs, packed=bits, container=container)
    want = pack_bits(np.clip(frame, 0, (1 << bits) - 1), bits)
    assert got.dtype == np.uint8 and got.size == want.size and np.array_equal(got.reshape(-1), want)
    back = unpack_bits(got.reshape(-1), bits, frame.size).astype(np.int64)
    if depth == bits:
        assert back.max() == (1 << bits) - 1 and (back[frame.reshape(-1) == 1 << bits] == (1 << bits) - 1).all()
    else:
        assert back.max() == 1 << depth and np.array_equal(back, frame.reshape(-1))


@pytest.mark.parametrize("pixels,depth", [((8, False), 8), ((16, True), 12)])
def test_decoder_pipe_pixels_clamp_to_the_depth(pixels, depth):
    cs, frame = overshooting(depth)
    got = one_frame(cs, pixels=pixels)
    want = np.transpose(np.clip(frame, 0, (1 << depth) - 1), (1, 2, 0)).astype(np.uint8 if pixels[0] == 8 else np.dtype(">u2" if pixels[1] else "<u2"))
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize and got.tobytes() == want.tobytes()
