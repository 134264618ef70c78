"""The frame pipes with a video buffer whose chroma format is not the plan's (ojphgpu_{enc,dec}_pipe_set_video_chroma; ojphgpu.h
section 7f).  The contract: every codestream of such an encoder pipe is byte for byte the plain encode of
pipeline.rechroma_frame(pipeline.unpack_video*(buffer), the format's cell, the plan's cell); every frame of such a decoder pipe is
pipeline.pack_video*(pipeline.rechroma_frame(decoded planes, the plan's cell, the format's cell)) of what codec.Decoder decodes,
the samples as the pipe's containers hold them.  Tiny frames (66 x 34 and 37 x 19), two decompositions, three frames through
two slots."""
import numpy as np
import pytest

from openjph_amd import capi, pipeline
from tests.chroma_cases import layout_any, pack_any, plane_shapes, unpack_any
from tests.video_cases import C420, C422, decoded_planes, edged_planes, feed_planes, make_plan

pytestmark = pytest.mark.gpu

SIZES = ((66, 34), (37, 19))
C444, C440 = (1, 1), (1, 2)


def plan_of(w, h, depth, rev, cell, **kw):
    return make_plan(w, h, depth, rev, cell, num_decomps=2, **kw)


def frames_of(rng, w, h, depth, cell, n=3):
    """n frames of different content in the chroma format `cell`: noise, a ramp with noise, blocks of the range's ends"""
    top = (1 << depth) - 1
    shapes = plane_shapes(w, h, cell)
    ramp = lambda sh, k: np.clip(np.arange(sh[1])[None, :] * top // max(sh[1] - 1, 1) + rng.integers(-9, 10, sh) + k * top // 5, 0, top)
    out = [[rng.integers(0, top + 1, sh) for sh in shapes], [ramp(sh, k) for k, sh in enumerate(shapes)],
           [p.astype(np.int64) for p in edged_planes(int(rng.integers(1, 99)), w, h, depth, cell)]]
    return (out * ((n + 2) // 3))[:n]


def plan_planes(planes, fmt, depth, pcell, w, h):
    """the numpy side of the encoder's contract, from the buffer"""
    buf = pack_any(planes, fmt, depth)
    out = pipeline.rechroma_frame(unpack_any(buf, fmt, w, h, depth), pipeline.video_cell(fmt), pcell)
    return buf, [p.astype(np.int32) for p in out]


# buffer in, the plan's depth and cell, containers, reversible: halve down; double across; double down; halve across; double
# both ways; double across and halve down in one pass
ENC_CASES = [("v210", 10, C420, 16, True), ("uyvy", 8, C444, 8, True), ("nv12", 8, C422, 16, False), ("v410", 10, C422, 16, True),
             ("p010", 10, C444, 32, True), ("yuy2", 8, C440, 16, False)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt,depth,cell,container,rev", ENC_CASES, ids=[c[0] for c in ENC_CASES])
def test_encoder_pipe_codes_buffers_of_another_chroma_format(fmt, depth, cell, container, rev, w, h):
    from openjph_amd import codec
    rng = np.random.default_rng(w + depth + 7 * cell[0] + cell[1])
    enc = codec.Encoder(plan=plan_of(w, h, depth, rev, cell))
    bufs, planes, want = [], [], []
    for f in frames_of(rng, w, h, depth, pipeline.video_cell(fmt)):         # three frames through two slots: nothing stale
        buf, p = plan_planes(f, fmt, depth, cell, w, h)
        bufs.append(buf); planes.append(p)
        want.append(enc.encode(p))
    pipe = pipeline.EncoderPipe(plan=plan_of(w, h, depth, rev, cell), depth=2, container=container, video=fmt, chroma="cosited")
    view = pipe.acquire()
    assert view.dtype == np.uint8 and view.shape == layout_any(fmt, w, h) == bufs[0].shape
    got = list(pipe.encode_sequence(bufs))
    pipe.close()
    assert len(set(want)) == 3 and got == want
    if rev:                                                     # and the codestream decodes to those planes
        for a, b in zip(decoded_planes(got[1]), planes[1]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("search", ["max_bytes", "min_psnr"])
def test_encoder_pipe_searches_on_the_plans_planes(search):
    from openjph_amd import codec
    from tests.synth import synth_image
    (w, h), depth = SIZES[0], 10
    sub = lambda p, c: np.ascontiguousarray(p[::c[1], ::c[0]])
    frames = [[p.astype(np.int64) if i == 0 else sub(p, C422).astype(np.int64) for i, p in enumerate(synth_image(3, h, w, depth, seed=s))] for s in (3, 4, 5)]
    pairs = [plan_planes(f, "v210", depth, C420, w, h) for f in frames]
    plain = [len(codec.Encoder(plan=plan_of(w, h, depth, False, C420)).encode(p)) for _, p in pairs]
    kw = dict(max_bytes=min(plain) * 2 // 3) if search == "max_bytes" else dict(min_psnr=38.0)
    pipe = pipeline.EncoderPipe(plan=plan_of(w, h, depth, False, C420), depth=2, video="v210", chroma="cosited", **kw)
    for buf, planes in pairs:
        view = pipe.acquire()
        view[...] = buf
        pipe.submit()
        got = pipe.collect()
        enc = codec.Encoder(plan=plan_of(w, h, depth, False, C420), **kw)
        assert got == enc.encode(planes)
        if search == "max_bytes":                               # the certificate of this frame, as the plain encoder measures it
            a, b = pipe.rate_info(), enc.rate_info()
            assert len(got) <= kw["max_bytes"] and all(a[k] == b[k] for k in ("grid_index", "qstep", "bytes", "bytes_finer"))
            assert a["bytes"] == len(got) and (a["grid_index"] == 0 or a["bytes_finer"] > kw["max_bytes"])
        else:                                                   # measured against the planes in the plan's chroma format
            a, b = pipe.quality_info(), enc.quality_info()
            assert all(a[k] == b[k] for k in ("grid_index", "qstep", "sse", "sse_coarser", "pae", "bytes", "comps"))
    pipe.close()


def held(planes, container):
    """decoded planes as a pipe's containers hold them: 8 / 16 bits saturate, 32 bits are int32"""
    return [p.astype(np.int64) if container == 32 else np.clip(p.astype(np.int64), 0, (1 << container) - 1) for p in planes]


def want_buffer(cs, fmt, depth, cell, container=16, **view):
    """the numpy side of the decoder's contract"""
    planes = held(decoded_planes(cs, **view), container)
    return pipeline.rechroma_frame(planes, cell, pipeline.video_cell(fmt)), planes


def sources(w, h, depth, cell, seed, lossy=False):
    """three codestreams of different content (one sequence: a pipe's frames share their coding parameters); lossy: frames of
    the range's ends at a coarse step, whose decode leaves the range"""
    from openjph_amd import codec
    rng = np.random.default_rng(seed)
    if lossy:
        return [codec.Encoder(plan=plan_of(w, h, depth, False, cell, qstep=0.05)).encode(edged_planes(seed + k, w, h, depth, cell)) for k in range(3)]
    return [codec.Encoder(plan=plan_of(w, h, depth, True, cell)).encode([p.astype(np.int32) for p in f]) for f in frames_of(rng, w, h, depth, cell)]


# the codestream's depth and cell, buffer out, containers, lossy, the view (a window: of the 66 x 34 or the 37 x 19 frame)
DEC_CASES = [(8, C420, "uyvy", 16, False, {}), (8, C444, "nv12", 16, False, {}), (10, C422, "v410", 16, False, {}),
             (10, C420, "v210", 16, False, dict(skip_res=1)), (8, C422, "nv12", 16, False, "window"), (8, C420, "uyvy", 32, True, {})]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("depth,cell,fmt,container,lossy,view", DEC_CASES, ids=["%s-%d%d%s" % (c[2], c[1][0], c[1][1], "-lossy" * c[4]) for c in DEC_CASES])
def test_decoder_pipe_hands_back_buffers_of_another_chroma_format(depth, cell, fmt, container, lossy, view, w, h):
    if view == "window":
        view = dict(region=(w // 4 * 2, 6, w // 3, h // 2))     # an even origin both ways: nv12 halves down
    seq = sources(w, h, depth, cell, seed=w + depth + cell[1], lossy=lossy)
    want = []
    for cs in seq:
        planes, plan_side = want_buffer(cs, fmt, depth, cell, container, **view)
        if lossy:                                               # the decode leaves the range, and int32 containers carry that into the stage
            lo, hi = min(int(p.min()) for p in plan_side), max(int(p.max()) for p in plan_side)
            assert lo < 0 or hi > (1 << depth) - 1, (lo, hi)
        want.append(pack_any(planes, fmt, depth))
    pipe = pipeline.DecoderPipe(seq[0], depth=2, container=container, video=fmt, chroma="cosited", **view)
    got = list(pipe.decode_sequence(seq))
    pipe.close()
    assert len({x.tobytes() for x in want}) == 3 and len(got) == 3
    for g, x in zip(got, want):
        assert g.dtype == np.uint8 and g.shape == x.shape and g.tobytes() == x.tobytes()


def test_equal_cells_are_the_plain_video_pipe():
    w, h = SIZES[1]
    rng = np.random.default_rng(3)
    bufs = [pack_any(f, "v210", 10) for f in frames_of(rng, w, h, 10, C422)]
    out = []
    for kw in (dict(chroma="cosited"), {}):
        pipe = pipeline.EncoderPipe(plan=plan_of(w, h, 10, True, C422), depth=2, video="v210", **kw)
        out.append(list(pipe.encode_sequence(bufs)))
        pipe.close()
    assert out[0] == out[1] and len(set(out[0])) == 3
    seq = sources(w, h, 8, C420, seed=4)
    out = []
    for kw in (dict(chroma="cosited"), {}):
        pipe = pipeline.DecoderPipe(seq[0], depth=2, video="nv12", **kw)
        out.append([g.tobytes() for g in pipe.decode_sequence(seq)])
        pipe.close()
    assert out[0] == out[1] and len(set(out[0])) == 3


def test_setter_refusals_leave_the_pipe_as_it_was():
    from openjph_amd import codec
    w, h = SIZES[0]
    rng = np.random.default_rng(11)
    COSITED = capi.CHROMA_COSITED

    def still_a_plane_pipe(pipe):
        ci = [pipe.plan.comp_info(c) for c in range(int(pipe.plan.params.num_comps))]
        planes = [rng.integers(0, 100, (i["h"], i["w"])).astype(np.int32) for i in ci]
        feed_planes(pipe, planes)
        return pipe.collect() == codec.Encoder(plan=pipe.plan).encode(planes)

    mk = lambda **kw: pipeline.EncoderPipe(plan=plan_of(w, h, 10, True, C420), depth=2, **kw)
    enc_set = lambda pipe, code, mode: pipe._lib.ojphgpu_enc_pipe_set_video_chroma(pipe._h, code, mode)
    # the plan judgement through the setter (all of it: tests/test_cpu_rechroma.py): an RGB name, a depth the format does not hold, a bad mode
    pipe = mk()
    for fmt in ("r210", "r10k", "uyvy", "nv12"):
        with pytest.raises(capi.OjphError) as e:
            pipe.set_video_chroma(fmt)
        assert e.value.code == capi.E_INVALID and pipe.video is None and pipe.chroma is None
    for mode in (0, 2, -1):
        assert enc_set(pipe, 0x03, mode) == capi.E_INVALID
    assert enc_set(pipe, 0, 2) == capi.E_INVALID and enc_set(pipe, 0, 0) == capi.OK and enc_set(pipe, 0, COSITED) == capi.OK
    assert still_a_plane_pipe(pipe)
    pipe.close()
    with pytest.raises(ValueError):
        mk(chroma="cosited")                                    # chroma= goes with video=
    with pytest.raises(ValueError):
        mk(video="r210", colour="bt709", chroma="cosited")      # ... and not with colour=
    with pytest.raises(ValueError):
        mk(video="v210", chroma="centred")
    # together with pixels / packed / the plain set_video / set_video_colour: either order
    pipe = mk(packed=10)
    assert enc_set(pipe, 0x03, COSITED) == capi.E_INVALID
    pipe.close()
    pipe = pipeline.EncoderPipe(plan=plan_of(w, h, 8, True, C444), depth=2, pixels=(8, False))
    assert enc_set(pipe, 0x01, COSITED) == capi.E_INVALID
    pipe.close()
    pipe = pipeline.EncoderPipe(plan=plan_of(w, h, 10, True, C422), depth=2, video="v210")
    assert enc_set(pipe, 0x21, COSITED) == capi.E_INVALID and enc_set(pipe, 0x03, COSITED) == capi.E_INVALID and enc_set(pipe, 0, 0) == capi.E_INVALID
    pipe.set_video("y210")                                      # (the plain setter is as it was: repeatable)
    pipe.close()
    pipe = mk(video="r210", colour="bt709")
    assert enc_set(pipe, 0x03, COSITED) == capi.E_INVALID
    pipe.set_video_colour("r10k", "bt601")
    pipe.close()
    pipe = mk(video="v210", chroma="cosited")
    assert pipe._lib.ojphgpu_enc_pipe_set_video(pipe._h, 0x13) == capi.E_INVALID                            # p010 would fit the plan
    assert pipe._lib.ojphgpu_enc_pipe_set_video_colour(pipe._h, 0x23, capi.ColourSpec(709, 0, 1, 0)) == capi.E_INVALID
    assert pipe._lib.ojphgpu_enc_pipe_set_packed(pipe._h, 10) == capi.E_INVALID
    assert pipe._lib.ojphgpu_enc_pipe_set_pixels(pipe._h, 16, 0) == capi.E_INVALID
    pipe.set_video_chroma("v410")                               # repeatable, also with an equal cell
    pipe.set_video_chroma("p010")
    assert pipe.video == "p010" and pipe.chroma == "cosited"
    pipe.set_video_chroma(None)                                 # format 0: planes again
    assert pipe.video is None and pipe.chroma is None
    pipe.set_video("p010")                                      # ... and then the plain setter passes
    pipe.set_video(None)
    assert still_a_plane_pipe(pipe)
    pipe.close()
    # after the first acquire()
    pipe = mk()
    pipe.acquire()
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video_chroma("v210")
    assert e.value.code == capi.E_INVALID and still_a_plane_pipe(pipe)
    pipe.close()
    # the decoder: an RGB name; the other hand-overs; a window from an odd row where only the format halves; after the first submit()
    dec_set = lambda pipe, code, mode: pipe._lib.ojphgpu_dec_pipe_set_video_chroma(pipe._h, code, mode)
    seq = sources(w, h, 10, C422, seed=3)
    pipe = pipeline.DecoderPipe(seq[0], depth=2)
    for fmt in ("r210", "uyvy", "y212"):
        with pytest.raises(capi.OjphError) as e:
            pipe.set_video_chroma(fmt)
        assert e.value.code == capi.E_INVALID and pipe.video is None
    assert dec_set(pipe, 0x13, 0) == capi.E_INVALID and dec_set(pipe, 0x13, 3) == capi.E_INVALID
    pipe.set_video("v210")
    assert dec_set(pipe, 0x13, COSITED) == capi.E_INVALID
    pipe.set_video(None)
    pipe.set_video_colour("r210", "bt709")
    assert dec_set(pipe, 0x13, COSITED) == capi.E_INVALID
    pipe.set_video_colour(None, "bt709")
    pipe.set_video_chroma("v410")
    assert pipe._lib.ojphgpu_dec_pipe_set_video(pipe._h, 0x03) == capi.E_INVALID
    assert pipe._lib.ojphgpu_dec_pipe_set_packed(pipe._h, 10) == capi.E_INVALID
    pipe.set_video_chroma("p010")
    got = list(pipe.decode_sequence(seq[:1]))[0]
    assert got.tobytes() == pack_any(want_buffer(seq[0], "p010", 10, C422)[0], "p010", 10).tobytes()
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video_chroma("v410")
    assert e.value.code == capi.E_INVALID
    pipe.close()
    pipe = pipeline.DecoderPipe(seq[0], depth=2, packed=10)
    assert dec_set(pipe, 0x13, COSITED) == capi.E_INVALID
    pipe.close()
    pipe = pipeline.DecoderPipe(seq[0], depth=2, region=(4, 5, 20, 10))
    with pytest.raises(capi.OjphError):
        pipe.set_video_chroma("p010")                           # an odd y0: p010 halves down
    pipe.set_video_chroma("v410")                               # ... v410 does not
    pipe.close()
