"""The frame pipes with a colour spec (ojphgpu_{enc,dec}_pipe_set_video_colour): an RGB buffer in, a Y, Cb, Cr 4:4:4 / 4:2:2 /
4:2:0 codestream out, and back.  The contract: every codestream of such an encoder pipe is byte for byte the plain encode of
pipeline.rgb_to_ycc(pipeline.unpack_video444(buffer)); every frame of such a decoder pipe is pipeline.pack_video444(
pipeline.ycc_to_rgb(decoded planes)) of what codec.Decoder decodes, the samples as the pipe's containers hold them.  Tiny
frames (66 x 34 and 37 x 19), two decompositions."""
import numpy as np
import pytest

from openjph_amd import pipeline
from openjph_amd.pipeline import Colour
from tests.colour_cases import PLAN_REFUSALS
from tests.video_cases import C420, C422, decoded_planes, edged_planes, feed_planes, make_plan

pytestmark = pytest.mark.gpu

SIZES = ((66, 34), (37, 19))


def plan_of(w, h, depth, rev, cell, **kw):
    return make_plan(w, h, depth, rev, cell, num_decomps=2, **kw)


def rgb_frames(rng, w, h, depth, n=3):
    """n frames of different content: noise, a ramp with noise, blocks of the range's ends"""
    top = (1 << depth) - 1
    x = np.arange(w)[None, :] * top // max(w - 1, 1)
    out = [[rng.integers(0, top + 1, (h, w)) for _ in range(3)],
           [np.clip(x + rng.integers(-9, 10, (h, w)) + k * top // 5, 0, top) for k in range(3)],
           [p.astype(np.int64) for p in edged_planes(int(rng.integers(1, 99)), w, h, depth)]]
    return (out * ((n + 2) // 3))[:n]


def ycc_planes(rgb, fmt, colour, rgb_depth, ycc_depth, cell, w, h):
    """the numpy side of the encoder's contract, from the buffer"""
    col = colour if isinstance(colour, Colour) else Colour(colour)
    table = pipeline.colour_table(col.standard, "forward", rgb_depth, ycc_depth, col.rgb_range, col.ycc_range)
    buf = pipeline.pack_video444(rgb, fmt, rgb_depth)
    planes = pipeline.rgb_to_ycc(pipeline.unpack_video444(buf, fmt, w, h, rgb_depth), table, *cell)
    return buf, [p.astype(np.int32) for p in planes]


# the three of the issue, and an encoder pipe with 32-bit containers, narrow-range RGB, vertical halving only
ENC_CASES = [("r210", "bt709", 10, 10, C422, 16, True), ("bgra", Colour("bt601", rgb_depth=8), 8, 10, C420, 16, False),
             ("rgba", Colour("bt2020", "full", "full"), 8, 8, (1, 1), 8, True), ("r10k", Colour("bt709", "narrow", "narrow", 10), 10, 12, (1, 2), 32, True)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt,colour,rgb_depth,ycc_depth,cell,container,rev", ENC_CASES, ids=[c[0] for c in ENC_CASES])
def test_encoder_pipe_codes_rgb_buffers_as_ycc(fmt, colour, rgb_depth, ycc_depth, cell, container, rev, w, h):
    from openjph_amd import codec
    rng = np.random.default_rng(w + rgb_depth + ycc_depth)
    enc = codec.Encoder(plan=plan_of(w, h, ycc_depth, rev, cell))
    bufs, want = [], []
    for rgb in rgb_frames(rng, w, h, rgb_depth):                # three frames through two slots: nothing stale
        buf, planes = ycc_planes(rgb, fmt, colour, rgb_depth, ycc_depth, cell, w, h)
        bufs.append(buf)
        want.append(enc.encode(planes))
    pipe = pipeline.EncoderPipe(plan=plan_of(w, h, ycc_depth, rev, cell), depth=2, container=container, video=fmt, colour=colour)
    view = pipe.acquire()
    assert view.dtype == np.uint8 and view.shape == (h, pipeline.video444_layout(fmt, w, h)[0])
    got = list(pipe.encode_sequence(bufs))
    pipe.close()
    assert len(set(want)) == 3 and got == want
    if rev:                                                     # and the codestream decodes to those planes
        for a, b in zip(decoded_planes(got[1]), ycc_planes(rgb_frames(np.random.default_rng(w + rgb_depth + ycc_depth), w, h, rgb_depth)[1], fmt, colour,
                                                           rgb_depth, ycc_depth, cell, w, h)[1]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("search", ["max_bytes", "min_psnr"])
def test_encoder_pipe_searches_on_the_ycc_planes(search):
    from openjph_amd import codec
    from tests.synth import synth_image
    w, h, depth = SIZES[0]+ (10,)
    frames = [[p.astype(np.int64) for p in synth_image(3, h, w, depth, seed=s)] for s in (3, 4, 5)]
    pairs = [ycc_planes(rgb, "r210", "bt709", depth, depth, C422, w, h) for rgb in frames]
    plain = [len(codec.Encoder(plan=plan_of(w, h, depth, False, C422)).encode(p)) for _, p in pairs]
    kw = dict(max_bytes=min(plain) * 2 // 3) if search == "max_bytes" else dict(min_psnr=38.0)
    pipe = pipeline.EncoderPipe(plan=plan_of(w, h, depth, False, C422), depth=2, video="r210", colour="bt709", **kw)
    for buf, planes in pairs:
        view = pipe.acquire()
        view[...] = buf
        pipe.submit()
        got = pipe.collect()
        enc = codec.Encoder(plan=plan_of(w, h, depth, False, C422), **kw)
        assert got == enc.encode(planes)
        if search == "max_bytes":                               # the certificate of this frame, as the plain encoder measures it
            a, b = pipe.rate_info(), enc.rate_info()
            assert len(got) <= kw["max_bytes"] and all(a[k] == b[k] for k in ("grid_index", "qstep", "bytes", "bytes_finer"))
            assert a["bytes"] == len(got) and (a["grid_index"] == 0 or a["bytes_finer"] > kw["max_bytes"])
        else:
            a, b = pipe.quality_info(), enc.quality_info()
            assert all(a[k] == b[k] for k in ("grid_index", "qstep", "sse", "sse_coarser", "pae", "bytes", "comps"))
    pipe.close()


def want_rgb(cs, fmt, colour, rgb_depth, ycc_depth, cell, container=16, **view):
    """the numpy side of the decoder's contract: the decoded planes as `container`-bit containers hold them, to RGB, packed"""
    col = colour if isinstance(colour, Colour) else Colour(colour)
    table = pipeline.colour_table(col.standard, "inverse", rgb_depth, ycc_depth, col.rgb_range, col.ycc_range)
    planes = [np.clip(p.astype(np.int64), 0, (1 << container) - 1) for p in decoded_planes(cs, **view)]
    return pipeline.pack_video444(pipeline.ycc_to_rgb(planes, table, *cell), fmt, rgb_depth)


def sources(w, h, depth, cell, seed):
    """four codestreams: three lossless ones of different content (one sequence: a pipe's frames share their coding
    parameters), and a lossy one whose decode leaves the range"""
    from openjph_amd import codec
    rng = np.random.default_rng(seed)
    sub = lambda p, c: p[::c[1], ::c[0]]
    out = []
    for rgb in rgb_frames(rng, w, h, depth, 3):
        out.append(codec.Encoder(plan=plan_of(w, h, depth, True, cell)).encode([rgb[0].astype(np.int32)] + [sub(p, cell).astype(np.int32) for p in rgb[1:]]))
    lossy = codec.Encoder(plan=plan_of(w, h, depth, False, cell, qstep=0.05)).encode(edged_planes(seed, w, h, depth, cell))
    assert max(int(p.max()) for p in decoded_planes(lossy)) > (1 << depth) - 1
    return out + [lossy]


# 4:2:2 -> bgra, 4:2:0 -> r210 (the issue's), 4:4:4 -> argb in 8-bit containers, 4:2:2 10-bit -> rgba 8-bit
DEC_CASES = [("bgra", "bt709", 8, 8, C422, 16), ("r210", Colour("bt2020", "full", "narrow", 10), 10, 10, C420, 16),
             ("argb", Colour("bt601", "full", "full"), 8, 8, (1, 1), 8), ("rgba", Colour("bt709", "narrow", "narrow", 8), 8, 10, C422, 16)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt,colour,rgb_depth,ycc_depth,cell,container", DEC_CASES, ids=[c[0] for c in DEC_CASES])
def test_decoder_pipe_hands_back_rgb_buffers(fmt, colour, rgb_depth, ycc_depth, cell, container, w, h):
    css = sources(w, h, ycc_depth, cell, seed=w + ycc_depth)
    for seq in (css[:3], css[3:] * 2):                          # three frames of different content through two slots; the lossy one
        want = [want_rgb(cs, fmt, colour, rgb_depth, ycc_depth, cell, container) for cs in seq]
        pipe = pipeline.DecoderPipe(seq[0], depth=2, container=container, video=fmt, colour=colour)
        got = list(pipe.decode_sequence(seq))
        pipe.close()
        assert len({x.tobytes() for x in want}) == len(set(seq)) and len(got) == len(seq)
        for g, x in zip(got, want):
            assert g.dtype == np.uint8 and g.shape == x.shape and g.tobytes() == x.tobytes()


@pytest.mark.parametrize("w,h", SIZES)
def test_decoder_pipe_views(w, h):
    """a reduced resolution always passes; a window with an even x0 where fx == 2 and an even y0 where fy == 2"""
    for cell, depth, fmt, views in ((C422, 8, "bgra", (dict(skip_res=1), dict(region=(w // 4 * 2, 5, w // 3, h // 2)), dict(skip_res=(1, 1), region=(4, 3, w // 3, h // 3)))),
                                    (C420, 10, "r210", (dict(skip_res=1), dict(region=(w // 4 * 2, 6, w // 3, h // 2)), dict(skip_res=(1, 1), region=(8, 4, w // 3, h // 3))))):
        css = sources(w, h, depth, cell, seed=h + depth)
        for view in views:
            for seq in (css[:3], css[3:]):
                want = [want_rgb(cs, fmt, "bt709", depth, depth, cell, **view) for cs in seq]
                pipe = pipeline.DecoderPipe(seq[0], depth=2, video=fmt, colour="bt709", **view)
                got = list(pipe.decode_sequence(seq))
                pipe.close()
                assert len(got) == len(seq)
                for g, x in zip(got, want):
                    assert g.shape == x.shape and g.tobytes() == x.tobytes(), (cell, view)


def test_decoder_pipe_window_refusals():
    from openjph_amd import capi
    w, h = SIZES[0]
    cs422, cs420 = sources(w, h, 8, C422, 1)[0], sources(w, h, 8, C420, 2)[0]
    # an odd x0 on 4:2:2, an odd y0 or x0 on 4:2:0; at a reduced resolution: an origin that is odd on the reduced grid
    for cs, region, skip in ((cs422, (5, 4, 20, 10), None), (cs420, (4, 5, 20, 10), None), (cs420, (7, 4, 20, 10), None), (cs420, (3, 3, 20, 10), None),
                             (cs422, (6, 4, 20, 10), (1, 1)), (cs420, (4, 6, 20, 10), (1, 1))):
        pipe = pipeline.DecoderPipe(cs, depth=2, region=region, skip_res=skip)
        with pytest.raises(capi.OjphError) as e:
            pipe.set_video_colour("bgra", "bt709")
        assert e.value.code == capi.E_INVALID and pipe.video is None and pipe.colour is None
        (got,) = list(pipe.decode_sequence([cs]))               # still a plane pipe
        planes = np.concatenate([p.reshape(-1) for p in decoded_planes(cs, region=region, skip_res=skip)])
        assert np.array_equal(got.reshape(-1), np.clip(planes, 0, 65535).astype(got.dtype))     # (a low-pass band may dip below 0: the container saturates)
        pipe.close()
    pipeline.DecoderPipe(cs422, depth=2, region=(4, 5, 20, 10), video="bgra", colour="bt709").close()      # an odd y0 on 4:2:2: no vertical cell
    with pytest.raises(capi.OjphError):                                                                     # 32-bit containers: int32 planes
        pipeline.DecoderPipe(cs422, depth=2, container=32, video="bgra", colour="bt709")


def test_setter_refusals_leave_the_pipe_as_it_was():
    from openjph_amd import capi, codec
    w, h = SIZES[0]
    rng = np.random.default_rng(11)

    def still_a_plane_pipe(pipe):
        ci = [pipe.plan.comp_info(c) for c in range(int(pipe.plan.params.num_comps))]
        planes = [rng.integers(0, 100, (i["h"], i["w"])).astype(np.int32) for i in ci]
        feed_planes(pipe, planes)
        return pipe.collect() == codec.Encoder(plan=pipe.plan).encode(planes)

    # the plan judgement, through the setter (the containers an encoder pipe takes)
    for fmt, colour, container, kw in PLAN_REFUSALS:
        kw = dict(kw)
        depth = kw.pop("depth")
        if depth > container or (container == 8 and depth > 8):
            continue                                            # (no such pipe: judged without one in tests/test_cpu_colour.py)
        pipe = pipeline.EncoderPipe(plan=plan_of(w, h, depth, True, kw.pop("cell", (1, 1)), **kw), depth=2, container=container)
        with pytest.raises(capi.OjphError) as e:
            pipe.set_video_colour(fmt, colour)
        assert e.value.code == capi.E_INVALID and pipe.video is None and pipe.colour is None, (fmt, colour, kw)
        if not kw.get("signs") and not kw.get("is_signed") and not kw.get("bit_depths"):
            assert still_a_plane_pipe(pipe), (fmt, colour, kw)
        pipe.close()
    good = capi.ColourSpec(709, 0, 1, 0)
    mk = lambda **kw: pipeline.EncoderPipe(plan=plan_of(w, h, 10, True, C422), depth=2, **kw)
    # a null spec, an unknown standard or range; colour= without video=
    pipe = mk()
    assert pipe._lib.ojphgpu_enc_pipe_set_video_colour(pipe._h, 0x23, None) == capi.E_INVALID
    for bad in (capi.ColourSpec(2021, 0, 1, 0), capi.ColourSpec(709, 3, 1, 0), capi.ColourSpec(709, 0, 2, 0)):
        assert pipe._lib.ojphgpu_enc_pipe_set_video_colour(pipe._h, 0x23, bad) == capi.E_INVALID
    assert still_a_plane_pipe(pipe)
    pipe.close()
    with pytest.raises(ValueError):
        mk(colour="bt709")
    with pytest.raises(ValueError):
        mk(video="r210", colour="bt470")
    # together with pixels / packed, and with the plain set_video: either order
    pipe = mk(packed=10)
    assert pipe._lib.ojphgpu_enc_pipe_set_video_colour(pipe._h, 0x23, good) == capi.E_INVALID
    pipe.close()
    pipe = pipeline.EncoderPipe(plan=plan_of(w, h, 8, True, (1, 1)), depth=2, pixels=(8, False))
    assert pipe._lib.ojphgpu_enc_pipe_set_video_colour(pipe._h, 0x27, good) == capi.E_INVALID
    pipe.close()
    pipe = pipeline.EncoderPipe(plan=plan_of(w, h, 10, True, (1, 1)), depth=2, video="r210")               # R, G, B coded as they are
    assert pipe._lib.ojphgpu_enc_pipe_set_video_colour(pipe._h, 0x23, good) == capi.E_INVALID
    pipe.set_video("v410")                                      # (the plain setter is as it was: repeatable)
    pipe.close()
    pipe = mk(video="r210", colour="bt709")
    assert pipe._lib.ojphgpu_enc_pipe_set_video(pipe._h, 0x03) == capi.E_INVALID                            # v210 would fit the plan
    assert pipe._lib.ojphgpu_enc_pipe_set_packed(pipe._h, 10) == capi.E_INVALID
    assert pipe._lib.ojphgpu_enc_pipe_set_pixels(pipe._h, 16, 0) == capi.E_INVALID
    pipe.set_video_colour("r10k", Colour("bt601", rgb_depth=8))  # repeatable
    pipe.set_video_colour(None, "bt709")                        # format 0: planes again
    assert pipe.video is None and pipe.colour is None
    pipe.set_video("v210")                                      # ... and then the plain setter passes
    pipe.set_video(None)
    assert still_a_plane_pipe(pipe)
    pipe.close()
    # after the first acquire()
    pipe = mk()
    pipe.acquire()
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video_colour("r210", "bt709")
    assert e.value.code == capi.E_INVALID and still_a_plane_pipe(pipe)
    pipe.close()
    # the decoder: a format that holds Y, Cb, Cr; packed frames; the plain setter; after the first submit()
    cs = sources(w, h, 10, C422, 3)[0]
    pipe = pipeline.DecoderPipe(cs, depth=2)
    for fmt in ("v410", "y410", "v210", "bgra"):                # (bgra: the plan's 10 bits are not what it holds)
        with pytest.raises(capi.OjphError) as e:
            pipe.set_video_colour(fmt, "bt709")
        assert e.value.code == capi.E_INVALID
    assert pipe._lib.ojphgpu_dec_pipe_set_video_colour(pipe._h, 0x23, None) == capi.E_INVALID
    pipe.set_video("v210")
    assert pipe._lib.ojphgpu_dec_pipe_set_video_colour(pipe._h, 0x23, good) == capi.E_INVALID
    pipe.set_video(None)
    pipe.set_video_colour("r210", "bt709")
    assert pipe._lib.ojphgpu_dec_pipe_set_video(pipe._h, 0x03) == capi.E_INVALID
    assert pipe._lib.ojphgpu_dec_pipe_set_packed(pipe._h, 10) == capi.E_INVALID
    pipe.set_video_colour("bgra", Colour("bt709", rgb_depth=8))
    (got,) = list(pipe.decode_sequence([cs]))
    assert got.tobytes() == want_rgb(cs, "bgra", "bt709", 8, 10, C422).tobytes()
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video_colour("r210", "bt709")
    assert e.value.code == capi.E_INVALID
    pipe.close()
    pipe = pipeline.DecoderPipe(cs, depth=2, packed=10)
    assert pipe._lib.ojphgpu_dec_pipe_set_video_colour(pipe._h, 0x23, good) == capi.E_INVALID
    pipe.close()
