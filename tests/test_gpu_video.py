"""4:2:2 video buffers on the device (ojphgpu.h section 7b, kernels_video.hip): the two stages against their numpy
statement (pipeline.pack_video / unpack_video) over every format, container and the widths around a pair, a v210 group, a
v210 line and a lane's unit; that nothing outside the destination is written; the clamp; and the frame pipelines fed with
and handing back such buffers, against the plain codec objects (and the reference where it is built)."""
import numpy as np
import pytest

from tests.test_cpu_video import garbage_in_padding, random_planes
from tests.video_cases import C422, GUARD, decoded_planes, edged_planes, feed_planes, make_plan, to_dev

pytestmark = pytest.mark.gpu

# name, bit depth, containers
FORMATS = (("uyvy", 8, (8, 16, 32)), ("yuy2", 8, (8, 16, 32)), ("v210", 10, (16, 32)), ("y210", 10, (16, 32)),
           ("y212", 12, (16, 32)), ("y216", 16, (16, 32)))
# around the pair, the v210 group (6), the v210 line and unit (48), the units of the other kernels (16 and 32 pixels) ...
WIDTHS = (1, 2, 3, 6, 7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 97, 200)
HEIGHTS = (1, 3)
WIDE = (6149, 5)            # ... and rows of more than 64 units of every kernel: several workgroups share a row; five rows: two workgroups deep
NP_DT = {8: np.uint8, 16: np.uint16, 32: np.int32}
DS422 = [(1, 1), (2, 1), (2, 1)]


def guarded(nbytes, container):
    """-> (the whole tensor, the destination inside it): GUARD bytes of a pattern either side"""
    import torch
    dt = {8: torch.uint8, 16: torch.int16, 32: torch.int32}[container]
    es = container // 8
    big = torch.full((nbytes // es + 2 * (GUARD // es),), {8: 0x5A, 16: 0x5A5A, 32: 0x5A5A5A5A}[container], dtype=dt, device="cuda")
    return big, big[GUARD // es: GUARD // es + nbytes // es]


def guards_intact(big, container):
    raw = big.cpu().numpy().view(np.uint8)
    return bool((raw[:GUARD] == 0x5A).all() and (raw[-GUARD:] == 0x5A).all())


def shapes():
    return [(w, h) for w in WIDTHS for h in HEIGHTS] + [WIDE]


@pytest.mark.parametrize("fmt,depth,container", [(f, b, c) for f, b, cs in FORMATS for c in cs])
def test_stages_against_the_numpy_pair_and_write_nothing_else(fmt, depth, container):
    from openjph_amd import codec
    from openjph_amd.pipeline import pack_video, video_layout
    rng = np.random.default_rng(depth * 1000 + container)
    for w, h in shapes():
        planes = random_planes(rng, w, h, depth)
        flat = np.concatenate([p.reshape(-1) for p in planes]).astype(NP_DT[container])
        buf = pack_video(planes, fmt, depth)
        row, total = video_layout(fmt, w, h)
        # unpack, with garbage in every padding position, into a flat buffer with the three planes inside it
        big, out = guarded(flat.size * (container // 8), container)
        got = codec.unpack_video(to_dev(garbage_in_padding(rng, buf, fmt, w, depth)), fmt, w, h, depth, out=out)
        assert got.data_ptr() == out.data_ptr() and got.numel() == flat.size
        assert np.array_equal(got.cpu().numpy().view(NP_DT[container]), flat), (fmt, container, w, h)
        assert guards_intact(big, container), (fmt, container, w, h)
        # pack: byte for byte, the zeros of the padding included
        big, out = guarded(total, 8)
        got = codec.pack_video(to_dev(flat), fmt, w, h, depth, out=out)
        assert got.shape == (h, row) and got.data_ptr() == out.data_ptr()
        assert got.cpu().numpy().tobytes() == buf.tobytes(), (fmt, container, w, h)
        assert guards_intact(big, 8), (fmt, container, w, h)
    # without out=: tensors of the stages' own
    w, h = 97, 3
    planes = random_planes(rng, w, h, depth)
    flat = np.concatenate([p.reshape(-1) for p in planes]).astype(NP_DT[container])
    import torch
    dt = {8: torch.uint8, 16: torch.int16, 32: torch.int32}[container]
    d = codec.unpack_video(to_dev(pack_video(planes, fmt, depth)), fmt, w, h, depth, dtype=dt)
    assert d.dtype == dt and np.array_equal(d.cpu().numpy().view(NP_DT[container]), flat)
    assert codec.pack_video(d, fmt, w, h, depth).cpu().numpy().tobytes() == pack_video(planes, fmt, depth).tobytes()


@pytest.mark.parametrize("fmt,depth", [(f, b) for f, b, _ in FORMATS])
def test_clamp_on_the_device(fmt, depth):
    from openjph_amd import codec
    from openjph_amd.pipeline import pack_video, unpack_video
    rng = np.random.default_rng(depth)
    for w, h in ((49, 3), (200, 2)):
        planes = [rng.choice(np.array([1 << depth, (1 << depth) + 5, -1, -70000, 0, (1 << depth) - 1, 3], np.int32), p.shape)
                  for p in random_planes(rng, w, h, depth)]
        flat = np.concatenate([p.reshape(-1) for p in planes]).astype(np.int32)
        got = codec.pack_video(to_dev(flat), fmt, w, h, depth).cpu().numpy()
        assert got.tobytes() == pack_video(planes, fmt, depth).tobytes()
        for a, b in zip(unpack_video(got, fmt, w, h, depth), planes):
            assert np.array_equal(a, np.clip(b, 0, (1 << depth) - 1))


def test_stage_refusals():
    import torch
    from openjph_amd import capi, codec
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    planes16 = torch.zeros(4096, dtype=torch.int16, device="cuda")
    planes8 = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    def invalid(fn, *a, **kw):
        with pytest.raises(capi.OjphError) as e:
            fn(*a, **kw)
        return e.value.code == capi.E_INVALID

    assert invalid(codec.unpack_video, buf[4:], "uyvy", 48, 2, 8, out=planes16)            # d_video not 16-byte aligned
    assert invalid(codec.pack_video, planes16, "v210", 48, 2, 10, out=buf[8:])
    assert invalid(codec.unpack_video, buf, "v210", 48, 2, 8, out=planes8)                 # container 8 with v210
    assert invalid(codec.pack_video, planes8, "v210", 48, 2, 8)
    assert invalid(codec.pack_video, planes8, "y210", 48, 2, 10)                           # a container narrower than the depth
    L = capi.lib()
    assert L.ojphgpu_unpack_video(None, 5, buf.data_ptr(), planes16.data_ptr(), 48, 2, 8, 16) == capi.E_INVALID
    assert L.ojphgpu_unpack_video(None, 1, None, planes16.data_ptr(), 48, 2, 8, 16) == capi.E_INVALID
    assert L.ojphgpu_unpack_video(None, 1, buf.data_ptr(), planes16.data_ptr(), 0, 2, 8, 16) == capi.E_INVALID
    assert L.ojphgpu_unpack_video(None, 3, buf.data_ptr(), planes16.data_ptr(), 48, 2, 11, 16) == capi.E_INVALID
    assert L.ojphgpu_pack_video(None, 4, planes16.data_ptr(), buf.data_ptr(), 48, 2, 16, 8) == capi.E_INVALID
    torch.cuda.synchronize()


# ---- the pipes
@pytest.mark.parametrize("fmt,w,depth,rev,container", [("v210", 98, 10, True, 16), ("v210", 98, 10, False, 16), ("y210", 98, 10, True, 16),
                                                        ("y210", 98, 10, False, 32), ("uyvy", 97, 8, True, 8), ("yuy2", 97, 8, True, 16),
                                                        ("y212", 98, 12, True, 16), ("y216", 98, 16, True, 32)])
def test_encoder_pipe_fed_video_buffers(fmt, w, depth, rev, container):
    from openjph_amd import codec
    from openjph_amd.pipeline import EncoderPipe, pack_video, video_layout
    from oracle import refbind
    rng = np.random.default_rng(depth + w)
    frames = [random_planes(rng, w, 34, depth) for _ in range(3)]
    enc = codec.Encoder(plan=make_plan(w, 34, depth, rev, C422))
    want = [enc.encode(enc.plan.pack_frame(p)) for p in frames]
    pipe = EncoderPipe(plan=make_plan(w, 34, depth, rev, C422), depth=2, container=container, video=fmt)     # three frames: the slots are recycled
    buf = pipe.acquire()
    assert buf.dtype == np.uint8 and buf.shape == (34, video_layout(fmt, w, 34)[0])
    got = list(pipe.encode_sequence(pack_video(p, fmt, depth) for p in frames))
    pipe.close()
    assert got == want
    if refbind.available(generic=not rev):               # the reference's own bytes for the same planes
        lib = refbind.Ref(generic=not rev)
        assert got[0] == lib.encode(frames[0], depth, reversible=rev, downsampling=DS422, size=(w, 34))


@pytest.mark.parametrize("fmt,w,depth", [("v210", 98, 10), ("y210", 98, 10), ("uyvy", 97, 8), ("yuy2", 97, 8)])
def test_decoder_pipe_hands_back_video_buffers(fmt, w, depth):
    from openjph_amd import codec
    from openjph_amd.pipeline import DecoderPipe, pack_video
    rng = np.random.default_rng(w + depth)
    lossless = codec.Encoder(plan=make_plan(w, 34, depth, True, C422)).encode(random_planes(rng, w, 34, depth))
    lossy = codec.Encoder(plan=make_plan(w, 34, depth, False, C422, qstep=0.05)).encode(edged_planes(5, w, 34, depth, C422))
    assert max(int(p.max()) for p in decoded_planes(lossy)) > (1 << depth) - 1          # the clamp has something to do
    for cs, view in ((lossless, {}), (lossy, {}), (lossless, dict(skip_res=1)), (lossless, dict(region=(32, 5, 49, 20))),
                     (lossy, dict(skip_res=(1, 1), region=(16, 2, 21, 9)))):
        want = pack_video(decoded_planes(cs, **view), fmt, depth)
        pipe = DecoderPipe(cs, depth=2, video=fmt, **view)
        got = list(pipe.decode_sequence([cs] * 3))
        pipe.close()
        for g in got:
            assert g.dtype == np.uint8 and g.shape == want.shape and g.tobytes() == want.tobytes(), (fmt, view)


def test_video_frames_through_the_searches():
    from openjph_amd import codec
    from openjph_amd.pipeline import EncoderPipe, pack_video
    from tests.synth import synth_image
    w, h, depth = 98, 34, 10
    img = synth_image(3, h, w, depth, seed=3)
    planes = [img[0], img[1][:, : (w + 1) // 2], img[2][:, : (w + 1) // 2]]
    plain = len(codec.Encoder(plan=make_plan(w, 34, depth, False, C422)).encode(planes))
    for kw in (dict(max_bytes=plain * 2 // 3), dict(min_psnr=38.0)):
        a = EncoderPipe(plan=make_plan(w, 34, depth, False, C422), depth=2, video="v210", **kw)
        got = list(a.encode_sequence([pack_video(planes, "v210", depth)]))
        a.close()
        b = EncoderPipe(plan=make_plan(w, 34, depth, False, C422), depth=2, **kw)
        feed_planes(b, planes)
        want = b.collect()
        b.close()
        assert got == [want] and ("max_bytes" not in kw or len(want) <= plain * 2 // 3)


def test_pipe_refusals_leave_a_plane_pipe():
    from openjph_amd import capi, codec
    from openjph_amd.pipeline import DecoderPipe, EncoderPipe
    rng = np.random.default_rng(11)

    def still_a_plane_pipe(pipe):
        ci = [pipe.plan.comp_info(c) for c in range(3)]
        planes = [rng.integers(0, 200, (i["h"], i["w"])).astype(np.int32) for i in ci]
        feed_planes(pipe, planes)
        return pipe.collect() == codec.Encoder(plan=pipe.plan).encode(planes)

    def enc_refuses(fmt, w=98, depth=10, **plan_kw):
        pipe = EncoderPipe(plan=make_plan(w, 34, depth, True, C422, **plan_kw), depth=2, container=16)
        with pytest.raises(capi.OjphError) as e:
            pipe.set_video(fmt)
        ok = e.value.code == capi.E_INVALID and pipe.video is None and still_a_plane_pipe(pipe)
        pipe.close()
        return ok

    assert enc_refuses("v210", downsampling=None)                                          # 4:4:4
    assert enc_refuses("v210", downsampling=[(1, 1), (2, 2), (2, 2)])                      # 4:2:0
    assert enc_refuses("v210", signs=[False, True, True])                                  # a signed component
    assert enc_refuses("v210", is_signed=True)
    assert enc_refuses("v210", bit_depths=[10, 8, 8])                                      # mixed depths
    assert enc_refuses("v210", depth=12)
    assert enc_refuses("y210", depth=8)
    assert enc_refuses("uyvy", depth=10)
    # video together with pixels / packed, either order
    pipe = EncoderPipe(plan=make_plan(98, 34, 10, True, C422), depth=2, packed=10)
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video("v210")
    assert e.value.code == capi.E_INVALID
    pipe.close()
    pipe = EncoderPipe(plan=make_plan(98, 34, 10, True, C422), depth=2, video="v210")
    assert pipe._lib.ojphgpu_enc_pipe_set_packed(pipe._h, 10) == capi.E_INVALID
    assert pipe._lib.ojphgpu_enc_pipe_set_pixels(pipe._h, 16, 0) == capi.E_INVALID
    pipe.set_video(None)                                                                   # 0 switches back to planes
    assert still_a_plane_pipe(pipe)
    pipe.close()
    with pytest.raises(capi.OjphError):
        EncoderPipe(plan=make_plan(98, 34, 8, True, C422, downsampling=None), depth=2, container=8, pixels=(8, False), video="uyvy")
    # a call after the first acquire()
    pipe = EncoderPipe(plan=make_plan(98, 34, 10, True, C422), depth=2)
    pipe.acquire()
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video("v210")
    assert e.value.code == capi.E_INVALID and still_a_plane_pipe(pipe)
    pipe.close()
    # the decoder: a window that starts on an odd column, packed frames, a call after the first submit()
    planes = random_planes(rng, 98, 34, 10)
    cs = codec.Encoder(plan=make_plan(98, 34, 10, True, C422)).encode(planes)
    for region in ((33, 5, 49, 20), (33, 5, 50, 20)):
        pipe = DecoderPipe(cs, depth=2, region=region)
        with pytest.raises(capi.OjphError) as e:
            pipe.set_video("v210")
        assert e.value.code == capi.E_INVALID and pipe.video is None
        (got,) = list(pipe.decode_sequence([cs]))
        assert np.array_equal(got, codec.decode(cs, region=region))
        pipe.close()
    pipe = DecoderPipe(cs, depth=2, packed=10)
    with pytest.raises(capi.OjphError):
        pipe.set_video("v210")
    pipe.close()
    with pytest.raises(capi.OjphError):
        DecoderPipe(cs, depth=2, video="y212").close()
    pipe = DecoderPipe(cs, depth=2)
    (got,) = list(pipe.decode_sequence([cs]))
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video("v210")
    assert e.value.code == capi.E_INVALID
    assert np.array_equal(pipe.plan.unpack_frame(got)[0], planes[0])
    pipe.close()
