"""4:2:0 video buffers on the device (ojphgpu.h section 7c, kernels_video420.hip): the two stages against their numpy
statement (pipeline.pack_video420 / unpack_video420) over every format and container, the widths around a pair, a lane's
piece and a wavefront's run, in the tight layout and in two pitched ones; that packing writes [0, row_bytes) of every row and
nothing else; the clamp; the refusals; and the frame pipelines fed with and handing back such buffers, against the plain codec
objects (and the reference where it is built)."""
import numpy as np
import pytest

from tests.test_cpu_video420 import garbage_in_padding420, random_planes420
from tests.video_cases import C420, FILL, GUARD, decoded_planes, edged_planes, feed_planes, guarded_bytes, make_plan, pitched, to_dev

pytestmark = pytest.mark.gpu

# name, bit depth, containers
FORMATS = (("nv12", 8, (8, 16, 32)), ("nv21", 8, (8, 16, 32)), ("p010", 10, (16, 32)), ("p012", 12, (16, 32)), ("p016", 16, (16, 32)))
# around the pair and a lane's piece (2, 4 or 8 pairs = 4, 8, 16 pixels) ...
WIDTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
# ... and what the list above does not straddle: the smallest piece (4 pixels) and a wavefront's run of 64 pieces (256, 512 or
# 1024 pixels)
WIDTHS += (4, 5, 511, 512, 1023, 1024, 1025)
HEIGHTS = (1, 2, 3, 5)
WIDE = (6149, 5)            # several workgroups share a row; 5 + 3 rows: two workgroups deep
NP_DT = {8: np.uint8, 16: np.uint16, 32: np.int32}
DS420 = [(1, 1), (2, 2), (2, 2)]
DS422 = [(1, 1), (2, 1), (2, 1)]


def shapes():
    return [(w, h) for w in WIDTHS for h in HEIGHTS] + [WIDE]


def elem(fmt):
    return 4 if fmt.startswith("p0") else 2


def layouts(fmt, w, h):
    """-> (luma pitch, chroma pitch, the chroma plane's offset inside a tensor of its own or None: one tensor)"""
    from openjph_amd.pipeline import video420_layout
    row = video420_layout(fmt, w, h)[0]
    big = -(-row // 256) * 256
    return ((row, row, None),                                      # tight
            (row + 3 * elem(fmt), row + 3 * elem(fmt), elem(fmt)),   # row_bytes + 6 / + 12: the alignment changes row by row; chroma one element off 16 bytes
            (big, big + 256, 0))                                   # both pitches a multiple of 256


def surface(buf, h, lp, cp, coff, rng=None):
    """the [H + ch, row_bytes] statement as the bytes of the surface's tensors, guards included -> (luma or whole, chroma or None)"""
    if coff is None:
        return guarded_bytes(buf.reshape(-1)), None
    return guarded_bytes(pitched(buf[:h], lp, rng)), guarded_bytes(pitched(buf[h:], cp, rng), GUARD + coff)


@pytest.mark.parametrize("fmt,depth,container", [(f, b, c) for f, b, cs in FORMATS for c in cs])
def test_stages_against_the_numpy_pair_and_write_nothing_else(fmt, depth, container):
    import torch
    from openjph_amd import codec
    from openjph_amd.pipeline import pack_video420, video420_layout
    rng = np.random.default_rng(depth * 1000 + container)
    es = container // 8
    for w, h in shapes():
        planes = random_planes420(rng, w, h, depth)
        flat = np.concatenate([p.reshape(-1) for p in planes]).astype(NP_DT[container])
        buf = pack_video420(planes, fmt, depth)
        row, off, total = video420_layout(fmt, w, h)
        assert buf.shape == (h + (h + 1) // 2, row)
        dirty = garbage_in_padding420(rng, buf, fmt, w, h, depth)
        for lp, cp, coff in layouts(fmt, w, h):
            what = (fmt, container, w, h, lp, cp, coff)
            kw = {} if coff is None else dict(luma_pitch=lp, chroma_pitch=cp)
            # unpack: garbage in every position it must not look at, pitch slack included, into a buffer between guards
            host_l, host_c = surface(dirty, h, lp, cp, coff, rng)
            d_l = to_dev(host_l)
            d_c = None if host_c is None else to_dev(host_c)
            big = torch.full((flat.size + 2 * GUARD // es,), {8: FILL, 16: 0x5A5A, 32: 0x5A5A5A5A}[container],
                             dtype={8: torch.uint8, 16: torch.int16, 32: torch.int32}[container], device="cuda")
            out = big[GUARD // es: GUARD // es + flat.size]
            got = codec.unpack_video420(d_l[GUARD:len(host_l) - GUARD], fmt, w, h, depth, out=out,
                                        chroma=None if d_c is None else d_c[GUARD + coff:len(host_c) - GUARD], **kw)
            assert got.data_ptr() == out.data_ptr() and got.numel() == flat.size
            assert np.array_equal(big.cpu().numpy().view(np.uint8), guarded_bytes(flat.view(np.uint8))), what
            # pack into a destination pre-filled with the pattern: [0, row_bytes) of every row is the numpy statement, padding
            # zeros included; the bytes between row_bytes and the pitch and the guards keep the pattern
            want_l, want_c = surface(buf, h, lp, cp, coff)
            d_l = torch.full((len(want_l),), FILL, dtype=torch.uint8, device="cuda")
            d_c = None if want_c is None else torch.full((len(want_c),), FILL, dtype=torch.uint8, device="cuda")
            got = codec.pack_video420(to_dev(flat), fmt, w, h, depth, out=d_l[GUARD:len(want_l) - GUARD],
                                      chroma=None if d_c is None else d_c[GUARD + coff:len(want_c) - GUARD], **kw)
            assert got.data_ptr() == d_l.data_ptr() + GUARD and (coff is not None or got.shape == buf.shape)
            assert np.array_equal(d_l.cpu().numpy(), want_l), what
            assert d_c is None or np.array_equal(d_c.cpu().numpy(), want_c), what
    # without out=: tensors of the stages' own, the tight layout
    w, h = 97, 3
    planes = random_planes420(rng, w, h, depth)
    flat = np.concatenate([p.reshape(-1) for p in planes]).astype(NP_DT[container])
    dt = {8: torch.uint8, 16: torch.int16, 32: torch.int32}[container]
    d = codec.unpack_video420(to_dev(pack_video420(planes, fmt, depth)), fmt, w, h, depth, dtype=dt)
    assert d.dtype == dt and np.array_equal(d.cpu().numpy().view(NP_DT[container]), flat)
    assert codec.pack_video420(d, fmt, w, h, depth).cpu().numpy().tobytes() == pack_video420(planes, fmt, depth).tobytes()


@pytest.mark.parametrize("fmt,depth", [(f, b) for f, b, _ in FORMATS])
def test_clamp_on_the_device(fmt, depth):
    from openjph_amd import codec
    from openjph_amd.pipeline import pack_video420, unpack_video420
    rng = np.random.default_rng(depth)
    for w, h in ((49, 3), (200, 5)):
        planes = [rng.choice(np.array([1 << depth, (1 << depth) + 5, -1, -70000, 0, (1 << depth) - 1, 3], np.int32), p.shape)
                  for p in random_planes420(rng, w, h, depth)]
        flat = np.concatenate([p.reshape(-1) for p in planes]).astype(np.int32)
        got = codec.pack_video420(to_dev(flat), fmt, w, h, depth).cpu().numpy()
        assert got.tobytes() == pack_video420(planes, fmt, depth).tobytes()
        for a, b in zip(unpack_video420(got, fmt, w, h, depth), planes):
            assert np.array_equal(a, np.clip(b, 0, (1 << depth) - 1))


def test_stage_refusals():
    import torch
    from openjph_amd import capi, codec
    buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    buf2 = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    planes32 = torch.zeros(4096, dtype=torch.int32, device="cuda")
    planes16 = torch.zeros(4096, dtype=torch.int16, device="cuda")
    planes8 = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    def invalid(fn, *a, **kw):
        with pytest.raises(capi.OjphError) as e:
            fn(*a, **kw)
        return e.value.code == capi.E_INVALID

    # 48 x 4: row_bytes 48 (nv12), 96 (p010)
    assert invalid(codec.unpack_video420, buf[1:], "nv12", 48, 4, 8, out=planes16)                          # a misaligned pointer: odd for NV12
    assert invalid(codec.pack_video420, planes16, "nv21", 48, 4, 8, out=buf[1:])
    assert invalid(codec.unpack_video420, buf[2:], "p010", 48, 4, out=planes16)                             # 2 mod 4 for P0XX
    assert invalid(codec.pack_video420, planes16, "p010", 48, 4, out=buf[2:])
    assert invalid(codec.unpack_video420, buf, "nv12", 48, 4, 8, out=planes16, luma_pitch=64, chroma=buf2[1:], chroma_pitch=64)
    assert invalid(codec.pack_video420, planes16, "p010", 48, 4, out=buf, luma_pitch=128, chroma=buf2[2:], chroma_pitch=128)
    assert invalid(codec.unpack_video420, buf, "nv12", 48, 4, 8, out=planes16, luma_pitch=49)               # a misaligned pitch
    assert invalid(codec.pack_video420, planes16, "nv12", 48, 4, 8, out=buf, luma_pitch=64, chroma=buf2, chroma_pitch=51)
    assert invalid(codec.unpack_video420, buf, "p010", 48, 4, out=planes16, luma_pitch=98)
    assert invalid(codec.pack_video420, planes16, "p010", 48, 4, out=buf, luma_pitch=128, chroma=buf2, chroma_pitch=102)
    assert invalid(codec.unpack_video420, buf, "nv12", 48, 4, 8, out=planes16, luma_pitch=46)               # a pitch below row_bytes
    assert invalid(codec.pack_video420, planes16, "p010", 48, 4, out=buf, luma_pitch=96, chroma=buf2, chroma_pitch=92)
    assert invalid(codec.unpack_video420, buf, "p010", 48, 4, out=planes8)                                  # container 8 with P0XX: below the depth
    assert invalid(codec.pack_video420, planes8, "p016", 48, 4)
    L = capi.lib()
    b, b2, p16, p32 = buf.data_ptr(), buf2.data_ptr(), planes16.data_ptr(), planes32.data_ptr()
    assert L.ojphgpu_unpack_video420(None, 0x11, b, 48, b2, 48, p16, 48, 4, 8, 16) == capi.OK               # (the calls below differ from this one in one thing)
    assert L.ojphgpu_pack_video420(None, 0x13, p32, b, 96, b2, 96, 48, 4, 32, 10) == capi.OK
    assert L.ojphgpu_unpack_video420(None, 0x11, b, 48, b2, 48, p16, 48, 4, 9, 16) == capi.E_INVALID        # depth 9 with NV12
    assert L.ojphgpu_pack_video420(None, 0x12, p16, b, 48, b2, 48, 48, 4, 16, 9) == capi.E_INVALID
    assert L.ojphgpu_unpack_video420(None, 0x13, b, 96, b2, 96, p16, 48, 4, 8, 16) == capi.E_INVALID        # depth 8 with P0XX
    assert L.ojphgpu_pack_video420(None, 0x13, p32, b, 96, b2, 96, 48, 4, 32, 17) == capi.E_INVALID
    assert L.ojphgpu_unpack_video420(None, 0x13, b, 96, b2, 96, p16, 48, 4, 12, 8) == capi.E_INVALID        # a container below the depth
    assert L.ojphgpu_unpack_video420(None, 0x11, b, 48, b2, 48, p16, 48, 4, 8, 4) == capi.E_INVALID
    for code in (5, 1, 0, 0x14):
        assert L.ojphgpu_unpack_video420(None, code, b, 96, b2, 96, p16, 48, 4, 8, 16) == capi.E_INVALID
        assert L.ojphgpu_pack_video420(None, code, p16, b, 96, b2, 96, 48, 4, 16, 8) == capi.E_INVALID
    for code in (0x11, 0x13):                                                                                  # section 7b keeps its four formats
        assert L.ojphgpu_unpack_video(None, code, b, p16, 48, 4, 8, 16) == capi.E_INVALID
    assert L.ojphgpu_unpack_video420(None, 0x11, None, 48, b2, 48, p16, 48, 4, 8, 16) == capi.E_INVALID     # a null pointer
    assert L.ojphgpu_unpack_video420(None, 0x11, b, 48, None, 48, p16, 48, 4, 8, 16) == capi.E_INVALID
    assert L.ojphgpu_unpack_video420(None, 0x11, b, 48, b2, 48, None, 48, 4, 8, 16) == capi.E_INVALID
    assert L.ojphgpu_pack_video420(None, 0x11, None, b, 48, b2, 48, 48, 4, 16, 8) == capi.E_INVALID
    assert L.ojphgpu_unpack_video420(None, 0x11, b, 48, b2, 48, p16, 0, 4, 8, 16) == capi.E_INVALID         # a zero size
    assert L.ojphgpu_pack_video420(None, 0x11, p16, b, 48, b2, 48, 48, 0, 16, 8) == capi.E_INVALID
    torch.cuda.synchronize()


# ---- the pipes
@pytest.mark.parametrize("fmt,w,h,depth,rev,container", [("nv12", 97, 33, 8, True, 8), ("nv21", 98, 34, 8, False, 16), ("p010", 98, 33, 10, True, 16),
                                                          ("p010", 97, 34, 10, False, 32), ("p012", 98, 34, 12, True, 16),
                                                          ("p016", 98, 34, 16, True, 32)])
def test_encoder_pipe_fed_420_buffers(fmt, w, h, depth, rev, container):
    from openjph_amd import codec
    from openjph_amd.pipeline import EncoderPipe, pack_video420, video420_layout
    from oracle import refbind
    rng = np.random.default_rng(depth + w + h)
    frames = [random_planes420(rng, w, h, depth) for _ in range(3)]
    enc = codec.Encoder(plan=make_plan(w, h, depth, rev, C420))
    want = [enc.encode(enc.plan.pack_frame(p)) for p in frames]
    pipe = EncoderPipe(plan=make_plan(w, h, depth, rev, C420), depth=2, container=container, video=fmt)     # three frames: the slots are recycled
    buf = pipe.acquire()
    assert buf.dtype == np.uint8 and buf.shape == (h + (h + 1) // 2, video420_layout(fmt, w, h)[0])
    got = list(pipe.encode_sequence(pack_video420(p, fmt, depth) for p in frames))
    pipe.close()
    assert got == want
    if refbind.available(generic=not rev):               # the reference's own bytes for the same planes
        lib = refbind.Ref(generic=not rev)
        assert got[0] == lib.encode(frames[0], depth, reversible=rev, downsampling=DS420, size=(w, h))


@pytest.mark.parametrize("fmt,w,h,depth", [("nv12", 97, 33, 8), ("nv21", 98, 34, 8), ("p010", 98, 34, 10)])
def test_decoder_pipe_hands_back_420_buffers(fmt, w, h, depth):
    from openjph_amd import codec
    from openjph_amd.pipeline import DecoderPipe, pack_video420
    rng = np.random.default_rng(w + depth)
    lossless = codec.Encoder(plan=make_plan(w, h, depth, True, C420)).encode(random_planes420(rng, w, h, depth))
    lossy = codec.Encoder(plan=make_plan(w, h, depth, False, C420, qstep=0.05)).encode(edged_planes(5, w, h, depth, C420))
    assert max(int(p.max()) for p in decoded_planes(lossy)) > (1 << depth) - 1          # the clamp has something to do
    for cs, view in ((lossless, {}), (lossy, {}), (lossless, dict(skip_res=1)), (lossy, dict(skip_res=1)), (lossless, dict(region=(32, 6, 49, 20))),
                     (lossy, dict(region=(32, 6, 49, 20))), (lossy, dict(skip_res=(1, 1), region=(16, 4, 21, 9)))):
        want = pack_video420(decoded_planes(cs, **view), fmt, depth)
        pipe = DecoderPipe(cs, depth=2, video=fmt, **view)
        got = list(pipe.decode_sequence([cs] * 3))
        pipe.close()
        for g in got:
            assert g.dtype == np.uint8 and g.shape == want.shape and g.tobytes() == want.tobytes(), (fmt, view)


def test_p010_frames_through_the_searches():
    from openjph_amd import codec
    from openjph_amd.pipeline import EncoderPipe, pack_video420
    from tests.synth import synth_image
    w, h, depth = 98, 34, 10
    img = synth_image(3, h, w, depth, seed=3)
    planes = [img[0], img[1][: (h + 1) // 2, : (w + 1) // 2], img[2][: (h + 1) // 2, : (w + 1) // 2]]
    plain = len(codec.Encoder(plan=make_plan(w, h, depth, False, C420)).encode(planes))
    for kw in (dict(max_bytes=plain * 2 // 3), dict(min_psnr=38.0)):                      # one budget pipe, one quality pipe
        a = EncoderPipe(plan=make_plan(w, h, depth, False, C420), depth=2, video="p010", **kw)
        got = list(a.encode_sequence([pack_video420(planes, "p010")]))
        a.close()
        b = EncoderPipe(plan=make_plan(w, h, depth, False, C420), depth=2, **kw)
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

    def enc_refuses(fmt, w=98, h=34, depth=10, container=16, **plan_kw):
        pipe = EncoderPipe(plan=make_plan(w, h, depth, True, C420, **plan_kw), depth=2, container=container)
        with pytest.raises(capi.OjphError) as e:
            pipe.set_video(fmt)
        ok = e.value.code == capi.E_INVALID and pipe.video is None and still_a_plane_pipe(pipe)
        pipe.close()
        return ok

    assert enc_refuses("nv12", depth=8, downsampling=DS422)                                # a 4:2:2 plan
    assert enc_refuses("nv12", depth=8, downsampling=None)                                 # 4:4:4
    assert enc_refuses("p010", downsampling=DS422)
    assert enc_refuses("v210")                                                             # a 4:2:2 format on a 4:2:0 plan
    assert enc_refuses("uyvy", depth=8)
    assert enc_refuses("p010", signs=[False, True, True])                                  # a signed component
    assert enc_refuses("p010", is_signed=True)
    assert enc_refuses("p010", bit_depths=[10, 8, 8])                                      # mixed depths
    assert enc_refuses("p010", depth=8)
    assert enc_refuses("p0xx", depth=8)
    assert enc_refuses("nv12", depth=10)
    assert enc_refuses("p012", depth=10)
    # p010 with container 8: such a pipe cannot exist on a 10-bit plan, so ask the library about 8-bit containers and P0XX on
    # the one plan that gets that far
    pipe = EncoderPipe(plan=make_plan(98, 34, 8, True, C420), depth=2, container=8)
    assert pipe._lib.ojphgpu_enc_pipe_set_video(pipe._h, 0x13) == capi.E_INVALID
    with pytest.raises(capi.OjphError):
        pipe.set_video("p010")
    assert pipe.video is None and still_a_plane_pipe(pipe)
    pipe.close()
    # video together with pixels / packed, either order
    pipe = EncoderPipe(plan=make_plan(98, 34, 10, True, C420), depth=2, packed=10)
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video("p010")
    assert e.value.code == capi.E_INVALID
    pipe.close()
    pipe = EncoderPipe(plan=make_plan(98, 34, 10, True, C420), depth=2, video="p010")
    assert pipe._lib.ojphgpu_enc_pipe_set_packed(pipe._h, 10) == capi.E_INVALID
    assert pipe._lib.ojphgpu_enc_pipe_set_pixels(pipe._h, 16, 0) == capi.E_INVALID
    pipe.set_video("p0xx")                                                                 # repeatable
    pipe.set_video(None)                                                                   # 0 switches back to planes
    assert pipe.video is None and still_a_plane_pipe(pipe)
    pipe.close()
    with pytest.raises(capi.OjphError):
        EncoderPipe(plan=make_plan(98, 34, 8, True, C420, downsampling=None), depth=2, container=8, pixels=(8, False), video="nv12")
    # a call after the first acquire()
    pipe = EncoderPipe(plan=make_plan(98, 34, 10, True, C420), depth=2)
    pipe.acquire()
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video("p010")
    assert e.value.code == capi.E_INVALID and still_a_plane_pipe(pipe)
    pipe.close()
    # the decoder: a window with odd x0; one with odd y0 and even height; packed frames; a call after the first submit()
    planes = random_planes420(rng, 98, 34, 10)
    cs = codec.Encoder(plan=make_plan(98, 34, 10, True, C420)).encode(planes)
    for region in ((33, 6, 49, 20), (33, 6, 50, 20), (32, 5, 49, 20), (32, 5, 50, 21)):
        pipe = DecoderPipe(cs, depth=2, region=region)
        with pytest.raises(capi.OjphError) as e:
            pipe.set_video("p010")
        assert e.value.code == capi.E_INVALID and pipe.video is None, region
        (got,) = list(pipe.decode_sequence([cs]))
        assert np.array_equal(got, codec.decode(cs, region=region))
        pipe.close()
    pipe = DecoderPipe(cs, depth=2, packed=10)
    with pytest.raises(capi.OjphError):
        pipe.set_video("p010")
    pipe.close()
    with pytest.raises(capi.OjphError):
        DecoderPipe(cs, depth=2, video="p012").close()
    with pytest.raises(capi.OjphError):
        DecoderPipe(cs, depth=2, video="v210").close()
    pipe = DecoderPipe(cs, depth=2, video="p010")
    pipe.set_video(None)
    (got,) = list(pipe.decode_sequence([cs]))
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video("p010")
    assert e.value.code == capi.E_INVALID
    assert np.array_equal(pipe.plan.unpack_frame(got)[0], planes[0])
    pipe.close()
