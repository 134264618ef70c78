"""4:4:4 packed video on the device (ojphgpu.h section 7d, kernels_video444.hip): the two stages against their numpy statement
(pipeline.pack_video444 / unpack_video444) over every format and container, the widths around a lane's piece and a
wavefront's run, in the tight layout and in two pitched ones; that packing writes [0, row_bytes) of every row and nothing
else; the clamp; the refusals; and the frame pipelines fed with and handing back such buffers, against the plain codec
objects."""
import numpy as np
import pytest

from tests.test_cpu_video444 import garbage_in_padding444, random_planes444
from tests.video_cases import FILL, GUARD, decoded_planes, edged_planes, feed_planes, guarded_bytes, make_plan, pitched, to_dev

pytestmark = pytest.mark.gpu

# name, bit depth, containers
FORMATS = (("v410", 10, (16, 32)), ("y410", 10, (16, 32)), ("r210", 10, (16, 32)), ("r10k", 10, (16, 32)), ("y412", 12, (16, 32)),
           ("y416", 16, (16, 32)), ("ayuv", 8, (8, 16, 32)), ("bgra", 8, (8, 16, 32)), ("rgba", 8, (8, 16, 32)), ("argb", 8, (8, 16, 32)))
# around a lane's piece (4 pixels, Y4XX: 2) and a wavefront's run of 64 pieces (256 pixels, Y4XX: 128)
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
HEIGHTS = (1, 2, 3, 5)
WIDE = (6149, 5)            # several workgroups share a row; 5 rows: two workgroups deep
NP_DT = {8: np.uint8, 16: np.uint16, 32: np.int32}


def shapes():
    return [(w, h) for w in WIDTHS for h in HEIGHTS] + [WIDE]


def layouts(fmt, w, h):
    """-> (pitch or None: the tight layout, the buffer's offset from a 256-byte boundary)"""
    from openjph_amd.pipeline import video444_layout
    row = video444_layout(fmt, w, h)[0]
    pixel = row // w
    return ((None, 0),                                             # tight
            (row + 3 * pixel, pixel),                              # one pixel off 16 bytes, and the alignment changes row by row
            (-(-row // 256) * 256, 0))                             # a multiple of 256


@pytest.mark.parametrize("fmt,depth,container", [(f, b, c) for f, b, cs in FORMATS for c in cs])
def test_stages_against_the_numpy_pair_and_write_nothing_else(fmt, depth, container):
    import torch
    from openjph_amd import codec
    from openjph_amd.pipeline import pack_video444, video444_layout
    rng = np.random.default_rng(depth * 1000 + container)
    es = container // 8
    for w, h in shapes():
        planes = random_planes444(rng, w, h, depth)
        flat = np.concatenate([p.reshape(-1) for p in planes]).astype(NP_DT[container])
        buf = pack_video444(planes, fmt, depth)
        row, total = video444_layout(fmt, w, h)
        assert buf.shape == (h, row)
        dirty = garbage_in_padding444(rng, buf, fmt, depth)
        for pitch, off in layouts(fmt, w, h):
            what = (fmt, container, w, h, pitch, off)
            kw = {} if pitch is None else dict(pitch=pitch)
            # unpack: garbage in every position it must not look at, pitch slack included, into a buffer between guards
            host = guarded_bytes(pitched(dirty, pitch, rng), GUARD + off)
            d_v = to_dev(host)
            big = torch.full((flat.size + 2 * GUARD // es,), {8: FILL, 16: 0x5A5A, 32: 0x5A5A5A5A}[container],
                             dtype={8: torch.uint8, 16: torch.int16, 32: torch.int32}[container], device="cuda")
            out = big[GUARD // es: GUARD // es + flat.size]
            got = codec.unpack_video444(d_v[GUARD + off:len(host) - GUARD], fmt, w, h, depth, out=out, **kw)
            assert got.data_ptr() == out.data_ptr() and got.numel() == flat.size
            assert np.array_equal(big.cpu().numpy().view(np.uint8), guarded_bytes(flat.view(np.uint8))), what
            # pack into a destination pre-filled with the pattern: [0, row_bytes) of every row is the numpy statement, padding
            # zeros and alpha included; the bytes between row_bytes and the pitch and the guards keep the pattern
            want = guarded_bytes(pitched(buf, pitch), GUARD + off)
            d_v = torch.full((len(want),), FILL, dtype=torch.uint8, device="cuda")
            got = codec.pack_video444(to_dev(flat), fmt, w, h, depth, out=d_v[GUARD + off:len(want) - GUARD], **kw)
            assert got.data_ptr() == d_v.data_ptr() + GUARD + off and (pitch is not None or got.shape == buf.shape)
            assert np.array_equal(d_v.cpu().numpy(), want), what
    # without out=: tensors of the stages' own, the tight layout
    w, h = 97, 3
    planes = random_planes444(rng, w, h, depth)
    flat = np.concatenate([p.reshape(-1) for p in planes]).astype(NP_DT[container])
    dt = {8: torch.uint8, 16: torch.int16, 32: torch.int32}[container]
    d = codec.unpack_video444(to_dev(pack_video444(planes, fmt, depth)), fmt, w, h, depth, dtype=dt)
    assert d.dtype == dt and np.array_equal(d.cpu().numpy().view(NP_DT[container]), flat)
    assert codec.pack_video444(d, fmt, w, h, depth).cpu().numpy().tobytes() == pack_video444(planes, fmt, depth).tobytes()
    if container == (8 if depth <= 8 else 16):                # the default container of unpacking
        d = codec.unpack_video444(to_dev(pack_video444(planes, fmt, depth)), fmt, w, h, depth)
        assert d.dtype == dt and np.array_equal(d.cpu().numpy().view(NP_DT[container]), flat)


@pytest.mark.parametrize("fmt,depth", [(f, b) for f, b, _ in FORMATS] + [("v410", 7), ("y4xx", 9), ("bgra", 1)])
def test_clamp_on_the_device(fmt, depth):
    from openjph_amd import codec
    from openjph_amd.pipeline import pack_video444, unpack_video444
    rng = np.random.default_rng(depth)
    top = (1 << depth) - 1
    for w, h in ((49, 3), (200, 5)):
        # 32-bit containers: below zero and above the range; 16-bit containers: above the range where the container holds such a
        # value (a uint16 sample has no sign)
        for container, values in ((32, [top + 1, top + 5, -1, -70000, 0, top, 3, 1 << 20]),
                                  (16, [v for v in (top + 1, top + 5, 0xFFFF, 0x8000, 0, top, 3) if v <= 0xFFFF])):
            planes = [rng.choice(np.array(values, np.int32), (h, w)) for _ in range(3)]
            flat = np.concatenate([p.reshape(-1) for p in planes]).astype(NP_DT[container])
            got = codec.pack_video444(to_dev(flat), fmt, w, h, depth).cpu().numpy()
            assert got.tobytes() == pack_video444(planes, fmt, depth).tobytes(), (w, h, container)
            for a, b in zip(unpack_video444(got, fmt, w, h, depth), planes):
                assert np.array_equal(a, np.clip(b, 0, top))


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

    # 48 x 4: row_bytes 192, y4xx: 384
    for off in (1, 2, 3):
        assert invalid(codec.unpack_video444, buf[off:], "v410", 48, 4, out=planes16)                      # a misaligned pointer
        assert invalid(codec.pack_video444, planes8, "bgra", 48, 4, out=buf[off:])
    assert invalid(codec.unpack_video444, buf[4:], "y416", 48, 4, out=planes16)                            # 4 mod 8 for Y4XX
    assert invalid(codec.pack_video444, planes16, "y412", 48, 4, out=buf[4:])
    assert invalid(codec.unpack_video444, buf, "r210", 48, 4, out=planes16, pitch=194)                     # a misaligned pitch
    assert invalid(codec.pack_video444, planes16, "r10k", 48, 4, out=buf, pitch=193)
    assert invalid(codec.unpack_video444, buf, "y416", 48, 4, out=planes16, pitch=388)
    assert invalid(codec.pack_video444, planes16, "y416", 48, 4, out=buf, pitch=388)
    assert invalid(codec.unpack_video444, buf, "y410", 48, 4, out=planes16, pitch=188)                     # a pitch below row_bytes
    assert invalid(codec.pack_video444, planes8, "argb", 48, 4, out=buf, pitch=188)
    assert invalid(codec.pack_video444, planes16, "y416", 48, 4, out=buf, pitch=376)
    assert invalid(codec.unpack_video444, buf, "v410", 48, 4, out=planes8)                                 # an 8-bit container with a dword format
    assert invalid(codec.pack_video444, planes8, "r210", 48, 4, 8)
    assert invalid(codec.pack_video444, planes8, "y416", 48, 4)
    L = capi.lib()
    b, b2, p8, p16, p32 = buf.data_ptr(), buf2.data_ptr(), planes8.data_ptr(), planes16.data_ptr(), planes32.data_ptr()
    assert L.ojphgpu_unpack_video444(None, 0x21, b, 192, p16, 48, 4, 10, 16) == capi.OK                    # (the calls below differ from these in one thing)
    assert L.ojphgpu_pack_video444(None, 0x25, p32, b, 384, 48, 4, 32, 12) == capi.OK
    assert L.ojphgpu_unpack_video444(None, 0x27, b, 192, p8, 48, 4, 8, 8) == capi.OK
    assert L.ojphgpu_pack_video444(None, 0x21, p16, b, 192, 48, 4, 16, 8) == capi.OK                       # v410 at 8 bits, 16-bit containers
    assert L.ojphgpu_unpack_video444(None, 0x21, b, 192, p16, 48, 4, 11, 16) == capi.E_INVALID             # depth 11 with v410
    assert L.ojphgpu_unpack_video444(None, 0x21, b, 192, p16, 48, 4, 0, 16) == capi.E_INVALID
    assert L.ojphgpu_pack_video444(None, 0x23, p16, b, 192, 48, 4, 16, 12) == capi.E_INVALID
    assert L.ojphgpu_pack_video444(None, 0x25, p32, b, 384, 48, 4, 32, 8) == capi.E_INVALID                # depth 8 with Y4XX
    assert L.ojphgpu_pack_video444(None, 0x25, p32, b, 384, 48, 4, 32, 17) == capi.E_INVALID
    assert L.ojphgpu_unpack_video444(None, 0x27, b, 192, p8, 48, 4, 9, 16) == capi.E_INVALID               # depth 9 with BGRA
    assert L.ojphgpu_unpack_video444(None, 0x25, b, 384, p8, 48, 4, 12, 8) == capi.E_INVALID               # a container below the depth
    assert L.ojphgpu_unpack_video444(None, 0x21, b, 192, p16, 48, 4, 10, 4) == capi.E_INVALID              # no such container
    assert L.ojphgpu_pack_video444(None, 0x21, p8, b, 192, 48, 4, 8, 8) == capi.E_INVALID                  # an 8-bit container, not a byte format
    assert L.ojphgpu_unpack_video444(None, 0x24, b, 192, p8, 48, 4, 8, 8) == capi.E_INVALID
    for code in (0, 1, 3, 4, 5, 0x11, 0x12, 0x13, 0x20, 0x2A):                                             # the codes of 7b and 7c among them
        assert L.ojphgpu_unpack_video444(None, code, b, 384, p16, 48, 4, 8, 16) == capi.E_INVALID
        assert L.ojphgpu_pack_video444(None, code, p16, b, 384, 48, 4, 16, 8) == capi.E_INVALID
    for code in range(0x21, 0x2A):                                                                          # sections 7b and 7c keep their formats
        assert L.ojphgpu_unpack_video(None, code, b, p16, 48, 4, 8, 16) == capi.E_INVALID
        assert L.ojphgpu_pack_video(None, code, p16, b, 48, 4, 16, 8) == capi.E_INVALID
        assert L.ojphgpu_unpack_video420(None, code, b, 384, b2, 384, p16, 48, 4, 8, 16) == capi.E_INVALID
        assert L.ojphgpu_pack_video420(None, code, p16, b, 384, b2, 384, 48, 4, 16, 8) == capi.E_INVALID
    assert L.ojphgpu_unpack_video444(None, 0x21, None, 192, p16, 48, 4, 10, 16) == capi.E_INVALID          # a null pointer
    assert L.ojphgpu_unpack_video444(None, 0x21, b, 192, None, 48, 4, 10, 16) == capi.E_INVALID
    assert L.ojphgpu_pack_video444(None, 0x25, None, b, 384, 48, 4, 32, 12) == capi.E_INVALID
    assert L.ojphgpu_pack_video444(None, 0x25, p32, None, 384, 48, 4, 32, 12) == capi.E_INVALID
    assert L.ojphgpu_unpack_video444(None, 0x21, b, 192, p16, 0, 4, 10, 16) == capi.E_INVALID              # a zero size
    assert L.ojphgpu_pack_video444(None, 0x25, p32, b, 384, 48, 0, 32, 12) == capi.E_INVALID
    assert L.ojphgpu_unpack_video444(None, 0x21, b, 188, p16, 48, 4, 10, 16) == capi.E_INVALID             # a pitch below row_bytes
    assert L.ojphgpu_unpack_video444(None, 0x21, b + 2, 192, p16, 48, 4, 10, 16) == capi.E_INVALID         # a misaligned pointer, pitch
    assert L.ojphgpu_pack_video444(None, 0x25, p32, b + 4, 384, 48, 4, 32, 12) == capi.E_INVALID
    assert L.ojphgpu_pack_video444(None, 0x25, p32, b, 388, 48, 4, 32, 12) == capi.E_INVALID
    assert L.ojphgpu_unpack_video444(None, 0x21, b, 0xFFFFFFFC, p16, 1 << 30, 1, 10, 16) == capi.E_INVALID  # row_bytes beyond 32 bits
    torch.cuda.synchronize()


# ---- the pipes
W, H = 98, 34


# one format of each pixel kind (little-endian dword, big-endian dword, four words, bytes), an RGB format on a plan with the colour
# transform on, reversible and irreversible
@pytest.mark.parametrize("fmt,depth,rev,container,ct", [("v410", 10, True, 16, False), ("y410", 10, False, 32, False), ("r210", 10, True, 16, True),
                                                         ("r10k", 10, False, 32, True), ("y412", 12, True, 16, False), ("y416", 16, False, 32, False),
                                                         ("ayuv", 8, True, 8, False), ("bgra", 8, False, 16, True), ("rgba", 8, True, 8, True),
                                                         ("argb", 8, False, 32, False)])
def test_encoder_pipe_fed_444_buffers(fmt, depth, rev, container, ct):
    from openjph_amd import codec
    from openjph_amd.pipeline import EncoderPipe, pack_video444, video444_layout
    rng = np.random.default_rng(depth + container)
    frames = [random_planes444(rng, W, H, depth) for _ in range(3)]
    enc = codec.Encoder(plan=make_plan(W, H, depth, rev, color_transform=ct))
    want = [enc.encode(enc.plan.pack_frame(p)) for p in frames]
    pipe = EncoderPipe(plan=make_plan(W, H, depth, rev, color_transform=ct), depth=2, container=container, video=fmt)     # three frames: the slots are recycled
    buf = pipe.acquire()
    assert buf.dtype == np.uint8 and buf.shape == (H, video444_layout(fmt, W, H)[0])
    got = list(pipe.encode_sequence(pack_video444(p, fmt, depth) for p in frames))
    pipe.close()
    assert got == want


@pytest.mark.parametrize("fmt,depth,ct", [("v410", 10, False), ("r210", 10, True), ("y412", 12, False), ("bgra", 8, True)])
def test_decoder_pipe_hands_back_444_buffers(fmt, depth, ct):
    from openjph_amd import codec
    from openjph_amd.pipeline import DecoderPipe, pack_video444
    rng = np.random.default_rng(depth)
    lossless = codec.Encoder(plan=make_plan(W, H, depth, True, color_transform=ct)).encode(random_planes444(rng, W, H, depth))
    lossy = codec.Encoder(plan=make_plan(W, H, depth, False, qstep=0.05)).encode(edged_planes(5, W, H, depth))
    assert max(int(p.max()) for p in decoded_planes(lossy)) > (1 << depth) - 1          # the clamp has something to do
    # plain, a reduced resolution, a window with odd x0 and odd y0, both
    for cs, view in ((lossless, {}), (lossy, {}), (lossless, dict(skip_res=1)), (lossy, dict(skip_res=1)), (lossless, dict(region=(33, 7, 49, 20))),
                     (lossy, dict(region=(33, 7, 49, 20))), (lossy, dict(skip_res=(1, 1), region=(17, 5, 21, 9)))):
        want = pack_video444(decoded_planes(cs, **view), fmt, depth)
        pipe = DecoderPipe(cs, depth=2, video=fmt, **view)
        got = list(pipe.decode_sequence([cs] * 3))
        pipe.close()
        for g in got:
            assert g.dtype == np.uint8 and g.shape == want.shape and g.tobytes() == want.tobytes(), (fmt, view)


def test_v410_frames_through_the_searches():
    from openjph_amd import codec
    from openjph_amd.pipeline import EncoderPipe, pack_video444
    from tests.synth import synth_image
    depth = 10
    img = synth_image(3, H, W, depth, seed=3)
    planes = [img[0], img[1], img[2]]
    plain = len(codec.Encoder(plan=make_plan(W, H, depth, False)).encode(planes))
    for kw in (dict(max_bytes=plain * 2 // 3), dict(min_psnr=38.0)):                      # one budget pipe, one quality pipe
        a = EncoderPipe(plan=make_plan(W, H, depth, False), depth=2, video="v410", **kw)
        got = list(a.encode_sequence([pack_video444(planes, "v410")]))
        a.close()
        want = codec.Encoder(plan=make_plan(W, H, depth, False), **kw).encode(planes)
        assert got == [want] and ("max_bytes" not in kw or len(want) <= plain * 2 // 3)


def test_pipe_refusals_leave_a_plane_pipe():
    from openjph_amd import capi, codec
    from openjph_amd.pipeline import DecoderPipe, EncoderPipe
    rng = np.random.default_rng(11)

    def still_a_plane_pipe(pipe):
        ci = [pipe.plan.comp_info(c) for c in range(int(pipe.plan.params.num_comps))]
        planes = [rng.integers(0, 100, (i["h"], i["w"])).astype(np.int32) for i in ci]
        feed_planes(pipe, planes)
        return pipe.collect() == codec.Encoder(plan=pipe.plan).encode(planes)

    def enc_refuses(fmt, depth=10, container=16, **plan_kw):
        pipe = EncoderPipe(plan=make_plan(W, H, depth, True, **plan_kw), depth=2, container=container)
        with pytest.raises(capi.OjphError) as e:
            pipe.set_video(fmt)
        ok = e.value.code == capi.E_INVALID and pipe.video is None and still_a_plane_pipe(pipe)
        pipe.close()
        return ok

    assert enc_refuses("v410", downsampling=[(1, 1), (2, 1), (2, 1)])                      # a sub-sampled plan: 4:2:2
    assert enc_refuses("bgra", depth=8, downsampling=[(1, 1), (2, 2), (2, 2)])             # 4:2:0
    assert enc_refuses("y412", depth=12, downsampling=[(1, 1), (1, 2), (1, 2)])
    assert enc_refuses("v210")                                                             # a 4:2:2 / 4:2:0 format on a 4:4:4 plan stays refused
    assert enc_refuses("uyvy", depth=8)
    assert enc_refuses("p010")
    assert enc_refuses("nv12", depth=8)
    assert enc_refuses("v410", num_comps=4)                                                # four components
    assert enc_refuses("bgra", depth=8, num_comps=4)
    assert enc_refuses("v410", signs=[False, True, True])                                  # a signed component
    assert enc_refuses("r210", is_signed=True)
    assert enc_refuses("v410", bit_depths=[10, 8, 8])                                      # mixed depths
    assert enc_refuses("y4xx", bit_depths=[12, 12, 10])
    assert enc_refuses("v410", depth=12)                                                   # a depth outside the column
    assert enc_refuses("y410", depth=11)
    assert enc_refuses("y4xx", depth=8)
    assert enc_refuses("y412", depth=10)                                                   # (the name fixes the depth)
    assert enc_refuses("bgra", depth=10)
    assert enc_refuses("argb", depth=9)
    # v410 with 8-bit containers: the plan has 8-bit samples, which v410 holds, but not in that container
    pipe = EncoderPipe(plan=make_plan(W, H, 8, True), depth=2, container=8)
    assert pipe._lib.ojphgpu_enc_pipe_set_video(pipe._h, 0x21) == capi.E_INVALID
    with pytest.raises(capi.OjphError):
        pipe.set_video("v410")
    assert pipe.video is None and still_a_plane_pipe(pipe)
    pipe.close()
    # video together with pixels / packed, either order
    pipe = EncoderPipe(plan=make_plan(W, H, 10, True), depth=2, packed=10)
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video("v410")
    assert e.value.code == capi.E_INVALID
    pipe.close()
    pipe = EncoderPipe(plan=make_plan(W, H, 8, True), depth=2, pixels=(8, False))
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video("bgra")
    assert e.value.code == capi.E_INVALID
    pipe.close()
    pipe = EncoderPipe(plan=make_plan(W, H, 10, True), depth=2, video="v410")
    assert pipe._lib.ojphgpu_enc_pipe_set_packed(pipe._h, 10) == capi.E_INVALID
    assert pipe._lib.ojphgpu_enc_pipe_set_pixels(pipe._h, 16, 0) == capi.E_INVALID
    pipe.set_video("y410")                                                                 # repeatable
    pipe.set_video(None)                                                                   # 0 switches back to planes
    assert pipe.video is None and still_a_plane_pipe(pipe)
    pipe.close()
    with pytest.raises(capi.OjphError):
        EncoderPipe(plan=make_plan(W, H, 8, True), depth=2, container=8, pixels=(8, False), video="bgra")
    # a call after the first acquire()
    pipe = EncoderPipe(plan=make_plan(W, H, 10, True), depth=2)
    pipe.acquire()
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video("v410")
    assert e.value.code == capi.E_INVALID and still_a_plane_pipe(pipe)
    pipe.close()
    # the decoder: a sub-sampled codestream, packed frames, a name of another depth, a call after the first submit()
    planes = random_planes444(rng, W, H, 10)
    cs = codec.Encoder(plan=make_plan(W, H, 10, True)).encode(planes)
    sub = make_plan(W, H, 10, True, downsampling=[(1, 1), (2, 1), (2, 1)])
    cs422 = codec.Encoder(plan=sub).encode([planes[0], planes[1][:, : (W + 1) // 2], planes[2][:, : (W + 1) // 2]])
    pipe = DecoderPipe(cs422, depth=2)
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video("v410")
    assert e.value.code == capi.E_INVALID and pipe.video is None
    (got,) = list(pipe.decode_sequence([cs422]))
    assert np.array_equal(got, codec.decode(cs422))
    pipe.close()
    pipe = DecoderPipe(cs, depth=2, packed=10)
    with pytest.raises(capi.OjphError):
        pipe.set_video("v410")
    pipe.close()
    with pytest.raises(capi.OjphError):
        DecoderPipe(cs, depth=2, video="y412").close()
    with pytest.raises(capi.OjphError):
        DecoderPipe(cs, depth=2, video="bgra").close()
    with pytest.raises(capi.OjphError):
        DecoderPipe(cs, depth=2, video="v210").close()
    pipe = DecoderPipe(cs, depth=2, video="v410")
    pipe.set_video(None)
    (got,) = list(pipe.decode_sequence([cs]))
    with pytest.raises(capi.OjphError) as e:
        pipe.set_video("v410")
    assert e.value.code == capi.E_INVALID
    assert np.array_equal(pipe.plan.unpack_frame(got)[0], planes[0])
    pipe.close()
