"""Decoder pipes that decode a view of every frame (ojphgpu_dec_pipe_create_view: reduced resolution, a window, both), and
the gather stage that uploads a view's bytes (ojphgpu_gather_runs, kernels_assemble.hip).  Everything is bit-exact: the
gather against its layout written in numpy, every frame out of a view pipe against codec.Decoder(cs, skip_res=, region=) of
that frame.  Codestreams are the small cases of tests/region_cases.py."""
import functools

import numpy as np
import pytest

from tests.region_cases import CASES, encode_case, planes_for

pytestmark = pytest.mark.gpu

SKIPS = [None, (1, 1), (2, 1)]
SEQ_CASES = ["rev-L5", "irv-L4", "odd-offsets-tiles", "420", "colour-irv", "block32", "block128x8"]
ORDERS = ["LRCP", "RLCP", "RPCL", "PCRL", "CPRL"]


def _case(name):
    return next((kw, size) for n, kw, size in CASES if n == name)


def _views(size):
    """(skip, region) of every view a sequence test runs: per skip an interior rectangle, one on the far edge, one sample,
    and the skip alone"""
    W, H = size
    regions = [(W // 3, H // 4, max(W // 3, 1), max(H // 3, 1)), (W - max(W // 4, 1), H - max(H // 3, 1), max(W // 4, 1), max(H // 3, 1)),
               (W // 2, H // 2, 1, 1), None]
    return [(s, r) for s in SKIPS for r in regions]


def _encode_frames(kw, size, n=5):
    """n codestreams of one geometry whose lengths go long, long, short, short, long: with depth 2 every slot takes a
    shorter frame after a longer one.  Irreversible cases change the step, reversible ones the amplitude."""
    from tests import cpu_pipeline as cp
    out = []
    for f in range(n):
        short = f % 4 >= 2
        k = {a: b for a, b in kw.items() if a != "nc"}
        planes = planes_for(kw, size, seed=11 + f)
        if not k.get("reversible", True):
            k["qstep"] = kw.get("qstep", 0.01) * (6.0 if short else 1.0)
        elif short:
            planes = [(q >> 3) + 100 for q in planes]
        k.setdefault("downsampling", [(1, 1)] * len(planes))
        out.append(cp.encode(planes, size=size, **k)[0])
    assert max(len(cs) for f, cs in enumerate(out) if f % 4 >= 2) < 0.8 * min(len(cs) for f, cs in enumerate(out) if f % 4 < 2)
    return out


@functools.lru_cache(maxsize=None)
def _streams(name):
    kw, size = _case(name)
    return _encode_frames(kw, size)


def _single(cs, skip, region, resilient=False, container=32):
    """the single decoder's frame of that view, flat, as a pipe of that container hands it out (narrow containers saturate)"""
    from openjph_amd import codec
    got = codec.Decoder(cs, skip_res=skip, region=region, resilient=resilient).decode().astype(np.int64).reshape(-1)
    return np.clip(got, 0, (1 << container) - 1) if container < 32 else got


def _run_pipe(streams, skip, region, **kw):
    from openjph_amd.pipeline import DecoderPipe
    pipe = DecoderPipe(streams[0], depth=2, skip_res=skip, region=region, **kw)
    try:
        return [f.astype(np.int64).reshape(-1) for f in pipe.decode_sequence(streams)]
    finally:
        pipe.close()


# ---- the gather stage --------------------------------------------------------------------------------------------------------
SRC_CAP = (1 << 20) + 64
LENGTHS = [1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 255, 4101, 70000]


def _layout(spans):
    """(src, n) sorted and apart -> run table with the places ojphgpu_plan_upload_runs gives, staged_len"""
    from openjph_amd.plan import run_dtype
    runs = np.zeros(len(spans), run_dtype)
    at = 0
    for i, (s, n) in enumerate(spans):
        at = ((at + 63) & ~63) + 64
        runs[i] = (s, at, n)
        at += n
    return runs, (((at + 63) & ~63) + 64 if spans else 0)


def _gather_spans():
    spans = [(0, 37)]                                            # a run at offset 0
    at = 37

    def add(res, n, gap=1):
        nonlocal at
        s = at + gap
        s += (res - s) % 16
        spans.append((s, n))
        at = s + n
    for res in range(16):                                         # every residue of src mod 16 with every short length
        for n in LENGTHS[:12]:
            add(res, n, gap=1 + (res * 7 + n) % 40)
    for i in range(300):                                          # a dense stretch: > 128 run starts in one 16 KB step
        add((i * 5) % 16, 1 + i % 3)
    for res in range(16):
        add(res, 4101, gap=1 + res % 3)
    for res in (3, 8, 14):
        add(res, 70000, gap=500)
    add(5, 300003, gap=17)                                        # crosses the workgroups' segments
    add(9, 16, gap=3)
    tail = 4099
    assert at + 1 < SRC_CAP - tail
    spans.append((SRC_CAP - tail, tail))                          # ends on the last byte of the source
    assert all(b[0] > a[0] + a[1] for a, b in zip(spans, spans[1:]))
    assert {s % 16 for s, _ in spans} == set(range(16)) and set(LENGTHS) <= {n for _, n in spans}
    return spans


def _check_gather(src_np, d_src, runs, staged):
    import torch
    from openjph_amd import codec
    want = np.zeros(staged, np.uint8)
    for r in runs:
        want[int(r["dst"]):int(r["dst"]) + int(r["n"])] = src_np[int(r["src"]):int(r["src"]) + int(r["n"])]
    out = torch.full((staged + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
    codec.gather_runs(d_src, runs, staged, out=out)
    got = out.cpu().numpy()
    assert (got[staged:] == 0xA5).all(), "the guard behind staged_len was written"
    bad = np.nonzero(got[:staged] != want)[0]
    assert bad.size == 0, "first difference at staged byte %d of %d" % (bad[0], staged)


def test_gather_stage_against_its_layout():
    import torch
    src_np = np.random.default_rng(5).integers(0, 256, SRC_CAP, dtype=np.uint8)
    d_src = torch.from_numpy(src_np).to("cuda:0")
    runs, staged = _layout(_gather_spans())
    assert staged % 64 == 0 and staged > 8 * 16384
    _check_gather(src_np, d_src, runs, staged)
    for spans in ([(1000, 5)], [(SRC_CAP - 1, 1)], [(0, 1), (2, 1), (SRC_CAP - 3, 3)], [(3, 16384 - 128)], [(3, 16384 - 127)]):
        _check_gather(src_np, d_src, *_layout(spans))


def test_gather_stage_empty_table_writes_nothing():
    import torch
    from openjph_amd import codec
    from openjph_amd.plan import run_dtype
    d_src = torch.zeros(SRC_CAP, dtype=torch.uint8, device="cuda:0")
    out = torch.full((512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    codec.gather_runs(d_src, np.zeros(0, run_dtype), 0, out=out)
    assert (out.cpu().numpy() == 0xA5).all()


# ---- sequences -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SEQ_CASES)
def test_view_pipe_matches_the_single_decoder(name):
    kw, size = _case(name)
    streams = _streams(name)
    for skip, region in _views(size):
        if skip is None and region is None:
            continue                                       # (the plain pipe: test_plain_pipes_are_unchanged)
        got = _run_pipe(streams, skip, region)
        assert len(got) == len(streams)
        for f, cs in enumerate(streams):
            assert np.array_equal(got[f], _single(cs, skip, region, container=16)), (name, skip, region, f)


@pytest.mark.parametrize("container", [8, 16, 32])
def test_view_pipe_containers(container):
    kw, size = _case("rev-L5")
    streams = _streams("rev-L5")
    for skip, region in (((1, 1), (20, 10, 40, 30)), (None, (50, 40, 27, 21)), ((2, 1), None)):
        got = _run_pipe(streams, skip, region, container=container)
        for f, cs in enumerate(streams):
            assert np.array_equal(got[f], _single(cs, skip, region, container=container)), (container, skip, region, f)


@pytest.mark.parametrize("order", ORDERS)
def test_view_pipe_progression_orders_small_precincts(order):
    kw, size = dict(reversible=True, num_decomps=3, prog_order=order, precinct=(32, 32), tile=(64, 64)), (128, 128)
    streams = _encode_frames(kw, size, n=3)
    for skip, region in (((1, 1), None), ((2, 1), (40, 50, 60, 30)), (None, (100, 90, 28, 38)), (None, (63, 64, 1, 1))):
        got = _run_pipe(streams, skip, region)
        for f, cs in enumerate(streams):
            assert np.array_equal(got[f], _single(cs, skip, region, container=16)), (order, skip, region, f)


# ---- hand-over forms -----------------------------------------------------------------------------------------------------------
def test_view_pipe_pixels_and_packed():
    from openjph_amd import codec
    from openjph_amd.pipeline import DecoderPipe, pack_bits
    kw, size = _case("colour")
    streams = _encode_frames(kw, size, n=3)
    for skip, region in ((None, (30, 20, 41, 33)), ((1, 1), (10, 8, 60, 50))):
        pipe = DecoderPipe(streams[0], depth=2, skip_res=skip, region=region, pixels=(8, False))
        got = list(pipe.decode_sequence(streams))
        pipe.close()
        for f, cs in enumerate(streams):
            d = codec.Decoder(cs, skip_res=skip, region=region)
            planes = d.run_device()
            assert d.failed_blocks() == 0
            want = codec.pack_pixels(planes, 8, pixel_bits=8).cpu().numpy()
            assert got[f].shape == want.shape == (planes.shape[1], planes.shape[2], 3)
            assert np.array_equal(got[f], want), (skip, region, f)
        pipe = DecoderPipe(streams[0], depth=2, skip_res=skip, region=region, packed=12)
        got = list(pipe.decode_sequence(streams))
        pipe.close()
        for f, cs in enumerate(streams):
            frame = np.clip(codec.Decoder(cs, skip_res=skip, region=region).decode(), 0, 4095)
            assert np.array_equal(got[f], pack_bits(frame, 12)), (skip, region, f)


def test_view_pipe_refuses_pixels_when_the_views_planes_differ():
    from openjph_amd import capi
    from openjph_amd.pipeline import DecoderPipe
    streams = _streams("420")
    with pytest.raises(capi.OjphError) as e:
        DecoderPipe(streams[0], depth=2, region=(10, 10, 30, 30), pixels=(8, False))
    assert e.value.code == capi.E_INVALID


# ---- view_info -----------------------------------------------------------------------------------------------------------------
def test_view_info():
    from openjph_amd.pipeline import DecoderPipe
    from openjph_amd.plan import parse_codestream
    for name in ("odd-offsets-tiles", "irv-L4"):
        kw, size = _case(name)
        streams = _streams(name)
        for skip, region in _views(size)[:8]:
            pipe = DecoderPipe(streams[0], depth=2, skip_res=skip, region=region)
            for f, frame in enumerate(pipe.decode_sequence(streams)):
                info = pipe.view_info()
                pl = parse_codestream(streams[f])
                nblocks = pl.num_blocks
                if skip:
                    pl.restrict_resolution(*skip)
                if region is not None:
                    pl.restrict_region(*region)
                sel, coded = pl.region_blocks(), pl.coded_blocks()
                assert info["blocks"] == int(sel.sum()) and info["plan_blocks"] == nblocks
                assert info["coded_bytes"] == int((coded["len1"].astype(np.int64) + coded["len2"])[sel].sum())
                if skip is None and region is None:      # a plain pipe: one byte range
                    lens = coded["len1"].astype(np.int64) + coded["len2"]
                    first = int(coded["offset"][lens > 0].min()) & ~15
                    last = int((coded["offset"].astype(np.int64) + lens)[lens > 0].max())
                    assert info["runs"] == 0 and info["staged_bytes"] == last - first
                else:
                    runs, staged = pl.upload_runs()
                    assert info["runs"] == runs.size and info["staged_bytes"] == staged
                    assert staged <= len(streams[f]) + 128 * runs.size + 128     # (a view may meet no coded block: 0 runs)
            pipe.close()


# ---- damage --------------------------------------------------------------------------------------------------------------------
def _collect_all(pipe, streams):
    """every frame's outcome in order: the frame, or the error code its collect raised"""
    from openjph_amd import capi
    out = []

    def take():
        try:
            out.append(pipe.collect().astype(np.int64).reshape(-1))
        except capi.OjphError as e:
            out.append(e.code)
    for cs in streams:
        buf = pipe.acquire(len(cs))
        while buf is None:
            take()
            buf = pipe.acquire(len(cs))
        buf[:] = np.frombuffer(cs, np.uint8)
        pipe.submit()
    while pipe.in_flight:
        take()
    return out


@pytest.mark.parametrize("skip,region", [((1, 1), (20, 15, 60, 40)), (None, (60, 30, 40, 50)), ((2, 1), None)], ids=["skip-window", "window", "skip"])
def test_view_pipe_with_a_damaged_frame(skip, region):
    from openjph_amd import capi, codec
    from openjph_amd.pipeline import DecoderPipe
    streams = list(_streams("odd-offsets-tiles"))
    good = list(streams)
    streams[2] = streams[2][:int(len(streams[2]) * 0.6)]
    pipe = DecoderPipe(good[0], depth=2, resilient=True, skip_res=skip, region=region)
    got = _collect_all(pipe, streams)
    pipe.close()
    for f, cs in enumerate(streams):
        assert not isinstance(got[f], int), (f, got[f])
        assert np.array_equal(got[f], _single(cs, skip, region, resilient=True, container=16)), f
    # not resilient: the damaged frame ends as it does in the single decoder, the sequence goes on
    try:
        verdict = _single(streams[2], skip, region, container=16)
    except capi.OjphError as e:
        verdict = e.code
    pipe = DecoderPipe(good[0], depth=2, skip_res=skip, region=region)
    got = _collect_all(pipe, streams)
    pipe.close()
    if isinstance(verdict, int):
        assert got[2] == verdict
    else:
        assert not isinstance(got[2], int) and np.array_equal(got[2], verdict)
    for f in (0, 1, 3, 4):
        assert np.array_equal(got[f], _single(streams[f], skip, region, container=16)), f


def test_view_pipe_codestream_of_another_geometry_fails_alone():
    from openjph_amd import capi
    from openjph_amd.pipeline import DecoderPipe
    streams = list(_streams("rev-L5"))
    other = _streams("block32")[0]
    region = (30, 20, 25, 30)
    seq = [streams[0], other, streams[1], streams[2]]
    pipe = DecoderPipe(streams[0], depth=2, skip_res=(1, 1), region=region)
    got = _collect_all(pipe, seq)
    pipe.close()
    assert got[1] == capi.E_INVALID
    for f in (0, 2, 3):
        assert np.array_equal(got[f], _single(seq[f], (1, 1), region, container=16)), f


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_view_pipe_refusals():
    """each refused with E_INVALID from create; a plain pipe (of the plain codestream) created afterwards works"""
    from openjph_amd import capi
    from openjph_amd.pipeline import DecoderPipe
    from tests import cpu_pipeline as cp
    from tests import part2_cases as p2
    kw, (W, H) = _case("rev-L5")
    streams = _streams("rev-L5")
    want = [_single(cs, None, None, container=16) for cs in streams]

    def part2(case):
        nc, h, w, bd, k = p2.split(case)
        return cp.encode(p2.image(nc, h, w, bd), **k)[0]
    refused = [(streams[0], dict(region=(0, 0, 0, 5))), (streams[0], dict(region=(0, 0, 5, 0))),
               (streams[0], dict(region=(W - 3, 0, 4, 2))), (streams[0], dict(region=(0, H, 1, 1))),
               (streams[0], dict(skip_res=(6, 6))), (streams[0], dict(skip_res=(1, 2))),
               (part2(p2.CASES[0]), dict(region=(0, 0, 8, 8))),
               (part2(dict(nc=1, h=64, w=64, bd=32, num_decomps=2)), dict(region=(0, 0, 8, 8), container=32))]
    for cs, view in refused:
        with pytest.raises(capi.OjphError) as e:
            DecoderPipe(cs, depth=2, **view)
        assert e.value.code == capi.E_INVALID, view
        pipe = DecoderPipe(streams[0], depth=2)
        got = [f.astype(np.int64).reshape(-1) for f in pipe.decode_sequence(streams)]
        pipe.close()
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), view


# ---- plain pipes ---------------------------------------------------------------------------------------------------------------
def test_plain_pipes_are_unchanged():
    from openjph_amd.pipeline import DecoderPipe
    for name in ("colour-irv", "odd-offsets-tiles"):
        streams = _streams(name)
        a = DecoderPipe(streams[0], depth=2)
        got_a = list(a.decode_sequence(streams))
        assert a.view_info()["runs"] == 0
        a.close()
        b = DecoderPipe(streams[0], depth=2, skip_res=None, region=None)
        got_b = list(b.decode_sequence(streams))
        assert b.view_info()["runs"] == 0
        b.close()
        for f, cs in enumerate(streams):
            assert np.array_equal(got_a[f], got_b[f])
            assert np.array_equal(got_a[f].astype(np.int64).reshape(-1), _single(cs, None, None, container=16))
