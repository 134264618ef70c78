"""Released decoder runs (include/ojphgpu.h, ojphgpu_decoder_run_device): with per-launch timing off a plain run of a
single-frame decoder that fuses issues its block launch (under OJPHGPU_DEC_AHEAD_LEVELS=1 synthesis levels L..2 too) on a
stream of the object's own -- behind the object's last upload and the last reader of the arena it writes, not behind the
caller's stream -- and the caller's stream waits for it in front of the synthesis; only the top level writes the image.
What can go wrong is a block launch that
overwrites planes a synthesis still reads (two arenas, or one), an upload that lands under a block launch, a consumer
that does not wait, and a path that must stay joined and is not.  Every image is compared exactly with the oracle
pipeline's samples and with those of a decoder created under OJPHGPU_NO_OVERLAP=1 (one stream, nothing released).

Frames: 192 x 160, three components, three decompositions, 64 x 64 code-blocks (tests/test_gpu_encoder_release.py's): 36
blocks of the top resolution and a non-empty set below, blocks 64 rows tall -- the decoder fuses and has a side stream.
A race on the arena is invisible while every run decodes the same bytes: B is A with bytes inside block bodies changed
(same layout), decoded resiliently; its expected samples and verdicts are the joined decoder's."""
import contextlib
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.synth import synth_image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, NC = 192, 160, 3
KINDS = {
    "irv97_12b": dict(bit_depth=12, reversible=False, qstep=0.002, num_decomps=3, block=(64, 64)),
    "rev53_8b_rct": dict(bit_depth=8, reversible=True, color_transform=True, num_decomps=3, block=(64, 64)),
}
NAMES = sorted(KINDS)
_REF = {}


@contextlib.contextmanager
def environ(**kw):
    """the switches are read when an object is created"""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def host(t, dtype=None):
    """a decoded image on the host; 16- / 8-bit containers of unsigned components read as unsigned"""
    a = t.cpu().numpy()
    if a.dtype == np.int16:
        a = a.view(np.uint16)
    if a.dtype == np.int8:
        a = a.view(np.uint8)
    return a.astype(np.int64)


def damaged(cs):
    """B: three block bodies of A with a byte changed in their first quarter (the magnitude bits), one block of every third
    of the plan's order -- lower resolutions and the top one"""
    from openjph_amd.plan import parse_codestream
    coded = parse_codestream(cs).coded_blocks()
    with_bytes = [i for i in range(len(coded)) if int(coded[i]["len1"]) >= 64]
    assert len(with_bytes) >= 3
    b = bytearray(cs)
    for i in (with_bytes[0], with_bytes[len(with_bytes) // 2], with_bytes[-1]):
        at = int(coded[i]["offset"]) + int(coded[i]["len1"]) // 4
        b[at] ^= 0x15
    return bytes(b)


def ref(name):
    """computed once and shared: codestream A of the kind (the oracle's), B, the oracle's samples of A, and what a decoder
    that never forks (OJPHGPU_NO_OVERLAP=1 at creation) gives for A (every container) and, resiliently, for B"""
    if name not in _REF:
        import torch
        from openjph_amd import codec
        from tests import cpu_pipeline as cp
        kw = KINDS[name]
        a = bytes(cp.encode(synth_image(NC, H, W, kw["bit_depth"], seed=5), **kw)[0])
        b = damaged(a)
        want_a = np.asarray(cp.decode(a)[0]).astype(np.int64)
        with environ(OJPHGPU_NO_OVERLAP="1"):
            plain = codec.Decoder(a, resilient=True)
        plain.set_timing(False)
        by_container = {}
        for bits, dt in ((32, torch.int32), (16, torch.int16), (8, torch.int8)):
            if kw["bit_depth"] > bits:
                continue
            out = plain.run_device(dtype=dt)
            assert not plain.pending()
            assert plain.failed_blocks() == 0
            by_container[bits] = host(out)
        assert np.array_equal(by_container[32], want_a)
        plain.upload(b)
        out = plain.run_device()
        failed_b = plain.failed_blocks()
        want_b = host(out)
        assert not np.array_equal(want_b, want_a)
        _REF[name] = dict(a=a, b=b, want_a=want_a, want_b=want_b, failed_b=failed_b, containers=by_container)
    return _REF[name]


def released(cs, **kw):
    """a decoder whose plain runs are released"""
    from openjph_amd import codec
    dec = codec.Decoder(cs, **kw)
    dec.set_timing(False)
    return dec


class Upload:
    """ojphgpu_decoder_upload_frame with the buffers kept alive: Decoder.upload synchronises the device and would hide an
    upload that lands under a block launch"""

    def __init__(self, dec):
        from openjph_amd import capi
        self.dec, self.lib, self.check, self.keep = dec, capi.lib(), capi.check, []

    def __call__(self, cs):
        buf = np.frombuffer(cs, dtype=np.uint8).copy()
        self.keep.append(buf)
        self.check(self.lib.ojphgpu_decoder_upload_frame(self.dec._h, 0, buf.ctypes.data, len(cs)), "decoder_upload_frame")


CONTAINERS = [(n, bits) for n in NAMES for bits in (32, 16, 8) if KINDS[n]["bit_depth"] <= bits]


@pytest.mark.parametrize("name,bits", CONTAINERS)
def test_a_released_run_is_pending_and_decodes_the_frame(name, bits):
    import torch
    r = ref(name)
    dec = released(r["a"])
    out = dec.run_device(dtype={32: torch.int32, 16: torch.int16, 8: torch.int8}[bits])
    assert dec.pending()
    assert np.array_equal(host(out), r["containers"][bits])
    if bits == 32:
        assert np.array_equal(host(out), r["want_a"])
    assert dec.failed_blocks() == 0
    assert not dec.pending()
    assert dec.fused_retries() == 0


def three_in_flight(r):
    import torch
    dec = released(r["a"], resilient=True)
    up = Upload(dec)
    outs = [torch.zeros(dec.shape, dtype=torch.int32, device="cuda") for _ in range(3)]
    dec.run_device(outs[0])                                # A (uploaded at creation)
    up(r["b"]); dec.run_device(outs[1])
    up(r["a"]); dec.run_device(outs[2])
    assert dec.pending()
    got = [host(o) for o in outs]
    assert np.array_equal(got[0], r["want_a"]), "run 0 (A)"
    assert np.array_equal(got[1], r["want_b"]), "run 1 (B)"
    assert np.array_equal(got[2], r["want_a"]), "run 2 (A)"
    assert dec.failed_blocks() == 0 and not dec.pending()
    up(r["b"]); dec.run_device(outs[0])
    assert dec.failed_blocks() == r["failed_b"]
    assert np.array_equal(host(outs[0]), r["want_b"])
    assert dec.fused_retries() == 0


@pytest.mark.parametrize("name", NAMES)
def test_three_runs_in_flight(name):
    three_in_flight(ref(name))


def test_the_caller_overwrites_the_image_behind_the_run():
    """only the top level writes the image, on the caller's stream: nothing of the run may land behind the fill"""
    r = ref("irv97_12b")
    dec = released(r["a"])
    for _ in range(3):
        out = dec.run_device()
        out.fill_(7)
        assert int((out != 7).sum().item()) == 0
    assert dec.failed_blocks() == 0


def test_a_caller_that_synchronises_only_its_own_stream():
    import torch
    r = ref("irv97_12b")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dec = released(r["a"])
        out = dec.run_device()
        assert dec.pending()
    s.synchronize()                                        # not the device
    assert np.array_equal(host(out), r["want_a"])
    with torch.cuda.stream(s):
        assert dec.failed_blocks() == 0
        del dec
    s.synchronize()


@pytest.mark.parametrize("name", NAMES)
def test_the_step_shape_twenty_times(name):
    """the benchmark's step at small size: a released encode and a released decode on one stream, both with timing off"""
    import torch
    from openjph_amd import codec
    from openjph_amd.plan import make_params
    r = ref(name)
    kw = KINDS[name]
    enc = codec.Encoder(make_params(W, H, NC, **kw))
    enc.set_timing(False)
    dec = released(r["a"])
    d_img = torch.from_numpy(synth_image(NC, H, W, kw["bit_depth"], seed=5).astype(np.int32)).cuda()
    d_out = torch.zeros_like(d_img)
    for k in range(20):
        enc.run_device(d_img)
        dec.run_device(d_out)
        if k % 5 == 4 or k == 19:
            assert dec.pending()
            assert np.array_equal(host(d_out), r["want_a"]), "step %d" % k
            d_out.zero_()
    assert dec.failed_blocks() == 0
    assert dec.fused_retries() == 0
    assert enc.finish() == r["a"]


def test_alternating_schedules_on_one_object():
    r = ref("irv97_12b")
    dec = released(r["a"], resilient=True)
    up = Upload(dec)
    a = dec.run_device()
    assert dec.pending()
    dec.set_timing(True)                                   # settles; the next run is joined, on the last run's arena
    assert not dec.pending()
    up(r["b"]); b = dec.run_device()
    assert not dec.pending()
    dec.set_timing(False)
    up(r["a"]); c = dec.run_device()
    assert dec.pending()
    up(r["b"]); d = dec.run_device()
    assert dec.pending()
    t = dec.timing()                                       # after a released run: returns, and settles it
    assert not dec.pending()
    assert np.isfinite(t["total_ms"]) and t["total_ms"] > 0
    for got, want in ((a, "want_a"), (b, "want_b"), (c, "want_a"), (d, "want_b")):
        assert np.array_equal(host(got), r[want])
    assert dec.failed_blocks() == r["failed_b"]


def test_paths_that_stay_joined_are_not_pending():
    from openjph_amd import codec
    from tests import cpu_pipeline as cp
    r = ref("irv97_12b")
    kw = KINDS["irv97_12b"]
    dec = codec.Decoder(r["a"])                            # per-launch timing is the default
    out = dec.run_device()
    assert not dec.pending() and np.array_equal(host(out), r["want_a"])
    batch = codec.Decoder([r["a"], r["a"]])
    batch.set_timing(False)
    out = batch.run_device()
    assert not batch.pending() and np.array_equal(host(out)[1], r["want_a"])
    img = synth_image(NC, H, W, 12, seed=5)
    tiled = bytes(cp.encode(img, **dict(kw, tile=(96, 80)))[0])
    part = codec.Decoder(tiled, tiles=(1, 2))
    part.set_timing(False)
    part.run_device()
    assert not part.pending() and part.failed_blocks() == 0
    region = codec.Decoder(r["a"], region=(32, 32, 96, 64))
    region.set_timing(False)
    region.run_device()
    assert not region.pending() and region.failed_blocks() == 0
    one = bytes(cp.encode(img, **dict(kw, num_decomps=1))[0])   # one decomposition: no levels below the top, no side stream
    flat = codec.Decoder(one)
    flat.set_timing(False)
    out = flat.run_device()
    assert not flat.pending() and np.array_equal(host(out), np.asarray(cp.decode(one)[0]).astype(np.int64))


def test_destroyed_with_runs_in_flight():
    import torch
    r = ref("irv97_12b")
    for n in (1, 2, 3):
        dec = released(r["a"])
        outs = [dec.run_device() for _ in range(n)]
        assert dec.pending()
        del dec                                            # no settling call: destroy drains the object's own stream itself
        gc.collect()
        torch.cuda.synchronize()
        assert all(np.array_equal(host(o), r["want_a"]) for o in outs)
    fresh = released(r["a"])
    out = fresh.run_device()
    assert np.array_equal(host(out), r["want_a"]) and fresh.failed_blocks() == 0


# ---- the switches that are read once per process or per object: child processes over the shared expected samples
CHILD = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
from openjph_amd import capi, codec
from tests import test_gpu_decoder_release as T
z = np.load(sys.argv[2])
r = dict(a=z["a"].tobytes(), b=z["b"].tobytes(), want_a=z["want_a"], want_b=z["want_b"], failed_b=int(z["failed_b"]))
mode = sys.argv[1]
if mode == "three":
    T.three_in_flight(r)
elif mode == "joined":
    dec = T.released(r["a"])
    out = dec.run_device()
    assert not dec.pending()
    assert np.array_equal(T.host(out), r["want_a"]) and dec.failed_blocks() == 0
elif mode == "repeat":
    dec = T.released(r["a"])
    out = dec.run_device()
    assert dec.pending()
    assert dec.failed_blocks() == 0                         # collects the released run: the repeat, joined, happens here
    assert not dec.pending()
    assert np.array_equal(T.host(out), r["want_a"])
    assert dec.fused_retries() == 1, dec.fused_retries()
    dec = T.released(r["a"])                                # a released run nobody collects: a later run says so
    dec.run_device(); torch.cuda.synchronize()
    try:
        dec.run_device()
        raise SystemExit("an uncollected repeat of a released run went unnoticed")
    except capi.OjphError as e:
        assert e.code == capi.E_UNCOLLECTED, e
    out = dec.run_device()
    assert dec.failed_blocks() == 0 and np.array_equal(T.host(out), r["want_a"])
print("OK")
''' % ROOT


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    r = ref("irv97_12b")
    path = str(tmp_path_factory.mktemp("dec_release") / "ref.npz")
    np.savez(path, a=np.frombuffer(r["a"], np.uint8), b=np.frombuffer(r["b"], np.uint8), want_a=r["want_a"], want_b=r["want_b"],
             failed_b=np.int64(r["failed_b"]))
    return path


def child(mode, shared, **env):
    r = subprocess.run([sys.executable, "-c", CHILD, mode, shared], env=dict(os.environ, **env), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and b"OK" in r.stdout, r.stderr[-3000:]


def test_three_runs_in_flight_on_one_arena(shared):
    child("three", shared, OJPHGPU_DEC_SETS="1")


@pytest.mark.parametrize("env", [dict(OJPHGPU_DEC_RELEASE="0"), dict(OJPHGPU_NO_OVERLAP="1")], ids=["release_0", "no_overlap"])
def test_switched_off_stays_joined(shared, env):
    child("joined", shared, **env)


def test_a_released_run_that_asks_for_the_repeat(shared):
    """OJPHGPU_FUSED_DBG=4 marks every fused run as if a wait had run out (tests/test_gpu_contention.py): collecting a released
    run settles it and repeats it joined through the separate launches; an uncollected one is reported by a later run"""
    child("repeat", shared, OJPHGPU_FUSED_DBG="4", OJPHGPU_DEC_FUSED="2")


@pytest.mark.parametrize("env", [dict(OJPHGPU_DEC_AHEAD_LEVELS="0"), dict(OJPHGPU_DEC_AHEAD_LEVELS="1"), dict(OJPHGPU_DEC_AHEAD_PRIO="high"),
                                 dict(OJPHGPU_DEC_AHEAD_PRIO="normal"), dict(OJPHGPU_DEC_AHEAD_PRIO="low")],
                         ids=["levels_0", "levels_1", "prio_high", "prio_normal", "prio_low"])
def test_the_two_switches_give_the_same_images(shared, env):
    child("three", shared, **env)
