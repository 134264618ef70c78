"""A reversible frame under a byte cap on the GPU (include/ojphgpu.h section 5f): the block coder's instantiations for
blocks that drop bit-planes against the oracle's block coder, the integer band statistics against numpy, and the encoder at
fixed levels and under caps against the CPU statement (tests/trunc_cases.py), the recorded digests of the reference's decode
(tests/golden/trunc.json) and the product's own decoders."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd.plan import Plan, make_params
from oracle import oraclebind as ob
from tests import trunc_cases as tc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "trunc.json")))["cases"]


# ---------------------------------------------------------------------------------------------
# the block coder
# ---------------------------------------------------------------------------------------------
SHAPES = [(64, 64), (32, 32), (60, 37), (4, 4), (1, 1), (128, 32), (256, 16), (1024, 4)]


def _block_values(rng, w, h, K, kind, t):
    """int32 coefficients of magnitudes below 2^K; kind: random (every bit length), below (all < 2^t), single (one = 2^t)"""
    if kind == "below":
        mag = rng.integers(0, 1 << t, (h, w), dtype=np.int64)
    elif kind == "single":
        mag = rng.integers(0, 1 << t, (h, w), dtype=np.int64)
        mag[h // 2, w // 3] = 1 << t
    else:
        bits = rng.integers(0, K + 1, (h, w))                   # a bit length per sample, then a value of that length
        mag = rng.integers(0, 1 << 62, (h, w), dtype=np.int64) & ((np.int64(1) << bits) - 1)
        mag[rng.random((h, w)) < 0.3] = 0
        mag[0, 0] = (1 << K) - 1
    sign = rng.integers(0, 2, (h, w)) * 2 - 1
    return (mag * sign).astype(np.int32)


class Blocks:
    """blocks in one arena (rows of odd pitch, poison between the planes), their descriptors and the oracle's bytes"""

    def __init__(self, specs, seed):
        from openjph_amd import codec
        from openjph_amd.csrc_consts import block_scratch_bytes
        rng = np.random.default_rng(seed)
        self.descs = np.zeros(len(specs), codec.cb_desc_dtype)
        planes, off = [], 0
        for i, (w, h, K, t, kind) in enumerate(specs):
            pitch = w + 3
            v = _block_values(rng, w, h, K, kind, 0 if t is None else t)
            planes.append((off, pitch, v))
            d = self.descs[i]
            d["coef_off"], d["pitch"], d["w"], d["h"], d["K_max"] = off, pitch, w, h, K
            d["reversible"] = 1 if t is None else 1 | 8         # t None: a plain block (the flag clear, missing_msbs not read)
            d["missing_msbs"] = 0 if t is None else K - 1 - t
            d["num_passes"] = 1
            off += pitch * h + 5
        self.coef = rng.integers(-2 ** 31, 2 ** 31, off + 8, dtype=np.int64).astype(np.int32)
        self.want = []
        for (o, pitch, v), (w, h, K, t, kind) in zip(planes, specs):
            np.lib.stride_tricks.as_strided(self.coef[o:], shape=v.shape, strides=(pitch * 4, 4))[:] = v
            tt = 0 if t is None else t
            q, mx = ob.quant_rev(np.ascontiguousarray(v), K)
            self.want.append(ob.ht_encode(q, w, h, w, K - 1 - tt) if mx >= (1 << (31 - K + tt)) else b"")
        self.out_cap = sum((block_scratch_bytes(w, h, K) + 3) & ~3 for (w, h, K, t, kind) in specs) + 64

    def run(self, widths=None):
        import torch
        from openjph_amd import codec
        return codec.ht_encode(self.descs, torch.from_numpy(self.coef).cuda(), 0, self.out_cap, widths=widths, scratch_caps_as_given=False)

    def problems(self, got):
        res, out, status = got[0], got[1], got[2]
        bad = [] if status == 0 else ["status %d" % status]
        for i, want in enumerate(self.want):
            o, n = int(res[i, 0]), int(res[i, 1])
            if (o, n) == (0xFFFFFFFF, 0xFFFFFFFF):
                bad.append("block %d: result never written" % i)
            elif n != len(want) or out[o:o + n].tobytes() != want:
                bad.append("block %d (%dx%d K %d missing_msbs %d): %d bytes, the oracle has %d%s" % (
                    i, self.descs[i]["w"], self.descs[i]["h"], self.descs[i]["K_max"], self.descs[i]["missing_msbs"], n, len(want),
                    "" if n != len(want) else ", bytes differ"))
        return bad


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_block_coder_drops_planes(shape):
    """every shape class (16 x 4 pairs, 8 x 8, ragged, tiny, 32 x 2, the wide kernel) at K_max 10 and 26, t = 1, 3, K_max - 1,
    with a block all below 2^t (not coded) and one with a single sample of 2^t, several workgroups per launch"""
    w, h = shape
    specs = []
    for K in (10, 26):
        for t in (1, 3, K - 1):
            specs += [(w, h, K, t, "random"), (w, h, K, t, "below"), (w, h, K, t, "single"), (w, h, K, t, "random")]
    B = Blocks(specs, seed=w * 131 + h)
    assert any(len(x) == 0 for x in B.want) and sum(len(x) > 0 for x in B.want) >= 2 * len(specs) // 3
    bad = B.problems(B.run())
    assert not bad, "\n".join(bad[:12])


def test_block_coder_mixed_launch():
    """flagged and plain blocks of every layout in one launch: each instantiation codes its own and skips the others'"""
    from openjph_amd import codec
    specs = []
    for (w, h) in ((64, 64), (20, 9), (128, 32), (256, 16)):
        for t in (None, 2, None, 5):
            specs.append((w, h, 12, t, "random"))
    B = Blocks(specs, seed=99)
    kinds = codec.ht_encode_kinds(B.descs)
    assert kinds & 128 and kinds & 4 and kinds & 3 == 3
    launches = codec.ht_encode_launches(len(specs), kinds)
    assert [(l["wide"], l["flag"], l["logp"]) for l in launches] == [(0, 1, 4), (1, 0, 0), (0, 3, 4), (1, 2, 0)]
    bad = B.problems(B.run())
    assert not bad, "\n".join(bad[:12])
    # without bit 7 nobody owns the flagged blocks: their results stay as the caller left them, the plain ones are coded
    got = B.run(widths=kinds & ~128)
    for i, (w, h, K, t, kind) in enumerate(specs):
        o, n = int(got[0][i, 0]), int(got[0][i, 1])
        if t is None:
            assert n == len(B.want[i]) and got[1][o:o + n].tobytes() == B.want[i]
        else:
            assert (o, n) == (0xFFFFFFFF, 0xFFFFFFFF)


def test_block_coder_launch_table():
    from openjph_amd import codec
    L = lambda n, w: [(l["wide"], l["flag"], l["logp"]) for l in codec.ht_encode_launches(n, w)]
    assert L(9, 1 | 128 | 16 | 64) == [(0, 3, 3)]
    assert L(9, 1 | 128 | 64) == [(0, 3, 4)]
    assert L(9, 2 | 128 | 64 | 16) == [(0, 3, 5)]
    assert L(9, 2 | 128 | 16) == [(1, 0, 0), (1, 2, 0)]          # (the plain wide kernel serves both wavelets: launched with bit 1)
    assert L(9, 3 | 4 | 8 | 32 | 128) == [(0, 1, 4), (0, 0, 4), (1, 0, 0), (1, 1, 0), (0, 3, 4), (1, 2, 0)]
    assert L(9, 3 | 32) == [(0, 1, 4), (0, 0, 4), (1, 0, 0), (1, 1, 0)]      # a caller that does not know: as before


def test_block_coder_refuses_ill_formed_descriptors():
    """validated on the host, where the kinds are taken: nothing is launched"""
    from openjph_amd import codec
    good = Blocks([(16, 16, 10, 3, "random")], seed=1)
    for field, value in (("missing_msbs", 10), ("missing_msbs", 200), ("reversible", 1 | 4 | 8), ("reversible", 8)):
        d = good.descs.copy()
        d[field] = value
        with pytest.raises(capi.OjphError) as e:
            codec.ht_encode_kinds(d)
        assert e.value.code == capi.E_INVALID
        bad = Blocks([(16, 16, 10, 3, "random")], seed=1)
        bad.descs = d
        with pytest.raises(capi.OjphError) as e:
            bad.run()                                           # (widths=None: the launch asks for the kinds first)
        assert e.value.code == capi.E_INVALID


# ---------------------------------------------------------------------------------------------
# the integer statistics
# ---------------------------------------------------------------------------------------------
SPECIAL = np.array([0, 1, -1, 2, -2, 3, 255, 256, -256, 2 ** 31 - 1, -2 ** 31, -2 ** 31 + 1, 2 ** 30, -2 ** 30, 2 ** 30 - 1], np.int64)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
def test_band_stats_int(aligned):
    import torch
    from openjph_amd import codec
    rng = np.random.default_rng(3 if aligned else 4)
    shapes = [(1, 9), (3, 5), (67, 33), (4097, 3), (64, 64), (130, 1)]
    descs = np.zeros(len(shapes), np.dtype(capi.StatsDesc))
    off = 0 if aligned else 1
    for i, (w, h) in enumerate(shapes):
        pitch = (w + 3) // 4 * 4 + 4 if aligned else w + 1 + (w + 1) % 2        # odd pitches
        descs[i] = (off, pitch, w, h, min(i, 4))                                 # the last two share a slot
        off += pitch * h + (8 if aligned else 7)
    arena = rng.integers(-2 ** 31, 2 ** 31, off + 8, dtype=np.int64).astype(np.int32)      # the padding is poison: it must not count
    want = np.zeros((5, 80), np.uint32)
    for i, (w, h) in enumerate(shapes):
        v = np.lib.stride_tricks.as_strided(arena[int(descs[i]["plane_off"]):], shape=(h, w), strides=(int(descs[i]["pitch"]) * 4, 4))
        bits = rng.integers(0, 33, (h, w))
        val = rng.integers(0, 2 ** 40, (h, w), dtype=np.int64) & ((np.int64(1) << bits) - 1)
        v[:] = np.where(rng.integers(0, 2, (h, w)) == 1, -val, val).astype(np.int64).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32)
        for p, s in zip(rng.permutation(w * h)[:len(SPECIAL)], SPECIAL):         # the special values, sprinkled in
            v[int(p) // w, int(p) % w] = np.int32(s)
        want[int(descs[i]["slot"])] += tc.bit_length_hist(v)
    assert want[:, 33:].sum() == 0 and want[:, 32].sum() >= 1 and want[:, 0].sum() >= 1
    d_arena = torch.from_numpy(arena).cuda()
    assert (codec.band_stats(descs, d_arena, 5, integer=True) == want).all()
    # ... and the entry point itself with guard words around the histogram
    G, n = 64, 5 * capi.STATS_BINS
    buf = torch.full((n + 2 * G,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda")
    buf[G:G + n] = 0
    d_descs = codec.to_device(descs, 0)
    capi.check(capi.lib().ojphgpu_band_stats_int(codec._stream_ptr(torch, 0), ctypes.c_void_p(d_descs.data_ptr()), len(descs), int(descs["w"].max()), int(descs["h"].max()),
                                                 ctypes.c_void_p(d_arena.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 4 * G)), "band_stats_int")
    torch.cuda.synchronize()
    out = buf.cpu().numpy().view(np.uint32)
    assert (out[:G] == 0xA5A5A5A5).all() and (out[G + n:] == 0xA5A5A5A5).all()
    hist = out[G:G + n].reshape(5, capi.STATS_BINS)
    assert (hist == want).all(), np.argwhere(hist != want)[:8]


# ---------------------------------------------------------------------------------------------
# the encoder
# ---------------------------------------------------------------------------------------------
def _encoder(name, **kw):
    from openjph_amd import codec
    c = tc.CASES[name]
    return codec.Encoder(make_params(c["w"], c["h"], c["nc"], **c["kw"]), **kw)


def _decoded_sha(cs):
    from openjph_amd import codec
    return tc.sha(np.ascontiguousarray(codec.decode(cs), dtype=np.int32).tobytes())


@pytest.mark.parametrize("name", tc.CODED)
def test_encoder_at_fixed_levels(name):
    from openjph_amd import codec
    plan, img, _ = tc.case_state(name)
    g = GOLD[name]
    plain = _encoder(name).encode(img)
    enc = _encoder(name)
    for j in tc.fixed_levels(plan) + [0]:
        enc.set_trunc_level(j)
        cs = enc.encode(img)
        assert len(cs) == g["sizes"][j] and tc.sha(cs) == g["codestream_sha256"][j], (name, j)
        assert cs == tc.cpu_codestream(name, j)
        assert _decoded_sha(cs) == g["decoded_sha256"][j], (name, j)         # the reference's planes
        info = enc.trunc_info()
        assert info == dict(level=j, passes=1, first_guess=j, max_dropped=int(plan.trunc_table(j).max()), lossless=int(j == 0),
                            bytes=len(cs), bytes_finer=0)
        if j == 0:
            assert cs == plain
    enc.set_trunc_level(None)                                    # the mode off: the plain encoder again
    assert enc.encode(img) == plain
    assert codec.encode(img, truncate_level=1, **tc.CASES[name]["kw"]) == tc.cpu_codestream(name, 1)


@pytest.mark.parametrize("form", [{"OJPHGPU_DEC_FUSED": "0"}, {"OJPHGPU_DEC_FUSED": "2"}], ids=["separate-launches", "fused-wherever-possible"])
def test_decoders_read_truncated_codestreams(form):
    """both launch forms of the block decoder (chosen per process) decode the cases to the reference's planes at every third
    distinct table and at the last level.  The codestreams are the CPU statement's: test_encoder_at_fixed_levels and
    test_encoder_under_a_cap show that the encoder writes those very bytes."""
    script = r'''
import sys, json, numpy as np
sys.path.insert(0, %r)
from openjph_amd import codec
from tests import trunc_cases as tc
gold = json.load(open(%r))["cases"]
for name in tc.CODED:
    plan = tc.case_state(name)[0]
    for j in tc.distinct_levels(plan)[::3] + [plan.trunc_levels - 1]:
        dec = codec.Decoder(tc.cpu_codestream(name, j))
        got = dec.decode()
        assert dec.failed_blocks() == 0
        assert tc.sha(np.ascontiguousarray(got, dtype=np.int32).tobytes()) == gold[name]["decoded_sha256"][j], (name, j)
print("OK")
''' % (ROOT, os.path.join(HERE, "golden", "trunc.json"))
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **form), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and b"OK" in r.stdout, r.stderr[-2000:]


@pytest.mark.parametrize("name", tc.CODED)
def test_encoder_under_a_cap(name):
    plan, img, _ = tc.case_state(name)
    sizes = GOLD[name]["sizes"]
    J = plan.trunc_levels
    plain = _encoder(name).encode(img)
    assert len(plain) == sizes[0]
    enc = _encoder(name)
    d = sorted(set(sizes), reverse=True)
    picks = [d[1], d[len(d) // 3], d[len(d) // 2], d[-2]]
    caps = sorted({c for s in picks for c in (s, s + 1, s - 1)} | {(d[2] + d[3]) // 2, d[-1]})
    for cap in caps:
        enc.set_truncation(cap)
        cs = enc.encode(img)
        info = enc.trunc_info()
        j = info["level"]
        assert len(cs) == info["bytes"] == sizes[j] <= cap and j > 0
        assert sizes[j - 1] > cap and info["bytes_finer"] == sizes[j - 1]      # the certificate, against the recorded sizes
        assert cs == tc.cpu_codestream(name, j)                                 # = the fixed-level encode of j* (test above)
        assert info["lossless"] == 0 and info["max_dropped"] == int(plan.trunc_table(j).max())
        assert 2 <= info["passes"] <= 2 + int(np.ceil(np.log2(J)))
    for cap in (sizes[0], sizes[0] + 1, 10 ** 9):                # the frame fits: lossless, the plain codestream, one pass
        enc.set_truncation(cap)
        assert enc.encode(img) == plain
        info = enc.trunc_info()
        assert (info["level"], info["lossless"], info["passes"], info["bytes"], info["bytes_finer"], info["max_dropped"]) == (0, 1, 1, sizes[0], 0, 0)
    enc.set_truncation(sizes[-1] - 1)                            # not even every band's top plane alone fits
    with pytest.raises(capi.OjphError) as e:
        enc.encode(img)
    assert e.value.code == capi.E_BUDGET
    enc.set_truncation(sizes[1])                                 # ... and the encoder stays usable
    assert enc.encode(img) == tc.cpu_codestream(name, 1)
    enc.set_truncation(0)
    assert enc.encode(img) == plain


def test_one_shot_helper():
    from openjph_amd import codec
    _, img, _ = tc.case_state("B")
    sizes = GOLD["B"]["sizes"]
    j = 20
    while sizes[j - 1] == sizes[j]:
        j += 1
    assert codec.encode(img, truncate_to=sizes[j], **tc.CASES["B"]["kw"]) == tc.cpu_codestream("B", j)


def test_refusals():
    """OJPHGPU_E_INVALID, the encoder as it was"""
    from openjph_amd import codec
    img = tc.case_image("A")

    def refused(f):
        with pytest.raises(capi.OjphError) as e:
            f()
        assert e.value.code == capi.E_INVALID

    P = lambda **kw: make_params(200, 136, 3, **dict(dict(bit_depth=8, num_decomps=3), **kw))
    for params in (P(reversible=False, qstep=0.01),                               # an irreversible component
                   P(reversible=True, coc={1: dict(reversible=False)}),
                   P(reversible=True, coc={2: dict(num_decomps=2)}),              # components that differ in decompositions
                   P(reversible=True, bit_depth=30),                              # the 64-bit sample path
                   P(reversible=True, wavelet=2, atk={2: dict(steps=[(1, 2, 2), (-1, 1, 1)])}),          # ATK
                   make_params(200, 136, 2, bit_depth=8, num_decomps=3, dfs={1: [1, 2, 3]}, coc={0: dict(dfs=1, num_decomps=3)})):   # DFS
        enc = codec.Encoder(params)
        refused(lambda: enc.set_truncation(10000))
        refused(lambda: enc.set_trunc_level(1))
    batch = codec.Encoder(P(), frames=2)
    refused(lambda: batch.set_truncation(10000))
    refused(lambda: batch.set_trunc_level(0))
    tiled = make_params(256, 192, 1, bit_depth=8, num_decomps=3, tile=(128, 128))
    part = codec.Encoder(tiled, tiles=(1, 2))
    refused(lambda: part.set_truncation(10000))
    enc = codec.Encoder(P())
    plain = enc.encode(img)
    refused(lambda: enc.set_trunc_level(Plan(P()).trunc_levels))                  # beyond the ladder
    refused(lambda: enc.set_budget(10000))                                        # section 5b stays closed to reversible plans
    refused(lambda: enc.set_quality(max_sse=1000))
    assert enc.encode(img) == plain
    enc.set_truncation(len(plain) // 2)
    refused(lambda: enc.set_budget(10000))
    refused(lambda: enc.set_quality(max_sse=1000))
    refused(enc.trunc_info)                                                       # nothing has been coded in the mode yet
    enc.run_device(__import__("torch").from_numpy(np.ascontiguousarray(img, dtype=np.int32)).cuda())
    refused(enc.finish_tiles)
    refused(enc.finish_tiles_device)
    cs = enc.finish()
    assert len(cs) <= len(plain) // 2 and enc.trunc_info()["level"] > 0


# ---------------------------------------------------------------------------------------------
# the facade and the command-line tool
# ---------------------------------------------------------------------------------------------
APPS = os.path.join(ROOT, "openjph_amd", "apps")


def run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)


def test_facade_truncation_budget(tmp_path):
    name = "A"
    c = tc.CASES[name]
    plan, img, _ = tc.case_state(name)
    sizes = GOLD[name]["sizes"]
    src = tmp_path / "in.i32"
    img.astype("<i4").tofile(src)
    prog = os.path.join(APPS, "facade_truncation_budget")
    args = [str(src), str(c["w"]), str(c["h"]), str(c["nc"]), str(c["bd"]), "5", "1"]
    for cap, j in ((sizes[0] + 5, 0), (sizes[11], 11), (sizes[10] - 1, 11)):
        out = tmp_path / ("out%d.j2c" % cap)
        r = run([prog] + args + [str(cap), str(out)])
        assert r.returncode == 0, r.stdout
        assert open(out, "rb").read() == tc.cpu_codestream(name, j)           # = the Python encoder's bytes (test_encoder_under_a_cap)
        assert r.stdout.decode().split()[:4] == ["level", str(j), "bytes", str(sizes[j])]
    out = tmp_path / "none.j2c"
    r = run([prog] + args + [str(sizes[-1] - 1), str(out)])
    assert r.returncode == 3, r.stdout
    assert not os.path.exists(out) or os.path.getsize(out) == 0
    r = run([prog] + args + [str(sizes[11]), str(out), "irreversible"])
    assert r.returncode == 4, r.stdout


def test_cli_truncate_to(tmp_path):
    from openjph_amd import codec
    from tests.synth import synth_image
    img = synth_image(3, 120, 160, 12, seed=5)
    src = tmp_path / "in.yuv"
    img.astype("<u2").tofile(src)
    compress = os.path.join(APPS, "ojph_compress")
    base = ["-i", str(src), "-dims", "{160,120}", "-num_comps", "3", "-signed", "false", "-bit_depth", "12", "-downsamp", "{1,1}"]
    common = base + ["-reversible", "true"]
    lossless = codec.encode(img, bit_depth=12, reversible=True)
    for cap in (len(lossless) * 2 // 3, len(lossless)):
        j2c = tmp_path / ("out%d.j2c" % cap)
        r = run([compress, "-o", str(j2c), "-truncate_to", str(cap)] + common)
        assert r.returncode == 0, r.stdout
        enc = codec.Encoder(make_params(160, 120, 3, bit_depth=12, reversible=True), truncate_to=cap)
        want = enc.encode(img)
        info = enc.trunc_info()
        got = open(j2c, "rb").read()
        assert got == want and len(got) <= cap and (cap < len(lossless)) == (info["level"] > 0)
        assert ("level %d" % info["level"]) in r.stdout.decode() and ("%d bytes" % len(got)) in r.stdout.decode()
    for args in (["-truncate_to", "20000", "-reversible", "false", "-qstep", "0.01"] + base, ["-truncate_to", "0"] + common):
        r = run([compress, "-o", str(tmp_path / "bad.j2c")] + args)
        assert r.returncode != 0 and b"-truncate_to" in r.stdout, (args, r.stdout)
    r = run([compress, "-o", str(tmp_path / "small.j2c"), "-truncate_to", "50"] + common)
    assert r.returncode != 0 and b"truncation budget" in r.stdout, r.stdout
