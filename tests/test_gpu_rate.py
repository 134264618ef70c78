"""Encoding to a byte budget on the GPU (include/ojphgpu.h section 5b): the band statistics kernel against its numpy
restatement, and budgeted encodes against the certificate of the grid, the reference's recorded lengths and digests
(tests/golden/rate_sizes.json), a plain encode at the chosen step and the oracle's decode."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd import plan as planmod
from openjph_amd.plan import Plan, make_params
from tests import cpu_pipeline as cp
from tests import rate_cases as rc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "rate_sizes.json")))
NAMES = sorted(rc.CASES)
APPS = os.path.join(ROOT, "openjph_amd", "apps")


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def case_params(name, qstep=-1.0):
    c = rc.CASES[name]
    return make_params(c["w"], c["h"], c["nc"], **rc.case_kwargs(name, qstep))


def case_frame(name, plan):
    """the frame of a case in the layout the codec calls take (flat for the 4:2:0 case), int32"""
    img, _ = rc.case_image(name)
    return plan.pack_frame(img) if isinstance(img, list) else img


def containers(name):
    bd = rc.CASES[name]["bd"]
    return [dt for dt, bits in ((np.uint8, 8), (np.uint16, 16), (np.int32, 32)) if bd <= bits]


def check_info(name, info, budget):
    sizes = GOLD["cases"][name]["sizes"]
    j = info["grid_index"]
    assert info["bytes"] == sizes[j] <= budget
    assert info["bytes_finer"] == (sizes[j + 1] if j + 1 < rc.GRID else 0)
    assert j == rc.GRID - 1 or sizes[j + 1] > budget           # the certificate
    assert info["qstep"] == rc.grid_qstep(j) == planmod.rate_grid_qstep(j)
    assert 1 <= info["passes"] <= 17                           # the search's 16, and j* coded once more when the last trial was j* + 1


# ---------------------------------------------------------------------------------------------
# the statistics kernel
# ---------------------------------------------------------------------------------------------
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00800000, 0x2F800000, 0x2FC00000, 0x30000000, 0x303FFFFF,
                     0x3F800000, 0xBF800000, 0x3FBFFFFF, 0x3FC00000, 0xBFC00000, 0x43800000, 0x437FFFFF, 0x43C00000, 0x7F7FFFFF,
                     0x7F800000, 0xFF800000, 0x7FC00000, 0xFFFFFFFF, 0x7F800001], np.uint32)


def _planes(rng, shapes, pitch_of):
    """an arena of poison with one plane per (w, h): random bit patterns of every exponent, the special values sprinkled in"""
    descs = np.zeros(len(shapes), dtype=np.dtype(capi.StatsDesc))
    off = 0
    for i, (w, h) in enumerate(shapes):
        pitch = pitch_of(w)
        descs[i] = (off, pitch, w, h, i)
        off += pitch * h + 64
    arena = rng.integers(0, 2 ** 32, off + 64, dtype=np.uint64).astype(np.uint32)      # the padding is poison: it must not count
    views = []
    for i, (w, h) in enumerate(shapes):
        v = np.lib.stride_tricks.as_strided(arena[int(descs[i]["plane_off"]):], shape=(h, w), strides=(int(descs[i]["pitch"]) * 4, 4))
        kind = i % 3
        if kind == 1:                                            # like a real band: a handful of exponents, both signs
            v[:] = (rng.normal(0, 0.01, (h, w)).astype(np.float32)).view(np.uint32)
        elif kind == 2:
            v[:] = 0
        n = min(v.size, len(SPECIALS))
        at = rng.choice(v.size, n, replace=False)
        v[at // w, at % w] = SPECIALS[:n]
        views.append(v)
    return arena, descs, views


@pytest.mark.parametrize("pitch_of", [lambda w: (w + 63) // 64 * 64, lambda w: (w + 63) // 64 * 64 + 64, lambda w: w + 3, lambda w: w],
                         ids=["pitch64", "padded", "odd", "tight"])
def test_band_stats_matches_numpy(pitch_of):
    import torch
    from openjph_amd import codec
    rng = np.random.default_rng(17)
    shapes = [(1, 1), (1, 37), (40, 1), (63, 65), (64, 64), (1000, 257), (5, 3), (257, 16), (1024, 33)]
    arena, descs, views = _planes(rng, shapes, pitch_of)
    for i, v in enumerate(views):                                # as_strided views write through: the planes are in the arena
        assert v.shape == (shapes[i][1], shapes[i][0])
    d_arena = torch.from_numpy(arena.view(np.int32)).cuda()
    got = codec.band_stats(descs, d_arena, len(shapes))
    for i, v in enumerate(views):
        assert np.array_equal(got[i], rc.band_hist(np.ascontiguousarray(v))), shapes[i]
        assert int(got[i].sum()) == shapes[i][0] * shapes[i][1]
    # several planes into one slot, one plane alone in a launch, an empty launch
    one = descs.copy()
    one["slot"] = 0
    got = codec.band_stats(one, d_arena, 1)
    assert np.array_equal(got[0], sum(rc.band_hist(np.ascontiguousarray(v)).astype(np.uint64) for v in views).astype(np.uint32))
    got = codec.band_stats(descs[5:6], d_arena, len(shapes))
    assert np.array_equal(got[5], rc.band_hist(np.ascontiguousarray(views[5]))) and got.sum() == got[5].sum()
    assert codec.band_stats(descs[:0], d_arena, 2).sum() == 0


def test_band_stats_one_value_everywhere():
    """every sample in one bin: the packed 16-bit counters of a workgroup must be flushed before they overflow"""
    import torch
    from openjph_amd import codec
    w, h = 4096, 1500
    descs = np.zeros(1, dtype=np.dtype(capi.StatsDesc))
    descs[0] = (0, w, w, h, 0)
    for word, bin_ in ((0x3F800000, 63), (0x3FC00000, 64), (0, 0)):
        d_arena = torch.full((w * h + 64,), int(np.uint32(word).view(np.int32)), dtype=torch.int32, device="cuda")
        got = codec.band_stats(descs, d_arena, 1)
        assert got[0][bin_] == w * h and got.sum() == w * h, (hex(word), got[0].nonzero())


@pytest.mark.parametrize("name", ["A", "C", "E"])
def test_band_stats_of_a_real_transform(name):
    import torch
    from openjph_amd import codec
    pl = Plan(case_params(name))
    img, _ = rc.case_image(name)
    arena = cp.forward_stages(pl, img)
    want = rc.plan_hists(pl, arena)
    bands = [i for i in range(pl.num_bands) if pl.bands[i]["w"] and pl.bands[i]["h"]]
    descs = np.zeros(len(bands), dtype=np.dtype(capi.StatsDesc))
    for k, i in enumerate(bands):
        b = pl.bands[i]
        descs[k] = (int(b["plane_off"]), int(b["pitch"]), int(b["w"]), int(b["h"]), i)
    got = codec.band_stats(descs, torch.from_numpy(arena.view(np.int32)).cuda(), pl.num_bands)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------
# budgeted encodes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_budgeted_encode(name):
    from openjph_amd import codec
    params = case_params(name)
    pl = Plan(params)
    frame = case_frame(name, pl)
    inr, below, above = rc.budgets(name)
    for budget in inr + [above]:
        first = None
        for dt in containers(name):
            enc = codec.Encoder(params, max_bytes=budget)
            cs = enc.encode(frame.astype(dt))
            info = enc.rate_info()
            print(name, budget, np.dtype(dt).name, info, enc.rate_timing())
            assert len(cs) <= budget and len(cs) == info["bytes"]
            check_info(name, info, budget)
            if first is None:
                first = cs
                gold = GOLD["cases"][name]["budgets"][str(budget)]
                assert info["grid_index"] == gold["j"]
                assert sha(cs) == gold["sha256"]
                plain = codec.Encoder(case_params(name, planmod.rate_grid_qstep(info["grid_index"]))).encode(frame)
                assert cs == plain
                if gold["sha256_finer"] is not None:
                    finer = codec.Encoder(case_params(name, planmod.rate_grid_qstep(info["grid_index"] + 1))).encode(frame)
                    assert sha(finer) == gold["sha256_finer"] and len(finer) == info["bytes_finer"] > budget
                dec = codec.Decoder(cs)
                got = dec.decode()
                want, _ = cp.decode(cs)
                if isinstance(want, list):
                    assert all(np.array_equal(a, b) for a, b in zip(dec.plan.unpack_frame(got), want))
                else:
                    assert np.array_equal(got, want)
            else:
                assert cs == first
    enc = codec.Encoder(params, max_bytes=below)
    with pytest.raises(capi.OjphError) as e:
        enc.encode(frame)
    assert e.value.code == capi.E_BUDGET
    enc.set_budget(inr[1])                                         # ... and the encoder codes the next frame
    cs = enc.encode(frame)
    assert sha(cs) == GOLD["cases"][name]["budgets"][str(inr[1])]["sha256"]


def test_one_encoder_three_frames_three_budgets_then_none():
    from openjph_amd import codec
    from tests.synth import synth_image
    name = "A"
    c = rc.CASES[name]
    params = case_params(name, 0.003)
    enc = codec.Encoder(params)
    plain = []
    for k, seed in enumerate((11, 12, 13)):
        img = synth_image(c["nc"], c["h"], c["w"], c["bd"], seed=seed)
        plain.append(enc.encode(img))
    for k, (seed, budget) in enumerate(((11, 37440), (12, 150000), (13, 9000))):
        img = synth_image(c["nc"], c["h"], c["w"], c["bd"], seed=seed)
        enc.set_budget(budget)
        cs = enc.encode(img)
        info = enc.rate_info()
        assert len(cs) == info["bytes"] <= budget
        j = info["grid_index"]
        assert cs == codec.Encoder(case_params(name, planmod.rate_grid_qstep(j))).encode(img)
        finer = codec.Encoder(case_params(name, planmod.rate_grid_qstep(j + 1))).encode(img)
        assert len(finer) == info["bytes_finer"] > budget
        if seed == 11:
            assert sha(cs) == GOLD["cases"][name]["budgets"]["37440"]["sha256"]
    enc.set_budget(0)
    img = synth_image(c["nc"], c["h"], c["w"], c["bd"], seed=13)
    assert enc.encode(img) == plain[2]
    want, *_ = cp.encode(img, **rc.case_kwargs(name, 0.003))
    assert plain[2] == want


def test_refusals():
    from openjph_amd import codec
    ok = dict(bit_depth=8, reversible=False)
    for kw in (dict(bit_depth=8, reversible=True), dict(ok, qfactor=85), dict(ok, coc={1: dict(reversible=True)}),
               dict(ok, qfactors={0: ("Y", 80)}),
               dict(ok, atk={2: dict(steps=[-0.443506852, -0.882911075, 0.052980118, 1.586134342], K=1.230174105)}, wavelet=2),
               dict(ok, dfs={1: [1, 2, 3]}, coc={0: dict(dfs=1, num_decomps=3)}, num_decomps=3)):
        enc = codec.Encoder(make_params(128, 128, 3, **kw))
        with pytest.raises(capi.OjphError) as e:
            enc.set_budget(10000)
        assert e.value.code == capi.E_INVALID, kw
    tiled = make_params(256, 256, 1, tile=(128, 128), **ok)
    with pytest.raises(capi.OjphError) as e:
        codec.Encoder(tiled, tiles=(0, 2)).set_budget(10000)
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.OjphError) as e:
        codec.Encoder(tiled, frames=2).set_budget(10000)
    assert e.value.code == capi.E_INVALID
    enc = codec.Encoder(tiled, max_bytes=10000)                    # every tile: fine
    with pytest.raises(capi.OjphError):
        enc.rate_info()                                            # nothing coded yet
    with pytest.raises(capi.OjphError):
        enc.finish_tiles()                                         # a budget is a property of the whole codestream


CHILD = """
import sys, hashlib
sys.path.insert(0, %r)
from openjph_amd import codec
from openjph_amd.plan import Plan
from tests import rate_cases as rc
from tests.test_gpu_rate import case_params, case_frame
for name in ("A", "C"):
    params = case_params(name)
    enc = codec.Encoder(params, max_bytes=rc.budgets(name)[0][2])
    cs = enc.encode(case_frame(name, Plan(params)))
    assert enc.top_blocks() == 0
    print(name, hashlib.sha256(cs).hexdigest(), enc.rate_info()["grid_index"])
"""


def test_no_overlap_gives_the_same_bytes():
    env = dict(os.environ, OJPHGPU_NO_OVERLAP="1")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()
    lines = [ln.split() for ln in r.stdout.decode().splitlines() if ln[:2] in ("A ", "C ")]
    assert len(lines) == 2
    for name, digest, j in lines:
        gold = GOLD["cases"][name]["budgets"][str(rc.budgets(name)[0][2])]
        assert digest == gold["sha256"] and int(j) == gold["j"]


def test_survey_c3_at_the_bench_budgets():
    """the 8K frame of tools/rate_bench.py, device resident in 16-bit containers, against the reference's digests"""
    import torch
    from openjph_amd import codec
    from tests import synth
    img = synth.survey_c3()
    d_img = torch.from_numpy(img.astype(np.uint16).view(np.int16)).cuda()
    enc = codec.Encoder(make_params(7680, 4320, 3, bit_depth=12, reversible=False, qstep=0.001))
    assert len(GOLD["survey_c3"]) == len(rc.SURVEY_BPS)
    for key, gold in GOLD["survey_c3"].items():
        budget = int(key)
        assert budget == int(img.size * gold["bps"])
        enc.set_budget(budget)
        enc.run_device(d_img)
        cs = enc.finish()
        info = enc.rate_info()
        print("survey_c3", budget, info, enc.rate_timing())
        assert info["grid_index"] == gold["j"] and info["bytes"] == gold["bytes"] == len(cs) <= budget
        assert info["bytes_finer"] == gold["bytes_finer"] > budget
        assert sha(cs) == gold["sha256"]
        assert info["passes"] <= 17
    enc.set_budget(0)
    j = GOLD["survey_c3"][str(int(img.size * 0.73))]["j"]
    finer = codec.Encoder(make_params(7680, 4320, 3, bit_depth=12, reversible=False, qstep=planmod.rate_grid_qstep(j + 1)))
    finer.run_device(d_img)
    assert sha(finer.finish()) == GOLD["survey_c3"][str(int(img.size * 0.73))]["sha256_finer"]


# ---------------------------------------------------------------------------------------------
# the facade and the command-line tool
# ---------------------------------------------------------------------------------------------
def run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)


def test_facade_byte_budget(tmp_path):
    name = "A"
    c = rc.CASES[name]
    img, _ = rc.case_image(name)
    src = tmp_path / "in.i32"
    img.astype("<i4").tofile(src)
    prog = os.path.join(APPS, "facade_byte_budget")
    inr, below, above = rc.budgets(name)
    for budget in (inr[1], inr[2]):
        out = tmp_path / ("out%d.j2c" % budget)
        r = run([prog, str(src), str(c["w"]), str(c["h"]), str(c["nc"]), str(c["bd"]), "4", "1", str(budget), str(out)])
        assert r.returncode == 0, r.stdout
        gold = GOLD["cases"][name]["budgets"][str(budget)]
        assert sha(open(out, "rb").read()) == gold["sha256"]
        assert r.stdout.decode().split()[:2] == ["j", str(gold["j"])]
    out = tmp_path / "none.j2c"
    r = run([prog, str(src), str(c["w"]), str(c["h"]), str(c["nc"]), str(c["bd"]), "4", "1", str(below), str(out)])
    assert r.returncode == 3, r.stdout
    assert not os.path.exists(out) or os.path.getsize(out) == 0
    r = run([prog, str(src), str(c["w"]), str(c["h"]), str(c["nc"]), str(c["bd"]), "4", "1", str(inr[1]), str(out), "reversible"])
    assert r.returncode == 4, r.stdout


def test_cli_max_bytes(tmp_path):
    from openjph_amd import codec
    from tests.synth import synth_image
    img = synth_image(3, 120, 160, 12, seed=5)
    src = tmp_path / "in.yuv"
    img.astype("<u2").tofile(src)
    compress = os.path.join(APPS, "ojph_compress")
    common = ["-i", str(src), "-dims", "{160,120}", "-num_comps", "3", "-signed", "false", "-bit_depth", "12", "-downsamp", "{1,1}"]
    budget = 20000
    j2c = tmp_path / "out.j2c"
    r = run([compress, "-o", str(j2c), "-max_bytes", str(budget)] + common)
    assert r.returncode == 0, r.stdout
    enc = codec.Encoder(make_params(160, 120, 3, bit_depth=12, reversible=False), max_bytes=budget)
    want = enc.encode(img)
    info = enc.rate_info()
    got = open(j2c, "rb").read()
    assert got == want and len(got) <= budget
    assert ("grid index %d)" % info["grid_index"]) in r.stdout.decode() and ("%d bytes" % len(got)) in r.stdout.decode()
    assert got == codec.encode(img, bit_depth=12, reversible=False, qstep=planmod.rate_grid_qstep(info["grid_index"]))
    for extra in (["-qstep", "0.01"], ["-qfactor", "80"], ["-reversible", "true"]):
        bad = tmp_path / "bad.j2c"
        r = run([compress, "-o", str(bad), "-max_bytes", str(budget)] + common + extra)
        assert r.returncode != 0 and b"-max_bytes" in r.stdout, (extra, r.stdout)
    r = run([compress, "-o", str(tmp_path / "small.j2c"), "-max_bytes", "50"] + common)
    assert r.returncode != 0 and b"byte budget" in r.stdout, r.stdout
