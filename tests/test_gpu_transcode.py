"""The transcoder on the GPU (include/ojphgpu.h section 5d): codec.transcode / codec.Transcoder against the oracle statement of
the contract (tests/transcode_cases.py cpu_transcode), the fixture made from the reference (tests/golden/transcode.json) and,
for the identity targets, the direct encode of the original image."""
import hashlib
import json
import os

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd import plan as planmod
from openjph_amd.plan import parse_codestream
from tests import cpu_pipeline as cp
from tests import rate_cases as rc
from tests import transcode_cases as tc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "transcode.json")))
IDS = [tc.case_id(n, r) for n, r in tc.CASES]
_sources = {}


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def gpu_encode(name, kw):
    from openjph_amd import codec
    img, _ = rc.case_image(name)
    return codec.Encoder(tc.case_params(name, kw)).encode(img)


def source(name, rev, index=tc.SRC_INDEX):
    """(codestream coded on the device -- the reference's bytes --, the planes the oracle's block decoder leaves of it), once"""
    key = (name, rev, index)
    if key not in _sources:
        cs = gpu_encode(name, tc.src_kwargs(name, rev, index))
        if index == tc.SRC_INDEX:
            g = GOLD["cases"][tc.case_id(name, rev)]["source"]
            assert (sha(cs), len(cs)) == (g["sha256"], g["len"])
        _sources[key] = (cs, tc.cpu_source_planes(cs)[1])
    return _sources[key]


def raises_code(code, fn):
    with pytest.raises(capi.OjphError) as ei:
        fn()
    assert ei.value.code == code, ei.value


# ---------------------------------------------------------------------------------------------
# 1. every case and target
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rev,target", [(n, r, t) for n, r in tc.CASES for t in tc.targets(r)],
                         ids=["%s-%s" % (tc.case_id(n, r), t) for n, r in tc.CASES for t in tc.targets(r)])
def test_transcode_is_cpu_transcode(name, rev, target):
    from openjph_amd import codec
    cs, arena = source(name, rev)
    kw = tc.out_kwargs(name, rev, target)
    got = codec.transcode(cs, **tc.transcode_kwargs(rev, target))
    want = tc.cpu_transcode_planes(arena, tc.case_params(name, kw))
    g = GOLD["cases"][tc.case_id(name, rev)]["targets"][target]
    print(target, len(got), len(want), g["len"])
    assert got == want
    assert (sha(got), len(got)) == (g["sha256"], g["len"])
    if tc.targets(rev)[target][2]:                           # the direct encode of the original image with the output parameters
        assert got == gpu_encode(name, kw)


# ---------------------------------------------------------------------------------------------
# 2. byte budgets
# ---------------------------------------------------------------------------------------------
def check_info(name, info, budget):
    """the certificate, with size(j) = len(T(cs, out at qstep(j))) as the fixture recorded it from cpu_transcode"""
    sizes = GOLD["cases"][tc.case_id(name, False)]["sizes"]
    j = info["grid_index"]
    assert info["bytes"] == sizes[j] <= budget
    assert info["bytes_finer"] == (sizes[j + 1] if j + 1 < rc.GRID else 0)
    assert j == rc.GRID - 1 or sizes[j + 1] > budget
    assert info["qstep"] == rc.grid_qstep(j) == planmod.rate_grid_qstep(j)
    assert 1 <= info["passes"] <= 17


@pytest.mark.parametrize("name", tc.IRV)
def test_transcode_to_a_budget(name):
    from openjph_amd import codec
    cs, arena = source(name, False)
    inr, below, above = rc.budgets(name)
    t = codec.Transcoder(cs, max_bytes=inr[0])
    for b in inr:
        t.set_budget(b)
        got = t.transcode(cs)
        info = t.rate_info()
        print(name, b, info, GOLD["cases"][tc.case_id(name, False)]["budgets"][str(b)])
        check_info(name, info, b)
        assert len(got) == info["bytes"]
        e = GOLD["cases"][tc.case_id(name, False)]["budgets"][str(b)]
        if info["grid_index"] == e["j"]:
            assert (info["bytes"], info["bytes_finer"]) == (e["bytes"], e["bytes_finer"])
        q = rc.grid_qstep(info["grid_index"])
        assert got == codec.transcode(cs, qstep=q)           # the fixed-step transcode at qstep(j*)
        assert got == tc.cpu_transcode_planes(arena, tc.case_params(name, tc.out_kwargs(name, False, "frac", q)))
    t.set_budget(below)
    raises_code(capi.E_BUDGET, lambda: t.transcode(cs))
    t.set_budget(above)                                      # the object is still usable
    got = t.transcode(cs)
    info = t.rate_info()
    check_info(name, info, above)
    assert info["grid_index"] == rc.GRID - 1 and len(got) == info["bytes"]


# ---------------------------------------------------------------------------------------------
# 3. one object, source after source
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.IRV)
def test_reuse_leaves_no_stale_plane(name):
    from openjph_amd import codec
    first, a_first = source(name, False)
    sparse, a_sparse = source(name, False, 0)                # step 0.5: most blocks are not coded
    coded = parse_codestream(first).coded_blocks()["len1"] > 0
    assert int((coded & ~(parse_codestream(sparse).coded_blocks()["len1"] > 0)).sum()) > coded.sum() // 2
    kw = tc.out_kwargs(name, False, "blk32")
    want = lambda arena: tc.cpu_transcode_planes(arena, tc.case_params(name, kw))
    t = codec.Transcoder(first, **tc.transcode_kwargs(False, "blk32"))
    assert t.transcode(first) == want(a_first)
    assert t.transcode(sparse) == want(a_sparse)
    assert t.transcode(first) == want(a_first)
    other = source("B" if name != "B" else "A", False)[0]    # another geometry: refused, and the object goes on
    raises_code(capi.E_INVALID, lambda: t.transcode(other))
    assert t.transcode(sparse) == want(a_sparse)
    assert t.failed_blocks == 0


# ---------------------------------------------------------------------------------------------
# 4. sources with SigProp / MagRef passes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "C"])
def test_source_with_refinement_passes(name):
    from openjph_amd import codec
    img, size = rc.case_image(name)
    cs0, plan, _, data, coded = cp.encode(img, **tc.src_kwargs(name, False))
    data2, coded2 = cp.add_refinement(data, coded, np.random.default_rng(23))
    cs = plan.t2_write(data2, coded2)
    src = parse_codestream(cs)
    assert int((src.coded_blocks()["num_passes"] > 1).sum()) > 10 and len(cs) > len(cs0)
    kw = tc.out_kwargs(name, False, "blk32")
    # (the passes refine below the source's step: at that step the planes quantise back to the cleanup pass's indices, so the
    # bytes are those of the plain source -- what is tested is the way there, the refinement launches of the block decoder)
    want = tc.cpu_transcode(cs, tc.case_params(name, kw))
    assert not np.array_equal(tc.cpu_source_planes(cs)[1], tc.cpu_source_planes(cs0)[1])
    assert codec.transcode(cs, **tc.transcode_kwargs(False, "blk32")) == want
    finer = tc.out_kwargs(name, False, "finer")              # ... and at a finer step they count
    want = tc.cpu_transcode(cs, tc.case_params(name, finer))
    assert want != tc.cpu_transcode(cs0, tc.case_params(name, finer))
    assert codec.transcode(cs, **tc.transcode_kwargs(False, "finer")) == want


# ---------------------------------------------------------------------------------------------
# 5. a damaged source
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "C"])
def test_damaged_source(name):
    from openjph_amd import codec
    cs, _ = source(name, False)
    sot = cs.rfind(b"\xff\x90\x00\x0a")
    cut = cs[:sot + (len(cs) - sot) // 2]                    # the middle of the last tile-part
    kw = tc.out_kwargs(name, False, "blk32")
    src = parse_codestream(cut, resilient=True)
    failed = tc.cpu_failed_blocks(src, cut)
    want = tc.cpu_transcode(cut, tc.case_params(name, kw), resilient=True)
    t = codec.Transcoder(cut, resilient=True, **tc.transcode_kwargs(False, "blk32"))
    got = t.transcode(cut)
    print(name, "failed blocks: oracle", failed, "device", t.failed_blocks)
    assert got == want and t.failed_blocks == failed
    assert got != tc.cpu_transcode_planes(source(name, False)[1], tc.case_params(name, kw))
    # not resilient: what codec.decode makes of the file
    try:
        codec.decode(cut)
        code = None
    except capi.OjphError as e:
        code = e.code
    assert code in (capi.E_BLOCK, capi.E_CODESTREAM)
    raises_code(code, lambda: codec.transcode(cut, **tc.transcode_kwargs(False, "blk32")))


# ---------------------------------------------------------------------------------------------
# 6. what the object refuses
# ---------------------------------------------------------------------------------------------
def test_object_refusals():
    import ctypes as C
    import torch
    from openjph_amd import codec
    cs, arena = source("B", False)
    t = codec.Transcoder(cs, block=(32, 32))                 # an irreversible output with neither a step nor a budget
    raises_code(capi.E_INVALID, lambda: t.submit(cs))
    raises_code(capi.E_INVALID, t.finish)
    t.set_budget(20000)                                      # ... becomes usable with a budget
    got = t.transcode(cs)
    assert len(got) <= 20000 and got == codec.transcode(cs, block=(32, 32), qstep=t.rate_info()["qstep"])
    t.set_budget(0)                                          # ... and is without a step again once the budget is off
    raises_code(capi.E_INVALID, lambda: t.submit(cs))
    # budget 0 after a budget was on: the plan's own step again, as an encoder does it
    q = rc.grid_qstep(tc.SRC_INDEX - 5)
    t = codec.Transcoder(cs, qstep=q, max_bytes=20000)
    assert len(t.transcode(cs)) <= 20000
    t.set_budget(0)
    assert t.transcode(cs) == tc.cpu_transcode_planes(arena, tc.case_params("B", tc.out_kwargs("B", False, "frac")))
    raises_code(capi.E_INVALID, t.rate_info)
    # a budget on a reversible output
    rev = source("D", True)[0]
    raises_code(capi.E_INVALID, lambda: codec.Transcoder(rev, max_bytes=20000))
    t = codec.Transcoder(rev)
    raises_code(capi.E_INVALID, lambda: t.set_budget(20000))
    assert t.transcode(rev) == rev                           # (nothing changed: the source again)
    # plans that do not share an arena
    a, b = parse_codestream(cs), parse_codestream(source("A", False)[0])
    out = planmod.transcode_plan(b, planmod.transcode_params(b, qstep=0.01))
    h = C.c_void_p()
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    assert capi.lib().ojphgpu_transcoder_create(a.handle, out.handle, 0, stream, C.byref(h)) == capi.E_INVALID and not h.value
    assert capi.lib().ojphgpu_transcoder_create(b.handle, b.handle, 0, stream, C.byref(h)) == capi.E_INVALID and not h.value


# ---------------------------------------------------------------------------------------------
# 7. the decoder and the encoder beside a transcoder
# ---------------------------------------------------------------------------------------------
def test_decoder_and_encoder_are_undisturbed():
    from openjph_amd import codec
    cs, _ = source("A", False)
    img, _ = rc.case_image("A")
    t = codec.Transcoder(cs, max_bytes=rc.budgets("A")[0][1], block=(32, 32))
    out = t.transcode(cs)
    tm = t.timing()
    assert tm["decode_ms"] > 0 and tm["stats_ms"] > 0 and tm["code_ms"] > 0 and tm["final_ms"] > 0
    dec = codec.Decoder(cs)
    want, _ = cp.decode(cs)
    assert np.array_equal(dec.decode(), want)
    assert t.transcode(cs) == out
    assert np.array_equal(dec.decode(), want)
    enc = codec.Encoder(tc.case_params("A", tc.src_kwargs("A", False)))
    assert enc.encode(img) == cs
    assert t.transcode(cs) == out
    assert enc.encode(img) == cs
    assert np.array_equal(codec.decode(out), cp.decode(out)[0])


# ---------------------------------------------------------------------------------------------
# 8. a one-launch block decoder run whose wait ran out is repeated before a block is coded
# ---------------------------------------------------------------------------------------------
REPEAT_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, %r)
from openjph_amd import codec
from tests import rate_cases as rc
from tests import transcode_cases as tc
name = "A"
cs = codec.Encoder(tc.case_params(name, tc.src_kwargs(name, False))).encode(rc.case_image(name)[0])
arena = tc.cpu_source_planes(cs)[1]
dec = codec.Decoder(cs)                                     # the switch is on for this codestream: a decoder repeats its run
dec.run_device()
assert dec.failed_blocks() == 0 and dec.fused_retries() == 1, dec.fused_retries()
kw = tc.out_kwargs(name, False, "blk32")
t = codec.Transcoder(cs, **tc.transcode_kwargs(False, "blk32"))
for run in range(2):                                        # (the first run starts from an arena of zeros: without the repeat the planes would be short)
    assert t.transcode(cs) == tc.cpu_transcode_planes(arena, tc.case_params(name, kw)), run
    assert t.failed_blocks == 0
budget = rc.budgets(name)[0][1]
t = codec.Transcoder(cs, max_bytes=budget)                  # ... and with a budget the search sees the repeated planes
got = t.transcode(cs)
info = t.rate_info()
sizes = json.load(open(os.path.join(%r, "tests", "golden", "transcode.json")))["cases"]["Airv"]["sizes"]
j = info["grid_index"]
assert len(got) == info["bytes"] == sizes[j] <= budget < sizes[j + 1] == info["bytes_finer"], info
assert got == tc.cpu_transcode_planes(arena, tc.case_params(name, tc.out_kwargs(name, False, "frac", rc.grid_qstep(j))))
print("OK")
''' % (os.path.dirname(HERE), os.path.dirname(HERE))


def test_a_wait_that_runs_out_is_repeated_before_coding():
    """OJPHGPU_FUSED_DBG=4 makes one worker wavefront of every one-launch block decoder run behave as if its wait for the
    chains had run out (tests/test_gpu_contention.py): the transcoder's finish repeats the run through the separate launches
    when it collects the verdicts, takes the statistics again, and only then codes -- the bytes are cpu_transcode's"""
    import subprocess
    import sys
    env = dict(os.environ, OJPHGPU_FUSED_DBG="4", OJPHGPU_DEC_FUSED="2")
    r = subprocess.run([sys.executable, "-c", REPEAT_SCRIPT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and b"OK" in r.stdout, r.stderr[-3000:]
