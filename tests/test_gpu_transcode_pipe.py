"""The transcode pipe on the GPU (include/ojphgpu.h section 6, ojphgpu_tc_pipe / pipeline.TranscoderPipe): sequences of the
small sources of tests/transcode_cases.py against codec.transcode of each source, the oracle statement of the contract
(tc.cpu_transcode*) and the fixture made from the reference (tests/golden/transcode.json)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd.plan import parse_codestream
from tests import cpu_pipeline as cp
from tests import rate_cases as rc
from tests import test_gpu_transcode as tg          # its sources (coded once per process), fixture and certificate check
from tests import transcode_cases as tc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = tg.GOLD
_sparse_rev = {}
_single = {}


def sparse_source(name, rev):
    """the same geometry with most blocks not coded: irreversible, the image coded at grid index 0 (step 0.5); reversible (no
    step to move), a flat mid-grey image -> (codestream, the planes the oracle's block decoder leaves of it)"""
    if not rev:
        return tg.source(name, rev, 0)
    if name not in _sparse_rev:
        from openjph_amd import codec
        img, _ = rc.case_image(name)
        flat = np.full_like(img, 1 << (rc.CASES[name]["bd"] - 1))
        cs = codec.Encoder(tc.case_params(name, tc.src_kwargs(name, True))).encode(flat)
        _sparse_rev[name] = (cs, tc.cpu_source_planes(cs)[1])
    return _sparse_rev[name]


def assert_sparse(first, sparse):
    coded = parse_codestream(first).coded_blocks()["len1"] > 0
    assert int((coded & ~(parse_codestream(sparse).coded_blocks()["len1"] > 0)).sum()) > coded.sum() // 2


def single(key, cs, **kw):
    """codec.transcode of a source, once per (source, target)"""
    from openjph_amd import codec
    if key not in _single:
        _single[key] = codec.transcode(cs, **kw)
    return _single[key]


def raises_code(code, fn):
    with pytest.raises(capi.OjphError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return ei.value


def feed(pipe, cs):
    buf = pipe.acquire(len(cs))
    assert buf is not None
    buf[:] = np.frombuffer(cs, dtype=np.uint8)
    pipe.submit()


# ---------------------------------------------------------------------------------------------
# 1. sequences at fixed targets
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("name,rev", tc.CASES, ids=tg.IDS)
def test_sequences_at_fixed_targets(name, rev, depth):
    from openjph_amd import pipeline
    dense, a_dense = tg.source(name, rev)
    sparse, a_sparse = sparse_source(name, rev)
    assert_sparse(dense, sparse)
    kinds = [("dense", dense, a_dense), ("sparse", sparse, a_sparse), ("dense", dense, a_dense)]
    seq = [kinds[i % 3] for i in range(2 * depth + 1)]
    for target in (["blk32"] if rev else ["blk32", "frac"]):
        kw = tc.out_kwargs(name, rev, target)
        tkw = tc.transcode_kwargs(rev, target)
        want = {k: tc.cpu_transcode_planes(a, tc.case_params(name, kw)) for k, _, a in kinds[:2]}
        g = GOLD["cases"][tc.case_id(name, rev)]["targets"][target]
        pipe = pipeline.TranscoderPipe(dense, depth=depth, **tkw)
        got = list(pipe.transcode_sequence([cs for _, cs, _ in seq]))
        assert len(got) == len(seq) and pipe.in_flight == 0
        for i, ((kind, cs, _), out) in enumerate(zip(seq, got)):
            assert out == single((name, rev, kind, target), cs, **tkw), (target, i, kind)
            assert out == want[kind], (target, i, kind)
            if kind == "dense":
                assert (tg.sha(out), len(out)) == (g["sha256"], g["len"]), (target, i)
        assert want["dense"] != want["sparse"]
        st = pipe.stats()
        assert st["frames"] == len(seq) and pipe.failed_blocks == 0
        pipe.close()


# ---------------------------------------------------------------------------------------------
# 2. budgets
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.IRV)
def test_budgets_frame_by_frame(name):
    from openjph_amd import pipeline
    cs, arena = tg.source(name, False)
    inr = rc.budgets(name)[0]
    budgets = [inr[0], inr[0], inr[1], inr[2], inr[2], inr[3], inr[1], inr[1], inr[1]]     # (each repeat: the hint's certificate)
    pipe = pipeline.TranscoderPipe(cs, depth=3, max_bytes=budgets[0])
    infos, outs = [], []
    for out in pipe.transcode_sequence([cs] * len(budgets), budgets=budgets):
        outs.append(out)
        infos.append(pipe.rate_info())
    assert len(outs) == len(budgets)
    for i, (b, out, info) in enumerate(zip(budgets, outs, infos)):
        print(name, i, b, info)
        tg.check_info(name, info, b)
        j = info["grid_index"]
        assert j < rc.GRID - 1 and len(out) == info["bytes"]      # (an in-range budget: the certificate has both halves)
        assert out == single((name, False, "dense", "q%d" % j), cs, qstep=rc.grid_qstep(j))
        if i and budgets[i - 1] == b:
            assert info["passes"] == 2 and info["grid_index"] == infos[i - 1]["grid_index"], (i, info)
    pipe.close()


# ---------------------------------------------------------------------------------------------
# 3. a frame that fails, mid-sequence
# ---------------------------------------------------------------------------------------------
def cut_source(name):
    cs, _ = tg.source(name, False)
    sot = cs.rfind(b"\xff\x90\x00\x0a")
    return cs[:sot + (len(cs) - sot) // 2]                   # the middle of the last tile-part


def decode_code(cut):
    from openjph_amd import codec
    try:
        codec.decode(cut)
    except capi.OjphError as e:
        return e.code
    return None


@pytest.mark.parametrize("name", ["A", "C"])
def test_a_frame_that_fails_mid_sequence(name):
    from openjph_amd import pipeline
    dense, a_dense = tg.source(name, False)
    sparse, a_sparse = tg.source(name, False, 0)
    other = tg.source("B", False)[0]
    cut = cut_source(name)
    code = decode_code(cut)
    assert code in (capi.E_BLOCK, capi.E_CODESTREAM)
    tkw = tc.transcode_kwargs(False, "blk32")
    params = tc.case_params(name, tc.out_kwargs(name, False, "blk32"))
    w_dense, w_sparse = tc.cpu_transcode_planes(a_dense, params), tc.cpu_transcode_planes(a_sparse, params)
    # a fixed step: another geometry, then a cut source, each between good frames (the sparse one right behind the failure: it
    # would show planes the failed frame left)
    pipe = pipeline.TranscoderPipe(dense, depth=2, **tkw)
    seq = [(dense, w_dense), (other, capi.E_INVALID), (sparse, w_sparse), (dense, w_dense), (cut, code), (sparse, w_sparse), (dense, w_dense)]
    done = 0
    for cs, _ in seq:
        while pipe.acquire(len(cs)) is None:
            done = collect_and_check(pipe, seq, done)
        feed(pipe, cs)
    while pipe.in_flight:
        done = collect_and_check(pipe, seq, done)
    assert done == len(seq)
    pipe.close()
    # the same cut source in a resilient pipe: its failed blocks are zero blocks of the output
    src = parse_codestream(cut, resilient=True)
    want = tc.cpu_transcode(cut, params, resilient=True)
    pipe = pipeline.TranscoderPipe(dense, depth=2, resilient=True, **tkw)
    got = list(pipe_outputs(pipe, [dense, cut, sparse]))
    assert got[0] == (w_dense, 0) and got[2] == (w_sparse, 0)
    print(name, "failed blocks: oracle", tc.cpu_failed_blocks(src, cut), "device", got[1][1])
    assert got[1] == (want, tc.cpu_failed_blocks(src, cut)) and want != w_dense
    pipe.close()


def collect_and_check(pipe, seq, done):
    want = seq[done][1]
    if isinstance(want, int):
        raises_code(want, pipe.collect)
    else:
        assert pipe.collect() == want, done
        assert pipe.failed_blocks == 0
    return done + 1


def pipe_outputs(pipe, sources):
    for cs in sources:
        feed(pipe, cs)
        yield pipe.collect(), pipe.failed_blocks


@pytest.mark.parametrize("name", ["A", "C"])
def test_a_budget_nothing_fits_mid_sequence(name):
    from openjph_amd import pipeline
    cs, _ = tg.source(name, False)
    b = rc.budgets(name)[0][1]
    pipe = pipeline.TranscoderPipe(cs, depth=2, max_bytes=b)
    outs, infos = [], []
    for budget in (b, b, 64, b, b):
        pipe.set_budget(budget)
        feed(pipe, cs)
        if budget == 64:
            raises_code(capi.E_BUDGET, pipe.collect)
            info = pipe.rate_info()
            assert info["passes"] >= 1 and 0 <= info["first_guess"] < rc.GRID
            outs.append(None)
        else:
            outs.append(pipe.collect())
        infos.append(pipe.rate_info())
    for i in (0, 1, 3, 4):
        tg.check_info(name, infos[i], b)
        assert outs[i] == outs[0] and len(outs[i]) == infos[i]["bytes"]
    assert outs[0] == single((name, False, "dense", "q%d" % infos[0]["grid_index"]), cs, qstep=rc.grid_qstep(infos[0]["grid_index"]))
    # the hint stayed where the last certified frame left it: the frame behind the failure costs the certificate's two trials
    assert [infos[i]["passes"] for i in (1, 3, 4)] == [2, 2, 2], infos
    pipe.close()


# ---------------------------------------------------------------------------------------------
# 4. a wait that runs out
# ---------------------------------------------------------------------------------------------
REPEAT_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, %r)
from openjph_amd import codec, pipeline
from tests import rate_cases as rc
from tests import transcode_cases as tc
name = "A"
cs = codec.Encoder(tc.case_params(name, tc.src_kwargs(name, False))).encode(rc.case_image(name)[0])
arena = tc.cpu_source_planes(cs)[1]
kw = tc.out_kwargs(name, False, "blk32")
want = tc.cpu_transcode_planes(arena, tc.case_params(name, kw))
pipe = pipeline.TranscoderPipe(cs, depth=2, **tc.transcode_kwargs(False, "blk32"))
got = list(pipe.transcode_sequence([cs] * 3))               # (the first run starts from an arena of zeros: without the repeat the planes would be short)
assert got == [want] * 3 and pipe.failed_blocks == 0
assert pipe.stats()["fused_retries"] == 3, pipe.stats()
pipe.close()
budget = rc.budgets(name)[0][1]
pipe = pipeline.TranscoderPipe(cs, depth=2, max_bytes=budget)   # ... and with a budget the search sees the repeated planes
sizes = json.load(open(os.path.join(%r, "tests", "golden", "transcode.json")))["cases"]["Airv"]["sizes"]
n = 0
for got in pipe.transcode_sequence([cs] * 3):
    info = pipe.rate_info()
    j = info["grid_index"]
    assert len(got) == info["bytes"] == sizes[j] <= budget < sizes[j + 1] == info["bytes_finer"], info
    assert got == tc.cpu_transcode_planes(arena, tc.case_params(name, tc.out_kwargs(name, False, "frac", rc.grid_qstep(j))))
    n += 1
assert n == 3 and pipe.stats()["fused_retries"] == 3, pipe.stats()
pipe.close()
print("OK")
''' % (os.path.dirname(HERE), os.path.dirname(HERE))


def test_a_wait_that_runs_out_is_repeated_before_coding():
    """OJPHGPU_FUSED_DBG=4 makes one worker wavefront of every one-launch block decoder run behave as if its wait for the
    chains had run out (tests/test_gpu_transcode.py): the pipe's device stage repeats the run through the separate launches
    when it collects the verdicts, takes the statistics again, and only then codes -- the bytes are cpu_transcode's"""
    env = dict(os.environ, OJPHGPU_FUSED_DBG="4", OJPHGPU_DEC_FUSED="2")
    r = subprocess.run([sys.executable, "-c", REPEAT_SCRIPT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and b"OK" in r.stdout, r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals():
    from openjph_amd import pipeline
    cs, _ = tg.source("B", False)
    pipe = pipeline.TranscoderPipe(cs, depth=2, block=(32, 32))      # an irreversible output with neither a step nor a budget
    raises_code(capi.E_INVALID, lambda: pipe.acquire(len(cs)))
    pipe.set_budget(20000)                                           # ... becomes usable with a budget, before the first acquire
    feed(pipe, cs)
    assert len(pipe.collect()) <= 20000
    raises_code(capi.E_INVALID, lambda: pipe.set_budget(0))          # not back to 0
    pipe.close()
    rev = tg.source("D", True)[0]                                    # a budget on a reversible output
    raises_code(capi.E_INVALID, lambda: pipeline.TranscoderPipe(rev, max_bytes=20000))
    pipe = pipeline.TranscoderPipe(rev, depth=2)
    raises_code(capi.E_INVALID, lambda: pipe.set_budget(20000))
    feed(pipe, rev)
    assert pipe.collect() == rev                                     # (nothing changed: the source again)
    pipe.close()
    q = rc.grid_qstep(tc.SRC_INDEX)
    pipe = pipeline.TranscoderPipe(cs, depth=2, qstep=q)
    feed(pipe, cs)
    raises_code(capi.E_INVALID, lambda: pipe.set_budget(20000))      # switching on after the first acquire
    feed(pipe, cs)
    assert pipe.acquire(len(cs)) is None                             # beyond depth: collect first
    first = pipe.collect()
    assert pipe.collect() == first                                   # (the codestream handed out before it is released now)
    assert pipe.acquire(len(cs)) is not None
    raises_code(capi.E_INVALID, pipe.collect)                        # nothing in flight
    assert pipe.in_flight == 0
    pipe.close()


# ---------------------------------------------------------------------------------------------
# 6. neighbours undisturbed
# ---------------------------------------------------------------------------------------------
def test_neighbours_are_undisturbed():
    from openjph_amd import codec, pipeline
    cs, arena = tg.source("A", False)
    img, _ = rc.case_image("A")
    tkw = tc.transcode_kwargs(False, "blk32")
    want = tc.cpu_transcode_planes(arena, tc.case_params("A", tc.out_kwargs("A", False, "blk32")))
    samples, _ = cp.decode(cs)
    t = codec.Transcoder(cs, **tkw)
    enc = pipeline.EncoderPipe(params=tc.case_params("A", tc.src_kwargs("A", False)), depth=2, container=32)
    dec = pipeline.DecoderPipe(cs, depth=2, container=32)

    def neighbours():
        assert t.transcode(cs) == want
        assert list(enc.encode_sequence([img, img])) == [cs, cs]
        for f in dec.decode_sequence([cs, cs]):
            assert np.array_equal(f, samples)

    neighbours()
    pipe = pipeline.TranscoderPipe(cs, depth=2, **tkw)
    feed(pipe, cs)
    feed(pipe, cs)
    neighbours()                                                     # ... with frames of the pipe in flight
    assert pipe.collect() == want and pipe.collect() == want
    assert list(pipe.transcode_sequence([cs] * 3)) == [want] * 3
    neighbours()
    pipe.close()
    neighbours()
    enc.close()
    dec.close()
