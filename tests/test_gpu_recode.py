"""The recoder on the GPU (include/ojphgpu.h section 5e): codec.recode / codec.Recoder against the fixture made from the
reference (tests/golden/recode.json: the fitted frame's digest, the reference's encode of it) and against the composition the
object stands for -- codec.Encoder of the output, in the same mode, given the same fitted frame."""
import json
import os

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd.pipeline import fit_container, fit_frame
from openjph_amd.plan import Plan, make_params
from tests import rate_cases as rc
from tests import recode_cases as rcc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "recode.json")))
_sources = {}


def gpu_source(src):
    from openjph_amd import codec
    c = rc.CASES[src[0]]
    img, _ = rc.case_image(src[0])
    return codec.Encoder(make_params(c["w"], c["h"], c["nc"], **rcc.src_kwargs(src))).encode(img)


def source(src):
    """a source coded on the device, once; the fixture's sources are the reference's bytes"""
    if src not in _sources:
        _sources[src] = gpu_source(src)
        for g in (GOLD["cases"][k]["source"] for k, c in rcc.CASES.items() if c["source"] == src):
            assert (rcc.sha(_sources[src]), len(_sources[src])) == (g["sha256"], g["len"])
    return _sources[src]


def raises_code(code, fn):
    with pytest.raises(capi.OjphError) as ei:
        fn()
    assert ei.value.code == code, ei.value


def planes_of(frame, plan):
    """a fitted frame (a tensor in its container) -> the list of its planes as int32, each read by its component's sign"""
    raw = frame.cpu().numpy().reshape(-1)
    out = []
    for c in range(int(plan.params.num_comps)):
        i, (_, sg) = plan.comp_info(c), plan.comp_format(c)
        q = raw[i["frame_off"]:i["frame_off"] + i["w"] * i["h"]]
        if raw.dtype.itemsize < 4:
            q = q.view(np.dtype("%s%d" % ("i" if sg else "u", raw.dtype.itemsize)))
        out.append(q.astype(np.int32).reshape(i["h"], i["w"]))
    return out


def composed(cs, view, out_kw, resilient=False, **mode):
    """what a recoder stands for, from its parts: a Decoder under the view, the fit in numpy, an Encoder of the output
    -> (codestream, failed blocks, the encoder)"""
    from openjph_amd import codec
    dec = codec.Decoder(cs, resilient=resilient, **view)
    img = dec.run_device()
    failed = dec.failed_blocks()
    src = rcc.view_plan(cs, view, resilient)
    out = Plan(rcc.recode_params(src, **out_kw))
    nc = int(out.params.num_comps)
    G = fit_frame(src.unpack_frame(img.cpu().numpy()), [src.comp_format(c)[0] for c in range(nc)], [out.comp_format(c)[0] for c in range(nc)],
                  [out.comp_format(c)[1] for c in range(nc)])
    enc = codec.Encoder(plan=out, **mode)
    frame = np.stack(G) if len(out.frame_shape) == 3 else np.concatenate([q.reshape(-1).view(G[0].dtype) for q in G])
    return enc.encode(frame), failed, enc


def settings(mode):
    """the settings a case's mode runs through: [(Encoder / Recoder keywords, which info to compare)]"""
    if mode[0] == "max_bytes":
        return [(dict(max_bytes=b), "rate_info") for b in mode[1]]
    if mode[0] == "min_psnr":
        return [(dict(min_psnr=mode[1]), "quality_info")]
    if mode[0] == "capped":
        return [(dict(min_psnr=mode[1], cap_bytes=cap), "capped_info") for cap in mode[2]]
    return [(dict(), None)]


# ---------------------------------------------------------------------------------------------
# 1. every case: the fitted frame, the fixture, the encoder of the same frame in the same mode
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(rcc.CASES))
def test_recode_is_the_encoder_of_the_fitted_frame(case):
    from openjph_amd import codec
    c = rcc.CASES[case]
    cs = source(c["source"])
    g = GOLD["cases"][case]
    rec = codec.Recoder(cs, **c["view"], **c["out"])
    enc = codec.Encoder(plan=Plan(rec.params))
    outcomes = []
    for kw, info in settings(c["mode"]):
        if "max_bytes" in kw:
            rec.set_budget(kw["max_bytes"]); enc.set_budget(kw["max_bytes"])
        elif kw:
            rec.set_quality(**kw); enc.set_quality(**kw)
        got = rec.recode(cs)
        assert rec.failed_blocks == 0
        G = rec.frame()
        depths = [rec.plan.comp_format(k)[0] for k in range(int(rec.params.num_comps))]
        assert tuple(G.shape) == tuple(rec.plan.frame_shape) and G.element_size() * 8 == fit_container(depths)
        planes = planes_of(G, rec.plan)
        assert [list(q.shape) for q in planes] == g["frame"]["shapes"]
        assert rcc.frame_digest(planes) == g["frame"]["sha256"]
        want = enc.encode(G.clone())
        print(case, kw, len(cs), "->", len(got), len(want))
        assert got == want
        if info:
            a, b = getattr(rec, info)(), getattr(enc, info)()
            print(a)
            assert a == b
            outcomes.append(a.get("outcome"))
            assert len(got) == a["bytes"]
        if c["ref"]:
            assert (rcc.sha(got), len(got)) == (g["output"]["sha256"], g["output"]["len"])
    if c["mode"][0] == "capped":
        assert outcomes == [capi.CAPPED_MET, capi.CAPPED_BY_BUDGET]     # one cap that does not bind, one that does
    kw = settings(c["mode"])[0][0]
    first = codec.recode(cs, **c["view"], **c["out"], **kw)              # the one-call form
    if len(settings(c["mode"])) == 1:
        assert first == got
    tm = rec.timing()
    assert tm["decode_ms"] > 0 and tm["fit_ms"] > 0 and tm["encode_ms"] > 0 and tm["finish_ms"] > 0


def test_rewrap_is_the_transcode_and_the_direct_encode():
    from openjph_amd import codec
    cs = source(("D", True, None))
    got = codec.recode(cs, block=(32, 32))
    assert got == codec.transcode(cs, block=(32, 32))
    img, _ = rc.case_image("D")
    assert got == codec.encode(img, **rcc.out_make_kwargs("rewrapD")[0])


def test_an_odd_chroma_origin_is_refused():
    from openjph_amd import codec
    c = rcc.REFUSED["cropEodd"]
    cs = source(c["source"])
    assert codec.decode(cs, **c["view"]).size > 0                        # (the decoder takes the window)
    raises_code(capi.E_INVALID, lambda: codec.Recoder(cs, **c["view"], **c["out"]))


# ---------------------------------------------------------------------------------------------
# 2. one object, source after source
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view,out", [(dict(), dict(bit_depth=10, qstep=rcc.Q150)),
                                      (dict(region=(40, 24, 128, 96)), dict(qstep=rcc.Q150)),
                                      (dict(skip_res=1), dict(bit_depth=20, qstep=rcc.Q150))], ids=["whole-16", "window-16", "proxy-32-in-place"])
def test_reuse_leaves_nothing_stale(view, out):
    from openjph_amd import codec
    fine, coarse = source(("A", False, rcc.SRC_INDEX)), source(("A", False, 0))      # step 0.5: most blocks are not coded
    assert len(coarse) < len(fine) // 2
    want = {k: composed(cs, view, out)[0] for k, cs in (("fine", fine), ("coarse", coarse))}
    assert want["fine"] != want["coarse"]
    rec = codec.Recoder(coarse, **view, **out)
    assert rec.recode(coarse) == want["coarse"]
    assert rec.recode(fine) == want["fine"]
    assert rec.recode(coarse) == want["coarse"]
    other = source(("B", False, rcc.SRC_INDEX))                        # another geometry: refused, and the object goes on
    raises_code(capi.E_INVALID, lambda: rec.recode(other))
    raises_code(capi.E_INVALID, rec.finish)                              # (nothing is submitted)
    assert rec.recode(fine) == want["fine"]
    rec.submit(coarse)                                                   # a source submitted and never finished is dropped
    assert rec.recode(fine) == want["fine"]
    assert rec.failed_blocks == 0


def test_modes_change_on_one_object():
    from openjph_amd import codec
    cs = source(("B", False, rcc.SRC_INDEX))
    rec = codec.Recoder(cs, qstep=rcc.Q150)
    plain = rec.recode(cs)
    budget = rc.budgets("B")[0][1]
    rec.set_budget(budget)
    a = rec.recode(cs)
    assert len(a) <= budget and a == composed(cs, {}, dict(qstep=rcc.Q150), max_bytes=budget)[0]
    raises_code(capi.E_INVALID, lambda: rec.set_quality(min_psnr=40))    # (a budget is set: as the encoder refuses it)
    rec.set_budget(rc.budgets("B")[1])
    raises_code(capi.E_BUDGET, lambda: rec.recode(cs))                   # ... and the object goes on
    rec.set_budget(0)
    rec.set_quality(min_psnr=40)
    b = rec.recode(cs)
    assert b == composed(cs, {}, dict(qstep=rcc.Q150), min_psnr=40)[0]
    rec.set_quality()
    assert rec.recode(cs) == plain
    raises_code(capi.E_INVALID, lambda: codec.Recoder(source(("D", True, None)), max_bytes=20000))   # a budget on a reversible output


# ---------------------------------------------------------------------------------------------
# 3. a damaged source
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "C"])
def test_damaged_source(name):
    from openjph_amd import codec
    cs = source((name, False, rcc.SRC_INDEX))
    sot = cs.rfind(b"\xff\x90\x00\x0a")
    cut = cs[:sot + (len(cs) - sot) // 2]                                # the middle of the last tile-part
    out = dict(bit_depth=rc.CASES[name]["bd"] - 2, qstep=rcc.Q150)
    want, failed, _ = composed(cut, {}, out, resilient=True)
    rec = codec.Recoder(cut, resilient=True, **out)
    got = rec.recode(cut)
    print(name, "failed blocks: decoder", failed, "recoder", rec.failed_blocks)
    assert got == want and rec.failed_blocks == failed
    assert got != composed(cs, {}, out)[0]
    # not resilient: what codec.decode makes of the file
    try:
        codec.decode(cut)
        code = None
    except capi.OjphError as e:
        code = e.code
    assert code in (capi.E_BLOCK, capi.E_CODESTREAM)
    raises_code(code, lambda: codec.recode(cut, **out))


def test_blocks_that_fail_to_decode():
    """a stretch of the last tile-part's block bytes zeroed: the headers parse, the blocks over it do not decode"""
    from openjph_amd import codec
    cs = source(("A", False, rcc.SRC_INDEX))
    sot = cs.rfind(b"\xff\x90\x00\x0a")
    mid = sot + (len(cs) - sot) // 2
    bad = cs[:mid] + bytes(3000) + cs[mid + 3000:]
    out = dict(bit_depth=10, qstep=rcc.Q150)
    want, failed, _ = composed(bad, {}, out, resilient=True)
    assert failed > 0
    rec = codec.Recoder(bad, resilient=True, **out)
    assert rec.recode(bad) == want and rec.failed_blocks == failed
    assert rec.recode(cs) == composed(cs, {}, out)[0] and rec.failed_blocks == 0
    rec = codec.Recoder(cs, **out)                                       # not resilient: E_BLOCK, and the object goes on
    raises_code(capi.E_BLOCK, lambda: codec.decode(bad))
    raises_code(capi.E_BLOCK, lambda: rec.recode(bad))
    assert rec.failed_blocks == failed
    raises_code(capi.E_INVALID, rec.finish)                              # (nothing was written, nothing is left to finish)
    assert rec.recode(cs) == composed(cs, {}, out)[0]


# ---------------------------------------------------------------------------------------------
# 4. a one-launch block decoder run whose wait ran out is repeated, fitted and coded again
# ---------------------------------------------------------------------------------------------
REPEAT_SCRIPT = r'''
import sys
sys.path.insert(0, %r)
from openjph_amd import codec
from tests import rate_cases as rc
from tests import recode_cases as rcc
from tests import test_gpu_recode as tg
src = ("A", False, rcc.SRC_INDEX)
cs = tg.gpu_source(src)
dec = codec.Decoder(cs)                                     # the switch is on for this codestream: a decoder repeats its run
dec.run_device()
assert dec.failed_blocks() == 0 and dec.fused_retries() == 1, dec.fused_retries()
for out in (dict(bit_depth=10, qstep=rcc.Q150), dict(bit_depth=20, qstep=rcc.Q150)):     # a frame of its own; fitted in place
    want = tg.composed(cs, {}, out)[0]
    rec = codec.Recoder(cs, **out)
    for run in range(2):
        assert rec.recode(cs) == want, (out, run)
        assert rec.failed_blocks == 0
budget = rc.budgets("A")[0][1]
want, _, enc = tg.composed(cs, {}, dict(), max_bytes=budget)    # ... and a search sees the repeated frame
rec = codec.Recoder(cs, max_bytes=budget)
assert rec.recode(cs) == want and rec.rate_info() == enc.rate_info()
want, _, enc = tg.composed(cs, {}, dict(), min_psnr=45)
rec = codec.Recoder(cs, min_psnr=45)
assert rec.recode(cs) == want and rec.quality_info() == enc.quality_info()
print("OK")
''' % (os.path.dirname(HERE),)


def test_a_wait_that_runs_out_is_repeated_fitted_and_coded_again():
    """OJPHGPU_FUSED_DBG=4 makes one worker wavefront of every one-launch block decoder run behave as if its wait for the
    chains had run out (tests/test_gpu_contention.py): the recoder's finish repeats the decode through the separate launches
    when it collects the verdicts, then the fit and the encoder's run -- the bytes are those of the composition"""
    import subprocess
    import sys
    env = dict(os.environ, OJPHGPU_FUSED_DBG="4", OJPHGPU_DEC_FUSED="2")
    r = subprocess.run([sys.executable, "-c", REPEAT_SCRIPT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and b"OK" in r.stdout, r.stderr[-3000:]
