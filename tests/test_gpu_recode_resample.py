"""The resampling recoder on the GPU (include/ojphgpu.h section 5e, "a resampling recode"): codec.Recoder(resample="cosited")
/ codec.recode against the contract stated with the oracle pipeline (tests/resample_cases.py: the frame G and, at the
output's own step, the codestream, byte for byte; the reference's encode of G where tests/golden/recode_resample.json has
it) and against the composition the object stands for -- codec.Encoder of the output, in the same mode, given G."""
import json
import os

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd.pipeline import fit_container
from openjph_amd.plan import Plan
from tests import recode_cases as rcc
from tests import resample_cases as rsc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD_PATH = os.path.join(HERE, "golden", "recode_resample.json")
GOLD = json.load(open(GOLD_PATH)) if os.path.exists(GOLD_PATH) else {"cases": {}}


def raises_code(code, fn):
    with pytest.raises(capi.OjphError) as ei:
        fn()
    assert ei.value.code == code, ei.value


def planes_of(frame, plan):
    """a frame G (a tensor in its container) -> the list of its planes as int32, each read by its component's sign"""
    raw = frame.cpu().numpy().reshape(-1)
    out = []
    for c in range(int(plan.params.num_comps)):
        i, (_, sg) = plan.comp_info(c), plan.comp_format(c)
        q = raw[i["frame_off"]:i["frame_off"] + i["w"] * i["h"]]
        if raw.dtype.itemsize < 4:
            q = q.view(np.dtype("%s%d" % ("i" if sg else "u", raw.dtype.itemsize)))
        out.append(q.astype(np.int32).reshape(i["h"], i["w"]))
    return out


def mode_kw(mode):
    return {"plain": {}, "max_bytes": dict(max_bytes=mode[-1]), "min_psnr": dict(min_psnr=mode[-1])}[mode[0]]


@pytest.mark.parametrize("case", list(rsc.CASES) + list(rsc.MORE))
def test_recode_is_the_statement(case):
    from openjph_amd import codec
    c = rsc.CASES.get(case) or rsc.MORE[case]
    cs = rsc.source(case)
    kw = mode_kw(c["mode"])
    G_cpu, params, out = rsc.cpu_fitted_resampled(cs, c["view"], c["out"])
    rec = codec.Recoder(cs, resample="cosited", **c["view"], **c["out"], **kw)
    assert bytes(rec.params) == bytes(params)
    got = rec.recode(cs)
    assert rec.failed_blocks == 0
    # frame() is G, in the output plan's shape and the container of its depths
    G = rec.frame()
    depths = [rec.plan.comp_format(k)[0] for k in range(int(rec.params.num_comps))]
    assert tuple(G.shape) == tuple(rec.plan.frame_shape) and G.element_size() * 8 == fit_container(depths)
    planes = planes_of(G, rec.plan)
    assert [q.shape for q in planes] == [q.shape for q in G_cpu]
    for k, (a, b) in enumerate(zip(planes, G_cpu)):
        assert np.array_equal(a, b.astype(np.int32)), (case, k)
    # the encoder of the output on G, in the same mode: the bytes and the infos
    enc = codec.Encoder(plan=Plan(rec.params), **kw)
    want = enc.encode(G.clone())
    print(case, kw, len(cs), "->", len(got), len(want))
    assert got == want
    info = {"plain": None, "max_bytes": "rate_info", "min_psnr": "quality_info"}[c["mode"][0]]
    if info:
        a, b = getattr(rec, info)(), getattr(enc, info)()
        print(a)
        assert a == b and len(got) == a["bytes"]
        if c["mode"][0] == "max_bytes":
            assert len(got) <= c["mode"][1]
    else:
        assert got == rcc.cpu_encode_planes(out, G_cpu)                  # the statement, byte for byte
    if case in GOLD["cases"]:
        g = GOLD["cases"][case]
        assert rcc.frame_digest(planes) == g["frame"]["sha256"]
        assert (rcc.sha(got), len(got)) == (g["output"]["sha256"], g["output"]["len"])
    assert codec.recode(cs, resample="cosited", **c["view"], **c["out"], **kw) == got     # the one-call form
    tm = rec.timing()
    assert tm["decode_ms"] > 0 and tm["fit_ms"] > 0 and tm["encode_ms"] > 0 and tm["finish_ms"] > 0


def test_reuse_leaves_nothing_stale():
    """one object over coarse / fine / coarse sources: G has a buffer of its own in the output's layout, written whole"""
    from openjph_amd import codec
    from tests import cpu_pipeline as cp
    from tests import rate_cases as rc
    img, _ = rc.case_image("A")
    fine = rsc.source("A420")
    coarse = cp.encode(img, **rcc.src_kwargs(("A", False, 0)))[0]        # step 0.5: most blocks are not coded
    assert len(coarse) < len(fine) // 2
    for out in (dict(downsampling=rsc.S420, bit_depth=10, color_transform=False, qstep=rsc.Q150),
                dict(downsampling=rsc.S422, bit_depth=20, color_transform=False, qstep=rsc.Q150)):      # 16- and 32-bit containers
        want = {k: rsc.cpu_recode_resampled(cs, {}, out) for k, cs in (("fine", fine), ("coarse", coarse))}
        assert want["fine"] != want["coarse"]
        rec = codec.Recoder(coarse, resample="cosited", **out)
        assert rec.recode(coarse) == want["coarse"]
        assert rec.recode(fine) == want["fine"]
        assert rec.recode(coarse) == want["coarse"]
        raises_code(capi.E_INVALID, lambda: rec.recode(rsc.source("C420")))     # another geometry: refused, and the object goes on
        rec.submit(coarse)                                               # a source submitted and never finished is dropped
        assert rec.recode(fine) == want["fine"] and rec.failed_blocks == 0


def test_without_resample_the_old_refusal_stands():
    from openjph_amd import codec
    cs = rsc.source("C422")
    out = rsc.CASES["C422"]["out"]
    raises_code(capi.E_INVALID, lambda: codec.Recoder(cs, **out))
    raises_code(capi.E_INVALID, lambda: codec.recode(cs, **out))
    raises_code(capi.E_INVALID, lambda: codec.Recoder(cs, resample="none", **out))
    with pytest.raises(ValueError):
        codec.Recoder(cs, resample="box", **out)
    # what the resampling rule refuses, through the object: a factor of 4, an odd window
    raises_code(capi.E_INVALID, lambda: codec.Recoder(cs, resample="cosited", downsampling=[(1, 1), (4, 1), (4, 1)], qstep=rsc.Q150))
    raises_code(capi.E_INVALID, lambda: codec.Recoder(cs, resample="cosited", region=(41, 24, 128, 96), downsampling=rsc.S422, qstep=rsc.Q150))
    # nothing to resample: resample="cosited" is the plain recoder
    same = dict(bit_depth=8, qstep=rsc.Q150)
    assert codec.recode(cs, resample="cosited", **same) == codec.recode(cs, **same)
