"""Encoding to a quality target under a byte cap on the GPU (include/ojphgpu.h section 5c, "under a byte cap"): the single
encoder against the set of answers the contract allows over the reference's recorded tables (tests/capped_cases.py), a plain
encode at the chosen step, the reference's digests and the recorded errors."""
import hashlib

import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd import plan as planmod
from openjph_amd.plan import Plan, make_params
from tests import capped_cases as cc
from tests import rate_cases as rc

pytestmark = pytest.mark.gpu

_PLAIN = {}


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def case_params(name, qstep=-1.0):
    c = rc.CASES[name]
    return make_params(c["w"], c["h"], c["nc"], **rc.case_kwargs(name, qstep))


def case_frame(name, plan):
    img, _ = rc.case_image(name)
    return plan.pack_frame(img) if isinstance(img, list) else img


def plain_encode(name, j, frame):
    """the plain encode of a case at grid index j, computed once"""
    from openjph_amd import codec
    if (name, j) not in _PLAIN:
        _PLAIN[(name, j)] = codec.Encoder(case_params(name, planmod.rate_grid_qstep(j))).encode(frame)
    return _PLAIN[(name, j)]


def check_capped(name, enc, cs, frame, T, B):
    """what every capped encode of a recorded frame must satisfy -> the info"""
    total, sizes = cc.tables(name)
    info = enc.capped_info()
    j = info["grid_index"]
    print(name, T, B, {k: v for k, v in info.items() if k != "comps"})
    assert (j, info["outcome"]) in cc.answers(total, sizes, T, B), info
    cc.check_info(info, total, sizes, T, B)
    assert cs == plain_encode(name, j, frame) and len(cs) == info["bytes"]
    assert info["comps"] == cc.comp_figures(name, j)
    assert info["pae"] == max(p for _, p in info["comps"])
    assert info["quality_passes"] <= 13 and info["rate_passes"] <= 18
    return info


@pytest.mark.parametrize("name", ["A", "B", "E"])
def test_encode_to_a_target_under_a_cap(name):
    from openjph_amd import codec
    params = case_params(name)
    pl = Plan(params)
    frame = case_frame(name, pl)
    gold = cc.QUAL["cases"][name]
    inr, _, _ = rc.budgets(name)
    enc = codec.Encoder(params)
    seen = set()
    for db in (40, 50):
        t = gold["targets"][str(db)]
        T = t["max_sse"]
        for k, B in enumerate(inr):
            if k % 2:
                enc.set_quality(min_psnr=db, cap_bytes=B)
            else:
                enc.set_quality(max_sse=T, cap_bytes=B)
            assert enc.max_sse == T and enc.cap_bytes == B
            cs = enc.encode(frame)
            info = check_capped(name, enc, cs, frame, T, B)
            seen.add(info["outcome"])
            if info["outcome"] == cc.MET:
                assert info["grid_index"] == t["certified"][0] and sha(cs) == t["sha256"]
                assert info["rate_passes"] == 1                          # the statistics and the stepper never ran
            else:
                assert info["quality_index"] == t["certified"][0]
    assert seen == {cc.MET, cc.BY_BUDGET}


def test_a_target_beyond_the_grid_ends_at_the_finest_step():
    from openjph_amd import codec
    name = "D"
    params = case_params(name)
    frame = case_frame(name, Plan(params))
    total, sizes = cc.tables(name)
    assert total[240] == 3284
    B = rc.budgets(name)[2]                                      # above size(240)
    enc = codec.Encoder(params, max_sse=3283, cap_bytes=B)
    cs = enc.encode(frame)
    info = check_capped(name, enc, cs, frame, 3283, B)
    assert (info["grid_index"], info["outcome"], info["quality_index"]) == (240, cc.BY_BUDGET, rc.GRID)
    assert info["sse"] == 3284 and info["bytes_finer"] == 0


def test_a_cap_nothing_fits_then_the_next_encode():
    from openjph_amd import codec
    name = "A"
    params = case_params(name)
    frame = case_frame(name, Plan(params))
    T = cc.QUAL["cases"][name]["targets"]["40"]["max_sse"]
    inr, below, _ = rc.budgets(name)
    enc = codec.Encoder(params, max_sse=T, cap_bytes=below)
    with pytest.raises(capi.OjphError) as e:
        enc.encode(frame)
    assert e.value.code == capi.E_BUDGET
    info = enc.capped_info()
    assert info["quality_passes"] >= 2 and info["rate_passes"] >= 2 and info["comps"] == []
    enc.set_quality(max_sse=T, cap_bytes=inr[1])                 # ... and the encoder stays usable
    check_capped(name, enc, enc.encode(frame), frame, T, inr[1])
    enc.set_quality(max_sse=T, cap_bytes=inr[3])
    assert check_capped(name, enc, enc.encode(frame), frame, T, inr[3])["outcome"] == cc.MET


def test_cap_zero_is_set_quality_and_the_mode_goes_off():
    from openjph_amd import codec
    name = "B"
    params = case_params(name, 0.01)
    frame = case_frame(name, Plan(params))
    t = cc.QUAL["cases"][name]["targets"]["40"]
    plain = codec.Encoder(params).encode(frame)
    enc = codec.Encoder(params, min_psnr=40, cap_bytes=0)
    assert enc.cap_bytes == 0
    cs = enc.encode(frame)
    assert sha(cs) == t["sha256"] and enc.quality_info()["grid_index"] == t["certified"][0]
    with pytest.raises(capi.OjphError):
        enc.capped_info()
    lib = capi.lib()
    assert lib.ojphgpu_encoder_set_quality_capped(enc._h, t["max_sse"], 0) == capi.OK      # the C call itself
    assert enc.encode(frame) == cs and enc.quality_info()["grid_index"] == t["certified"][0]
    enc.set_quality(min_psnr=40, cap_bytes=rc.budgets(name)[0][0])
    bound = enc.encode(frame)
    assert enc.capped_info()["outcome"] == cc.BY_BUDGET and len(bound) <= rc.budgets(name)[0][0]
    enc.set_quality(min_psnr=40)                                 # the cap goes, the target stays
    assert enc.encode(frame) == cs
    enc.set_quality()                                            # both off
    assert enc.max_sse is None and enc.cap_bytes == 0 and enc.encode(frame) == plain


@pytest.mark.parametrize("name,dt", [("B", np.uint8), ("A", np.uint16)], ids=["B-8bit", "A-16bit"])
def test_narrow_containers(name, dt):
    from openjph_amd import codec
    params = case_params(name)
    frame = case_frame(name, Plan(params))
    inr, _, _ = rc.budgets(name)
    enc = codec.Encoder(params)
    for db, B in ((50, inr[1]), (40, inr[2])):
        T = cc.QUAL["cases"][name]["targets"][str(db)]["max_sse"]
        enc.set_quality(max_sse=T, cap_bytes=B)
        check_capped(name, enc, enc.encode(frame.astype(dt)), frame, T, B)


def test_refusals():
    import torch
    from openjph_amd import codec
    ok = dict(bit_depth=8, reversible=False)
    for kw in (dict(bit_depth=8, reversible=True), dict(ok, qfactor=85), dict(bit_depth=17, reversible=False)):
        enc = codec.Encoder(make_params(128, 128, 3, **kw))
        with pytest.raises(capi.OjphError) as e:
            enc.set_quality(max_sse=10000, cap_bytes=5000)
        assert e.value.code == capi.E_INVALID, kw
    tiled = make_params(256, 256, 1, tile=(128, 128), **ok)
    for kw in (dict(tiles=(0, 2)), dict(frames=2)):
        with pytest.raises(capi.OjphError) as e:
            codec.Encoder(tiled, **kw).set_quality(max_sse=10000, cap_bytes=5000)
        assert e.value.code == capi.E_INVALID
    enc = codec.Encoder(tiled, max_bytes=10000)                    # a byte budget at the same time, either way round
    with pytest.raises(capi.OjphError) as e:
        enc.set_quality(max_sse=10000, cap_bytes=5000)
    assert e.value.code == capi.E_INVALID
    enc = codec.Encoder(tiled, max_sse=10000, cap_bytes=50000)
    with pytest.raises(capi.OjphError) as e:
        enc.set_budget(10000)
    assert e.value.code == capi.E_INVALID
    for call in (enc.capped_info, enc.quality_info, enc.rate_info):
        with pytest.raises(capi.OjphError):
            call()                                                 # nothing coded yet
    enc.run_device(torch.zeros((1, 256, 256), dtype=torch.int32, device="cuda"))
    with pytest.raises(capi.OjphError):
        enc.finish_tiles()
    enc.finish()
    assert enc.capped_info()["outcome"] == cc.MET                  # (a flat frame: nothing is lost at any step)
    for call in (enc.quality_info, enc.rate_info):                 # ... and these two stay refused while a cap is set
        with pytest.raises(capi.OjphError) as e:
            call()
        assert e.value.code == capi.E_INVALID
    with pytest.raises(ValueError):
        codec.Encoder(tiled, cap_bytes=5000)                       # a cap without a target
    with pytest.raises(ValueError):
        enc.set_quality(cap_bytes=5000)
    with pytest.raises(ValueError):
        codec.encode(np.zeros((1, 64, 64), np.int32), cap_bytes=5000, **ok)
    with pytest.raises(ValueError):
        enc.set_quality(max_sse=1, min_psnr=40, cap_bytes=5000)
