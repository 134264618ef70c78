"""CPU-side gates (run with -m "not gpu"; no GPU needed):

 1. the C-ABI library loads and exports every symbol include/ojphgpu.h declares;
 2. the ORACLE (oracle/ht_oracle.c, our restatement of the reference's hot path) reproduces the
    reference's outputs stored in tests/golden/ (made by tests/golden/make_golden.py from the real
    reference build) and -- where oracle/_ref/*.so is present -- the live reference;
 3. the product's HOST logic (plan geometry + Tier-2 writer/parser behind the C ABI), glued to the
    oracle's stages by tests/cpu_pipeline.py, emits codestreams byte-identical to the reference's.

Nothing here exercises a HIP kernel; those are the `-m gpu` tests.
"""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from tests.golden_cases import (BLOCK_CASES, COC_CASES, coc_case, NLT_CASES, nlt_case, CQF_CASES, cqf_case, FORMAT_CASES, GRID_CASES, REFINE_CASES, SKIP_CASES, STREAM_CASES, TILEPART_CASES,
                                format_case, grid_kwargs, refine_case, skip_case, stream_kwargs, tilepart_case)
from tests.synth import c1_image, ka2_block, random_block, synth_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
GOLD_BLOBS = np.load(os.path.join(ROOT, "tests", "golden", "golden_blocks.npz"))


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


# ------------------------------------------------------------------------------------------------
# 1. C ABI
# ------------------------------------------------------------------------------------------------
def test_abi_exports_every_declared_symbol():
    from openjph_amd import capi
    hdr = open(os.path.join(ROOT, "include", "ojphgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ojphgpu_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 30
    L = C.CDLL(capi.LIB_PATH)
    missing = [n for n in sorted(declared) if not hasattr(L, n)]
    assert not missing, "libojphgpu.so does not export: %s" % missing
    unbound = declared - set(capi.SIGNATURES)
    assert not unbound, "capi.py does not bind: %s" % sorted(unbound)
    assert capi.lib().ojphgpu_version().decode().startswith("openjph_amd")


def test_device_entry_points_fail_loudly_without_gpu():
    """No CPU fallback: without a GPU the codec objects raise instead of computing on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from openjph_amd import codec
    with pytest.raises(RuntimeError):
        codec.encode(c1_image(), bit_depth=8)


def test_params_validation():
    from openjph_amd.plan import Plan, make_params
    from openjph_amd.capi import OjphError
    for bad in (dict(width=0, height=10), dict(width=10, height=10, num_decomps=33),
                dict(width=10, height=10, block=(3, 64)), dict(width=10, height=10, block=(2048, 2)),
                dict(width=10, height=10, block=(128, 128)), dict(width=10, height=10, bit_depth=0)):
        with pytest.raises(OjphError):
            Plan(make_params(**bad))


# ------------------------------------------------------------------------------------------------
# 2. oracle vs reference (golden + live)
# ------------------------------------------------------------------------------------------------
def test_ka2_block_oracle_matches_golden():
    from oracle import oraclebind as ob
    buf = ka2_block()
    b = ob.ht_encode(buf, 64, 64, 64, 9)
    assert len(b) == 3900 == GOLD["ka2"]["len"]
    assert sha(b) == GOLD["ka2"]["sha256"]
    assert b == GOLD_BLOBS["ka2"].tobytes()
    ok, dec = ob.ht_decode(b, 64, 64, 64, 9)
    assert ok
    K = 10
    centre = np.where(buf & 0x7FFFFFFF, np.uint32(1 << (30 - K)), np.uint32(0))
    assert np.array_equal(dec, buf | centre)               # bin-centre bit on non-zero samples


def _block_case(i):
    w, h, kmax, density, amp, seed = BLOCK_CASES[i]
    rng = np.random.default_rng(seed)
    stride = (w + 15) // 16 * 16
    q, _ = random_block(rng, w, h, stride, kmax, density, amp)
    q[:, w:] = 0
    return q, w, h, stride, kmax


@pytest.mark.parametrize("i", range(len(BLOCK_CASES)))
def test_block_oracle_matches_golden(i):
    from oracle import oraclebind as ob
    q, w, h, stride, kmax = _block_case(i)
    g = GOLD["blocks"][i]
    b = ob.ht_encode(q, w, h, stride, kmax - 1)
    assert len(b) == g["len"] and sha(b) == g["sha256"]
    key = "block%d" % i
    if key in GOLD_BLOBS:
        assert b == GOLD_BLOBS[key].tobytes()
    ok, dec = ob.ht_decode(b, w, h, stride, kmax - 1)
    assert ok and sha(np.ascontiguousarray(dec[:, :w]).tobytes()) == g["dec_sha256"]


@pytest.mark.parametrize("i", range(len(BLOCK_CASES)))
def test_block_oracle_matches_live_reference(i, ref):
    from oracle import oraclebind as ob
    q, w, h, stride, kmax = _block_case(i)
    want = ref.encode_block(q, kmax - 1, w, h, stride)
    assert ob.ht_encode(q, w, h, stride, kmax - 1) == want
    for variant in (0, 1):                                   # generic and AVX2 reference decoders
        okr, decr = ref.decode_block(want, kmax - 1, w, h, stride, variant=variant)
        ok, dec = ob.ht_decode(want, w, h, stride, kmax - 1)
        assert ok and okr and np.array_equal(dec[:, :w], decr[:, :w])


@pytest.mark.parametrize("i", range(len(REFINE_CASES)))
def test_refinement_passes_oracle_matches_golden(i):
    """SigProp + MagRef (ojph_block_decoder32.cpp:1318-1609): random refinement bytes behind a
    cleanup pass; the reference's decode of them is stored in tests/golden."""
    from oracle import oraclebind as ob
    q, w, h, stride, kmax, npass, causal, tail = refine_case(i)
    cup = ob.ht_encode(q, w, h, stride, kmax - 1)
    ok, dec = ob.ht_decode(cup + tail, w, h, stride, kmax - 1, len2=len(tail), num_passes=npass, stripe_causal=causal)
    assert ok and sha(np.ascontiguousarray(dec[:, :w]).tobytes()) == GOLD["refine"][i]["dec_sha256"]


def test_refinement_passes_oracle_matches_live_reference(ref):
    from oracle import oraclebind as ob
    rng = np.random.default_rng(123)
    shapes = [(64, 64), (32, 32), (17, 64), (64, 17), (5, 7), (4, 1024), (1024, 4), (63, 63), (128, 32), (1, 1)]
    for it in range(60):
        w, h = shapes[it % len(shapes)]
        st = (w + 7) & ~7
        kmax = int(rng.integers(3, 20))
        sm, v = random_block(rng, w, h, w, kmax, float(rng.choice([0.02, 0.2, 0.6])), int(min(2 ** kmax - 1, rng.choice([3, 40, 700]))))
        if not np.any(v[:, :w]):
            continue
        cup = ob.ht_encode(sm, w, h, w, kmax - 1)
        tail = bytes(rng.integers(0, 256, size=int(rng.integers(1, 400)), dtype=np.uint8))
        for npass in (2, 3):
            for causal in (False, True):
                for variant in (0, 1):
                    okr, decr = ref.decode_block(cup + tail, kmax - 1, w, h, st, len2=len(tail), num_passes=npass,
                                                 variant=variant, stripe_causal=causal)
                    ok, dec = ob.ht_decode(cup + tail, w, h, st, kmax - 1, len2=len(tail), num_passes=npass,
                                           stripe_causal=causal)
                    assert ok == okr and np.array_equal(dec[:, :w], decr[:, :w])


def test_multi_pass_codestream_matches_live_reference(refgen):
    """A codestream whose blocks carry SigProp / MagRef segments (built with the product's Tier-2
    writer from random refinement bytes): the reference library decodes it to the same image."""
    from tests import cpu_pipeline as cp
    rng = np.random.default_rng(5)
    for kw in (dict(bit_depth=8), dict(bit_depth=10, reversible=False, qstep=0.004, tile=(128, 128))):
        img = synth_image(1 if "tile" in kw else 3, 200, 260, kw["bit_depth"], seed=2)
        cs0, plan, arena, data, coded = cp.encode(img, **kw)
        data2, coded2 = cp.add_refinement(data, coded, rng)
        cs = plan.t2_write(data2, coded2)
        assert len(cs) > len(cs0)
        want, _ = refgen.decode(cs)
        got, plan2 = cp.decode(cs)
        assert int((plan2.coded_blocks()["num_passes"] > 1).sum()) > 10
        assert np.array_equal(got, want)


def _foreign():
    import hashlib, json
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "foreign.json")))
    rd = lambda e: open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", e["file"]), "rb").read()
    sha = lambda a: hashlib.sha256(a if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a).tobytes()).hexdigest()
    return g, rd, sha


def test_foreign_codestream_of_the_reference_tree():
    """tests/golden/foreign_test.j2c = the reference tree's subprojects/js/html/test.j2c (a foreign encoder's stream:
    per-resolution precincts, ICT, 77 blocks with SigProp / MagRef passes): the oracle decodes what the reference's
    generic build decodes (digest by tests/golden/make_foreign.py; the live library is asked too where it is built)."""
    from tests import cpu_pipeline as cp
    from oracle import refbind
    g, rd, sha = _foreign()
    cs = rd(g["test_j2c"])
    assert sha(cs) == g["test_j2c"]["sha256"]                    # the fixture IS the tree's file (its digest, by make_foreign.py)
    got, plan = cp.decode(cs)
    assert int((plan.coded_blocks()["num_passes"] > 1).sum()) == g["test_j2c"]["blocks_with_refinement_passes"] == 77
    assert sha(got.astype(np.int32)) == g["test_j2c"]["decoded_sha256_generic"]
    if refbind.available(generic=True):
        want, _ = refbind.Ref(generic=True).decode(cs)
        assert np.array_equal(got, want)


def test_encoder_fuzz_seed_of_the_reference_tree():
    """tests/golden/fuzz_seed_*.bin = the seed of the reference's encoder fuzz target (128x128, 2 components, 12-bit
    signed, 5/3, ONE decomposition, planar): the oracle pipeline writes the codestream the reference writes"""
    from tests import cpu_pipeline as cp
    from tests.golden_cases import fuzz_seed_case
    from oracle import refbind
    g, rd, sha = _foreign()
    img, kw = fuzz_seed_case(rd(g["fuzz_seed"]))
    assert kw == g["fuzz_seed"]["params"] and sha(img) == g["fuzz_seed"]["image_sha256"]
    okw = {k: v for k, v in kw.items() if k != "planar"}
    cs, *_ = cp.encode(img, **okw)
    assert len(cs) == g["fuzz_seed"]["bytes"] and sha(cs) == g["fuzz_seed"]["sha256"]
    dec, _ = cp.decode(cs)
    assert np.array_equal(dec, img)
    if refbind.available():
        assert refbind.Ref().encode(img, kw["bit_depth"], is_signed=True, reversible=True, num_decomps=1, planar=True) == cs


def test_decoder_rejects_what_the_reference_rejects(ref):
    """Corrupt / truncated cleanup segments: same accept/reject verdict and, when accepted, the
    same samples as ojph_decode_codeblock32 (ojph_block_decoder32.cpp:752-819, :1114, :1224)."""
    from oracle import oraclebind as ob
    q, w, h, stride, kmax = _block_case(0)
    good = ob.ht_encode(q, w, h, stride, kmax - 1)
    rng = np.random.default_rng(99)
    trials = [good[:1], good[:2], good[:len(good) // 2], good[:-1], b"\x00\x00", b"\xff\xff\xff\xff"]
    for _ in range(40):
        b = bytearray(good)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        trials.append(bytes(b))
    agree = 0
    for t in trials:
        okr, decr = ref.decode_block(t, kmax - 1, w, h, stride)
        ok, dec = ob.ht_decode(t, w, h, stride, kmax - 1)
        assert ok == okr
        if ok:
            assert np.array_equal(dec[:, :w], decr[:, :w])
            agree += 1
    assert agree >= 1


# ------------------------------------------------------------------------------------------------
# 3. host logic (plan + Tier-2) + oracle stages == reference codestream
# ------------------------------------------------------------------------------------------------
def test_c1_codestream_is_the_reference_codestream():
    """BASELINE config #1 (KA-1): 256x256 8-bit, 5/3, defaults -> 54 702 bytes."""
    from tests import cpu_pipeline as cp
    cs, *_ = cp.encode(c1_image(), bit_depth=8)
    assert len(cs) == 54702 == GOLD["ka1"]["len"]
    assert sha(cs) == GOLD["ka1"]["sha256"]
    dec, _ = cp.decode(cs)
    assert np.array_equal(dec, c1_image())


@pytest.mark.parametrize("i", range(len(STREAM_CASES)), ids=lambda i: "case%d" % i)
def test_codestream_matches_golden(i):
    from tests import cpu_pipeline as cp
    img, kw = stream_kwargs(STREAM_CASES[i])
    g = GOLD["streams"][i]
    cs, *_ = cp.encode(img, **kw)
    assert len(cs) == g["len"], "codestream size %d, reference %d" % (len(cs), g["len"])
    assert sha(cs) == g["sha256"]
    dec, _ = cp.decode(cs)
    assert sha(dec.astype(np.int32).tobytes()) == g["dec_sha256"]
    if kw.get("reversible", True):
        assert np.array_equal(dec, img)


@pytest.mark.parametrize("i", [0, 1, 4, 5, 17, 18, 20])
def test_codestream_matches_live_reference(i, ref, refgen):
    from tests import cpu_pipeline as cp
    img, kw = stream_kwargs(STREAM_CASES[i], seed=11)
    r = ref if kw.get("reversible", True) else refgen       # 9/7 is pinned on the generic build
    want = r.encode(img, **kw)
    cs, *_ = cp.encode(img, **kw)
    assert cs == want
    dec, _ = cp.decode(want)
    wdec, _ = r.decode(want)
    assert np.array_equal(dec, wdec)


def _planes_bytes(planes):
    return b"".join(np.ascontiguousarray(q, dtype=np.int32).tobytes() for q in planes)


def _as_list(dec, n):
    return [dec[c] for c in range(n)]


@pytest.mark.parametrize("i", range(len(GRID_CASES)), ids=lambda i: "grid%d" % i)
def test_grid_codestream_matches_golden(i):
    """Sub-sampled components, image offsets and tile offsets: plan geometry + Tier-2 + oracle stages
    against the stored reference codestreams (ojph_codestream_local.cpp:113-163, ojph_tile.cpp:253-289)."""
    from tests import cpu_pipeline as cp
    planes, kw, size = grid_kwargs(GRID_CASES[i])
    g = GOLD["grid"][i]
    cs, plan, *_ = cp.encode(planes, size=size, **kw)
    assert len(cs) == g["len"], "codestream size %d, reference %d" % (len(cs), g["len"])
    assert sha(cs) == g["sha256"]
    assert [(c["h"], c["w"]) for c in (plan.comp_info(k) for k in range(len(planes)))] == [q.shape for q in planes]
    dec, _ = cp.decode(cs)
    dec = _as_list(dec, len(planes))
    assert sha(_planes_bytes(dec)) == g["dec_sha256"]
    if kw.get("reversible", True):
        assert all(np.array_equal(a, b) for a, b in zip(dec, planes))


@pytest.mark.parametrize("i", [0, 2, 5, 6])
def test_grid_codestream_matches_live_reference(i, ref, refgen):
    from tests import cpu_pipeline as cp
    planes, kw, size = grid_kwargs(GRID_CASES[i], seed=12)
    r = ref if kw.get("reversible", True) else refgen
    want = r.encode(planes, size=size, **kw)
    cs, *_ = cp.encode(planes, size=size, **kw)
    assert cs == want
    dec, _ = cp.decode(want)
    wdec, _ = r.decode(want)
    assert all(np.array_equal(a, b) for a, b in zip(_as_list(dec, len(planes)), _as_list(wdec, len(planes))))


@pytest.mark.parametrize("i", range(len(SKIP_CASES)), ids=lambda i: "%s%d-skip%d_%d" % SKIP_CASES[i])
def test_reduced_resolution_decode_matches_golden(i):
    """codestream::restrict_input_resolution (ojph_codestream_local.cpp:883-900): resolutions that are
    not read decode as zeros, resolutions that are not reconstructed shrink the output"""
    from tests import cpu_pipeline as cp
    planes, kw, size, skip = skip_case(i)
    cs, *_ = cp.encode(planes if size else np.stack(planes), **(dict(kw, size=size) if size else kw))
    dec, _ = cp.decode(cs, skip=skip)
    dec = _as_list(dec, len(planes))
    g = GOLD["skip"][i]
    assert [list(d.shape) for d in dec] == g["shapes"]
    assert sha(_planes_bytes(dec)) == g["dec_sha256"]


def test_reduced_resolution_validation():
    from openjph_amd import capi
    from openjph_amd.plan import Plan, make_params, parse_codestream
    from tests import cpu_pipeline as cp
    cs, *_ = cp.encode(synth_image(1, 64, 64, 8, seed=1), bit_depth=8, num_decomps=3)
    pl = parse_codestream(cs)
    with pytest.raises(capi.OjphError):
        pl.restrict_resolution(1, 2)                      # data < recon (:886)
    with pytest.raises(capi.OjphError):
        pl.restrict_resolution(4, 4)                      # more than the decomposition levels (:891)
    with pytest.raises(capi.OjphError):
        Plan(make_params(64, 64, 1)).restrict_resolution(1, 1)   # not a parsed codestream
    pl.restrict_resolution(3, 1)
    assert pl.frame_shape == (1, 32, 32)


def _truncation_image():
    y, x = np.mgrid[0:256, 0:256]                              # the image of tests/test_truncated_decode.cpp:107-113
    return ((x * 7 + y * 13 + ((x * y) >> 3)) & 0xFF).astype(np.int32)[None]


TRUNC_PARAMS = [dict(), dict(tile=(128, 128)), dict(prog_order="LRCP", precinct=(64, 64)),
                dict(tile=(100, 100), prog_order="CPRL"), dict(num_decomps=2, block=(32, 32), prog_order="PCRL", precinct=(128, 128))]


@pytest.mark.parametrize("k", range(len(TRUNC_PARAMS)))
def test_truncated_codestreams_behave_like_the_reference(k, ref):
    """The reference's tests/test_truncated_decode.cpp, made stricter: at every cut the parser must
    raise exactly when the reference raises (a cut in an SOT, a tile-part header or a packet header
    without resilience; ojph_codestream_local.cpp:912-1113, ojph_tile.cpp:777-935) and otherwise
    reconstruct the very same image from what was received (ojph_precinct.cpp:530-560)."""
    from openjph_amd import capi
    from openjph_amd.plan import parse_codestream
    from tests import cpu_pipeline as cp
    img = _truncation_image()
    kw = dict(dict(num_decomps=5), **TRUNC_PARAMS[k])
    cs = ref.encode(img, 8, reversible=True, **kw)
    sot = cs.find(b"\xff\x90")                                 # every byte of the first SOT segment and its neighbourhood as well
    cuts = sorted(set([len(cs) * c // 16 for c in range(1, 16)] + list(range(2, 330, 9)) + list(range(sot - 2, sot + 16)) +
                      [len(cs) - 1, len(cs) - 2, len(cs) - 3]))
    detected = 0
    for n in cuts:
        part = cs[:n]
        for resilient in (False, True):
            try:
                want, _ = ref.decode(part, resilient=resilient)
            except RuntimeError:
                want = None
            try:
                pl = parse_codestream(part, resilient=resilient)
                got = cp.inverse_stages(pl, cp.decode_blocks(pl, part))
            except capi.OjphError:
                got = None
            assert (want is None) == (got is None), "cut at %d of %d, resilient=%s" % (n, len(cs), resilient)
            if want is not None:
                assert np.array_equal(got, want), "cut at %d of %d, resilient=%s" % (n, len(cs), resilient)
            detected += want is None
    assert detected > 0


@pytest.mark.parametrize("i", range(len(TILEPART_CASES)), ids=lambda i: "%s-%s" % TILEPART_CASES[i][:2])
def test_tilepart_divisions_match_golden(i):
    """tile::flush with tile-part divisions (ojph_tile.cpp:584-774) and the TLM entries per tile-part
    (:529-580); what a progression order cannot honour is dropped (ojph_codestream_local.cpp:582-620)"""
    from tests import cpu_pipeline as cp
    img, kw = tilepart_case(i)
    g = GOLD["tileparts"][i]
    cs, plan, *_ = cp.encode(img, **kw)
    assert len(cs) == g["len"] and sha(cs) == g["sha256"]
    dec, _ = cp.decode(cs)                                  # the parser walks the tile-parts back
    if kw.get("reversible", True):
        assert np.array_equal(dec, img)


def test_tileparts_comments_profile_match_live_reference(ref):
    from openjph_amd import capi
    from openjph_amd.plan import Plan, make_params
    from tests import cpu_pipeline as cp
    img = synth_image(3, 150, 200, 8, seed=7)
    for po in ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL"):
        for tp in ("R", "C", "RC"):
            kw = dict(bit_depth=8, prog_order=po, tileparts=tp, tile=(96, 96), tlm=True)
            cs, *_ = cp.encode(img, **kw)
            assert cs == ref.encode(img, **kw), (po, tp)
    plan = Plan(make_params(200, 150, 3, bit_depth=8))
    plan.set_comments(["a comment", b"\x00\x01binary"])
    data, coded = cp.encode_blocks(plan, cp.forward_stages(plan, img))
    got = plan.t2_write(data, coded)
    assert b"a comment" in got[:400] and b"\x00\x01binary" in got[:400]
    plan.set_comments(["a comment"])
    assert plan.t2_write(data, coded) == ref.encode(img, 8, com="a comment")
    with pytest.raises(capi.OjphError):                      # 40 components x 7 resolutions > 255 tile-parts
        Plan(make_params(64, 64, 40, num_decomps=6, prog_order="LRCP", tileparts="RC"))


@pytest.mark.parametrize("i", range(len(FORMAT_CASES)), ids=lambda i: "fmt%d" % i)
def test_component_formats_and_qfactor_match_golden(i):
    """components of different bit depth / signedness get their own QCC (ojph_params.cpp:1411-1432);
    the qfactor mode derives visually weighted steps and a QCC for every component (:1378-1407,
    :1553-1599).  Marker segments, K_max / step sizes and the per-component level shift are all
    pinned here against the reference's codestreams."""
    from tests import cpu_pipeline as cp
    planes, kw, size = format_case(i)
    g = GOLD["formats"][i]
    cs, plan, *_ = cp.encode(planes, size=size, **kw)
    assert len(cs) == g["len"] and sha(cs) == g["sha256"]
    dec, _ = cp.decode(cs)
    dec = _as_list(dec, len(planes))
    assert sha(_planes_bytes(dec)) == g["dec_sha256"]
    if kw.get("reversible", True):
        assert all(np.array_equal(a, b) for a, b in zip(dec, planes))


@pytest.mark.parametrize("i", range(len(COC_CASES)), ids=lambda i: "coc%d" % i)
def test_component_coding_styles_match_golden(i):
    """COC marker segments (param_cod's comp_idx setters, ojph_params.cpp:255-282): a component with
    its own decompositions / block size / precincts / wavelet.  Pinned against the reference's
    codestreams: marker order (COD, COCs in creation order, QCD made for the first component without
    a COC, QCCs where is_qcc_needed says so), packet sequences when components run out of resolutions,
    tile-part numbering with gaps, and the decoded samples (also at reduced resolution).  Case 0 is
    the reference's own tests/test_mixed_coc.cpp."""
    from tests import cpu_pipeline as cp
    from openjph_amd.plan import parse_codestream
    planes, kw, size, skip, resilient = coc_case(i)
    g = GOLD["coc"][i]
    cs, plan, *_ = cp.encode(planes, size=size, **kw)
    assert len(cs) == g["len"] and sha(cs) == g["sha256"]
    for c, st in kw["coc"].items():
        got = plan.comp_style(c)
        assert got["has_coc"] and got["reversible"] == bool(st.get("reversible", False)) and got["num_decomps"] == st.get("num_decomps", 5)
    pl = parse_codestream(cs, resilient=resilient)
    for c in range(len(planes)):                            # what read_headers reports per component (test_mixed_coc.cpp:139-150)
        assert pl.comp_style(c) == plan.comp_style(c)
    if skip:
        pl.restrict_resolution(*skip)
    dec = _as_list(cp.inverse_stages(pl, cp.decode_blocks(pl, cs)), len(planes))
    assert [list(d.shape) for d in dec] == g["shapes"]
    assert sha(_planes_bytes(dec)) == g["dec_sha256"]
    if not skip:
        for c in range(len(planes)):                        # a reversibly coded component comes back exactly
            if plan.comp_style(c)["reversible"] and not (kw.get("color_transform") and c < 3 and not kw.get("reversible", True)):
                assert np.array_equal(dec[c], planes[c]), c


@pytest.mark.parametrize("i", range(len(NLT_CASES)), ids=lambda i: "nlt%d" % i)
def test_nonlinearity_type3_matches_golden(i):
    """NLT marker segments (param_nlt, ojph_params.cpp:2087-2266) and the type 3 non-linearity on signed
    components (negative v <-> -v - 2^(B-1) - 1 around the level shift / float conversion,
    ojph_colour.cpp:273-311, :344-352, :406-412; ojph_tile.cpp:352-365, :446-460): which segments the
    library writes for an ALL_COMPS request over components of one or of several formats, Rsiz flags,
    coded bytes and decoded samples, against the reference's codestreams."""
    from tests import cpu_pipeline as cp
    planes, kw, size = nlt_case(i)
    g = GOLD["nlt"][i]
    cs, plan, *_ = cp.encode(planes, size=size, **kw)
    assert len(cs) == g["len"] and sha(cs) == g["sha256"]
    assert any(plan.comp_style(c)["nlt3"] for c in range(len(planes)))
    dec, pl = cp.decode(cs)
    dec = _as_list(dec, len(planes))
    assert [pl.comp_style(c)["nlt3"] for c in range(len(planes))] == [plan.comp_style(c)["nlt3"] for c in range(len(planes))]
    assert sha(_planes_bytes(dec)) == g["dec_sha256"]
    for c in range(len(planes)):
        if plan.comp_style(c)["reversible"] and not (kw.get("color_transform") and c < 3 and not kw.get("reversible", True)):
            assert np.array_equal(dec[c], planes[c]), c


@pytest.mark.parametrize("i", range(len(CQF_CASES)), ids=lambda i: "cqf%d" % i)
def test_component_quality_factors_match_golden(i):
    """param_qcd::set_qfactor(comp_idx, ctype, qfactor) (ojph_params.cpp:2021-2035): a QCC per named
    component with its own visual weights; marker order (user-made QCCs first), the component the QCD
    is made for, and the interplay with the top-level qfactor, qstep and COCs against the reference"""
    from tests import cpu_pipeline as cp
    img, kw = cqf_case(i)
    g = GOLD["cqf"][i]
    cs, plan, *_ = cp.encode(img, **kw)
    assert len(cs) == g["len"] and sha(cs) == g["sha256"]
    dec, _ = cp.decode(cs)
    assert sha(np.ascontiguousarray(dec, dtype=np.int32).tobytes()) == g["dec_sha256"]


def test_absurd_sizes_are_refused_not_fatal():
    """nothing leaves the C ABI as a C++ exception: a frame no device could hold, or tables the host
    cannot allocate, come back as a status (the process used to die in std::bad_alloc)"""
    from openjph_amd import capi
    from openjph_amd.plan import Plan, make_params
    for w, h, kw in [(1 << 31, 1 << 31, dict(block=(4, 4))), (4000000, 4000000, dict(block=(4, 4), num_decomps=0)),
                     (1 << 20, 1 << 20, dict(tile=(4096, 4096)))]:
        with pytest.raises(capi.OjphError):
            Plan(make_params(w, h, 1, **kw))


def test_parser_survives_mutated_codestreams():
    """a few hundred random mutations (bit flips, overwritten / removed / inserted bytes, cuts; mostly
    in the main header) of codestreams with tiles, tile-parts, COC and NLT segments: the parser returns a
    plan or an error, in both modes, and every code-block it reports lies inside the buffer"""
    import random
    from openjph_amd import capi
    from openjph_amd.plan import parse_codestream
    from tests import cpu_pipeline as cp
    img = synth_image(3, 70, 90, 8, seed=1)
    seeds = [bytes(cp.encode(img, bit_depth=8, **kw)[0]) for kw in (
        dict(), dict(reversible=False, qstep=0.05), dict(tile=(32, 32), tlm=True, prog_order="CPRL", tileparts="C"),
        dict(color_transform=True, precinct=(32, 32), prog_order="PCRL"))]
    for i in (0, 2, 5):
        pl, kw, size, _, _ = coc_case(i)
        seeds.append(bytes(cp.encode(pl, size=size, **kw)[0]))
    pl, kw, size = nlt_case(1)
    seeds.append(bytes(cp.encode(pl, size=size, **kw)[0]))
    rng = random.Random(7)
    parsed = refused = 0
    for _ in range(400):
        b = bytearray(rng.choice(seeds))
        hdr_end = b.find(b"\xff\x90")
        for _ in range(rng.randint(1, 4)):
            pos = min(rng.randrange(2, hdr_end + 40) if rng.random() < 0.7 else rng.randrange(len(b)), len(b) - 1)
            mode = rng.random()
            if mode < 0.5:
                b[pos] ^= 1 << rng.randrange(8)
            elif mode < 0.7:
                b[pos] = rng.randrange(256)
            elif mode < 0.8:
                del b[pos:pos + rng.randint(1, 8)]
            elif mode < 0.9:
                b[pos:pos] = bytes(rng.randrange(256) for _ in range(rng.randint(1, 8)))
            else:
                b = b[:max(pos, 4)]
            if len(b) < 4:
                break
        for resilient in (False, True):
            try:
                p = parse_codestream(bytes(b), resilient=resilient)
            except capi.OjphError:
                refused += 1
                continue
            parsed += 1
            cb = p.coded_blocks()
            if len(cb):
                assert int((cb["offset"].astype(np.int64) + cb["len1"] + cb["len2"]).max()) <= len(b)
    assert parsed > 50 and refused > 50


def test_nlt_validation():
    from openjph_amd import capi
    from openjph_amd.plan import Plan, make_params, parse_codestream
    from tests import cpu_pipeline as cp
    with pytest.raises(ValueError):
        make_params(64, 64, 1, nlt={0: 1})                   # gamma style: not in the reference either
    with pytest.raises(ValueError):
        make_params(64, 64, 20, nlt={16: 3})
    # unsigned components: the segment is written, nothing changes in the samples
    img = np.arange(64 * 64, dtype=np.int32).reshape(1, 64, 64) % 251
    a, pa, *_ = cp.encode(img, bit_depth=8, nlt={"all": 3})
    b, *_ = cp.encode(img, bit_depth=8)
    assert not pa.comp_style(0)["nlt3"] and len(a) == len(b) + 8 and a[6:8] == b"\xc2\x00" and b[6:8] == b"\x40\x00"
    # a BDnlt that contradicts the SIZ marker segment is refused (ojph_tile.cpp:292-299)
    k = a.find(b"\xff\x76")
    bad = bytearray(a); bad[k + 6] ^= 0x80
    with pytest.raises(capi.OjphError):
        parse_codestream(bytes(bad))


def test_coc_validation_and_gapped_tile_parts():
    from openjph_amd import capi
    from openjph_amd.plan import Plan, make_params, parse_codestream
    from tests import cpu_pipeline as cp
    with pytest.raises(capi.OjphError):                     # colour transform over components of different wavelets (ojph_tile.cpp:147-163)
        Plan(make_params(64, 64, 3, color_transform=True, reversible=True, coc={1: dict(reversible=False)}))
    with pytest.raises(capi.OjphError):
        Plan(make_params(64, 64, 2, coc={1: dict(num_decomps=33)}))
    with pytest.raises(capi.OjphError):
        Plan(make_params(64, 64, 2, coc={1: dict(block=(2048, 2))}))
    with pytest.raises(ValueError):
        make_params(64, 64, 20, coc={17: dict(num_decomps=1)})
    # RC tile-parts of components with different decompositions leave gaps in the tile-part numbers:
    # the reference refuses its own codestream ("wrong tile part index") unless it reads resiliently
    planes, kw, size, _, _ = coc_case(5)
    cs, *_ = cp.encode(planes, size=size, **kw)
    with pytest.raises(capi.OjphError):
        parse_codestream(cs)
    assert parse_codestream(cs, resilient=True).num_blocks > 0
    # reduced resolution beyond what a component has is refused (the reference's arithmetic wraps there)
    planes, kw, size, _, _ = coc_case(4)                     # component 2 has no decomposition at all
    cs, *_ = cp.encode(planes, size=size, **kw)
    pl = parse_codestream(cs)
    with pytest.raises(capi.OjphError):
        pl.restrict_resolution(1, 1)


def test_qfactor_validation():
    from openjph_amd import capi
    from openjph_amd.plan import Plan, make_params
    with pytest.raises(capi.OjphError):
        Plan(make_params(64, 64, 1, reversible=False, qfactor=101))
    with pytest.raises(capi.OjphError):                     # 4:1:1-like sampling has no weight table
        Plan(make_params(64, 64, 3, reversible=False, qfactor=50, downsampling=[(1, 1), (4, 1), (4, 1)]))
    with pytest.raises(capi.OjphError):                     # the colour transform needs one sample format
        Plan(make_params(64, 64, 3, color_transform=True, bit_depths=[8, 10, 8]))
    pl = Plan(make_params(64, 64, 3, bit_depths=[8, 12, 8], signs=[False, True, False]))
    assert [pl.comp_format(c) for c in range(3)] == [(8, False), (12, True), (8, False)]


def test_grid_parameter_validation():
    """the reference's SIZ rules (ojph_params_local.h:235-249) and the colour-transform rule (:455-480)"""
    from openjph_amd import capi
    from openjph_amd.plan import Plan, make_params
    with pytest.raises(capi.OjphError):
        Plan(make_params(64, 64, 1, image_offset=(2, 2), tile_offset=(3, 0)))          # tile offset > image offset
    with pytest.raises(capi.OjphError):
        Plan(make_params(64, 64, 1, image_offset=(40, 0), tile=(32, 32)))              # first tile misses the image
    with pytest.raises(capi.OjphError):
        Plan(make_params(64, 64, 3, color_transform=True, downsampling=[(1, 1), (2, 2), (2, 2)]))
    pl = Plan(make_params(64, 64, 3, downsampling=[(1, 1), (2, 2), (2, 2)]))
    assert pl.frame_shape == (64 * 64 + 2 * 32 * 32,)
    assert Plan(make_params(64, 64, 3)).frame_shape == (3, 64, 64)


def test_oracle_equals_reference_on_sparse_blocks(ref):
    """the planes of tests/test_gpu_codec.py::test_encoder_mel_regimes (long runs of empty quads, isolated significant
    samples at fixed and random distances: the MEL coder's regimes, ojph_block_encoder.cpp:317-362) through the oracle
    pipeline and through the reference: the same codestream"""
    from tests import cpu_pipeline as cp
    from tests.test_gpu_codec import _sparse_plane
    for kind in ("one-late", "every1", "every2", "every3", "every7", "every33", "every100", "every1000", "p4", "p20", "p150", "p2000", "bands"):
        for bd, h, w, block in ((10, 128, 192, (64, 64)), (8, 70, 130, (32, 32)), (12, 64, 256, (128, 32))):
            img = _sparse_plane(kind, h, w, bd, seed=len(kind) + bd)
            kw = dict(bit_depth=bd, num_decomps=0, block=block)
            assert cp.encode(img, **kw)[0] == ref.encode(img, **kw), (kind, bd)


def test_irreversible_tolerance_vs_simd_reference(ref):
    """9/7 against the SIMD build of the reference (which is not bit-stable against its own generic
    build): same rule as the reference's tests (tests/test_executables.cpp:132-133): MSE within 1 %,
    PAE within 1, and codestream size within 0.01 %."""
    from tests import cpu_pipeline as cp
    img = synth_image(3, 240, 320, 12, seed=5)
    kw = dict(bit_depth=12, reversible=False, qstep=0.001)
    want = ref.encode(img, **kw)
    cs, *_ = cp.encode(img, **kw)
    assert abs(len(cs) - len(want)) <= max(16, 1e-4 * len(want))
    a, _ = cp.decode(cs)
    b, _ = ref.decode(want)

    def stats(x):
        e = x.astype(np.int64) - img
        return float((e * e).mean()), int(np.abs(e).max())
    (m1, p1), (m2, p2) = stats(a), stats(b)
    assert abs(m1 - m2) <= 0.01 * m2 + 1e-9 and abs(p1 - p2) <= 1
    c, _ = cp.decode(want)                                  # decoder vs decoder on the same stream
    assert int(np.abs(c.astype(np.int64) - b).max()) <= 1


def test_parser_rejects_malformed_codestreams():
    from tests import cpu_pipeline as cp
    from openjph_amd.plan import parse_codestream
    from openjph_amd.capi import OjphError
    cs, *_ = cp.encode(synth_image(1, 64, 64, 8, seed=1), bit_depth=8)
    for bad in (b"", cs[:1], cs[:20], b"\x00" + cs[1:], cs[:2] + b"\xff\x00" + cs[4:]):
        with pytest.raises(OjphError):
            parse_codestream(bad)


def test_plan_geometry_block_counts():
    """6 321 blocks for C2, 24 669 for C3, 259 per 1024x1024 tile for C4."""
    from openjph_amd.plan import Plan, make_params
    assert Plan(make_params(3840, 2160, 3, bit_depth=8, color_transform=True)).num_blocks == 6321
    assert Plan(make_params(7680, 4320, 3, bit_depth=12, reversible=False, qstep=0.001)).num_blocks == 24669
    p = Plan(make_params(4096, 2048, 1, bit_depth=16, tile=(1024, 1024)))
    assert p.num_tiles == 8 and p.num_blocks == 8 * 259
    assert Plan(make_params(256, 256, 1, bit_depth=8)).num_blocks == 25


@pytest.mark.parametrize("chunk", range(4))
def test_random_coc_parameter_sets_match_live_reference(chunk, refgen):
    """80 seeded random parameter sets with COC marker segments on random components
    (tests/random_cases.py: random_coc_case): same bytes as the reference, same samples, the same
    refusals -- also of its own codestreams when RC tile-parts leave gaps in the numbering"""
    from openjph_amd import capi
    from tests import cpu_pipeline as cp
    from tests.random_cases import random_coc_case
    compared = 0
    for seed in range(chunk * 20, chunk * 20 + 20):
        planes, kw, size = random_coc_case(seed)
        if any(q.size == 0 for q in planes):
            continue
        k2 = dict(kw)
        bd, sg = k2.pop("bit_depth"), k2.pop("is_signed")
        try:
            want = refgen.encode(planes, bd, is_signed=sg, size=size, **k2)
        except RuntimeError:
            want = None
        try:
            got, *_ = cp.encode(planes, size=size, **kw)
        except capi.OjphError:
            got = None
        assert (want is None) == (got is None), "seed %d: %s" % (seed, kw)
        if want is None:
            continue
        assert got == want, "seed %d: %s" % (seed, kw)
        try:
            rdec, _ = refgen.decode(want)
        except RuntimeError:
            rdec = None
        try:
            dec, _ = cp.decode(want)
        except capi.OjphError:
            dec = None
        assert (rdec is None) == (dec is None), "seed %d: %s" % (seed, kw)
        if rdec is None:
            continue
        assert all(np.array_equal(dec[c], rdec[c]) for c in range(len(planes))), "seed %d" % seed
        compared += 1
    assert compared >= 8


@pytest.mark.parametrize("chunk", range(6))
def test_random_parameter_sets_match_live_reference(chunk, ref, refgen):
    """120 seeded random parameter sets (tests/random_cases.py): the oracle pipeline + plan + Tier-2
    emit the reference's bytes, decode to the reference's samples, and reject what it rejects"""
    from openjph_amd import capi
    from tests import cpu_pipeline as cp
    from tests.random_cases import random_case
    compared = 0
    for seed in range(chunk * 20, chunk * 20 + 20):
        planes, kw, size = random_case(seed)
        if any(q.size == 0 for q in planes):
            continue
        lib = ref if kw["reversible"] else refgen
        k2 = dict(kw)
        bd, sg = k2.pop("bit_depth"), k2.pop("is_signed")
        try:
            want = lib.encode(planes, bd, is_signed=sg, size=size, **k2)
        except RuntimeError:
            want = None
        try:
            got, *_ = cp.encode(planes, size=size, **kw)
        except capi.OjphError:
            got = None
        assert (want is None) == (got is None), "seed %d: %s" % (seed, kw)
        if want is None:
            continue
        assert got == want, "seed %d: %s" % (seed, kw)
        dec, _ = cp.decode(want)
        rdec, _ = lib.decode(want)
        assert all(np.array_equal(dec[c], rdec[c]) for c in range(len(planes))), "seed %d" % seed
        compared += 1
    assert compared >= 12


def test_damaged_codestreams_are_read_like_the_reference(refgen):
    """a few seconds of tools/fuzz_flip_cpu.py: codestreams of random parameter sets with one to three bytes changed behind the
    first SOD (packet headers, code-block bytes, SOT segments), read with and without resilience -- the live reference's verdict
    and its image (profiles/r04_b_flip_fuzz.txt)"""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_flip_cpu
    assert fuzz_flip_cpu.main(seconds=8.0, seed=600000, header=False) == 0


def test_damaged_main_headers_are_read_like_the_reference(refgen):
    """the same with the changed bytes in the main header (a worker process stands in for the cases the reference spins on);
    seeds whose known deviations are listed in DESIGN.md section 8 are not among these"""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_flip_cpu
    assert fuzz_flip_cpu.main(seconds=10.0, seed=630000, header=True, sources=4) == 0
