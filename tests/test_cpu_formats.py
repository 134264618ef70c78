"""The sample formats on the CPU (no GPU needed): every bit depth from 1 to 32.
(a) a plain numpy restatement of the sample transfer -- level shift, type 3 non-linearity, RCT in int64; int <-> float with
    np.float32 one operation at a time (round to nearest, as __fmul_rn / __fadd_rn), truncation of t +- 0.5 with the depth's
    clamps, saturation to 8- / 16-bit containers -- against the oracle's conversion functions at every depth, edge values
    included.  tests/test_gpu_formats.py holds the kernels to the same restatement.
(b) the oracle pipeline against the live reference on tests/format_cases.py: same bytes, same samples at full and reduced
    resolution, the same refusals.
(c) the oracle block coder against the reference's at K_max 1-2 and 22-30, and the decoder's missing_msbs rules (28, 29, 30)."""
import numpy as np
import pytest

from tests.synth import random_block

F32 = np.float32
ALPHA_RF, ALPHA_GF, ALPHA_BF = F32(0.299), F32(0.587), F32(0.114)


# ------------------------------------------------------------------------------------------------------------------------
# (a) the restatement
# ------------------------------------------------------------------------------------------------------------------------
def sample_range(bd, signed):
    return (-(1 << (bd - 1)), (1 << (bd - 1)) - 1) if signed else (0, (1 << bd) - 1)


def half(bd, signed):
    return 0 if signed else 1 << (bd - 1)


def wrap32(v):
    return np.asarray(v, np.int64).astype(np.uint64).astype(np.uint32).view(np.int32)


def nlt3(v, bd):
    """type 3 non-linearity of a signed component (its own inverse): negative v <-> -v - 2^(B-1) - 1, in int64"""
    v = np.asarray(v, np.int64)
    return np.where(v >= 0, v, -v - ((1 << (bd - 1)) + 1))


def rev_forward(v, bd, signed, nl=False):
    """image sample -> reversible working sample (int64; the 32-bit path keeps the low 32 bits).  The sample is taken as the
    int32 an image line holds (si32): an unsigned 32-bit sample of 2^31 or more is negative there, as in the reference."""
    v = wrap32(v).astype(np.int64)
    return nlt3(v, bd) if nl else v - half(bd, signed)


def rev_inverse(v, bd, signed, nl=False):
    v = np.asarray(v, np.int64)
    return nlt3(v, bd) if nl else v + half(bd, signed)


def irv_to_float(v, bd, signed):
    """(v - half) * 2^-B: the difference in int32 (it wraps for unsigned 32-bit samples, to the right value), converted to
    float with round to nearest, one rounded multiplication"""
    d = wrap32(np.asarray(v, np.int64) - half(bd, signed)).astype(F32)
    return d * F32(2.0 ** -bd)


def irv_to_int(f, bd, signed):
    """float -> image sample: t = f * 2^B (rounded), truncation of t + 0.5 (t - 0.5 below zero, rounded), t below -2^(B-1)
    -> -2^(B-1), t at or above 2^(B-1) -> 2^(B-1) - 1, then + half (int32 arithmetic)"""
    f = np.asarray(f, F32)
    with np.errstate(over="ignore"):
        t = f * F32(2.0 ** bd)
    u = t + np.where(t >= 0, F32(0.5), F32(-0.5)).astype(F32)
    lo, hi = -(1 << (bd - 1)), (1 << (bd - 1)) - 1
    with np.errstate(invalid="ignore"):
        v = np.trunc(u.astype(np.float64)).clip(-2.0 ** 62, 2.0 ** 62).astype(np.int64)
    v = np.where(t >= F32(lo), v, lo)
    v = np.where(t < F32(-lo), v, hi)
    return wrap32(v + half(bd, signed))


def saturate(v, container, signed):
    """a sample leaving in an 8- / 16-bit container (two's complement when signed, else the container's unsigned range)"""
    if container == 32:
        return wrap32(v)
    lo, hi = (-(1 << (container - 1)), (1 << (container - 1)) - 1) if signed else (0, (1 << container) - 1)
    return np.clip(np.asarray(v, np.int64), lo, hi)


def rct_forward(r, g, b):
    r, g, b = (np.asarray(x, np.int64) for x in (r, g, b))
    return (r + 2 * g + b) >> 2, b - g, r - g


def rct_inverse(y, cb, cr):
    y, cb, cr = (np.asarray(x, np.int64) for x in (y, cb, cr))
    g = y - ((cb + cr) >> 2)
    return cr + g, g, cb + g


def ict_forward(r, g, b):
    beta_cb, beta_cr = F32(0.5 / (1 - float(ALPHA_BF))), F32(0.5 / (1 - float(ALPHA_RF)))
    y = (ALPHA_RF * r + ALPHA_GF * g) + ALPHA_BF * b
    return y, beta_cb * (b - y), beta_cr * (r - y)


def ict_inverse(y, cb, cr):
    g_cb2g = F32(2.0 * float(ALPHA_BF) * (1.0 - float(ALPHA_BF)) / float(ALPHA_GF))
    g_cr2g = F32(2.0 * float(ALPHA_RF) * (1.0 - float(ALPHA_RF)) / float(ALPHA_GF))
    g_cb2b, g_cr2r = F32(2.0 * (1.0 - float(ALPHA_BF))), F32(2.0 * (1.0 - float(ALPHA_RF)))
    return y + g_cr2r * cr, (y - g_cr2g * cr) - g_cb2g * cb, y + g_cb2b * cb


def edge_samples(bd, signed, rng, n=200):
    """the range's ends, zero, the mid-point, and random samples (true values, int64)"""
    lo, hi = sample_range(bd, signed)
    fixed = [lo, hi, 0, 1, -1, lo + 1, hi - 1, 1 << (bd - 1), (1 << (bd - 1)) - 1, -(1 << (bd - 1)), (1 << bd) - 1]
    fixed = [v for v in fixed if lo <= v <= hi]
    return np.concatenate([np.array(fixed, np.int64), rng.integers(lo, hi + 1, n, dtype=np.int64)])


def edge_floats(bd, rng, n=200):
    """working samples for the way back: ties at .5 of the sample grid, -0.0, the clamps' edges and beyond, random"""
    s = F32(2.0 ** -bd)
    k = np.concatenate([np.arange(-4, 5), rng.integers(-(1 << (bd - 1)) - 3, (1 << (bd - 1)) + 3, 40)]).astype(np.float64)
    ties = (k + 0.5).astype(F32) * s
    grid = k.astype(F32) * s
    lim = F32(2.0 ** (bd - 1)) * s
    fixed = np.array([0.0, -0.0, 0.5, -0.5, 0.49999997, -0.49999997, 0.75, -0.75, 1.0, -1.0, 3.5, -3.5, 1e30, -1e30],
                     F32)
    near = np.array([lim, -lim, np.nextafter(lim, F32(0)), np.nextafter(-lim, F32(0)), np.nextafter(lim, F32(1)),
                     np.nextafter(-lim, F32(-1))], F32)
    return np.concatenate([fixed, near, ties, grid, ((rng.random(n) - 0.5) * 1.2).astype(F32)]).astype(F32)


def _ob():
    from oracle import oraclebind as ob
    return ob


@pytest.mark.parametrize("bd", range(1, 33))
def test_restatement_matches_oracle_conversion(bd):
    """numpy restatement == ojo_rev_convert*, ojo_irv_to_float / _to_int at this depth, signed and unsigned, every edge"""
    ob = _ob()
    L = ob.lib()
    rng = np.random.default_rng(bd)
    for signed in (False, True):
        v = edge_samples(bd, signed, rng)
        src = wrap32(v)                                          # what an int32 image plane holds
        n = src.size
        # reversible, 32-bit lines (ojo_rev_convert: v + shift in 32-bit arithmetic)
        dst = np.empty(n, np.int32)
        L.ojo_rev_convert(src.ctypes.data, dst.ctypes.data, n, int(wrap32(-half(bd, signed))))
        assert np.array_equal(dst, wrap32(rev_forward(v, bd, signed))), "rev forward B=%d signed=%s" % (bd, signed)
        # reversible, 64-bit lines, with and without the type 3 non-linearity (signed components only)
        for nl in ((False, True) if signed else (False,)):
            shift = ((1 << (bd - 1)) + 1) if nl else -half(bd, signed)
            d64 = np.empty(n, np.int64)
            L.ojo_rev_convert_to64(src.ctypes.data, d64.ctypes.data, n, shift, int(nl))
            want = rev_forward(v, bd, signed, nl)
            assert np.array_equal(d64, want), "rev forward 64 B=%d signed=%s nlt3=%s" % (bd, signed, nl)
            back = np.empty(n, np.int32)
            L.ojo_rev_convert_from64(d64.ctypes.data, back.ctypes.data, n, -shift if not nl else shift, int(nl))
            assert np.array_equal(back, wrap32(rev_inverse(want, bd, signed, nl))), "rev inverse 64 B=%d" % bd
            assert np.array_equal(back, src)
        # irreversible: to float ...
        fl = np.empty(n, F32)
        L.ojo_irv_to_float(src.ctypes.data, fl.ctypes.data, n, bd, int(signed))
        assert np.array_equal(fl.view(np.uint32), irv_to_float(v, bd, signed).view(np.uint32)), "to float B=%d signed=%s" % (bd, signed)
        # ... and back, from the converted samples and from the edge cases of the way back
        for f in (fl, edge_floats(bd, rng)):
            f = np.ascontiguousarray(f, F32)
            got = np.empty(f.size, np.int32)
            L.ojo_irv_to_int(f.ctypes.data, got.ctypes.data, f.size, bd, int(signed))
            assert np.array_equal(got, irv_to_int(f, bd, signed)), "to int B=%d signed=%s" % (bd, signed)
        got = np.empty(n, np.int32)
        L.ojo_irv_to_int(fl.ctypes.data, got.ctypes.data, n, bd, int(signed))
        if bd <= 24:                                             # exact in float: the round trip is lossless
            assert np.array_equal(got, src)


@pytest.mark.parametrize("bd", range(1, 33))
def test_restatement_matches_oracle_colour(bd):
    """RCT (32- and 64-bit Y Cb Cr) and ICT: restatement == ojo_rct_* / ojo_ict_* on samples of this depth"""
    ob = _ob()
    L = ob.lib()
    rng = np.random.default_rng(100 + bd)
    for signed in (False, True):
        rgb = [rng.permutation(edge_samples(bd, signed, rng, 100)) for _ in range(3)]
        n = rgb[0].size
        w = [np.ascontiguousarray(rev_forward(x, bd, signed)) for x in rgb]      # level-shifted, int64
        w32 = [np.ascontiguousarray(wrap32(x)) for x in w]
        want = rct_forward(*w)
        y64 = [np.empty(n, np.int64) for _ in range(3)]
        L.ojo_rct_fwd64(*[x.ctypes.data for x in w32], *[x.ctypes.data for x in y64], n)
        if bd < 32:                                              # 64-bit Y Cb Cr from 32-bit R G B: exact
            assert all(np.array_equal(a, b) for a, b in zip(y64, want)), "rct fwd64 B=%d" % bd
        back = [np.empty(n, np.int32) for _ in range(3)]
        L.ojo_rct_inv64(*[x.ctypes.data for x in y64], *[x.ctypes.data for x in back], n)
        assert all(np.array_equal(a, wrap32(b)) for a, b in zip(back, rct_inverse(*y64))), "rct inv64 B=%d" % bd
        if bd <= 30:                                             # the 32-bit RCT: exact while Cb, Cr fit
            y32 = [np.empty(n, np.int32) for _ in range(3)]
            L.ojo_rct_fwd(*[x.ctypes.data for x in w32], *[x.ctypes.data for x in y32], n)
            assert all(np.array_equal(a, wrap32(b)) for a, b in zip(y32, want)), "rct fwd B=%d" % bd
            L.ojo_rct_inv(*[x.ctypes.data for x in y32], *[x.ctypes.data for x in back], n)
            assert all(np.array_equal(a, wrap32(b)) for a, b in zip(back, w)), "rct inv B=%d" % bd
        f = [np.ascontiguousarray(irv_to_float(x, bd, signed)) for x in rgb]
        ycc = [np.empty(n, F32) for _ in range(3)]
        L.ojo_ict_fwd(*[x.ctypes.data for x in f], *[x.ctypes.data for x in ycc], n)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(ycc, ict_forward(*f))), "ict fwd B=%d" % bd
        out = [np.empty(n, F32) for _ in range(3)]
        L.ojo_ict_inv(*[x.ctypes.data for x in ycc], *[x.ctypes.data for x in out], n)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(out, ict_inverse(*ycc))), "ict inv B=%d" % bd


def test_restatement_saturates_containers():
    """8- / 16-bit containers saturate at their own range; 32-bit ones keep the low 32 bits"""
    v = np.array([-70000, -32769, -32768, -129, -128, -1, 0, 255, 256, 32767, 32768, 65535, 65536, 1 << 31], np.int64)
    assert saturate(v, 16, True).tolist() == [-32768, -32768, -32768, -129, -128, -1, 0, 255, 256, 32767, 32767, 32767, 32767, 32767]
    assert saturate(v, 16, False).tolist() == [0, 0, 0, 0, 0, 0, 0, 255, 256, 32767, 32768, 65535, 65535, 65535]
    assert saturate(v, 8, True).tolist() == [-128, -128, -128, -128, -128, -1, 0, 127, 127, 127, 127, 127, 127, 127]
    assert saturate(v, 8, False).tolist() == [0, 0, 0, 0, 0, 0, 0, 255, 255, 255, 255, 255, 255, 255]
    assert saturate(v, 32, False)[-1] == -(1 << 31)


# ------------------------------------------------------------------------------------------------------------------------
# (b) whole codestreams against the reference
# ------------------------------------------------------------------------------------------------------------------------
def reference_for(kw, ref, refgen):
    """the 5/3 alone: the SIMD build; anything with the 9/7 in it: the generic build (the SIMD 9/7 rounds differently)"""
    irv = not kw["reversible"] or any(not st.get("reversible", False) for st in (kw.get("coc") or {}).values())
    return refgen if irv else ref


N_RANDOM = 120


@pytest.mark.parametrize("chunk", range(4))
def test_format_cases_match_live_reference(chunk, ref, refgen):
    """tests/format_cases.py: the oracle pipeline emits the reference's bytes, decodes them to the reference's samples at full
    and reduced resolution, and refuses what it refuses.  ATK codestreams come from this
    repository's writer (the reference reads ATK marker segments only): the reference decodes them to the same samples."""
    from openjph_amd import capi
    from tests import cpu_pipeline as cp
    from tests.format_cases import all_cases
    cases = all_cases(N_RANDOM)[chunk::4]
    compared = 0
    for name, planes, kw, size in cases:
        if any(q.size == 0 for q in planes):
            continue
        lib = reference_for(kw, ref, refgen)
        try:
            got, *_ = cp.encode(planes, size=size, **kw)
        except capi.OjphError:
            got = None
        if kw.get("atk"):
            assert got is not None, name
            want = got
        else:
            k2 = dict(kw)
            bd, sg = k2.pop("bit_depth"), k2.pop("is_signed")
            try:
                want = lib.encode(planes, bd, is_signed=sg, size=size, **k2)
            except RuntimeError:
                want = None
            assert (want is None) == (got is None), "%s: %s" % (name, kw)
            if want is None:
                continue
            assert got == want, "%s: %s" % (name, kw)
        dec, _ = cp.decode(want)
        rdec, _ = lib.decode(want)
        for c in range(len(planes)):
            assert np.array_equal(dec[c], rdec[c]), "%s component %d: %s" % (name, c, kw)
        nd = min([kw.get("num_decomps", 5)] + [st.get("num_decomps", 5) for st in (kw.get("coc") or {}).values()])
        if nd >= 1:
            skip = 1 + compared % nd
            dec, _ = cp.decode(want, skip=(skip, skip))
            rdec, _ = lib.decode(want, skip=(skip, skip))
            for c in range(len(planes)):
                assert np.array_equal(dec[c], rdec[c]), "%s skip %d component %d: %s" % (name, skip, c, kw)
        compared += 1
    assert compared >= len(cases) * 3 // 4


def test_format_cases_cover_the_depths():
    """the generator reaches every depth from 1 to 32, signed and unsigned, the 64-bit path beside the 32-bit one, the
    fused conversion's edge depths 25-26 and 32-bit-path K_max up to 30"""
    from openjph_amd.plan import Plan, make_params
    from tests.format_cases import all_cases
    depths, wide_mix, kmax32 = set(), 0, set()
    for name, planes, kw, size in all_cases(N_RANDOM):
        p = Plan(make_params(size[0], size[1], len(planes), **kw))
        styles = [p.comp_style(c) for c in range(len(planes))]
        depths |= {(bd, sg) for bd, sg in zip(kw["bit_depths"], kw["signs"])}
        wide_mix += any(s["wide"] for s in styles) and not all(s["wide"] for s in styles)
        kmax32 |= {int(b["K_max"]) for b in p.bands if not styles[int(b["comp"])]["wide"]}
    assert {bd for bd, _ in depths} == set(range(1, 33))
    assert sum(1 for bd, sg in depths if sg) >= 24 and sum(1 for bd, sg in depths if not sg) >= 24
    assert wide_mix >= 5
    assert max(kmax32) >= 29 and {20, 22, 24, 26, 28} <= kmax32


# ------------------------------------------------------------------------------------------------------------------------
# (c) the block coder at the edges of the 32-bit path
# ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 64), (32, 32), (17, 64), (64, 17), (5, 7), (4, 1024), (1024, 4), (63, 63), (128, 32), (1, 1), (8, 8), (2, 64)]
HIGH_K = [1, 2] + list(range(22, 31))


def high_k_block(rng, w, h, kmax, full=False):
    """sign-magnitude samples with up to K_max magnitude bits (the top one set somewhere), stride w"""
    dens = 1.0 if full else float(rng.choice([0.05, 0.4, 1.0]))
    amp = (1 << kmax) - 1
    sm, v = random_block(rng, w, h, w, kmax, dens, amp if full or rng.random() < 0.7 else max(1, amp >> int(rng.integers(1, kmax + 1))))
    if not np.any(v):
        v[0, 0] = amp
    v.reshape(-1)[int(rng.integers(0, w * h))] = -amp                    # the largest magnitude, negative
    sm = (((v < 0).astype(np.uint64) << 31) | (np.abs(v).astype(np.uint64) << (31 - kmax))).astype(np.uint32)
    return sm, v


@pytest.mark.parametrize("kmax", HIGH_K)
def test_block_coder_at_high_and_low_K_max_matches_reference(kmax, ref):
    """oracle encoder == reference encoder, oracle decoder == reference decoders (generic and AVX2), every block shape"""
    ob = _ob()
    rng = np.random.default_rng(700 + kmax)
    for i, (w, h) in enumerate(SHAPES):
        sm, v = high_k_block(rng, w, h, kmax, full=i % 3 == 0)
        want = ref.encode_block(sm, kmax - 1, w, h, w)
        assert ob.ht_encode(sm, w, h, w, kmax - 1) == want, "K_max %d %dx%d" % (kmax, w, h)
        ok, dec = ob.ht_decode(want, w, h, w, kmax - 1)
        assert ok and np.array_equal(ob.dequant_rev(dec, kmax), v), "K_max %d %dx%d: not lossless" % (kmax, w, h)
        st = (w + 7) & ~7                                        # (the reference's decoders store whole groups of 8)
        for variant in (0, 1):
            okr, decr = ref.decode_block(want, kmax - 1, w, h, st, variant=variant)
            assert okr and np.array_equal(decr[:, :w], dec), "K_max %d %dx%d variant %d" % (kmax, w, h, variant)


@pytest.mark.parametrize("mm", [27, 28, 29, 30])
def test_block_decoder_missing_msbs_edges_match_reference(mm, ref):
    """missing_msbs 28 decodes its refinement passes, 29 drops them (the cleanup pass alone), 30 and beyond reject the block
    (block_decoder32's tests): 1-3 passes, causal and not, the oracle's verdict and samples == the reference's"""
    ob = _ob()
    rng = np.random.default_rng(900 + mm)
    kmax = min(mm + 1, 30)
    n_ok = 0
    for i, (w, h) in enumerate(SHAPES):
        sm, v = high_k_block(rng, w, h, kmax, full=i % 4 == 0)
        cup = ob.ht_encode(sm, w, h, w, kmax - 1)
        tail = bytes(rng.integers(0, 256, size=int(rng.integers(1, 300)), dtype=np.uint8))
        for npass in (1, 2, 3):
            for causal in (False, True):
                data, len2 = (cup, 0) if npass == 1 else (cup + tail, len(tail))
                ok, dec = ob.ht_decode(data, w, h, w, mm, len2=len2, num_passes=npass, stripe_causal=causal)
                for variant in (0, 1):
                    okr, decr = ref.decode_block(data, mm, w, h, (w + 7) & ~7, len2=len2, num_passes=npass, variant=variant,
                                                 stripe_causal=causal)
                    assert ok == okr, "mm %d %dx%d passes %d causal %s variant %d" % (mm, w, h, npass, causal, variant)
                    if ok:
                        assert np.array_equal(dec[:, :w], decr[:, :w]), "mm %d %dx%d passes %d causal %s" % (mm, w, h, npass, causal)
                if mm == 29 and npass > 1 and ok:                # the refinement passes are not read
                    ok1, dec1 = ob.ht_decode(cup, w, h, w, mm)
                    assert ok1 and np.array_equal(dec[:, :w], dec1[:, :w])
                n_ok += ok
    assert (n_ok == 0) == (mm >= 30)
