"""RGB <-> YCbCr (include/ojphgpu.h section 7e) without a device: the library's table against the numpy statement, entry
for entry; what the green-coefficient rule promises (grey -> mid chroma, black and white -> the ends of the luma range);
forward then inverse; the decimating and interpolating statements against a brute-force float evaluation of the same taps
with the REAL matrix."""
import itertools

import numpy as np
import pytest

from openjph_amd import codec, pipeline

STANDARDS = ("bt601", "bt709", "bt2020")
RANGES = ("full", "narrow")
DEPTHS = (8, 10, 12, 16)
# what rounding a coefficient moves it by, in units of 2^-16: a rounded one half a unit; forward green, the rounded total
# minus two rounded ones, three halves
FWD_COEF_ERR = (0.5, 1.5, 0.5)


def real_matrix(standard, direction, rgb_depth, ycc_depth, rgb_range, ycc_range):
    """the unrounded statement: out = M . in + o, in doubles, written independently of pipeline.colour_table"""
    Kr, Kb = pipeline.COLOUR_STANDARDS[standard]
    Kg = 1.0 - Kr - Kb
    o_rgb, s_rgb, _, _ = pipeline.colour_range(rgb_depth, rgb_range)
    o_y, s_y, o_c, s_c = pipeline.colour_range(ycc_depth, ycc_range)
    A = np.array([[Kr, Kg, Kb], [-Kr, -Kg, 1 - Kb], [1 - Kr, -Kg, -Kb]], np.float64)
    A[1] /= 2 * (1 - Kb)
    A[2] /= 2 * (1 - Kr)
    S = np.diag([s_y, s_c, s_c]) / float(s_rgb)
    F = S @ A                                                      # ycc = F (rgb - o_rgb) + o_ycc
    o_ycc = np.array([o_y, o_c, o_c], np.float64)
    if direction == "forward":
        return F, o_ycc - F @ np.full(3, float(o_rgb))
    Fi = np.linalg.inv(F)
    return Fi, np.full(3, float(o_rgb)) - Fi @ o_ycc


def test_c_table_equals_numpy_table():
    n = 0
    for std, direction, rr, yr, rd, yd in itertools.product(STANDARDS, ("forward", "inverse"), RANGES, RANGES, DEPTHS, DEPTHS):
        want = pipeline.colour_table(std, direction, rd, yd, rr, yr)
        got = codec.colour_table(std, direction, rd, yd, rr, yr)
        assert got == want, (std, direction, rr, yr, rd, yd, got, want)
        assert want.k == 16 and want.lo == (0, 0, 0) and want.hi == ((1 << (yd if direction == "forward" else rd)) - 1,) * 3
        assert all(abs(x) < 2 ** 31 for r in want.m for x in r)
        n += 1
    assert n == 3 * 2 * 4 * 16


def test_table_is_close_to_the_real_matrix():
    """every coefficient within its rounding of the real one (the inverse: the closed form IS the matrix inverse), every
    offset within what the coefficients' roundings move it by"""
    for std, direction, rr, yr, rd, yd in itertools.product(STANDARDS, ("forward", "inverse"), RANGES, RANGES, DEPTHS, DEPTHS):
        t = pipeline.colour_table(std, direction, rd, yd, rr, yr)
        M, o = real_matrix(std, direction, rd, yd, rr, yr)
        err = np.abs(np.array(t.m, np.float64) - M * 65536.0)
        tol = np.array([FWD_COEF_ERR] * 3) if direction == "forward" else np.full((3, 3), 0.5)
        assert (err <= tol + 1e-6).all(), (std, direction, rr, yr, rd, yd, err)
        if direction == "inverse":
            assert t.m[0][1] == 0 and t.m[2][2] == 0 and t.m[0][0] == t.m[1][0] == t.m[2][0]
        assert (np.abs(np.array(t.off, np.float64) / 65536.0 - o) <= 4.0 * (1 << max(rd, yd)) / 65536.0 + 1e-6).all()


def test_table_refusals():
    with pytest.raises(ValueError):
        pipeline.colour_table("bt470", "forward", 8, 8)
    with pytest.raises(ValueError):
        pipeline.colour_table("bt709", "sideways", 8, 8)
    for rd, yd in ((7, 8), (8, 17), (0, 8)):
        with pytest.raises(ValueError):
            pipeline.colour_table("bt709", "forward", rd, yd)
        with pytest.raises(codec.capi.OjphError) as e:
            codec.colour_table("bt709", "forward", rd, yd)
        assert e.value.code == codec.capi.E_INVALID
    L = codec.capi.lib()
    t = codec.capi.ColourTable()
    for args in ((600, 0, 8, 8, 0, 0), (709, 2, 8, 8, 0, 0), (709, 0, 8, 8, 2, 0), (709, 0, 8, 8, 0, -1)):
        assert L.ojphgpu_colour_table_make(*args, t) == codec.capi.E_INVALID
    assert L.ojphgpu_colour_table_make(709, 0, 8, 8, 0, 0, None) == codec.capi.E_INVALID


@pytest.mark.parametrize("std", STANDARDS)
def test_grey_black_and_white_are_exact(std):
    """the green-coefficient rule: every grey gives exactly mid chroma, black and white exactly the luma range's ends"""
    for rr, yr, rd, yd in itertools.product(RANGES, RANGES, DEPTHS, DEPTHS):
        t = pipeline.colour_table(std, "forward", rd, yd, rr, yr)
        top = (1 << rd) - 1
        grey = np.unique(np.concatenate([np.arange(0, min(top, 1023) + 1), np.linspace(0, top, 257).astype(np.int64), [top - 1, top]]))[None, :]
        y, cb, cr = pipeline.rgb_to_ycc([grey, grey, grey], t)
        mid = 1 << (yd - 1)
        assert (cb == mid).all() and (cr == mid).all(), (std, rr, yr, rd, yd)
        o_rgb, s_rgb, _, _ = pipeline.colour_range(rd, rr)
        o_y, s_y, _, _ = pipeline.colour_range(yd, yr)
        ends = np.array([[o_rgb, o_rgb + s_rgb]])
        y = pipeline.rgb_to_ycc([ends, ends, ends], t)[0]
        assert y.tolist() == [[o_y, o_y + s_y]], (std, rr, yr, rd, yd, y)
        assert all(sum(r) == 0 for r in t.m[1:])


def _nominal_rgb(rng, depth, rrange, n):
    """greys, the cube's corners and random triples inside the nominal RGB range -> three [1, N] planes"""
    o, s, _, _ = pipeline.colour_range(depth, rrange)
    corners = np.array(list(itertools.product((o, o + s), repeat=3))).T
    greys = np.linspace(o, o + s, 64).astype(np.int64)
    rnd = rng.integers(o, o + s + 1, size=(3, n))
    v = np.concatenate([corners, np.stack([greys] * 3), rnd], axis=1)
    return [v[i][None, :] for i in range(3)]


def roundtrip_bound(fwd, inv, depth):
    """what forward-then-inverse at 4:4:4 may move a sample of the nominal RGB range by, from the two tables alone.  The two
    real matrices are each other's inverse, so the error is what the roundings add: a YCbCr sample is off by its own
    rounding (1/2) and by the forward coefficients' roundings on samples below 2^depth; the inverse spreads that by the
    absolute row sums of its matrix, and adds its own coefficients' roundings on samples below 2^depth and its own 1/2."""
    top = float(1 << depth)
    e_ycc = 0.5 + sum(FWD_COEF_ERR) * top / 65536.0
    return max(0.5 + sum(abs(x) / 65536.0 * e_ycc + (0.5 * top / 65536.0 if x else 0.0) for x in inv.m[c]) for c in range(3))


def test_forward_then_inverse_is_within_the_tables_bound():
    rng = np.random.default_rng(5)
    worst = {}
    for std, rr, yr, depth in itertools.product(STANDARDS, RANGES, RANGES, DEPTHS):
        fwd = pipeline.colour_table(std, "forward", depth, depth, rr, yr)
        inv = pipeline.colour_table(std, "inverse", depth, depth, rr, yr)
        rgb = _nominal_rgb(rng, depth, rr, 4000)
        back = pipeline.ycc_to_rgb(pipeline.rgb_to_ycc(rgb, fwd), inv)
        err = max(int(np.abs(b - a).max()) for a, b in zip(rgb, back))
        bound = roundtrip_bound(fwd, inv, depth)
        worst[(depth, rr, yr)] = max(worst.get((depth, rr, yr), 0), err)
        assert err <= bound, (std, rr, yr, depth, err, bound)
    for key in sorted(worst):
        print("round trip, depth %2d, RGB %-6s YCbCr %-6s: at most %d LSB" % (key + (worst[key],)))


def _brute_forward(rgb, M, o, fx, fy):
    """float: the real matrix per pixel, then per output sample the taps (1, 2, 1) / 4 around source sample (fx i, fy j),
    indices clamped -- sample by sample"""
    h, w = rgb[0].shape
    t = [sum(M[c][i] * rgb[i].astype(np.float64) for i in range(3)) + o[c] for c in range(3)]
    out = [t[0]]
    cw, ch = (w + 1) // 2 if fx == 2 else w, (h + 1) // 2 if fy == 2 else h
    for c in (1, 2):
        q = np.zeros((ch, cw))
        for j in range(ch):
            for i in range(cw):
                ys = [(fy * j + d, wt) for d, wt in ((-1, 0.25), (0, 0.5), (1, 0.25))] if fy == 2 else [(j, 1.0)]
                xs = [(fx * i + d, wt) for d, wt in ((-1, 0.25), (0, 0.5), (1, 0.25))] if fx == 2 else [(i, 1.0)]
                q[j, i] = sum(wy * wx * t[c][min(max(yy, 0), h - 1), min(max(xx, 0), w - 1)] for yy, wy in ys for xx, wx in xs)
        out.append(q)
    return out


def _brute_inverse(ycc, M, o, fx, fy):
    """float: per luma sample the chroma under it -- C[x / 2] for even x, the mean of C[(x - 1) / 2] and C[min((x + 1) / 2,
    cw - 1)] for odd x, rows alike -- then the real matrix"""
    y, cb, cr = [p.astype(np.float64) for p in ycc]
    h, w = y.shape
    ch, cw = cb.shape
    out = [np.zeros((h, w)) for _ in range(3)]
    for r in range(h):
        for x in range(w):
            ys = [r] if fy == 1 else [r // 2] if r % 2 == 0 else [(r - 1) // 2, min((r + 1) // 2, ch - 1)]
            xs = [x] if fx == 1 else [x // 2] if x % 2 == 0 else [(x - 1) // 2, min((x + 1) // 2, cw - 1)]
            v = [y[r, x]] + [sum(q[a, b] for a in ys for b in xs) / (len(ys) * len(xs)) for q in (cb, cr)]
            for c in range(3):
                out[c][r, x] = M[c] @ np.array(v) + o[c]
    return out


@pytest.mark.parametrize("fx,fy", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_stages_against_brute_force_float(fx, fy):
    """within 0.5 LSB (the one rounding) plus what the coefficients' roundings move a sum of samples below 2^depth by"""
    rng = np.random.default_rng(fx * 10 + fy)
    for std, (rd, yd), (rr, yr), (h, w) in itertools.product(STANDARDS, ((8, 10), (10, 10), (16, 12)), (("full", "narrow"), ("narrow", "full")),
                                                              ((1, 1), (5, 7), (4, 6))):
        o_rgb, s_rgb, _, _ = pipeline.colour_range(rd, rr)
        rgb = [rng.integers(o_rgb, o_rgb + s_rgb + 1, size=(h, w)) for _ in range(3)]
        t = pipeline.colour_table(std, "forward", rd, yd, rr, yr)
        M, o = real_matrix(std, "forward", rd, yd, rr, yr)
        got = pipeline.rgb_to_ycc(rgb, t, fx, fy)
        want = _brute_forward(rgb, M, o, fx, fy)
        tol = 0.5 + sum(FWD_COEF_ERR) * (1 << rd) / 65536.0 + 1e-6
        cw, ch = (w + 1) // 2 if fx == 2 else w, (h + 1) // 2 if fy == 2 else h
        assert [g.shape for g in got] == [(h, w), (ch, cw), (ch, cw)]
        for g, q in zip(got, want):
            assert np.abs(g - np.clip(q, 0, (1 << yd) - 1)).max() <= tol, (std, rd, yd, rr, yr, h, w)
        # the inverse, on the planes the forward statement made
        ti = pipeline.colour_table(std, "inverse", rd, yd, rr, yr)
        Mi, oi = real_matrix(std, "inverse", rd, yd, rr, yr)
        goti = pipeline.ycc_to_rgb(got, ti, fx, fy)
        wanti = _brute_inverse(got, Mi, oi, fx, fy)
        toli = 0.5 + 3 * 0.5 * (1 << yd) / 65536.0 + 1e-6
        for g, q in zip(goti, wanti):
            assert g.shape == (h, w)
            assert np.abs(g - np.clip(q, 0, (1 << rd) - 1)).max() <= toli, (std, rd, yd, rr, yr, h, w)


def test_statement_refusals_and_wrapping_sums():
    t = pipeline.colour_table("bt709", "forward", 8, 8)
    p = np.zeros((2, 2), np.int64)
    for fx, fy in ((0, 1), (1, 3), (4, 1)):
        with pytest.raises(ValueError):
            pipeline.rgb_to_ycc([p, p, p], t, fx, fy)
        with pytest.raises(ValueError):
            pipeline.ycc_to_rgb([p, p, p], t, fx, fy)
    with pytest.raises(ValueError):
        pipeline.rgb_to_ycc([p, p, p], t._replace(k=15))
    with pytest.raises(ValueError):
        pipeline.ycc_to_rgb([p, p[:1], p[:1]], t, 2, 1)
    # a hostile table: the sums are 64-bit two's complement, as Python's integers reduced to 64 bits
    h = pipeline.ColourTable(((2 ** 31 - 1, -(2 ** 31 - 1), 2 ** 30), (-(2 ** 31 - 1), 2 ** 31 - 1, 12345), (2 ** 31 - 1,) * 3),
                             (2 ** 62, -(2 ** 61), -7), (0, 5, 0), (2 ** 31 - 1, 1000, 70000), 16)
    a = [np.array([[4294967295, 7, 65535]]), np.array([[1, 4294967295, 65535]]), np.array([[4294967295, 4294967295, 0]])]
    got = pipeline.rgb_to_ycc(a, h)
    for c in range(3):
        for i in range(3):
            s = sum(h.m[c][k] * int(a[k][0, i]) for k in range(3)) + h.off[c] + (1 << 15)
            s = ((s + 2 ** 63) % 2 ** 64 - 2 ** 63) >> 16
            assert got[c][0, i] == min(max(s, h.lo[c]), h.hi[c])


# ---- the plan judgement of the pipes' set_video_colour (ojphgpu_video_colour_fit): what needs no device
from tests.colour_cases import C, H, PLAN_REFUSALS, W  # noqa: E402


def _plan(depth=10, rev=True, cell=(1, 1), w=W, h=H, **kw):
    from tests.video_cases import make_plan
    return make_plan(w, h, depth, rev, cell, num_decomps=2, **kw)


@pytest.mark.parametrize("decoding", [False, True])
def test_plan_judgement_refusals(decoding):
    from openjph_amd import capi
    for fmt, colour, container, kw in PLAN_REFUSALS:
        plan = _plan(**kw)                              # (the plan itself is a valid one)
        with pytest.raises(capi.OjphError) as e:
            pipeline.video_colour_fit(plan, fmt, colour, container, decoding)
        assert e.value.code == capi.E_INVALID, (fmt, colour, container, kw)
    L, plan = capi.lib(), _plan(cell=(2, 1))
    good = capi.ColourSpec(709, 0, 1, 0)
    assert L.ojphgpu_video_colour_fit(plan.handle, 16, decoding, 0x23, good, None, None, None) == capi.OK
    for bad in (capi.ColourSpec(710, 0, 1, 0), capi.ColourSpec(0, 0, 1, 0), capi.ColourSpec(709, 2, 1, 0), capi.ColourSpec(709, 0, -1, 0),
                capi.ColourSpec(709, 0, 1, 11), capi.ColourSpec(709, 0, 1, 4)):
        assert L.ojphgpu_video_colour_fit(plan.handle, 16, decoding, 0x23, bad, None, None, None) == capi.E_INVALID   # standard, range, RGB depth
    assert L.ojphgpu_video_colour_fit(plan.handle, 16, decoding, 0x23, None, None, None, None) == capi.E_INVALID      # no spec
    assert L.ojphgpu_video_colour_fit(None, 16, decoding, 0x23, good, None, None, None) == capi.E_INVALID
    for container in (0, 12, 64):
        assert L.ojphgpu_video_colour_fit(plan.handle, container, decoding, 0x23, good, None, None, None) == capi.E_INVALID
    for code in (0, 0x20, 0x2A, 0x03, 0x13):
        assert L.ojphgpu_video_colour_fit(plan.handle, 16, decoding, code, good, None, None, None) == capi.E_INVALID
    # a decoder pipe's 32-bit planes are int32: refused there, taken by an encoder pipe
    assert (L.ojphgpu_video_colour_fit(plan.handle, 32, decoding, 0x23, good, None, None, None) == capi.E_INVALID) == decoding


@pytest.mark.parametrize("decoding", [False, True])
def test_plan_judgement_passes_444_422_420(decoding):
    direction = "inverse" if decoding else "forward"
    for cell, (w, h) in itertools.product(((1, 1), (2, 1), (1, 2), (2, 2)), ((66, 34), (37, 19), (1, 1))):
        for fmt, colour, container, depth, rgb_depth in (("r210", "bt709", 16, 10, 10), ("bgra", C("bt601", rgb_depth=8), 16, 10, 8),
                                                         ("rgba", C("bt2020", "narrow", "full"), 8, 8, 8), ("r10k", C("bt709", rgb_depth=8), 16, 16, 8),
                                                         ("argb", "bt709", 16, 8, 8)):
            col = colour if isinstance(colour, C) else C(colour)
            got = pipeline.video_colour_fit(_plan(depth=depth, cell=cell, w=w, h=h), fmt, colour, container, decoding)
            assert got["table"] == pipeline.colour_table(col.standard, direction, rgb_depth, depth, col.rgb_range, col.ycc_range)
            assert (got["fx"], got["fy"]) == cell and got["bytes"] == pipeline.video444_layout(fmt, w, h)[1]
    # an even image offset keeps phase 0; a colour transform over a 4:4:4 plan is the plan's business
    pipeline.video_colour_fit(_plan(cell=(2, 2), image_offset=(2, 4)), "r210", "bt709", 16, decoding)
    pipeline.video_colour_fit(_plan(cell=(2, 1), image_offset=(0, 1)), "r210", "bt709", 16, decoding)
    pipeline.video_colour_fit(_plan(color_transform=True), "r210", "bt709", 16, decoding)
