"""The sample formats on the GPU: every bit depth from 1 to 32, signed and unsigned, the type 3 non-linearity, both wavelets in
one frame, the colour transform, containers of 8, 16 and 32 bits, and the block coder at the top of the 32-bit path.
Stages are compared bit for bit (uint32 views) with the numpy restatement of tests/test_cpu_formats.py and with the oracle,
both pinned to the reference there; whole codestreams (tests/format_cases.py) with the oracle pipeline."""
import numpy as np
import pytest

from tests import test_cpu_formats as rs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _params(**kw):
    from openjph_amd.plan import make_params
    return make_params(8, 8, **kw)


def _to_container(v, container):
    """true sample values -> the bits an image container holds (low 8 / 16 / 32 bits)"""
    bits = np.asarray(v, np.int64).astype(np.uint64)
    return {32: bits.astype(np.uint32).view(np.int32), 16: bits.astype(np.uint16).view(np.int16),
            8: bits.astype(np.uint8).view(np.int8)}[container]


def _from_container(raw, container, signed):
    raw = np.asarray(raw)
    if container == 32:
        return raw.astype(np.int64)
    return raw.astype(np.int64) if signed else raw.view(np.uint16 if container == 16 else np.uint8).astype(np.int64)


def _containers(depths):
    return [c for c in (32, 16, 8) if max(depths) <= (31 if c == 32 else c)] if max(depths) <= 31 else [32]


# ------------------------------------------------------------------------------------------------------------------------
# conversion kernels (ojphgpu_convert_forward_ex / _inverse_ex)
# ------------------------------------------------------------------------------------------------------------------------
def _conv_forward_want(v, bd, sg, rev, nl, wide):
    """-> the arena's 32-bit words of the converted plane (two per sample on the 64-bit path)"""
    if rev and wide:
        return rs.rev_forward(v, bd, sg, nl).astype(np.int64).view(np.uint32)
    if rev:
        return rs.wrap32(rs.rev_forward(v, bd, sg, nl)).view(np.uint32)
    x = rs.wrap32(rs.nlt3(rs.wrap32(v).astype(np.int64), bd)) if nl else v
    return rs.irv_to_float(x, bd, sg).view(np.uint32)


def _conv_inverse_want(a, bd, sg, rev, nl, wide, container):
    """arena words -> the samples the container receives (true values)"""
    if rev and wide:
        v = a.view(np.int64)
        out = rs.nlt3(v, bd) if nl else v + rs.half(bd, sg)
        return rs.saturate(rs.wrap32(out).astype(np.int64), container, sg)
    if rev:
        v = rs.wrap32(a.view(np.int32).astype(np.int64) + rs.half(bd, sg)).astype(np.int64)
    else:
        v = rs.irv_to_int(a.view(np.float32), bd, sg).astype(np.int64)
    if nl:
        v = rs.wrap32(rs.nlt3(v, bd)).astype(np.int64)
    return rs.saturate(v, container, sg)


FORMATS = [(bd, sg, rev, nl) for bd in range(1, 33) for sg in (False, True) for rev in (True, False) for nl in ((False, True) if sg else (False,))]


@pytest.mark.parametrize("container", [32, 16, 8])
def test_convert_kernels_every_format(container):
    """every depth / sign / wavelet / NLT3 / 64-bit-path combination whose samples fit the container, as components of one
    launch (each with its own fmt); the inverse gets working samples that overshoot the range"""
    from openjph_amd import codec
    rng = np.random.default_rng(container)
    comps = [(bd, sg, rev, nl, rev and bd >= 28) for (bd, sg, rev, nl) in FORMATS if bd <= container]
    h, w = 3, 97
    descs = np.zeros(len(comps), codec.convert_desc_dtype)
    img_vals, img_off, arena_off = [], 0, 0
    for i, (bd, sg, rev, nl, wide) in enumerate(comps):
        d = descs[i]
        d["plane_off"], d["pitch"], d["w"], d["h"] = arena_off, w + 3, w, h
        d["img_pitch"], d["img_off"] = w, img_off
        d["fmt"] = bd | (0x100 if sg else 0) | 0x200 | (0x400 if rev else 0) | (0x800 if nl else 0) | (0x1000 if wide else 0)
        img_vals.append(rs.edge_samples(bd, sg, rng, h * w)[:h * w].reshape(h, w))
        img_off += h * w
        arena_off += (w + 3) * h * (2 if wide else 1) + 16
    image = np.concatenate([_to_container(v, container).ravel() for v in img_vals])
    params = _params(num_comps=len(comps), bit_depth=min(max(c[0] for c in comps), container))
    arena = torch.zeros(arena_off + 64, dtype=torch.int32, device="cuda")
    codec.convert("forward", params, descs, torch.from_numpy(image).cuda(), arena, w, h, container)
    got = arena.cpu().numpy().view(np.uint32)
    for i, (bd, sg, rev, nl, wide) in enumerate(comps):
        d = descs[i]
        n = 2 if wide else 1
        plane = got[int(d["plane_off"]):int(d["plane_off"]) + (w + 3) * h * n].reshape(h, (w + 3) * n)[:, :w * n]
        want = _conv_forward_want(img_vals[i].ravel(), bd, sg, rev, nl, wide).reshape(h, w * n)
        assert np.array_equal(plane, want), "forward B=%d signed=%s rev=%s nlt3=%s wide=%s container %d" % (bd, sg, rev, nl, wide, container)
    # the way back, from working samples in and beyond the range
    words = np.zeros(arena_off + 64, np.uint32)
    wants = []
    for i, (bd, sg, rev, nl, wide) in enumerate(comps):
        d = descs[i]
        n = h * w
        if rev:
            lo = -(1 << (bd - 1))
            v = np.concatenate([rs.rev_forward(img_vals[i].ravel(), bd, sg, nl)[: n // 2],
                                rng.integers(2 * lo - 5, -2 * lo + 5, n - n // 2, dtype=np.int64)])
            a = v.astype(np.int64).view(np.uint32) if wide else rs.wrap32(v).view(np.uint32)
        else:
            a = rs.edge_floats(bd, rng, n)[:n].astype(np.float32).view(np.uint32)
        k = 2 if wide else 1
        dst = words[int(d["plane_off"]):int(d["plane_off"]) + (w + 3) * h * k].reshape(h, (w + 3) * k)
        dst[:, :w * k] = a.reshape(h, w * k)
        wants.append(_conv_inverse_want(a, bd, sg, rev, nl, wide, container).reshape(h, w))
    out = torch.zeros(image.size + 64, dtype={32: torch.int32, 16: torch.int16, 8: torch.int8}[container], device="cuda")
    codec.convert("inverse", params, descs, out, torch.from_numpy(words.view(np.int32)).cuda(), w, h, container)
    back = out.cpu().numpy()
    for i, (bd, sg, rev, nl, wide) in enumerate(comps):
        g = _from_container(back[int(descs[i]["img_off"]):int(descs[i]["img_off"]) + h * w], container, sg).reshape(h, w)
        assert np.array_equal(g, wants[i]), "inverse B=%d signed=%s rev=%s nlt3=%s wide=%s container %d: %d differ" % (
            bd, sg, rev, nl, wide, container, int((g != wants[i]).sum()))


GEOMETRY_TILES = [[(513, 5), (256, 2), (1, 1)], [(257, 2), (255, 5), (513, 1)]]          # (w, h) of the three tiles of a launch


def _window(buf, off, pitch, h, w):
    return np.lib.stride_tricks.as_strided(buf[off:], (h, w), (pitch * buf.itemsize, buf.itemsize))


def _geometry_launch(container, colour, rev, tiles, rng):
    """one forward and one inverse launch over three tiles of different sizes, each a window (src_x0, src_y0 > 0, img_pitch >
    w) of a larger image, arena pitches wider than the planes.  Colour off: component 0 full size, component 1 half as wide,
    component 2 with w = 0.  Colour on: a triple of one geometry with three formats (one signed) and a fourth, plain
    component half as wide behind it.  The whole arena (forward) and the whole image (inverse) are compared: planes and
    windows with the restatement, every other element with what it held."""
    from openjph_amd import codec
    deep = (8, 7, 6) if container == 8 else (8, 10, 12)
    fmts = [(deep[0], False), (deep[1], True), (deep[2], False)] + ([(min(container, 11), False)] if colour else [])
    nc, nt = len(fmts), len(tiles)

    def width(c, w):
        return (w if c < 3 else (w + 1) // 2) if colour else (w, (w + 1) // 2, 0)[c]
    descs = np.zeros(nt * nc, codec.convert_desc_dtype)
    rows = max(1 + t + h for t, (w, h) in enumerate(tiles)) + 1
    img_len = 5
    for c, (bd, sg) in enumerate(fmts):
        pitch, x0 = 2 + sum(width(c, w) + 3 for w, h in tiles), 2
        for t, (w, h) in enumerate(tiles):
            d = descs[t * nc + c]
            d["w"], d["h"], d["src_x0"], d["src_y0"], d["img_pitch"], d["img_off"] = width(c, w), h, x0, 1 + t, pitch, img_len
            d["fmt"] = bd | (0x100 if sg else 0) | 0x200 | (0x400 if rev else 0)
            x0 += width(c, w) + 3
        img_len += pitch * rows + 7
    arena_len = 9
    for d in descs:
        d["pitch"], d["plane_off"] = int(d["w"]) + 5, arena_len
        arena_len += (int(d["w"]) + 5) * int(d["h"]) + 16
    assert all(d["src_x0"] > 0 and d["src_y0"] > 0 and d["img_pitch"] > d["w"] and d["pitch"] > d["w"] for d in descs)
    max_w, max_h = max(w for w, h in tiles), max(h for w, h in tiles)
    params = _params(num_comps=nc, bit_depth=8, reversible=rev, color_transform=colour)
    cdt = {32: np.int32, 16: np.int16, 8: np.int8}[container]
    tdt = {32: torch.int32, 16: torch.int16, 8: torch.int8}[container]
    tag = "container %d colour %s rev %s tiles %s" % (container, colour, rev, tiles)

    def image_window(buf, d):
        return _window(buf, int(d["img_off"]) + int(d["src_y0"]) * int(d["img_pitch"]) + int(d["src_x0"]), int(d["img_pitch"]), int(d["h"]), int(d["w"]))

    def plane(buf, d):
        return _window(buf, int(d["plane_off"]), int(d["pitch"]), int(d["h"]), int(d["w"]))

    # forward: image -> arena
    image = rng.integers(-128, 128, img_len).astype(cdt)
    arena0 = rng.integers(0, 1 << 32, arena_len, dtype=np.uint64).astype(np.uint32)
    want = arena0.copy()
    for t in range(nt):
        vals = []
        for c, (bd, sg) in enumerate(fmts):
            d = descs[t * nc + c]
            n = int(d["w"]) * int(d["h"])
            vals.append(rs.edge_samples(bd, sg, rng, n)[:n].reshape(int(d["h"]), int(d["w"])))
            image_window(image, d)[...] = _to_container(vals[c], container)
        first = 0
        if colour:
            first = 3
            if rev:
                out = [rs.wrap32(x).view(np.uint32) for x in rs.rct_forward(*[rs.rev_forward(vals[c], *fmts[c]) for c in range(3)])]
            else:
                out = [x.view(np.uint32) for x in rs.ict_forward(*[rs.irv_to_float(vals[c], *fmts[c]) for c in range(3)])]
            for c in range(3):
                plane(want, descs[t * nc + c])[...] = out[c]
        for c in range(first, nc):
            d = descs[t * nc + c]
            if d["w"]:
                plane(want, d)[...] = _conv_forward_want(vals[c].ravel(), fmts[c][0], fmts[c][1], rev, False, False).reshape(vals[c].shape)
    arena = torch.from_numpy(arena0.view(np.int32)).cuda()
    codec.convert("forward", params, descs, torch.from_numpy(image).cuda(), arena, max_w, max_h, container)
    got = arena.cpu().numpy().view(np.uint32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "forward %s: %d arena words differ, the first at %d" % (tag, bad.size, bad[0])
    # inverse: arena -> image, from working samples in and beyond the range
    words = rng.integers(0, 1 << 32, arena_len, dtype=np.uint64).astype(np.uint32)
    image0 = rng.integers(-128, 128, img_len).astype(cdt)
    want = image0.copy()
    for t in range(nt):
        src = []
        for c, (bd, sg) in enumerate(fmts):
            d = descs[t * nc + c]
            n = int(d["w"]) * int(d["h"])
            lo = -(1 << (bd - 1))
            a = rs.wrap32(rng.integers(2 * lo - 5, -2 * lo + 5, n, dtype=np.int64)).view(np.uint32) if rev else rs.edge_floats(bd, rng, n)[:n].astype(np.float32).view(np.uint32)
            src.append(a.reshape(int(d["h"]), int(d["w"])))
            plane(words, d)[...] = src[c]
        first = 0
        if colour:
            first = 3
            if rev:
                rgb = rs.rct_inverse(*[x.view(np.int32) for x in src[:3]])
                out = [rs.wrap32(rgb[c] + rs.half(*fmts[c])).astype(np.int64) for c in range(3)]
            else:
                rgb = rs.ict_inverse(*[x.view(np.float32) for x in src[:3]])
                out = [rs.irv_to_int(rgb[c], *fmts[c]).astype(np.int64) for c in range(3)]
            for c in range(3):
                image_window(want, descs[t * nc + c])[...] = _to_container(rs.saturate(out[c], container, fmts[c][1]), container)
        for c in range(first, nc):
            d = descs[t * nc + c]
            if d["w"]:
                v = _conv_inverse_want(src[c].ravel(), fmts[c][0], fmts[c][1], rev, False, False, container).reshape(src[c].shape)
                image_window(want, d)[...] = _to_container(v, container)
    out = torch.from_numpy(image0).cuda()
    assert out.dtype == tdt
    codec.convert("inverse", params, descs, out, torch.from_numpy(words.view(np.int32)).cuda(), max_w, max_h, container)
    got = out.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "inverse %s: %d image samples differ, the first at %d" % (tag, bad.size, bad[0])
    return {(d["w"] > 0, int(d["w"]) < max_w) for d in descs}


@pytest.mark.parametrize("container", [32, 16, 8])
def test_convert_kernels_geometry(container):
    """the stand-alone conversion kernels beyond one tile at the origin: blockIdx.z tiles of different sizes, window offsets,
    components narrower than the launch and one that is empty, rows wider than one 256-thread workgroup, the colour branches
    with mixed formats inside the triple and a component behind it -- both kinds, both directions.  (The 64-bit RCT stays with
    the whole codestreams of tests/format_cases.py.)"""
    rng = np.random.default_rng(40 + container)
    ran, widths, heights, shapes = set(), set(), set(), set()
    for i, (colour, rev) in enumerate([(False, True), (True, False), (True, True), (False, False)]):
        for tiles in (GEOMETRY_TILES[i % 2], GEOMETRY_TILES[1 - i % 2][::-1]):
            shapes |= _geometry_launch(container, colour, rev, tiles, rng)
            ran.add((colour, rev))
            widths |= {w for w, h in tiles}
            heights |= {h for w, h in tiles}
            assert len(set(tiles)) == 3
    assert ran == {(c, r) for c in (False, True) for r in (False, True)}
    assert widths == {1, 255, 256, 257, 513} and heights == {1, 2, 5}
    assert (False, True) in shapes and (True, True) in shapes and (True, False) in shapes      # an empty, a narrower and a full-width component


# ------------------------------------------------------------------------------------------------------------------------
# the top DWT level with the conversion fused in (ojphgpu_dwt_{forward,inverse}_image_ex, _general_image)
# ------------------------------------------------------------------------------------------------------------------------
def _layout(shapes):
    offs, total = [], 0
    for (h, w) in shapes:
        pitch = (max(w, 1) + 15) & ~15
        offs.append((total, pitch))
        total = (total + pitch * max(h, 1) + 64 + 63) & ~63
    return offs, total


def _strided(a, off, pitch, h, w):
    return np.lib.stride_tricks.as_strided(a[off:], (h, w), (pitch * a.itemsize, a.itemsize))


def _image_level(rev, formats, container, colour, general=None, seed=0):
    """one launch over planes of different formats: forward (bands vs the restatement + oracle DWT), then the inverse from the
    oracle's bands (image samples vs oracle DWT + restatement, saturated to the container)"""
    from openjph_amd import codec
    from oracle import oraclebind as ob
    rng = np.random.default_rng(seed)
    geo = [(37, 61, 1, 1), (20, 33, 0, 1), (9, 2, 1, 0), (1, 17, 0, 0), (16, 16, 1, 1), (33, 1, 1, 1)]
    planes = []                                               # (h, w, xe, ye, bd, sg)
    for i, (bd, sg) in enumerate(formats):
        h, w, xe, ye = geo[(i // 3 if colour else i) % len(geo)]
        planes.append((h, w, xe, ye, bd, sg))
    dt = np.int32 if rev else np.float32
    shapes = []
    for (h, w, xe, ye, bd, sg) in planes:
        lw, hw, lh, hh = ob.band_dims(w, h, bool(xe), bool(ye))
        shapes += [(lh, lw), (lh, hw), (hh, lw), (hh, hw)]
    offs, total = _layout(shapes)
    descs = np.zeros(len(planes), codec.dwt_desc_dtype)
    vals, img_off = [], 0
    for i, (h, w, xe, ye, bd, sg) in enumerate(planes):
        d = descs[i]
        d["src_off"], d["src_pitch"] = img_off, w
        for k, name in enumerate(("ll", "hl", "lh", "hh")):
            d[name + "_off"], d[name + "_pitch"] = offs[4 * i + k]
        d["w"], d["h"], d["x_even"], d["y_even"], d["reserved"] = w, h, xe, ye, bd | (0x100 if sg else 0)
        vals.append(rs.edge_samples(bd, sg, rng, h * w)[:h * w].reshape(h, w) if h * w > 12 else
                    rng.integers(*rs.sample_range(bd, sg), (h, w), endpoint=True))
        img_off += h * w
    work = []
    for i, (h, w, xe, ye, bd, sg) in enumerate(planes):
        v = vals[i].ravel()
        work.append((rs.wrap32(rs.rev_forward(v, bd, sg)) if rev else rs.irv_to_float(v, bd, sg)).reshape(h, w))
    if colour:
        for t in range(0, len(planes), 3):
            r, g, b = work[t:t + 3]
            if rev:
                work[t:t + 3] = [rs.wrap32(x).reshape(r.shape) for x in rs.rct_forward(r.astype(np.int64), g.astype(np.int64), b.astype(np.int64))]
            else:
                work[t:t + 3] = list(rs.ict_forward(r, g, b))
    bands = []
    for i, (h, w, xe, ye, bd, sg) in enumerate(planes):
        if general is not None:
            bands.append(ob.dwt_fwd_gen(work[i].astype(dt), general, 1.0, True, True, bool(xe), bool(ye)))
        else:
            bands.append((ob.dwt53_fwd if rev else ob.dwt97_fwd)(work[i].astype(dt), bool(xe), bool(ye)))
    image = np.concatenate([_to_container(v, container).ravel() for v in vals])
    params = _params(num_comps=1, bit_depth=min(max(p[4] for p in planes), 31 if container == 32 else container),
                     reversible=rev, color_transform=colour)
    arena = torch.zeros(total + 64, dtype=torch.int32, device="cuda")
    max_w, max_h = max(p[1] for p in planes), max(p[0] for p in planes)
    d_img = torch.from_numpy(image).cuda()
    if general is not None:
        codec.dwt_general_image("forward", general, 0 if rev else 2, params, descs, d_img, arena, max_w, max_h, container=container)
    else:
        codec.dwt_image("forward", params, descs, d_img, arena, max_w, max_h, container, colour)
    got = arena.cpu().numpy().view(np.uint32)
    tag = "rev=%s container=%d colour=%s general=%s" % (rev, container, colour, general is not None)
    for i, p in enumerate(planes):
        for k, name in enumerate(("ll", "hl", "lh", "hh")):
            e = bands[i][k]
            if e.size:
                g = _strided(got, offs[4 * i + k][0], offs[4 * i + k][1], *e.shape)
                assert np.array_equal(g, np.ascontiguousarray(e).view(np.uint32)), "forward plane %d %s band %s, %s" % (i, p, name, tag)
    # the way back from bands pushed past the range (the low band scaled up), so that the stores saturate / clamp
    over = np.array(got, copy=True)
    for i, (h, w, xe, ye, bd, sg) in enumerate(planes):
        ll = np.ascontiguousarray(bands[i][0])
        if ll.size:
            ll = (ll.astype(np.int64) * 9 // 8).astype(np.int32) if rev else (ll * np.float32(1.125)).astype(np.float32)
            bands[i] = (ll,) + tuple(bands[i][1:])
            _strided(over, offs[4 * i][0], offs[4 * i][1], *ll.shape)[:] = ll.view(np.uint32)
    arena = torch.from_numpy(over.view(np.int32)).cuda()
    out = torch.full((image.size + 64,), 0x55, dtype={32: torch.int32, 16: torch.int16, 8: torch.int8}[container], device="cuda")
    if general is not None:
        codec.dwt_general_image("inverse", general, 0 if rev else 2, params, descs, out, arena, max_w, max_h, container=container)
    else:
        codec.dwt_image("inverse", params, descs, out, arena, max_w, max_h, container, colour)
    back = out.cpu().numpy()
    syn = []
    for i, (h, w, xe, ye, bd, sg) in enumerate(planes):
        if general is not None:
            syn.append(ob.dwt_inv_gen(*bands[i], w, h, general, 1.0, True, True, bool(xe), bool(ye)))
        else:
            syn.append((ob.dwt53_inv if rev else ob.dwt97_inv)(*bands[i], w, h, bool(xe), bool(ye)))
    if colour:
        for t in range(0, len(planes), 3):
            y, cb, cr = syn[t:t + 3]
            syn[t:t + 3] = list(rs.rct_inverse(y, cb, cr)) if rev else list(rs.ict_inverse(y, cb, cr))
    for i, (h, w, xe, ye, bd, sg) in enumerate(planes):
        if rev:
            want = rs.wrap32(np.asarray(syn[i], np.int64) + rs.half(bd, sg)).astype(np.int64)
        else:
            want = rs.irv_to_int(syn[i], bd, sg).astype(np.int64)
        want = rs.saturate(want, container, sg).reshape(h, w)
        o = int(descs[i]["src_off"])
        g = _from_container(back[o:o + h * w], container, sg).reshape(h, w)
        assert np.array_equal(g, want), "inverse plane %d %s, %s: %d differ" % (i, planes[i], tag, int((g != want).sum()))


def _formats(rng, n, container, colour):
    top = 26 if container == 32 else container
    if colour:
        out = []
        for _ in range(n):
            bd, sg = int(rng.integers(1, top + 1)), bool(rng.integers(0, 2))
            out += [(bd, sg)] * 3
        return out
    fixed = [(1, False), (1, True), (top, False), (top, True), (max(top - 1, 1), True)]
    return fixed + [(int(rng.integers(1, top + 1)), bool(rng.integers(0, 2))) for _ in range(n - len(fixed))]


@pytest.mark.parametrize("colour", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("container", [32, 16, 8])
@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
def test_dwt_image_level_mixed_formats(rev, container, colour):
    """one launch of the fused top level over planes of different depths (1-26) and signs, every container"""
    rng = np.random.default_rng(container * 4 + 2 * rev + colour)
    _image_level(rev, _formats(rng, 4 if colour else 12, container, colour), container, colour, seed=container + rev)
    if container == 32:                                      # the edge of the fused conversion: 25 and 26 bits
        _image_level(rev, [(25, False), (25, True), (26, False), (26, True)] * (3 if colour else 1), container, colour, seed=7)


@pytest.mark.parametrize("container", [32, 16, 8])
@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irv"])
def test_dwt_general_image_level_mixed_formats(rev, container):
    """the general lifting kernels' fused top level (ATK wavelets) over planes of different depths and signs"""
    from oracle import oraclebind as ob
    steps = ob.REV53 if rev else [0.25, -0.5, 0.125]
    rng = np.random.default_rng(40 + container + rev)
    _image_level(rev, _formats(rng, 8, container, False), container, False, general=steps, seed=container)


def test_dwt_inverse_region_signed_odd_depths():
    """region synthesis of the top level into containers, signed and odd-depth formats: the region == that part of the
    whole plane's synthesis"""
    from openjph_amd import codec
    from oracle import oraclebind as ob
    rng = np.random.default_rng(17)
    for rev in (True, False):
        for container, bd, sg in ((32, 25, True), (32, 13, True), (16, 15, True), (16, 9, False), (8, 7, True), (8, 3, False)):
            h, w = 41, 53
            lw, hw, lh, hh = ob.band_dims(w, h)
            offs, total = _layout([(lh, lw), (lh, hw), (hh, lw), (hh, hw)])
            v = rng.integers(*rs.sample_range(bd, sg), (h, w), endpoint=True)
            work = rs.wrap32(rs.rev_forward(v.ravel(), bd, sg)).reshape(h, w) if rev else rs.irv_to_float(v.ravel(), bd, sg).reshape(h, w)
            bands = (ob.dwt53_fwd if rev else ob.dwt97_fwd)(work)
            arena = np.zeros(total + 64, np.uint32)
            for k, b in enumerate(bands):
                _strided(arena, offs[k][0], offs[k][1], *b.shape)[:] = np.ascontiguousarray(b).view(np.uint32)
            syn = (ob.dwt53_inv if rev else ob.dwt97_inv)(*bands, w, h)
            full = rs.wrap32(syn.astype(np.int64) + rs.half(bd, sg)).astype(np.int64) if rev else rs.irv_to_int(syn, bd, sg).astype(np.int64)
            full = rs.saturate(full, container, sg)
            x0, y0, x1, y1 = 5, 3, 44, 40
            descs = np.zeros(1, codec.dwt_desc_dtype)
            d = descs[0]
            for k, name in enumerate(("ll", "hl", "lh", "hh")):
                d[name + "_off"], d[name + "_pitch"] = offs[k]
            d["w"], d["h"], d["x_even"], d["y_even"], d["reserved"] = w, h, 1, 1, bd | (0x100 if sg else 0)
            regs = np.zeros(1, codec.dwt_region_dtype)
            regs[0]["rx0"], regs[0]["ry0"], regs[0]["rx1"], regs[0]["ry1"] = x0, y0, x1, y1
            regs[0]["out_off"], regs[0]["out_pitch"] = 0, x1 - x0
            out = torch.zeros((y1 - y0) * (x1 - x0) + 64, dtype={32: torch.int32, 16: torch.int16, 8: torch.int8}[container], device="cuda")
            codec.dwt_inverse_region(rev, descs, regs, torch.from_numpy(arena.view(np.int32)).cuda(), out, container)
            g = _from_container(out.cpu().numpy()[:(y1 - y0) * (x1 - x0)], container, sg).reshape(y1 - y0, x1 - x0)
            assert np.array_equal(g, full[y0:y1, x0:x1]), "rev=%s container %d B=%d signed=%s" % (rev, container, bd, sg)


# ------------------------------------------------------------------------------------------------------------------------
# the block coder at the top of the 32-bit path
# ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 64), (32, 32), (128, 32), (32, 128), (4, 1024), (1024, 4), (64, 17), (17, 64), (1, 1), (3, 3), (5, 64), (64, 5),
          (2, 64), (63, 63), (33, 31), (8, 8), (1, 64), (64, 1)]


def _high_k_cases():
    out = []
    for kmax in rs.HIGH_K:
        for i, (w, h) in enumerate(SHAPES):
            out.append((w, h, kmax, i % 3 == 0))
    return out


def test_ht_encode_high_and_low_K_max():
    """K_max 1-2 and 22-30, every block shape, amplitudes up to 2^K - 1 at full density (more than 3 bytes per sample at the
    top: far past the encoder's LDS output stage)"""
    from openjph_amd import codec
    from openjph_amd.csrc_consts import block_scratch_bytes
    from oracle import oraclebind as ob
    rng = np.random.default_rng(61)
    cases = _high_k_cases()
    descs = np.zeros(len(cases), codec.cb_desc_dtype)
    coefs, expect, off, soff = [], [], 0, 0
    for i, (w, h, kmax, full) in enumerate(cases):
        pitch = (w + 63) & ~63
        sm, v = rs.high_k_block(rng, w, h, kmax, full)
        plane = np.zeros((h, pitch), np.int32); plane[:, :w] = v
        coefs.append(plane.ravel())
        q, mx = ob.quant_rev(plane[:, :w], kmax)
        expect.append(ob.ht_encode(q, w, h, w, kmax - 1, 0))
        d = descs[i]
        d["coef_off"], d["pitch"], d["w"], d["h"] = off, pitch, w, h
        d["K_max"], d["reversible"], d["delta"] = kmax, 1, 0.0
        d["data_off"], d["scratch_cap"] = soff, block_scratch_bytes(w, h, kmax)
        off += plane.size; soff += int(d["scratch_cap"])
    assert max(len(e) / (c[0] * c[1]) for e, c in zip(expect, cases)) > 3.0
    coef = torch.from_numpy(np.concatenate(coefs)).cuda()
    res, out, status = codec.ht_encode(descs, coef, soff, soff)
    assert status == 0
    bad = [(i, cases[i], int(res[i, 1]), len(e)) for i, e in enumerate(expect)
           if out[int(res[i, 0]):int(res[i, 0]) + int(res[i, 1])].tobytes() != e]
    assert not bad, "HT encode mismatches (idx, (w, h, K_max, full), got_len, want_len): %s" % bad[:8]


def test_ht_decode_high_K_max_and_missing_msbs_edges():
    """cleanup-only blocks at K_max 1-2 and 22-30, then missing_msbs 27-30 with 1-3 passes, causal and not, both wavelets:
    verdicts and samples == the oracle's (29: the refinement passes are dropped; 30: the block is rejected)"""
    from openjph_amd import codec
    from oracle import oraclebind as ob
    rng = np.random.default_rng(62)
    trials = []
    for (w, h, kmax, full) in _high_k_cases():
        sm, v = rs.high_k_block(rng, w, h, kmax, full)
        trials.append((w, h, kmax, kmax - 1, ob.ht_encode(sm, w, h, w, kmax - 1), b"", 1, False, True))
    for mm in (27, 28, 29, 30):
        kmax = min(mm + 1, 30)
        for i, (w, h) in enumerate(SHAPES):
            sm, v = rs.high_k_block(rng, w, h, kmax, i % 4 == 0)
            cup = ob.ht_encode(sm, w, h, w, kmax - 1)
            tail = bytes(rng.integers(0, 256, size=int(rng.integers(1, 300)), dtype=np.uint8))
            npass = 1 + i % 3
            trials.append((w, h, kmax, mm, cup, tail if npass > 1 else b"", npass, bool(i % 2), bool((i // 2) % 2)))
    descs = np.zeros(len(trials), codec.cb_desc_dtype)
    datas, expect, off, doff = [], [], 0, 0
    for i, (w, h, kmax, mm, cup, tail, npass, causal, rev) in enumerate(trials):
        pitch = (w + 63) & ~63
        d = descs[i]
        d["coef_off"], d["pitch"], d["w"], d["h"] = off, pitch, w, h
        d["K_max"], d["reversible"], d["missing_msbs"] = mm + 1, (1 if rev else 0) | (2 if causal else 0), mm
        d["delta"] = 0.37 / (1 << 24)
        d["num_passes"], d["len1"], d["len2"], d["data_off"] = npass, len(cup), len(tail), doff
        ok, dec = ob.ht_decode(cup + tail, w, h, w, mm, len2=len(tail), num_passes=npass, stripe_causal=causal)
        want = (ob.dequant_rev(dec, mm + 1) if rev else ob.dequant_irv(dec, float(d["delta"])).view(np.int32)) if ok else np.zeros((h, w), np.int32)
        expect.append((ok, want[:, :w]))
        datas.append(np.frombuffer(cup + tail, np.uint8))
        off += pitch * h; doff += len(cup) + len(tail)
    assert sum(1 for ok, _ in expect if not ok) >= len(SHAPES) and sum(1 for ok, _ in expect if ok) > len(trials) // 2
    coef = torch.full((off + 64,), 0x5A5A5A5A, dtype=torch.int32).cuda()
    status = codec.ht_decode(descs, np.concatenate(datas), coef)
    got = coef.cpu().numpy()
    for i, (ok, want) in enumerate(expect):
        w, h, kmax, mm = trials[i][:4]
        assert (status[i] == 0) == ok, "trial %d (w %d h %d mm %d passes %d): GPU status %d, oracle ok=%s" % (i, w, h, mm, trials[i][6], status[i], ok)
        d = descs[i]
        g = _strided(got, int(d["coef_off"]), int(d["pitch"]), h, w)
        assert np.array_equal(g, want), "trial %d (w %d h %d mm %d passes %d): %d samples differ" % (
            i, w, h, mm, trials[i][6], int((g != want).sum()))


# ------------------------------------------------------------------------------------------------------------------------
# whole codestreams
# ------------------------------------------------------------------------------------------------------------------------
N_RANDOM = 40


def _unpack(plan, raw, container, signs):
    comps = plan.unpack_frame(raw)
    return [_from_container(np.asarray(c).ravel(), container, s).reshape(np.asarray(c).shape) for c, s in zip(comps, signs)]


def _whole(name, planes, kw, size, containers=True, batch=False, region=False):
    from openjph_amd import capi, codec
    from openjph_amd.plan import make_params
    from tests import cpu_pipeline as cp
    want, plan, *_ = cp.encode(planes, size=size, **kw)
    wdec, _ = cp.decode(want)
    wdec = [np.asarray(x, np.int64) for x in wdec]
    signs, depths = kw["signs"], kw["bit_depths"]
    enc = codec.Encoder(make_params(size[0], size[1], len(planes), **kw))
    for container in (_containers(depths) if containers else [32]):
        frame = plan.pack_frame([np.asarray(p, np.int32) for p in planes])
        if container != 32:                               # the low bits: unsigned, or two's complement for signed components
            frame = _to_container(np.asarray(frame).astype(np.int64), container)
        got = enc.encode(frame)
        assert got == want, "%s container %d: codestream differs (%d vs %d bytes) %s" % (name, container, len(got), len(want), kw)
        dec = codec.Decoder(want)
        raw = dec.run_device(dtype={32: torch.int32, 16: torch.int16, 8: torch.int8}[container])
        assert dec.failed_blocks() == 0
        out = _unpack(dec.plan, raw.cpu().numpy(), container, signs)
        for c in range(len(planes)):
            w = rs.saturate(wdec[c], container, signs[c]) if container != 32 else wdec[c]
            assert np.array_equal(out[c], w), "%s container %d component %d: %d samples differ %s" % (
                name, container, c, int((out[c] != w).sum()), kw)
    if batch:
        frames = [planes, [np.ascontiguousarray(p[::-1]) for p in planes], [np.ascontiguousarray(p[:, ::-1]) for p in planes]]
        wants = [want] + [cp.encode(f, size=size, **kw)[0] for f in frames[1:]]
        benc = codec.Encoder(make_params(size[0], size[1], len(planes), **kw), frames=3)
        got = benc.encode(np.stack([plan.pack_frame([np.asarray(p, np.int32) for p in f]) for f in frames]))
        assert got == wants, "%s: batch codestreams differ" % name
        bdec = codec.Decoder(wants)
        frames_out = bdec.decode()
        for f in range(3):
            wd, _ = cp.decode(wants[f])
            out = bdec.plan.unpack_frame(frames_out[f])
            for c in range(len(planes)):
                assert np.array_equal(np.asarray(out[c], np.int64), np.asarray(wd[c], np.int64)), "%s batch frame %d component %d" % (name, f, c)
    if region:
        from tests.region_cases import crop, regions_for
        full = codec.Decoder(want)
        ffull = full.run_device().cpu().numpy().astype(np.int64)
        for r in regions_for(size, seed=len(name))[:3]:
            try:
                reg = codec.Decoder(want, region=r)
            except capi.OjphError:
                continue
            g = reg.plan.unpack_frame(reg.run_device().cpu().numpy().astype(np.int64))
            assert reg.failed_blocks() == 0
            for c, (a, b) in enumerate(zip(g, crop(full.plan, ffull, reg.plan))):
                assert np.array_equal(a, b), "%s region %s component %d" % (name, r, c)


def _cases():
    from tests.format_cases import all_cases
    return all_cases(N_RANDOM)


def _part1_narrow(kw):
    return not kw.get("atk") and max(kw["bit_depths"]) <= 26


def test_predicted_failure_32_bit_component_0_beside_a_fused_component():
    """a 32-bit component 0 beside a narrow component whose top level converts its own samples (the other wavelet by COC; an
    ATK wavelet): the launch of the narrow component was validated against component 0's format (E_INVALID)"""
    from tests.format_cases import fixed_case
    for i in (0, 1, 2):
        planes, kw, size = fixed_case(i)
        _whole("fixed%d" % i, planes, kw, size)


@pytest.mark.parametrize("chunk", range(4))
def test_format_cases_whole_codestreams(chunk):
    """tests/format_cases.py through codec.Encoder / Decoder: the oracle pipeline's bytes and samples in every container the
    samples fit; every fourth case also as a batch of three frames, Part-1 cases of at most 26 bits also region-decoded"""
    from openjph_amd import capi
    from tests import cpu_pipeline as cp
    done = 0
    for k, (name, planes, kw, size) in enumerate(_cases()[chunk::4]):
        if any(q.size == 0 for q in planes):
            continue
        try:
            cp.encode(planes, size=size, **kw)
        except capi.OjphError:
            continue                                      # refused (as by the reference: tests/test_cpu_formats.py)
        _whole(name, planes, kw, size, batch=k % 4 == 0, region=k % 2 == 0 and _part1_narrow(kw))
        done += 1
    assert done >= 8


@pytest.mark.parametrize("switch", ["OJPHGPU_NO_COLOUR_FUSION", "OJPHGPU_NO_GENERAL_FUSION"])
def test_format_cases_without_fusion(switch, monkeypatch):
    """the same codestreams with the colour / general-lifting conversion left to the conversion kernels"""
    from openjph_amd import capi
    from tests import cpu_pipeline as cp
    monkeypatch.setenv(switch, "1")
    done = 0
    for name, planes, kw, size in _cases():
        if any(q.size == 0 for q in planes):
            continue
        if switch == "OJPHGPU_NO_COLOUR_FUSION" and not kw.get("color_transform"):
            continue
        if switch == "OJPHGPU_NO_GENERAL_FUSION" and not (kw.get("atk") or max(kw["bit_depths"]) > 26):
            continue
        try:
            cp.encode(planes, size=size, **kw)
        except capi.OjphError:
            continue
        _whole(name, planes, kw, size, containers=False)
        done += 1
    assert done >= 3


def test_format_cases_under_the_fused_decoder_schedule(tmp_path):
    """the fixed cases (deep components, K_max up to 30, incompressible 25- / 26-bit frames) decoded with OJPHGPU_DEC_FUSED=2
    (the one-launch block decoder wherever it can run; chosen once per process, so in a child): the oracle's samples"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = r'''
import sys, numpy as np
sys.path.insert(0, %r)
from openjph_amd import codec
from tests import cpu_pipeline as cp
from tests.format_cases import FIXED, fixed_case
for i in range(len(FIXED)):
    planes, kw, size = fixed_case(i)
    cs, *_ = cp.encode(planes, size=size, **kw)
    want, _ = cp.decode(cs)
    dec = codec.Decoder(cs)
    for _ in range(2):
        got = dec.plan.unpack_frame(dec.run_device().cpu().numpy())
        assert dec.failed_blocks() == 0, i
        for c in range(len(planes)):
            assert np.array_equal(got[c], want[c]), (i, c)
print("ok", len(FIXED))
''' % root
    f = tmp_path / "fused.py"
    f.write_text(script)
    r = subprocess.run([sys.executable, str(f)], env=dict(os.environ, OJPHGPU_DEC_FUSED="2"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
