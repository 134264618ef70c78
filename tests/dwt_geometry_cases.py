"""Launches for tests/test_gpu_dwt_geometry.py: every whole-plane DWT launch form (and the colour region synthesis) over planes
built around the kernels' work split -- the 120-column strip of a wavefront, the vertical chunk of `rp` row pairs, the origin
parities -- with the expected contents of every output rectangle from the oracle and the numpy restatement of the sample
conversion (tests/test_cpu_formats.py).  Pure numpy + oracle: no GPU, so tests/test_cpu_dwt_geometry.py checks the harness
itself where there is none.

A Launch holds the buffers as they are before the launch (inputs in place, everything else a sentinel), the descriptors, and
`rects`: the rectangles the descriptors name as outputs with what they must hold afterwards.  verify() compares those bit for
bit and requires every other element of every buffer to be what it was -- padding, gaps, guards and the inputs alike."""
import functools

import numpy as np

from tests import test_cpu_formats as rs

VALID_PAIRS = 60                                    # column pairs a wavefront produces (kernels_dwt.hip: VALID) = 120 columns
WIDTHS = (1, 2, 3, 119, 120, 121, 122, 239, 240, 241, 250, 361, 400)
WIDE = (241, 250, 361, 400)                         # three or more strips: a middle strip takes the unchecked interior path
TALL_W = 130
SENT_I, SENT_F = 0x5A5A5A5A, 0x7FA5A5A5             # int planes / float planes (a NaN: no transform of finite samples yields one)
# image samples: a 32-bit container never holds SENT_I (depths of at most 26 bits); every value of a 16- / 8-bit container is
# a legitimate sample, so those launches run twice, under complementary sentinels -- an element nobody stored differs from
# the expectation under at least one of them
IMAGE_SENTINELS = {32: (SENT_I,), 16: (0x5A5A, 0xA5A5), 8: (0x5A, 0xA5)}

GEN_REV = ("rev-3steps", np.int32, [(1, 2, 2), (-1, 1, 1), (3, 4, 3)], 1.0)        # from tests/test_gpu_wide.py: KERNELS
GEN_IRV = ("irv-3steps", np.float32, [0.2, -0.4, 0.1], 1.1)                        # (odd step counts: the band swap as well)

SETTINGS = {                                        # OJPHGPU_DWT_<knob>, read once per process: one child process each
    "default": {},                                                      # what a small frame gets today
    "shortest": dict(RP_MIN=2, RP_COLOUR=2, TRIP=1, XCD=0),             # every chunk is mostly halo and warm-up
    "odd": dict(RP_MIN=5, RP_COLOUR=6, TRIP=2, XCD=1),                  # an odd chunk height under two row pairs per trip
    "mid": dict(RP_MIN=12, RP_COLOUR=12, TRIP=2, XCD=0),
    "large": dict(RP_MIN=20, RP_COLOUR=24, TRIP=2, XCD=1),              # the large-level production geometry, the tallest colour chunk
    "caps": dict(RP_MIN=20, RP_INV=28, RP_FWD=36),                      # the caps of the large launches (codec.dwt only)
}


def knobs_of(environ):
    """the knobs as kernels_dwt.hip reads them (a value outside a knob's range counts as unset)"""
    def num(name, lo, hi):
        try:
            v = int(environ.get("OJPHGPU_DWT_" + name, "0"))
        except ValueError:
            v = 0
        return v if lo <= v <= hi else 0
    xcd = environ.get("OJPHGPU_DWT_XCD")
    return dict(RP_MIN=num("RP_MIN", 2, 20), RP_COLOUR=num("RP_COLOUR", 2, 64), RP_INV=num("RP_INV", 4, 256),
                RP_FWD=num("RP_FWD", 4, 256), XCD=1 if xcd is None else int(xcd != "0"))


def chunk_heights(knobs):
    """row pairs per vertical chunk of each launch form under these knobs, for planes as small as the ones here.  With nothing
    set that is 4 for the synthesis kernels, 8 for the analysis kernels (pick_row_pairs' floors: what small planes get) and 4
    for the colour kernels (fit_rounds returns its first candidate while the grid fits the device in one round)."""
    rp = knobs["RP_MIN"]
    fwd, inv = rp or 8, rp or 4
    return dict(fwd=fwd, inv=inv, colour=knobs["RP_COLOUR"] or 4,
                plain_fwd=knobs["RP_FWD"] if fwd == 20 and knobs["RP_FWD"] else fwd,     # the caps act at 20 only, and only in
                plain_inv=knobs["RP_INV"] if inv == 20 and knobs["RP_INV"] else inv,     # the 5/3 and 9/7 launches
                region_colour=4)                                                         # (always fit_rounds)


# Restatements of the launch arithmetic (kernels_dwt.hip: dwt_grid, pick_row_pairs).  They only check that the inputs are the
# intended ones -- that the planes below give the chunk height and the grid the test is about -- not the kernel.
def dwt_grid(n, max_w, max_h, rp):
    npx, npy = (max_w + 2) >> 1, (max_h + 2) >> 1
    return ((-(-npx // VALID_PAIRS) + 3) // 4, -(-npy // rp), n)


def pick_row_pairs(n, max_w, max_h, synthesis, rp_env=0):
    npx, npy = (max_w + 2) >> 1, (max_h + 2) >> 1
    chunks = max(-(-4096 // (-(-npx // VALID_PAIRS) * n)), 1)
    rp, rp_min = -(-npy // chunks), rp_env or (4 if synthesis else 8)
    rp = (rp + 3) & ~3 if rp_min >= 4 else (rp + 1) & ~1
    return min(max(rp, rp_min), 20)


def heights(rp):
    return (1, 2, 3, 2 * rp - 1, 2 * rp, 2 * rp + 1, 2 * rp + 2, 4 * rp - 1, 4 * rp + 1, 6 * rp + 3)


def tall_height(rp):
    """18 chunks: with the one workgroup column of these widths, 18 workgroups per plane -- 16 or more, so the XCD permutation
    engages, and no multiple of 8, so every plane after the first starts at another XCD (about 700 rows at 20 row pairs)"""
    return 34 * rp + 3


def planes(rp):
    """[(h, w, x_even, y_even)]: every width with a height of three chunks or more, every height with a width of three strips
    or more, the tall narrow plane last; the parities cycle"""
    hs = heights(rp)
    hw = [(hs[8 + i % 2], w) for i, w in enumerate(WIDTHS)] + [(h, WIDE[i % 4]) for i, h in enumerate(hs)] + [(tall_height(rp), TALL_W)]
    return [(h, w, i & 1, (i >> 1) & 1) for i, (h, w) in enumerate(hw)]


def strips_of(w, x_even):
    return -(-((w + (0 if x_even else 1) + 1) >> 1) // VALID_PAIRS)


def chunks_of(h, y_even, rp):
    return -(-((h + (0 if y_even else 1) + 1) >> 1) // rp)


def coverage_problems(ps, rp):
    """what the plane set must satisfy (-> a list of what it does not)"""
    bad = []
    if {(xe, ye) for (_, _, xe, ye) in ps} != {(0, 0), (0, 1), (1, 0), (1, 1)}:
        bad.append("not all four origin parities")
    for w in WIDTHS:
        if not any(pw == w and chunks_of(h, ye, rp) >= 3 for (h, pw, xe, ye) in ps):
            bad.append("width %d with no height of three chunks" % w)
    for h in heights(rp):
        if not any(ph == h and strips_of(w, xe) >= 3 for (ph, w, xe, ye) in ps):
            bad.append("height %d with no width of three strips" % h)
    if len(ps) < 9:
        bad.append("fewer than 9 planes")
    gx, gy, _ = dwt_grid(len(ps), max(p[1] for p in ps), max(p[0] for p in ps), rp)
    if gx * gy < 16 or gx * gy % 8 == 0:
        bad.append("%d x %d workgroups per plane: the XCD permutation needs 16 or more, and no multiple of 8" % (gx, gy))
    return bad


class Launch:
    """tag; planes [(h, w, x_even, y_even)]; descs (tests build codec.dwt_desc_dtype from these dicts); arena (uint32) and
    image (unsigned, container-sized; None: no image side) as they are before the launch; out = "arena" | "image";
    rects [(plane index, name, off, pitch, want)] inside buffer `out`, want 2-D unsigned; sentinels: the values the image is
    filled with (inverse image forms: the launch runs once per value); extra: per-form data"""
    def __init__(self, **kw):
        self.regions, self.sentinels, self.extra, self.image = None, (), {}, None
        self.__dict__.update(kw)

    @property
    def max_w(self):
        return max(p[1] for p in self.planes)

    @property
    def max_h(self):
        return max(p[0] for p in self.planes)


def rect_index(off, pitch, h, w):
    return off + np.arange(h, dtype=np.int64)[:, None] * pitch + np.arange(w, dtype=np.int64)[None, :]


def rect_problems(rects, size):
    """the output rectangles lie inside their buffer and no two share an element"""
    count = np.zeros(size, np.uint8)
    bad = []
    for (i, name, off, pitch, want) in rects:
        h, w = want.shape
        if not want.size:
            continue
        if off < 0 or pitch < w or off + (h - 1) * pitch + w > size:
            bad.append("plane %d %s leaves its buffer" % (i, name))
            continue
        count[rect_index(off, pitch, h, w)] += 1
    if count.max(initial=0) > 1:
        bad.append("%d elements in more than one output rectangle" % int((count > 1).sum()))
    return bad


def verify(launch, before, after, tag):
    """`after` (the output buffer read back) against the launch's rectangles, bit for bit; every element outside them must be
    what `before` held.  Reports the smallest failing plane."""
    covered = np.zeros(after.size, bool)
    failed = []
    for (i, name, off, pitch, want) in launch.rects:
        if not want.size:
            continue
        idx = rect_index(off, pitch, *want.shape)
        got = after[idx]
        covered[idx] = True
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            h, w, xe, ye = launch.planes[i]
            failed.append((h * w, "plane %d (%d rows x %d columns, x_even %d, y_even %d) %s: %d of %d differ, rows %d-%d, columns %d-%d"
                           % (i, h, w, xe, ye, name, len(bad), want.size, bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max())))
    assert not failed, "%s: %d output rectangles differ from the oracle; the smallest plane: %s" % (tag, len(failed), min(failed)[1])
    stray = np.flatnonzero((before != after) & ~covered)
    assert not stray.size, "%s: %d elements outside the output rectangles changed, the first at element %d (0x%x -> 0x%x)" % (
        tag, stray.size, stray[0], int(before[stray[0]]), int(after[stray[0]]))


class _Arena:
    """planes in a flat arena the way the codec lays them out (pitch a multiple of 64) but never tight: a pitch beyond the
    width and 64 to 192 elements of gap after every plane"""
    def __init__(self):
        self.total, self.n = 64, 0

    def place(self, h, w):
        pitch = (w & ~63) + 64
        off = self.total
        self.total += pitch * max(h, 1) + 64 * (1 + self.n % 3)
        self.n += 1
        return off, pitch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _ob():
    from oracle import oraclebind as ob
    return ob


# ---- arena planes: codec.dwt (5/3, 9/7) and codec.dwt_general (an ATK kernel; both directions, rows only, columns only) ----
def _kernel(kind):
    """-> (dtype, forward, inverse, horz, vert) of "53" | "97" | "rev" | "irv" [+ "-horz" | "-vert"]"""
    ob = _ob()
    base, _, mode = kind.partition("-")
    horz, vert = mode != "vert", mode != "horz"
    if base == "53":
        return np.int32, ob.dwt53_fwd, ob.dwt53_inv, True, True
    if base == "97":
        return np.float32, ob.dwt97_fwd, ob.dwt97_inv, True, True
    _, dt, steps, K = GEN_REV if base == "rev" else GEN_IRV
    return (dt, lambda s, xe, ye: ob.dwt_fwd_gen(s, steps, K, horz, vert, xe, ye),
            lambda ll, hl, lh, hh, w, h, xe, ye: ob.dwt_inv_gen(ll, hl, lh, hh, w, h, steps, K, horz, vert, xe, ye), horz, vert)


@functools.lru_cache(maxsize=None)
def arena_launches(kind, rp):
    """-> (forward, inverse) launches of one kernel over planes(rp).  Integers of +-40000 (a wrap would show), floats in
    +-0.5; the inverse starts from the oracle's bands"""
    ob = _ob()
    dt, fwd, inv, horz, vert = _kernel(kind)
    ps = planes(rp)
    rng = np.random.default_rng(1000 + rp)
    ar = _Arena()
    descs, srcs, bands, where = [], [], [], []
    for (h, w, xe, ye) in ps:
        lw, hw, lh, hh = ob.band_dims(w, h, bool(xe), bool(ye))
        if not horz:
            lw, hw = w, 0
        if not vert:
            lh, hh = h, 0
        src = rng.integers(-40000, 40000, size=(h, w)).astype(np.int32) if dt == np.int32 else (rng.random((h, w)) - 0.5).astype(np.float32)
        o = [ar.place(h, w)] + [ar.place(bh, bw) for (bh, bw) in ((lh, lw), (lh, hw), (hh, lw), (hh, hw))]
        d = dict(w=w, h=h, x_even=xe, y_even=ye, src_off=o[0][0], src_pitch=o[0][1])
        for k, name in enumerate(("ll", "hl", "lh", "hh")):
            d[name + "_off"], d[name + "_pitch"] = o[1 + k]
        descs.append(d); srcs.append(src); where.append(o)
        bands.append([np.ascontiguousarray(b).reshape(s) for b, s in zip(fwd(src, bool(xe), bool(ye)), ((lh, lw), (lh, hw), (hh, lw), (hh, hw)))])
    sent = SENT_I if dt == np.int32 else SENT_F
    a_f, a_i = np.full(ar.total, sent, np.uint32), np.full(ar.total, sent, np.uint32)
    r_f, r_i = [], []
    for i, (h, w, xe, ye) in enumerate(ps):
        o = where[i]
        a_f[rect_index(o[0][0], o[0][1], h, w)] = _bits(srcs[i])
        for k, name in enumerate(("ll", "hl", "lh", "hh")):
            b = bands[i][k]
            r_f.append((i, name, o[1 + k][0], o[1 + k][1], _bits(b)))
            if b.size:
                a_i[rect_index(o[1 + k][0], o[1 + k][1], *b.shape)] = _bits(b)
        r_i.append((i, "plane", o[0][0], o[0][1], _bits(inv(*bands[i], w, h, bool(xe), bool(ye)))))
    common = dict(planes=ps, descs=descs, out="arena", nc=1, extra=dict(kind=kind, dtype=dt, horz=horz, vert=vert, srcs=srcs, sentinel=sent))
    return (Launch(tag="%s forward rp=%d" % (kind, rp), arena=a_f, rects=r_f, **common),
            Launch(tag="%s inverse rp=%d" % (kind, rp), arena=a_i, rects=r_i, **common))


# ---- image planes: codec.dwt_image (plain and colour) and codec.dwt_general_image ------------------------------------------
def to_container(v, container):
    """true sample values -> the bits an image container holds (low 8 / 16 / 32 bits), unsigned view"""
    bits = np.asarray(v, np.int64).astype(np.uint64)
    return bits.astype({32: np.uint32, 16: np.uint16, 8: np.uint8}[container])


def formats(n, container, colour, rng):
    """a depth and a sign per plane (per triple when colour): both ends of what the container takes, then random ones"""
    top = 26 if container == 32 else container
    fixed = [(top, False), (top, True), (1, False), (1, True), (max(top - 1, 1), True)]
    groups = n // 3 if colour else n
    out = [fixed[i] if i < len(fixed) else (int(rng.integers(1, top + 1)), bool(rng.integers(0, 2))) for i in range(groups)]
    return [f for f in out for _ in range(3)] if colour else out


@functools.lru_cache(maxsize=None)
def image_launches(rev, container, colour, general, rp):
    """-> (forward, inverse) launches of the fused top level, the expectations built the way tests/test_gpu_formats.py:
    _image_level builds them: the restatement for level shift / float conversion / RCT / ICT, the oracle for the lifting,
    saturation to the container on the way back (the low band pushed up by 9/8 so that the stores do saturate).
    general: None, or True for the ATK kernel of this reversibility.  inverse.extra["full"]: the expected image planes."""
    ob = _ob()
    geo = planes(rp)
    nc = 3 if colour else 1
    ps = [g for g in geo for _ in range(nc)]
    rng = np.random.default_rng(2000 + 8 * container + 4 * rev + 2 * colour + bool(general) + 100 * rp)
    fm = formats(len(ps), container, colour, rng)
    dt = np.int32 if rev else np.float32
    if general:
        _, _, steps, K = GEN_REV if rev else GEN_IRV
        fwd = lambda s, xe, ye: ob.dwt_fwd_gen(s, steps, K, True, True, xe, ye)
        inv = lambda ll, hl, lh, hh, w, h, xe, ye: ob.dwt_inv_gen(ll, hl, lh, hh, w, h, steps, K, True, True, xe, ye)
    else:
        fwd, inv = (ob.dwt53_fwd, ob.dwt53_inv) if rev else (ob.dwt97_fwd, ob.dwt97_inv)
    # the image: a few guard elements, then the planes back to back -- every other plane (triple) with a padded pitch
    ar = _Arena()
    descs, vals, img_off = [], [], 7
    for i, (h, w, xe, ye) in enumerate(ps):
        bd, sg = fm[i]
        pitch = w if (i // nc) % 2 == 0 else w + 5
        lw, hw, lh, hh = ob.band_dims(w, h, bool(xe), bool(ye))
        d = dict(w=w, h=h, x_even=xe, y_even=ye, src_off=img_off, src_pitch=pitch, reserved=bd | (0x100 if sg else 0))
        for name, (bh, bw) in zip(("ll", "hl", "lh", "hh"), ((lh, lw), (lh, hw), (hh, lw), (hh, hw))):
            d[name + "_off"], d[name + "_pitch"] = ar.place(bh, bw)
        descs.append(d)
        vals.append(rs.edge_samples(bd, sg, rng, h * w)[:h * w].reshape(h, w) if h * w > 12 else
                    rng.integers(*rs.sample_range(bd, sg), (h, w), endpoint=True))
        img_off += pitch * h
    img_size = img_off + 9
    work = [(rs.wrap32(rs.rev_forward(v.ravel(), bd, sg)) if rev else rs.irv_to_float(v.ravel(), bd, sg)).reshape(v.shape)
            for v, (bd, sg) in zip(vals, fm)]
    if colour:
        for t in range(0, len(ps), 3):
            r, g, b = work[t:t + 3]
            if rev:
                work[t:t + 3] = [rs.wrap32(x).reshape(r.shape) for x in rs.rct_forward(r.astype(np.int64), g.astype(np.int64), b.astype(np.int64))]
            else:
                work[t:t + 3] = list(rs.ict_forward(r, g, b))
    bands = [[np.ascontiguousarray(b) for b in fwd(work[i].astype(dt), bool(xe), bool(ye))] for i, (h, w, xe, ye) in enumerate(ps)]
    udt = {32: np.uint32, 16: np.uint16, 8: np.uint8}[container]
    image = np.full(img_size, IMAGE_SENTINELS[container][0], udt)
    arena_f = np.full(ar.total, SENT_I if rev else SENT_F, np.uint32)
    r_f = []
    for i, (h, w, xe, ye) in enumerate(ps):
        d = descs[i]
        image[rect_index(d["src_off"], d["src_pitch"], h, w)] = to_container(vals[i], container)
        for k, name in enumerate(("ll", "hl", "lh", "hh")):
            r_f.append((i, name, d[name + "_off"], d[name + "_pitch"], _bits(bands[i][k])))
    # the way back, from bands pushed past the range
    arena_i = np.full(ar.total, SENT_I if rev else SENT_F, np.uint32)
    syn = []
    for i, (h, w, xe, ye) in enumerate(ps):
        d = descs[i]
        bs = list(bands[i])
        if bs[0].size:
            bs[0] = (bs[0].astype(np.int64) * 9 // 8).astype(np.int32) if rev else (bs[0] * np.float32(1.125)).astype(np.float32)
        for k, name in enumerate(("ll", "hl", "lh", "hh")):
            if bs[k].size:
                arena_i[rect_index(d[name + "_off"], d[name + "_pitch"], *bs[k].shape)] = _bits(bs[k])
        syn.append(inv(*bs, w, h, bool(xe), bool(ye)))
    if colour:
        for t in range(0, len(ps), 3):
            y, cb, cr = syn[t:t + 3]
            syn[t:t + 3] = list(rs.rct_inverse(y, cb, cr)) if rev else list(rs.ict_inverse(y, cb, cr))
    r_i, full = [], []
    for i, (h, w, xe, ye) in enumerate(ps):
        bd, sg = fm[i]
        want = rs.wrap32(np.asarray(syn[i], np.int64) + rs.half(bd, sg)).astype(np.int64) if rev else rs.irv_to_int(syn[i], bd, sg).astype(np.int64)
        full.append(to_container(rs.saturate(want, container, sg), container).reshape(h, w))
        r_i.append((i, "image", descs[i]["src_off"], descs[i]["src_pitch"], full[-1]))
    tag = "%s%s container %d%s" % ("ATK " if general else "", "5/3" if rev else "9/7", container, " colour" if colour else "")
    common = dict(planes=ps, descs=descs, nc=nc)
    extra = dict(rev=rev, container=container, colour=colour, general=general, formats=fm, image_size=img_size, full=full, sentinel=SENT_I if rev else SENT_F,
                 bit_depth=min(max(f[0] for f in fm), 31 if container == 32 else container))
    return (Launch(tag="%s forward rp=%d" % (tag, rp), arena=arena_f, image=image, out="arena", rects=r_f, extra=extra, **common),
            Launch(tag="%s inverse rp=%d" % (tag, rp), arena=arena_i, image=None, out="image", rects=r_i, extra=extra,
                   sentinels=IMAGE_SENTINELS[container], **common))


# ---- codec.dwt_inverse_region, colour ------------------------------------------------------------------------------------
def _region_of(i, h, w, x_even, y_even, rp, whole_height):
    """a region whose first and last column lie inside the first, a middle or the last strip (planes of three strips and
    more; the pattern cycles with i) and whose first and last row lie in different vertical chunks where the plane has them"""
    ox = 0 if x_even else 1
    ns = strips_of(w, x_even)

    def col(s, quarter):                                    # a column inside strip s
        lo, hi = max(2 * VALID_PAIRS * s - ox, 0), min(2 * VALID_PAIRS * (s + 1) - ox, w)
        return lo + (hi - lo) * quarter // 4
    sa, sb = [(0, ns - 1), (0, ns // 2), (ns // 2, ns - 1), (ns // 2, ns // 2), (0, 0), (ns - 1, ns - 1)][i % 6] if ns >= 3 else (0, ns - 1)
    x0 = min(col(sa, 1), w - 1)
    x1 = min(max(col(sb, 3), x0 + 1), w)
    ya, yb = (1, h - 1) if whole_height else [(0, h), (1, h - 1), (2 * rp + 1, h - 2), (2 * rp - 1, 4 * rp + 2), (3, 2 * rp + 3), (h // 2, h // 2 + 1)][(i // 2) % 6]
    y0 = min(ya, h - 1)
    y1 = min(max(yb, y0 + 1), h)
    return x0, y0, x1, y1


def region_grid(planes_, regions):
    """restatement of dwt_region_grid_add (kernels_dwt.hip) -> (strips, row pairs) the launch is sized from; input check only"""
    strips = pairs = 0
    for (h, w, xe, ye), (x0, y0, x1, y1) in zip(planes_, regions):
        ox, oy = 1 - xe, 1 - ye
        px0, px1 = (x0 + ox) >> 1, ((x1 - 1 + ox) >> 1) + 1
        py0, py1 = (y0 + oy) >> 1, ((y1 - 1 + oy) >> 1) + 1
        strips = max(strips, (px1 - 1) // VALID_PAIRS - px0 // VALID_PAIRS + 1)
        pairs = max(pairs, py1 - py0)
    return strips, pairs


@functools.lru_cache(maxsize=None)
def region_launch(rev, container, rp):
    """the colour triples of image_launches(...)[1] synthesised through a window each: the expectation is the crop of the whole
    plane's.  The region frames lie back to back behind a few guard elements, every other triple with a padded pitch."""
    inv = image_launches(rev, container, True, None, rp)[1]
    regions, rects, off = [], [], 5
    for i, (h, w, xe, ye) in enumerate(inv.planes):
        t = i // 3
        x0, y0, x1, y1 = _region_of(t, h, w, xe, ye, rp, whole_height=(w == TALL_W))
        pitch = (x1 - x0) + (3 if t % 2 else 0)
        regions.append(dict(rx0=x0, ry0=y0, rx1=x1, ry1=y1, out_off=off, out_pitch=pitch))
        rects.append((i, "region (%d, %d)-(%d, %d)" % (x0, y0, x1, y1), off, pitch, np.ascontiguousarray(inv.extra["full"][i][y0:y1, x0:x1])))
        off += pitch * (y1 - y0)
    extra = dict(inv.extra, image_size=off + 9)
    return Launch(tag="region %s rp=%d" % (inv.tag, rp), planes=inv.planes, descs=inv.descs, regions=regions, arena=inv.arena, image=None,
                  out="image", rects=rects, extra=extra, sentinels=IMAGE_SENTINELS[container], nc=3)


# ---- the sweep: (test id, builder) of every launch pair; `h` = chunk_heights(...) ---------------------------------------
ARENA_KINDS = ("53", "97", "rev", "rev-horz", "rev-vert", "irv", "irv-horz", "irv-vert")
IMAGE_FORMS = [(rev, container, colour, general) for general in (None, True) for rev in (True, False) for container in (32, 16, 8)
               for colour in ((False, True) if not general else (False,))]
REGION_FORMS = [(rev, container) for rev in (True, False) for container in (32, 16, 8)]


def arena_rp(kind, direction, h):
    """the chunk height a launch of this kernel gets (the caps only in the 5/3 and 9/7 launches; the one-direction modes and
    the ATK kernels go through pick_row_pairs alone)"""
    return h[("plain_" if kind in ("53", "97") else "") + ("fwd" if direction == "forward" else "inv")]


def image_rp(colour, direction, h):
    return h["colour"] if colour else h["fwd" if direction == "forward" else "inv"]
