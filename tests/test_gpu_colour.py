"""ojphgpu_frame_rgb_to_ycc / _ycc_to_rgb (openjph_amd/csrc/kernels_colour.hip) against pipeline.rgb_to_ycc / ycc_to_rgb, bit
for bit: both directions, the four factor pairs, every size from 1 x 1 to 19 x 7, the nine container pairings, planes that
start on every residue of their 16 bytes, a destination two bytes off, tables of several standards and depths and a hostile
one, a frame wide and tall enough that threads take further turns under OJPHGPU_COLOUR_WGS=2, the refusals -- and a
sentinel around every destination plane."""
import itertools

import numpy as np
import pytest

from openjph_amd import pipeline

pytestmark = pytest.mark.gpu

GAP = 3                                                      # sentinel elements between planes
SENTINEL = {8: 0x5A, 16: 0x5A5A, 32: 0x5A5A5A5A}
NP = {8: np.uint8, 16: np.uint16, 32: np.uint32}
FACTORS = ((1, 1), (2, 1), (1, 2), (2, 2))
# large coefficients of mixed sign, offsets far out both ways, a clamp that is not the container's: the 64-bit sum, both clamp ends
HOSTILE = pipeline.ColourTable(((2 ** 30 + 12345, -(2 ** 30) + 7, 999), (-(2 ** 31) + 1, 2 ** 31 - 1, -3), (2 ** 29, 2 ** 29 + 1, -(2 ** 30))),
                               (-(2 ** 44), 2 ** 40 + 5, 2 ** 45), (3, 0, 17), (200, 2 ** 31 - 1, 40000), 16)


def tables(direction, sbits):
    """[(table, the depth its source side holds)]: tables whose source side fits the source's containers"""
    d = min(sbits, 16)
    mk = lambda std, sd, dd, rr, yr: (pipeline.colour_table(std, direction, *((sd, dd) if direction == "forward" else (dd, sd)), rr, yr), sd)
    t = [mk("bt709", d, d, "full", "narrow"), mk("bt601", d, 10, "full", "full"), mk("bt2020", d, 16, "narrow", "narrow"), (HOSTILE, d),
         mk("bt709", d, 8, "narrow", "full")]
    if sbits > 8:
        t += [mk("bt2020", 10, 10, "full", "narrow"), mk("bt601", 12, 8, "narrow", "narrow")]
    return t


def plane_shapes(direction, w, h, fx, fy):
    cw, ch = (w + 1) // 2 if fx == 2 else w, (h + 1) // 2 if fy == 2 else h
    rgb, ycc = [(h, w)] * 3, [(h, w), (ch, cw), (ch, cw)]
    return (rgb, ycc) if direction == "forward" else (ycc, rgb)


def samples(shape, sbits, depth, rng):
    """mostly inside the depth's range, one in eight anywhere in the container"""
    v = rng.integers(0, 1 << depth, size=shape, dtype=np.int64)
    wild = rng.integers(0, 1 << sbits, size=shape, dtype=np.int64)
    return np.where(rng.random(shape) < 0.125, wild, v)


def run_frames(direction, sbits, dbits, cases, dst_off=0, seed=1):
    """cases: [(w, h, fx, fy, table, depth)]; every frame's six planes laid out with gaps in one source and one destination
    buffer, source plane p of case i on residue (i + 5 p) of its 16 bytes, destination plane on residue (3 i + 7 p)"""
    import torch
    from openjph_amd import codec
    rng = np.random.default_rng(seed)
    sper, dper = 16 // (sbits // 8), 16 // (dbits // 8)
    top = 2 ** 31 - 1 if dbits == 32 else (1 << dbits) - 1
    stage, state = (codec.rgb_to_ycc, pipeline.rgb_to_ycc) if direction == "forward" else (codec.ycc_to_rgb, pipeline.ycc_to_rgb)
    s_at, d_at, frames, chunks = GAP, GAP, [], []
    for i, (w, h, fx, fy, table, depth) in enumerate(cases):
        sshape, dshape = plane_shapes(direction, w, h, fx, fy)
        sfirst, dfirst, planes = [], [], []
        for p in range(3):
            s_at += (i + 5 * p - s_at) % sper
            d_at += (3 * i + 7 * p - d_at) % dper
            q = samples(sshape[p], sbits, depth, rng)
            sfirst.append(s_at); dfirst.append(d_at); planes.append(q)
            chunks.append((s_at, q))
            s_at += q.size + GAP
            d_at += dshape[p][0] * dshape[p][1] + GAP
        want = [np.clip(g, 0, top) for g in state(planes, table, fx, fy)]     # [lo, hi] narrowed to the container
        assert [g.shape for g in want] == list(dshape)
        frames.append((w, h, fx, fy, table, sfirst, dfirst, want))
    src = np.full(s_at + GAP, SENTINEL[sbits], np.int64)
    for first, q in chunks:
        src[first:first + q.size] = q.ravel()
    src = src.astype(NP[sbits])
    total = d_at + GAP
    view = lambda a: a.view(np.int32) if a.dtype == np.uint32 else a
    d_src = torch.from_numpy(view(src)).cuda()
    buf = torch.from_numpy(view(np.full(total + dst_off + 16, SENTINEL[dbits], NP[dbits]))).cuda()
    assert buf.data_ptr() % 16 == 0 and d_src.data_ptr() % 16 == 0
    d_out = buf[dst_off:dst_off + total]
    for (w, h, fx, fy, table, sfirst, dfirst, want) in frames:
        kw = dict(rgb_first=sfirst, ycc_first=dfirst) if direction == "forward" else dict(ycc_first=sfirst, rgb_first=dfirst)
        stage(d_src, table, w, h, fx, fy, out=d_out, **kw)
    mask = (1 << dbits) - 1
    got = d_out.cpu().numpy().astype(np.int64) & mask
    keep = np.ones(total, bool)
    for i, (w, h, fx, fy, table, sfirst, dfirst, want) in enumerate(frames):
        for p in range(3):
            g = want[p].ravel()
            assert np.array_equal(got[dfirst[p]:dfirst[p] + g.size], g), (direction, sbits, dbits, i, p, cases[i][:4])
            keep[dfirst[p]:dfirst[p] + g.size] = False
    assert (got[keep] == SENTINEL[dbits]).all(), "written outside a destination plane"
    assert np.array_equal(d_src.cpu().numpy(), view(src))      # the source is only read
    whole = buf.cpu().numpy().astype(np.int64) & mask
    assert (whole[:dst_off] == SENTINEL[dbits]).all() and (whole[dst_off + total:] == SENTINEL[dbits]).all()


def small_cases(direction, sbits, widths=range(1, 20), heights=range(1, 8)):
    """every size under the four factor pairs, the tables taken in turn (seven or five of them against four factor pairs: coprime)"""
    tabs = tables(direction, sbits)
    return [(w, h, fx, fy) + tabs[i % len(tabs)] for i, (w, h, (fx, fy)) in enumerate(itertools.product(widths, heights, FACTORS))]


@pytest.mark.parametrize("dbits", [8, 16, 32])
@pytest.mark.parametrize("sbits", [8, 16, 32])
@pytest.mark.parametrize("direction", ["forward", "inverse"])
def test_every_small_size_factor_and_container_pairing(direction, sbits, dbits):
    cases = small_cases(direction, sbits)
    assert len(cases) == 19 * 7 * 4
    run_frames(direction, sbits, dbits, cases)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("direction", ["forward", "inverse"])
def test_a_destination_two_bytes_off(direction, bits):
    cases = small_cases(direction, 16, widths=(4, 8, 9, 16, 17, 19), heights=(1, 2, 3, 7))
    run_frames(direction, 16, bits, cases, dst_off=2 // (bits // 8), seed=3)


def test_a_32_bit_destination_one_element_off():
    for direction in ("forward", "inverse"):
        cases = small_cases(direction, 8, widths=(4, 8, 9, 16, 17, 19), heights=(1, 2, 3, 7))
        run_frames(direction, 8, 32, cases, dst_off=1, seed=4)


@pytest.mark.parametrize("sbits,dbits", [(16, 16), (8, 32), (32, 8)])
@pytest.mark.parametrize("direction", ["forward", "inverse"])
def test_threads_take_second_and_third_turns(direction, sbits, dbits, monkeypatch):
    """two workgroups, 512 threads, over a 2100 x 37 frame: 263 (16-bit and 8-bit sources) or 525 (32-bit) column groups x 3 to
    5 row bands, so every thread comes round again and a band -- rows walked down with the carried sums -- begins in one
    turn's threads and ends in the next turn's.  Rows of 2100 samples stand on the load's boundary only every other (or
    fourth) row: both the wide and the sample-by-sample path; rows of 2104 always do."""
    monkeypatch.setenv("OJPHGPU_COLOUR_WGS", "2")
    d = min(sbits, 16)
    t = pipeline.colour_table("bt709", direction, d, d)
    cases = [(2100, 37, fx, fy, t, d) for fx, fy in FACTORS] + [(2104, 38, 2, 2, t, d), (2099, 36, 2, 1, HOSTILE, d)]
    run_frames(direction, sbits, dbits, cases, seed=5)


def test_defaults_and_the_grid_cap_does_not_change_the_result(monkeypatch):
    """planes one after the other, a new output tensor; any OJPHGPU_COLOUR_WGS (a useless one: the default) gives the same"""
    import torch
    from openjph_amd import codec
    rng = np.random.default_rng(8)
    w, h = 67, 21
    rgb = [rng.integers(0, 1024, size=(h, w)) for _ in range(3)]
    fwd, inv = pipeline.colour_table("bt709", "forward", 10, 10), pipeline.colour_table("bt709", "inverse", 10, 10)
    d_rgb = torch.from_numpy(np.stack(rgb).astype(np.uint16)).cuda()
    for fx, fy in FACTORS:
        want = pipeline.rgb_to_ycc(rgb, fwd, fx, fy)
        flat = np.concatenate([q.ravel() for q in want])
        back = np.concatenate([q.ravel() for q in pipeline.ycc_to_rgb(want, inv, fx, fy)])
        for wgs in ("1", "3", "0", "junk", None):
            if wgs is None:
                monkeypatch.delenv("OJPHGPU_COLOUR_WGS", raising=False)
            else:
                monkeypatch.setenv("OJPHGPU_COLOUR_WGS", wgs)
            d_ycc = codec.rgb_to_ycc(d_rgb, fwd, w, h, fx, fy)
            assert d_ycc.dtype == torch.uint16 and np.array_equal(d_ycc.cpu().numpy().astype(np.int64), flat)
            d_back = codec.ycc_to_rgb(d_ycc, inv, w, h, fx, fy, dtype=torch.int32)
            assert d_back.dtype == torch.int32 and np.array_equal(d_back.cpu().numpy().astype(np.int64), back)


def test_refusals():
    import ctypes as C
    import torch
    from openjph_amd import capi
    L = capi.lib()
    src = torch.zeros(4096, dtype=torch.int32, device="cuda")
    out = torch.full((4096,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    good_t = capi.ColourTable()
    assert L.ojphgpu_colour_table_make(709, 0, 8, 8, 0, 1, good_t) == capi.OK

    def frame(w=8, h=4, fx=2, fy=2, rgb=(0, 32, 64), ycc=(0, 32, 40)):
        f = capi.ColourFrame(w, h, fx, fy)
        f.rgb_first[:] = rgb
        f.ycc_first[:] = ycc
        return f

    def table(**kw):
        t = capi.ColourTable()
        C.memmove(C.byref(t), C.byref(good_t), C.sizeof(t))
        for k, v in kw.items():
            if k == "k":
                t.k = v
            else:
                getattr(t, k)[:] = v
        return t
    for fn in (L.ojphgpu_frame_rgb_to_ycc, L.ojphgpu_frame_ycc_to_rgb):
        ok = lambda s=p(src), sb=8, d=p(out), db=8, f=frame(), t=good_t: fn(None, s, sb, d, db, C.byref(f) if f is not None else None, C.byref(t) if t is not None else None)
        for fx, fy in ((0, 1), (1, 0), (3, 1), (1, 4), (2 ** 32 - 1, 2)):
            assert ok(f=frame(fx=fx, fy=fy)) == capi.E_INVALID                  # a factor other than 1 or 2
        assert ok(t=table(k=15)) == capi.E_INVALID and ok(t=table(k=0)) == capi.E_INVALID
        for bits in (0, 12, 24, 64, -8):
            assert ok(sb=bits) == capi.E_INVALID and ok(db=bits) == capi.E_INVALID   # no such container
        assert ok(f=frame(w=0)) == capi.E_INVALID and ok(f=frame(h=0)) == capi.E_INVALID
        assert ok(s=None) == capi.E_INVALID and ok(d=None) == capi.E_INVALID and ok(f=None) == capi.E_INVALID and ok(t=None) == capi.E_INVALID
        assert ok(s=p(src, 1), sb=16) == capi.E_INVALID and ok(d=p(out, 2), db=32) == capi.E_INVALID   # off the container's alignment
        assert ok(t=table(lo=(9, 0, 0), hi=(3, 255, 255))) == capi.E_INVALID
        assert ok(t=table(lo=(300, 0, 0), hi=(1000, 255, 255))) == capi.E_INVALID                    # nothing of [lo, hi] fits the container
        # overlapping source and destination: in place, a destination plane inside a source plane, the last byte of one on
        # the first of the other
        assert ok(d=p(src)) == capi.E_INVALID
        assert ok(d=p(src, 40)) == capi.E_INVALID
        assert ok(d=p(src, 95), f=frame(fx=1, fy=1, ycc=(0, 32, 64))) == capi.E_INVALID
        assert ok(d=p(src, 96), f=frame(fx=1, fy=1, ycc=(0, 32, 64))) == capi.OK                     # behind it: apart
    torch.cuda.synchronize()
    # the refused calls wrote nothing; the two accepted ones (8-bit containers, 3 x 32 samples from byte 96 of src) are not in `out`
    assert (out.cpu().numpy() == 0x5A5A5A5A).all()
