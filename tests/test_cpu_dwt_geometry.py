"""The harness of tests/test_gpu_dwt_geometry.py checked without a GPU: the case set of every knob setting is built whole
(tests/dwt_geometry_cases.py: numpy + oracle) and must be a sound net -- output rectangles disjoint and inside their buffers,
the planes around every strip / chunk / parity boundary of the chunk height the setting yields, a sentinel no expectation
holds, and an oracle whose 5/3 synthesis undoes its analysis on every plane."""
import numpy as np
import pytest

from tests import dwt_geometry_cases as gc


def _heights(name):
    env = {"OJPHGPU_DWT_" + k: str(v) for k, v in gc.SETTINGS[name].items()}
    return gc.chunk_heights(gc.knobs_of(env))


def test_chunk_heights_of_the_settings():
    """the knob table -> the chunk heights the sweep builds its planes around"""
    want = {"default": (8, 4, 4, 8, 4), "shortest": (2, 2, 2, 2, 2), "odd": (5, 5, 6, 5, 5), "mid": (12, 12, 12, 12, 12),
            "large": (20, 20, 24, 20, 20), "caps": (20, 20, 4, 36, 28)}
    for name, w in want.items():
        h = _heights(name)
        assert (h["fwd"], h["inv"], h["colour"], h["plain_fwd"], h["plain_inv"]) == w, name
    assert gc.knobs_of({"OJPHGPU_DWT_RP_MIN": "21", "OJPHGPU_DWT_XCD": "0"}) == dict(RP_MIN=0, RP_COLOUR=0, RP_INV=0, RP_FWD=0, XCD=0)


@pytest.mark.parametrize("rp", sorted({v for name in gc.SETTINGS for v in _heights(name).values()}))
def test_plane_set_covers_the_boundaries(rp):
    ps = gc.planes(rp)
    assert not gc.coverage_problems(ps, rp)
    assert 9 <= len(ps) <= 36
    # the launch arithmetic gives this chunk height to these planes (up to 20: beyond, only a cap or the colour knob sets it)
    for synthesis in (False, True):
        floor = 4 if synthesis else 8
        if floor <= rp <= 20:
            assert gc.pick_row_pairs(len(ps), max(p[1] for p in ps), max(p[0] for p in ps), synthesis, rp if rp != floor else 0) == rp
    if rp < 4:
        assert gc.pick_row_pairs(len(ps), max(p[1] for p in ps), max(p[0] for p in ps), True, rp) == rp
    # strips: a partial strip beside interior ones, exact multiples of the strip, one column more
    assert {gc.strips_of(w, xe) for (_, w, xe, _) in ps} >= {1, 2, 3, 4}


def _launches(name):
    h = _heights(name)
    plain_only = name == "caps"
    for kind in (("53", "97") if plain_only else gc.ARENA_KINDS):
        for k, direction in enumerate(("forward", "inverse")):
            yield gc.arena_launches(kind, gc.arena_rp(kind, direction, h))[k]
    if plain_only:
        return
    for (rev, container, colour, general) in gc.IMAGE_FORMS:
        for k, direction in enumerate(("forward", "inverse")):
            yield gc.image_launches(rev, container, colour, general, gc.image_rp(colour, direction, h))[k]
    for (rev, container) in gc.REGION_FORMS:
        yield gc.region_launch(rev, container, h["region_colour"])


@pytest.mark.parametrize("name", list(gc.SETTINGS))
def test_case_set_is_a_sound_net(name):
    n = 0
    for L in _launches(name):
        out = L.arena if L.out == "arena" else np.zeros(L.extra["image_size"], np.uint8)
        assert not gc.rect_problems(L.rects, out.size), L.tag
        assert len(L.planes) // L.nc >= 9, L.tag
        if L.out == "arena":                                   # the sentinel occurs in no expected output
            sent = L.extra["sentinel"]
            for (i, nm, off, pitch, want) in L.rects:
                assert not (want == sent).any(), (L.tag, i, nm)
        elif L.extra["container"] == 32:
            for (i, nm, off, pitch, want) in L.rects:
                assert not (want == gc.SENT_I).any(), (L.tag, i, nm)
        else:                                                  # every value is a sample: two runs under different sentinels
            assert len(set(L.sentinels)) == 2, L.tag
        # arena forms: outputs start as the sentinel, and outside them only the inputs differ from it -- so verify(), which
        # wants everything outside the rectangles unchanged, guards the inputs as well as the padding
        if L.out == "arena" and L.image is None:
            covered = np.zeros(L.arena.size, bool)
            for (i, nm, off, pitch, want) in L.rects:
                if want.size:
                    covered[gc.rect_index(off, pitch, *want.shape)] = True
            assert (L.arena[covered] == sent).all(), L.tag
            assert (L.arena[~covered] != sent).sum() == sum(p[0] * p[1] for p in L.planes), L.tag
        if L.regions is not None:
            gx, gy = gc.region_grid(L.planes[::3], [(r["rx0"], r["ry0"], r["rx1"], r["ry1"]) for r in L.regions[::3]])
            t = ((gx + 3) // 4) * -(-gy // 4)
            assert t >= 16 and t % 8, L.tag
            ns = [gc.strips_of(p[1], p[2]) for p in L.planes[::3]]
            assert sum(1 for s in ns if s >= 3) >= 9
        n += 1
    assert n == (4 if name == "caps" else 2 * len(gc.ARENA_KINDS) + 2 * len(gc.IMAGE_FORMS) + len(gc.REGION_FORMS))


def test_verify_notices_a_stray_store_and_a_wrong_sample():
    """verify() itself: a changed element in a gap, in an input, and inside a rectangle"""
    fwd, _ = gc.arena_launches("53", 4)
    good = fwd.arena.copy()
    for (i, nm, off, pitch, want) in fwd.rects:
        if want.size:
            good[gc.rect_index(off, pitch, *want.shape)] = want
    gc.verify(fwd, fwd.arena, good, "ok")
    d = fwd.descs[5]
    for at in (d["ll_off"] + fwd.rects[4 * 5][4].shape[1], d["src_off"], d["hh_off"] + 1):      # pitch padding, an input, an output
        bad = good.copy()
        bad[at] ^= 1
        with pytest.raises(AssertionError):
            gc.verify(fwd, fwd.arena, bad, "bad")


def test_oracle_53_synthesis_undoes_its_analysis():
    for rp in (2, 4, 5, 8, 12, 20, 24, 28, 36):
        fwd, inv = gc.arena_launches("53", rp)
        for (i, nm, off, pitch, want), src in zip(inv.rects, fwd.extra["srcs"]):
            assert np.array_equal(want.view(np.int32), src), (rp, fwd.planes[i])
