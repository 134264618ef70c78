"""Region decoding on the host (ojphgpu_plan_restrict_region): the block selection is the dependency rule -- decoding only the
selected blocks and synthesising the whole frame gives the region's samples exactly -- the region frame's geometry, and the
calls that are refused.  No GPU: the oracle pipeline does the decoding."""
import numpy as np
import pytest

from openjph_amd import capi
from openjph_amd.plan import parse_codestream
from tests import cpu_pipeline as cp
from tests.region_cases import CASES, SKIPS, crop, encode_case, random_cs, regions_for


def _block_view(plan, arena, k):
    blk = plan.blocks[k]
    band = plan.bands[int(blk["band"])]
    off = int(band["plane_off"]) + int(blk["y0"]) * int(band["pitch"]) + int(blk["x0"])
    return cp._view(arena, off, int(band["pitch"]), int(blk["w"]), int(blk["h"]), np.uint32)


def check_garbage(cs, region, skip=None, seed=0):
    """decode every block, overwrite those the region does not select with random bits, synthesise: the region is unchanged"""
    full = parse_codestream(cs)
    reg = parse_codestream(cs)
    if skip:
        full.restrict_resolution(*skip)
        reg.restrict_resolution(*skip)
    reg.restrict_region(*region)
    mask = reg.region_blocks()
    readable = full.region_blocks()                      # the blocks a whole-frame decode decodes
    assert not (mask & ~readable).any()
    arena = cp.decode_blocks(full, cs)
    want = crop(full, cp.inverse_stages(full, arena.copy()), reg)
    rng = np.random.default_rng(seed)
    for k in np.nonzero(readable & ~mask)[0]:
        v = _block_view(full, arena, int(k))
        v[:] = rng.integers(0, 1 << 32, v.shape, dtype=np.uint64).astype(np.uint32)
    got = crop(full, cp.inverse_stages(full, arena), reg)
    for c, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape
        assert np.array_equal(a, b), "component %d of region %s differs" % (c, region)
    return int(mask.sum()), int(readable.sum())


@pytest.mark.parametrize("name,kw,size", CASES, ids=[c[0] for c in CASES])
def test_unselected_blocks_do_not_reach_the_region(name, kw, size):
    cs = encode_case(kw, size)
    for i, r in enumerate(regions_for(size)):
        check_garbage(cs, r, seed=i)


@pytest.mark.parametrize("skip", [s[1] for s in SKIPS], ids=[s[0] for s in SKIPS])
@pytest.mark.parametrize("name", ["rev-L5", "irv-L4", "420", "colour"])
def test_unselected_blocks_with_skipped_resolutions(name, skip):
    _, kw, size = next(c for c in CASES if c[0] == name)
    cs = encode_case(kw, size)
    for i, r in enumerate(regions_for(size, seed=7)):
        check_garbage(cs, r, skip=skip, seed=i)


@pytest.mark.parametrize("seed", range(8))
def test_unselected_blocks_random_parameter_sets(seed):
    cs, size = random_cs(seed)
    for i, r in enumerate(regions_for(size, seed=seed)[:6]):
        check_garbage(cs, r, seed=i)


def _ceil(a, b):
    return -(-a // b)


@pytest.mark.parametrize("skip", [None, (1, 1), (2, 1)])
def test_region_frame_geometry(skip):
    _, kw, size = next(c for c in CASES if c[0] == "420")
    cs = encode_case(kw, size)
    pl = parse_codestream(cs)
    if skip:
        pl.restrict_resolution(*skip)
    x0, y0, w, h = 3, 5, 40, 33
    pl.restrict_region(x0, y0, w, h)
    p = pl.params
    ax0, ay0 = p.image_x0 + x0, p.image_y0 + y0
    off = 0
    for c in range(int(p.num_comps)):
        ci = pl.comp_info(c)
        fx, fy = ci["dx"] << (skip[1] if skip else 0), ci["dy"] << (skip[1] if skip else 0)
        assert (ci["x0"], ci["y0"]) == (_ceil(ax0, fx), _ceil(ay0, fy))
        assert (ci["w"], ci["h"]) == (_ceil(ax0 + w, fx) - ci["x0"], _ceil(ay0 + h, fy) - ci["y0"])
        assert ci["frame_off"] == off
        off += ci["w"] * ci["h"]
    assert pl.frame_elems == off


def test_full_region_selects_the_blocks_of_a_full_decode():
    for name in ("rev-L5", "odd-offsets-tiles", "420"):
        _, kw, size = next(c for c in CASES if c[0] == name)
        cs = encode_case(kw, size)
        pl = parse_codestream(cs)
        want = pl.region_blocks()
        pl.restrict_region(0, 0, *size)
        assert np.array_equal(pl.region_blocks(), want)


def test_small_interior_region_selects_few_blocks():
    cs = encode_case(dict(reversible=True, num_decomps=5, block=(64, 64)), (2048, 2048))
    pl = parse_codestream(cs)
    assert pl.num_blocks == 1024
    pl.restrict_region(1000, 900, 64, 64)
    assert pl.region_blocks().sum() < 0.1 * 1024


def test_refusals_leave_the_plan_usable():
    _, kw, size = next(c for c in CASES if c[0] == "rev-L5")
    cs = encode_case(kw, size)
    W, H = size
    want, _ = cp.decode(cs)
    pl = parse_codestream(cs)
    for r in [(0, 0, 0, 5), (0, 0, 5, 0), (W, 0, 1, 1), (0, H, 1, 1), (W - 3, 0, 4, 2), (0, H - 1, 1, 2)]:
        with pytest.raises(capi.OjphError) as e:
            pl.restrict_region(*r)
        assert e.value.code == capi.E_INVALID
    assert pl.frame_elems == W * H
    np.testing.assert_array_equal(cp.inverse_stages(pl, cp.decode_blocks(pl, cs)), want)
    pl.restrict_region(1, 2, 10, 10)
    with pytest.raises(capi.OjphError) as e:                # a second restriction
        pl.restrict_region(0, 0, 5, 5)
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.OjphError) as e:                # restrict_resolution after restrict_region
        pl.restrict_resolution(1, 1)
    assert e.value.code == capi.E_INVALID


def test_general_lifting_plans_are_refused():
    from tests import part2_cases as p2
    cases = [p2.CASES[0], p2.CASES[2], p2.CASES[-1]]   # an ATK wavelet, a DFS decomposition, 64-bit samples under a DFS one
    cases.append(dict(nc=1, h=64, w=64, bd=32, num_decomps=2))      # 64-bit samples alone
    for case in cases:
        nc, h, w, bd, kw = p2.split(case)
        img = p2.image(nc, h, w, bd)
        cs = cp.encode(img, **kw)[0]
        want, _ = cp.decode(cs)
        pl = parse_codestream(cs)
        with pytest.raises(capi.OjphError) as e:
            pl.restrict_region(0, 0, 8, 8)
        assert e.value.code == capi.E_INVALID
        got = cp.inverse_stages(pl, cp.decode_blocks(pl, cs))
        np.testing.assert_array_equal(np.asarray(got), np.asarray(want))
