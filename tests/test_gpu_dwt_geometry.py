"""The DWT kernels under every launch geometry: each whole-plane launch form (codec.dwt, codec.dwt_image plain and colour,
codec.dwt_general in its three modes, codec.dwt_general_image) and the colour region synthesis, over planes built around the
120-column strip, the vertical chunk and the origin parities (tests/dwt_geometry_cases.py), bit for bit against the oracle --
and every element outside the output rectangles (pitch padding, gaps, guards, the inputs) must be what it was before the launch.

The work split comes from knobs that are read once per process (OJPHGPU_DWT_RP_MIN / _RP_COLOUR / _RP_INV / _RP_FWD / _TRIP /
_XCD): the test_sweep_* tests run under whatever the environment sets -- nothing, when the suite runs them -- and build their
planes around the chunk heights that yields; test_sweep_under_knobs starts them again in a child process per setting."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dwt_geometry_cases as gc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _heights():
    return gc.chunk_heights(gc.knobs_of(os.environ))


def _tag(launch):
    k = gc.knobs_of(os.environ)
    return "%s [RP_MIN %d RP_COLOUR %d RP_INV %d RP_FWD %d TRIP %s XCD %d]" % (
        launch.tag, k["RP_MIN"], k["RP_COLOUR"], k["RP_INV"], k["RP_FWD"], os.environ.get("OJPHGPU_DWT_TRIP", "-"), k["XCD"])


def _descs(launch):
    from openjph_amd import codec
    descs = np.zeros(len(launch.descs), codec.dwt_desc_dtype)
    for d, src in zip(descs, launch.descs):
        for k, v in src.items():
            d[k] = v
    return descs


def _check_inputs(launch, rp, pick=None):
    """the planes are the intended ones for this launch: the chunk height the launch arithmetic gives them is `rp`, and a plane
    takes 16 or more workgroups, no multiple of 8, so that the XCD permutation runs with a per-plane offset.  (Restatements
    of dwt_grid / pick_row_pairs: they check the inputs, not the kernel.)"""
    n = len(launch.planes) // launch.nc
    gx, gy, _ = gc.dwt_grid(n, launch.max_w, launch.max_h, rp)
    assert gx * gy >= 16 and (gx * gy) % 8 != 0 and n >= 9
    assert not gc.coverage_problems(launch.planes[::launch.nc], rp)
    if pick is not None:
        assert pick == rp


def _picked(launch, synthesis, capped):
    """pick_row_pairs' answer for this launch under the environment's knobs, then the caps of the 5/3 and 9/7 launches"""
    k = gc.knobs_of(os.environ)
    rp = gc.pick_row_pairs(len(launch.planes), launch.max_w, launch.max_h, synthesis, k["RP_MIN"])
    cap = k["RP_INV" if synthesis else "RP_FWD"]
    return cap if capped and cap and rp == 20 else rp


def _dev32(a):
    return torch.from_numpy(a.view(np.int32)).cuda()


def _image_tensor(a):
    return torch.from_numpy(a.view({1: np.int8, 2: np.int16, 4: np.int32}[a.dtype.itemsize])).cuda()


def _back(t, like):
    return t.cpu().numpy().view(like.dtype)


# ---- arena planes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["forward", "inverse"])
@pytest.mark.parametrize("kind", gc.ARENA_KINDS)
def test_sweep_arena(kind, direction):
    """codec.dwt (5/3, 9/7) and codec.dwt_general (a reversible and an irreversible ATK kernel; both directions, rows only,
    columns only): bands / planes == the oracle's, nothing else in the arena touched"""
    from openjph_amd import codec
    rp = gc.arena_rp(kind, direction, _heights())
    L = gc.arena_launches(kind, rp)[direction == "inverse"]
    _check_inputs(L, rp, _picked(L, direction == "inverse", kind in ("53", "97")))
    arena = _dev32(L.arena)
    if kind in ("53", "97"):
        codec.dwt(direction, kind == "53", _descs(L), arena, L.max_w, L.max_h)
    else:
        _, dt, steps, K = gc.GEN_REV if kind.startswith("rev") else gc.GEN_IRV
        codec.dwt_general(direction, steps, 0 if dt == np.int32 else 2, _descs(L), arena, L.max_w, L.max_h, K, L.extra["horz"], L.extra["vert"])
    gc.verify(L, L.arena, _back(arena, L.arena), _tag(L))


# ---- image planes ----------------------------------------------------------------------------------------------------------
def _params(L):
    from openjph_amd.plan import make_params
    e = L.extra
    return make_params(8, 8, num_comps=1, bit_depth=e["bit_depth"], reversible=e["rev"], color_transform=e["colour"])


def _run_image(L, direction, image, arena):
    from openjph_amd import codec
    e = L.extra
    if e["general"]:
        _, dt, steps, K = gc.GEN_REV if e["rev"] else gc.GEN_IRV
        codec.dwt_general_image(direction, steps, 0 if e["rev"] else 2, _params(L), _descs(L), image, arena, L.max_w, L.max_h, K, e["container"])
    else:
        codec.dwt_image(direction, _params(L), _descs(L), image, arena, L.max_w, L.max_h, e["container"], e["colour"])


@pytest.mark.parametrize("direction", ["forward", "inverse"])
@pytest.mark.parametrize("rev,container,colour,general", gc.IMAGE_FORMS,
                         ids=["%s%s-%d%s" % ("atk-" if g else "", "53" if r else "97", c, "-colour" if col else "") for (r, c, col, g) in gc.IMAGE_FORMS])
def test_sweep_image(rev, container, colour, general, direction):
    """the fused top level -- codec.dwt_image plain and in colour triples, codec.dwt_general_image -- on 32-, 16- and 8-bit
    containers, planes of mixed depths and signs: forward, the bands == restatement + oracle and the image untouched; inverse
    from bands pushed past the range, the image == oracle + restatement saturated to the container, the guards, the pitch
    padding and the arena untouched"""
    rp = gc.image_rp(colour, direction, _heights())
    L = gc.image_launches(rev, container, colour, general, rp)[direction == "inverse"]
    _check_inputs(L, rp, None if colour else _picked(L, direction == "inverse", not general))
    arena = _dev32(L.arena)
    if direction == "forward":
        image = _image_tensor(L.image)
        _run_image(L, direction, image, arena)
        gc.verify(L, L.arena, _back(arena, L.arena), _tag(L))
        assert np.array_equal(_back(image, L.image), L.image), "%s: the image was written" % _tag(L)
        return
    for s in L.sentinels:
        before = np.full(L.extra["image_size"], s, L.rects[0][4].dtype)
        image = _image_tensor(before)
        _run_image(L, direction, image, arena)
        gc.verify(L, before, _back(image, before), "%s, image filled with 0x%x" % (_tag(L), s))
    assert np.array_equal(_back(arena, L.arena), L.arena), "%s: the bands were written" % _tag(L)


# ---- colour region synthesis -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rev,container", gc.REGION_FORMS, ids=["%s-%d" % ("53" if r else "97", c) for (r, c) in gc.REGION_FORMS])
def test_sweep_region_colour(rev, container):
    """codec.dwt_inverse_region on colour triples, both wavelets, every container, planes of one to four strips: windows that
    begin and end inside the first, a middle and the last strip and in different vertical chunks == that part of the whole
    plane's synthesis; the rest of the region frames and the arena untouched.  (These launches always size their chunks with
    fit_rounds -- no knob reaches them -- so the planes are built around its first candidate, 4, under every setting; the trip
    and the XCD order still vary.)"""
    from openjph_amd import codec
    rp = _heights()["region_colour"]
    L = gc.region_launch(rev, container, rp)
    strips, pairs = gc.region_grid(L.planes[::3], [(r["rx0"], r["ry0"], r["rx1"], r["ry1"]) for r in L.regions[::3]])
    t = ((strips + 3) // 4) * -(-pairs // rp)                 # workgroups per triple (input check, as in _check_inputs)
    assert t >= 16 and t % 8 != 0 and len(L.planes) // 3 >= 9
    regs = np.zeros(len(L.regions), codec.dwt_region_dtype)
    for r, src in zip(regs, L.regions):
        for k, v in src.items():
            r[k] = v
    arena = _dev32(L.arena)
    for s in L.sentinels:
        before = np.full(L.extra["image_size"], s, L.rects[0][4].dtype)
        image = _image_tensor(before)
        codec.dwt_inverse_region(rev, _descs(L), regs, arena, image, container, colour=True)
        gc.verify(L, before, _back(image, before), "%s, image filled with 0x%x" % (_tag(L), s))
    assert np.array_equal(_back(arena, L.arena), L.arena), "%s: the bands were written" % _tag(L)


# ---- the same under the other geometries -----------------------------------------------------------------------------------
N_ARENA, N_IMAGE, N_REGION = 2 * len(gc.ARENA_KINDS), 2 * len(gc.IMAGE_FORMS), len(gc.REGION_FORMS)


@pytest.mark.parametrize("name", [n for n in gc.SETTINGS if n != "default"])
def test_sweep_under_knobs(name):
    """the sweep above in a child process per knob setting (tests/dwt_geometry_cases.py: SETTINGS; the knobs are read once per
    process): the shortest chunks, an odd chunk height under two row pairs per trip, a middle one, the large-level production
    geometry with the tallest colour chunk -- each with its trip and XCD order -- and the caps of the large 5/3 and 9/7
    launches, which no other form reads.  The children run one after another; one that fails is reported, not retried."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("OJPHGPU_DWT_")}
    env.update({"OJPHGPU_DWT_" + k: str(v) for k, v in gc.SETTINGS[name].items()})
    select, n = ("test_sweep_arena and (53 or 97)", 4) if name == "caps" else ("test_sweep_arena or test_sweep_image or test_sweep_region_colour", N_ARENA + N_IMAGE + N_REGION)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_dwt_geometry.py"), "-q", "-x", "-m", "gpu",
                        "-k", select, "-p", "no:cacheprovider"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and ("%d passed" % n).encode() in r.stdout, "setting %s %s:\n%s" % (
        name, gc.SETTINGS[name], r.stdout[-3000:].decode(errors="replace"))
