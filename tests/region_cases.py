"""Codestreams and regions the region-decoding tests share (tests/test_cpu_region.py, tests/test_gpu_region.py)."""
import numpy as np

from tests.random_cases import random_case

# (name, kwargs of plan.make_params, (W, H) on the reference grid)
CASES = [("rev-L%d" % L, dict(reversible=True, num_decomps=L), (77, 61)) for L in range(7)]
CASES += [("irv-L%d" % L, dict(reversible=False, num_decomps=L, qstep=0.01), (77, 61)) for L in range(7)]
CASES += [
    ("odd-offsets-tiles", dict(reversible=True, num_decomps=3, image_offset=(5, 3), tile=(40, 33), tile_offset=(2, 1)), (101, 90)),
    ("irv-odd-offsets-tiles", dict(reversible=False, num_decomps=4, qstep=0.02, image_offset=(7, 9), tile=(48, 40), tile_offset=(3, 4)), (110, 95)),
    ("tiles-2x2", dict(reversible=True, num_decomps=3, tile=(64, 64)), (128, 128)),
    ("420", dict(reversible=True, num_decomps=3, downsampling=[(1, 1), (2, 2), (2, 2)], image_offset=(1, 1)), (91, 67)),
    ("422-irv", dict(reversible=False, num_decomps=3, qstep=0.02, downsampling=[(1, 1), (2, 1), (2, 1)], image_offset=(3, 0)), (90, 64)),
    ("colour", dict(reversible=True, num_decomps=4, color_transform=True, nc=3), (96, 80)),
    ("colour-irv", dict(reversible=False, num_decomps=4, color_transform=True, qstep=0.01, nc=3), (96, 80)),
    ("block32", dict(reversible=True, num_decomps=4, block=(32, 32)), (150, 130)),
    ("block128x8", dict(reversible=False, num_decomps=3, block=(128, 8), qstep=0.02), (150, 100)),
]
SKIPS = [("skip11", (1, 1)), ("skip21", (2, 1))]


def planes_for(kw, size, seed=3):
    """per-component planes on the components' own grids for make_params' downsampling / offset"""
    w, h = size
    ox, oy = kw.get("image_offset", (0, 0))
    nc = kw.get("nc", len(kw.get("downsampling", [(1, 1)])))
    ds = kw.get("downsampling", [(1, 1)] * nc)
    bd = kw.get("bit_depth", 8)
    rng = np.random.default_rng(seed)
    out = []
    for c, (dx, dy) in enumerate(ds):
        cw = -(-(ox + w) // dx) - -(-ox // dx)
        ch = -(-(oy + h) // dy) - -(-oy // dy)
        yy, xx = np.mgrid[0:ch, 0:cw]
        base = ((np.sin(xx / 5.0 + c) + np.cos(yy / 3.0)) * 0.22 + 0.5) * ((1 << bd) - 1)
        out.append(np.clip(base + rng.integers(-12, 13, base.shape), 0, (1 << bd) - 1).astype(np.int32))
    return out


def encode_case(kw, size):
    from tests import cpu_pipeline as cp
    k = dict(kw)
    k.pop("nc", None)
    planes = planes_for(kw, size)
    if "downsampling" not in k:
        k["downsampling"] = [(1, 1)] * len(planes)
    return cp.encode(planes, size=size, **k)[0]


def random_cs(seed):
    """a codestream of tests/random_cases.py's seeded random parameter sets: the first of seeds seed, seed + 100, ... whose
    parameters can be coded and whose components are not empty"""
    from openjph_amd import capi
    from tests import cpu_pipeline as cp
    for s in range(seed, seed + 10000, 100):
        planes, kw, size = random_case(s)
        if any(q.size == 0 for q in planes):
            continue
        try:
            return cp.encode(planes, size=size, **kw)[0], size
        except capi.OjphError:
            continue
    raise AssertionError("no codable parameter set")


def regions_for(size, seed=0):
    """regions (x0, y0, w, h) relative to the image origin: every edge, the interior, 1 x 1, 1 x N, N x 1, the whole image"""
    W, H = size
    rng = np.random.default_rng(seed)
    out = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (W // 2, 0, 1, H), (0, H // 2, W, 1)]
    out += [(0, 0, max(W // 3, 1), max(H // 3, 1)), (W - max(W // 3, 1), H - max(H // 4, 1), max(W // 3, 1), max(H // 4, 1))]
    out += [(0, H // 3, max(W // 4, 1), max(H // 3, 1)), (W // 2, 0, W - W // 2, max(H // 5, 1))]
    for _ in range(3):
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        out.append((x0, y0, int(rng.integers(1, W - x0 + 1)), int(rng.integers(1, H - y0 + 1))))
    return sorted(set(out))


def crop(full_plan, full_frame, reg_plan):
    """the region frame's planes cut out of the whole frame (list of 2-D arrays per component)"""
    fp = list(full_frame) if isinstance(full_frame, list) else full_plan.unpack_frame(np.asarray(full_frame))
    out = []
    for c in range(int(reg_plan.params.num_comps)):
        f, r = full_plan.comp_info(c), reg_plan.comp_info(c)
        y0, x0 = r["y0"] - f["y0"], r["x0"] - f["x0"]
        out.append(fp[c][y0:y0 + r["h"], x0:x0 + r["w"]])
    return out
