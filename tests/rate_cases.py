"""Cases of the byte-budget tests (tests/test_cpu_rate.py, tests/test_gpu_rate.py, tests/golden/make_rate_golden.py):
five small irreversible frames, the budgets each is coded to, the grid of quantisation steps in numpy and a numpy
restatement of the band statistics kernel (openjph_amd/csrc/kernels_stats.hip)."""
import numpy as np

from tests.synth import synth_image

GRID = 241                                    # OJPHGPU_RATE_GRID
BINS = 80                                     # OJPHGPU_STATS_BINS
BPS = (0.05, 0.2, 0.73, 1.3)                  # the in-range budgets, bytes per sample of the frame
SURVEY_BPS = (0.73, 0.2, 0.05)                # tools/rate_bench.py: the C3 frame


def grid_qstep(j):
    """qstep(j) = (float) exp2(-1 - j / 16), evaluated in double and rounded once to float"""
    return float(np.float32(2.0 ** (-1.0 - j / 16.0)))


CASES = {
    "A": dict(nc=3, h=200, w=312, bd=12, kw=dict(num_decomps=4, color_transform=True)),
    "B": dict(nc=1, h=301, w=257, bd=8, kw=dict(num_decomps=5)),
    "C": dict(nc=3, h=256, w=384, bd=10, kw=dict(num_decomps=3, tile=(128, 128), tlm=True, block=(32, 32))),
    "D": dict(nc=1, h=180, w=220, bd=16, kw=dict(num_decomps=2, prog_order="CPRL")),
    "E": dict(nc=3, h=190, w=250, bd=8, kw=dict(num_decomps=4, downsampling=[(1, 1), (2, 2), (2, 2)]), sub=True),
}


def case_image(name):
    """-> (image: int32 [C,H,W], or the list of planes of the 4:2:0 case; (W, H) on the reference grid)"""
    c = CASES[name]
    img = synth_image(c["nc"], c["h"], c["w"], c["bd"], seed=11)
    if c.get("sub"):
        return [np.ascontiguousarray(img[0]), np.ascontiguousarray(img[1][::2, ::2]), np.ascontiguousarray(img[2][::2, ::2])], (c["w"], c["h"])
    return img, (c["w"], c["h"])


def case_kwargs(name, qstep=-1.0):
    """keyword arguments plan.make_params, cpu_pipeline.encode and the reference binding share"""
    c = CASES[name]
    return dict(c["kw"], bit_depth=c["bd"], reversible=False, qstep=float(qstep))


def case_samples(name):
    img, _ = case_image(name)
    return int(sum(q.size for q in img)) if isinstance(img, list) else int(img.size)


def budgets(name):
    """-> (in-range budgets in bytes, one below size(0), one above size(240))"""
    n = case_samples(name)
    return [int(n * b) for b in BPS], 64, 8 * n + (1 << 20)


def band_hist(v):
    """80-bin half-octave histogram of the magnitudes of fp32 coefficients given as their uint32 bit patterns"""
    u = np.ascontiguousarray(v).view(np.uint32).ravel()
    e = np.clip(((u >> np.uint32(22)) & np.uint32(0x1FF)).astype(np.int64) - 191, 0, BINS - 1)
    return np.bincount(e, minlength=BINS).astype(np.uint32)


def plan_hists(plan, arena):
    """the histogram of every band of the plan over the arena cpu_pipeline.forward_stages returns: uint32 [num_bands, 80]"""
    a = np.ascontiguousarray(arena).view(np.uint32)
    H = np.zeros((plan.num_bands, BINS), np.uint32)
    for i, b in enumerate(plan.bands):
        w, h = int(b["w"]), int(b["h"])
        if w == 0 or h == 0:
            continue
        off, pitch = int(b["plane_off"]), int(b["pitch"])
        H[i] = band_hist(np.lib.stride_tricks.as_strided(a[off:], shape=(h, w), strides=(pitch * 4, 4)))
    return H


def bisect_passes(size, budget):
    """what a caller without the feature does: both ends, then halving -> (j* or None, encodes made)"""
    asked = {0: size(0)}
    if asked[0] > budget:
        return None, 1
    asked[GRID - 1] = size(GRID - 1)
    if asked[GRID - 1] <= budget:
        return GRID - 1, 2
    lo, hi = 0, GRID - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        asked[mid] = size(mid)
        if asked[mid] <= budget:
            lo = mid
        else:
            hi = mid
    return lo, len(asked)
