"""Seeded parameter sets over the sample formats: every bit depth from 1 to 32 per component, signed and unsigned, the type 3
non-linearity on signed components, both wavelets and COC mixes of them, an ATK wavelet beside deep components, the colour
transform over three components of one format (1-26 bits), qstep values that push the irreversible K_max into the 20s, and
sub-sampling / tiles / odd offsets as in random_cases.  Shared by the CPU pins (tests/test_cpu_formats.py, against the
reference) and the GPU tests (tests/test_gpu_formats.py, against the oracle pipeline).  What the plan refuses is left to the
reference to refuse: the CPU test pins the refusals."""
import numpy as np

REV53_ATK = dict(steps=[(1, 2, 2), (-1, 1, 1)])
A97 = [0.443506852043971, 0.882911075530934, -0.052980118572961, -1.586134342059924]
K97 = 1.230174104914001


def format_plane(rng, h, w, bd, signed, noise=False):
    """int32 samples of a bd-bit component (unsigned 32-bit samples as their two's-complement int32 bits): a smooth
    field over the whole range with noise, plus the extreme values at a few places; noise=True: uniform over the range"""
    lo, hi = (-(1 << (bd - 1)), (1 << (bd - 1)) - 1) if signed else (0, (1 << bd) - 1)
    if noise:
        v = rng.integers(lo, hi + 1, (h, w), dtype=np.int64)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        base = (np.sin(xx / 4.0 + rng.random() * 6) * np.cos(yy / 3.0) * 0.45 + 0.5) * (hi - lo) + lo
        spread = max((hi - lo) // 8, 1)
        v = np.clip(base.astype(np.int64) + rng.integers(-spread, spread + 1, (h, w), dtype=np.int64), lo, hi)
    flat = v.reshape(-1)
    for k, val in enumerate((lo, hi, lo, hi, 0 if signed else lo, -1 if signed else hi)):
        if flat.size:
            flat[int(rng.integers(0, flat.size))] = val
    return v.astype(np.uint64).astype(np.uint32).view(np.int32).reshape(h, w)


def _depth(rng):
    r = rng.random()
    if r < 0.25:
        return int(rng.integers(1, 5))          # 1-4
    if r < 0.45:
        return int(rng.integers(5, 17))         # 5-16
    if r < 0.8:
        return int(rng.integers(17, 27))        # 17-26: the 32-bit path at high K_max
    return int(rng.integers(27, 33))            # 27-32: the conversion kernels / the 64-bit path


def _planes(rng, w, h, ds, depths, signs, offset, noise=False):
    ox, oy = offset
    out = []
    for (dx, dy), bd, sg in zip(ds, depths, signs):
        cw = -(-(ox + w) // dx) - -(-ox // dx)
        ch = -(-(oy + h) // dy) - -(-oy // dy)
        out.append(format_plane(rng, max(ch, 1), max(cw, 1), bd, sg, noise)[:ch, :cw])
    return out


def format_case(seed):
    """-> (planes, kwargs for plan.make_params / refbind.Ref.encode / cpu_pipeline.encode, (W, H))"""
    rng = np.random.default_rng(51000 + seed)
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]
    w, h = int(rng.integers(1, 90)), int(rng.integers(1, 70))
    if rng.random() < 0.1:
        w = pick([1, 2, 3])
    if rng.random() < 0.1:
        h = pick([1, 2, 3])
    nc = pick([1, 2, 2, 3, 3, 4])
    reversible = bool(rng.random() < 0.55)
    color = nc >= 3 and rng.random() < 0.35
    depths = [_depth(rng) for _ in range(nc)]
    signs = [bool(rng.random() < 0.35) for _ in range(nc)]
    ds = [(1, 1) if (color and c < 3) else pick([(1, 1), (1, 1), (1, 1), (2, 2), (2, 1), (1, 2)]) for c in range(nc)]
    if color:
        ds = [(dx, 1) for dx, _ in ds]
        ds[:3] = [ds[0]] * 3
        depths[:3] = [int(rng.integers(1, 27))] * 3
        signs[:3] = [signs[0]] * 3
    ox, oy = (int(rng.integers(0, 30)), int(rng.integers(0, 30))) if rng.random() < 0.35 else (0, 0)
    kw = dict(reversible=reversible, color_transform=color, num_decomps=int(rng.integers(0, 6)),
              block=pick([(64, 64), (32, 32), (16, 64), (8, 8), (4, 128)]), prog_order=pick(["LRCP", "RPCL", "CPRL"]),
              image_offset=(ox, oy), bit_depth=depths[0], is_signed=signs[0], downsampling=ds, bit_depths=depths, signs=signs)
    if rng.random() < 0.4:
        tw, th = int(rng.integers(17, 80)), int(rng.integers(17, 80))
        kw["tile"] = (tw, th)
        if ox or oy:
            kw["tile_offset"] = (int(rng.integers(0, ox + 1)), int(rng.integers(0, oy + 1)))
            kw["tile"] = (max(tw, ox - kw["tile_offset"][0] + 1), max(th, oy - kw["tile_offset"][1] + 1))
    if rng.random() < 0.4:                      # the other wavelet on some components
        coc = {}
        for c in range(nc):
            if (color and c < 3) or rng.random() < 0.5:
                continue
            coc[c] = dict(reversible=not reversible, num_decomps=int(rng.integers(0, 6)))
        if coc:
            kw["coc"] = coc
    nlt = {c: 3 for c in range(nc) if signs[c] and rng.random() < 0.4}
    if nlt:
        kw["nlt"] = nlt
    if rng.random() < 0.75:                     # irreversible components: K_max from the teens into the 20s
        kw["qstep"] = float(pick([0.1, 0.01, 1e-4, 1e-5, 1e-6, 2e-7]))
    return _planes(rng, w, h, ds, depths, signs, (ox, oy)), kw, (w, h)


def _fixed(spec, seed):
    rng = np.random.default_rng(52000 + seed)
    sp = dict(spec)
    w, h, depths = sp.pop("w"), sp.pop("h"), sp.pop("depths")
    signs = sp.pop("signs", [False] * len(depths))
    noise = sp.pop("noise", False)
    ds = sp.get("downsampling") or [(1, 1)] * len(depths)
    kw = dict(sp, bit_depth=depths[0], is_signed=signs[0], bit_depths=list(depths), signs=list(signs))
    return _planes(rng, w, h, ds, depths, signs, sp.get("image_offset", (0, 0)), noise), kw, (w, h)


# Cases every run includes: a component of the 64-bit path (or a 27-32-bit one of the conversion kernels) beside
# 32-bit-path components, component 0 the deep one in most; the two wavelets mixed by COC and an ATK component under a
# 32-bit component 0 (the top level of the narrow components is fused with its conversion, component 0's is not);
# irreversible K_max in the 20s; one incompressible frame of 24-26 bits.
FIXED = [
    dict(w=70, h=50, depths=[32, 8], reversible=True, coc={1: dict(reversible=False)}, num_decomps=3, qstep=0.01),
    dict(w=61, h=45, depths=[32, 12], reversible=False, qstep=0.01, coc={1: dict(reversible=True, wavelet=2)}, atk={2: REV53_ATK},
         num_decomps=3),
    dict(w=61, h=45, depths=[30, 20], signs=[True, False], reversible=False, qstep=1e-6,
         coc={1: dict(reversible=True, wavelet=3)}, atk={3: REV53_ATK}, num_decomps=2),
    dict(w=57, h=41, depths=[31, 5, 26], signs=[False, True, False], reversible=True, num_decomps=4),
    dict(w=57, h=41, depths=[12, 32, 1], signs=[True, False, False], reversible=True, num_decomps=2, tile=(40, 33)),
    dict(w=66, h=39, depths=[28, 17, 3, 24], signs=[True, True, False, False], reversible=False, qstep=1e-5,
         coc={2: dict(reversible=True), 3: dict(reversible=True)}, num_decomps=3),
    dict(w=48, h=40, depths=[26, 26, 26], signs=[True] * 3, reversible=False, color_transform=True, qstep=2e-7, num_decomps=3),
    dict(w=48, h=40, depths=[25, 25, 25, 32], reversible=True, color_transform=True, num_decomps=3),
    dict(w=50, h=37, depths=[1, 1, 1], reversible=True, color_transform=True, num_decomps=2, image_offset=(3, 1)),
    dict(w=45, h=33, depths=[22, 19], signs=[True, True], reversible=True, nlt={0: 3, 1: 3}, num_decomps=3),
    dict(w=64, h=64, depths=[25], signs=[True], reversible=True, noise=True, num_decomps=2),
    dict(w=64, h=64, depths=[26], reversible=False, qstep=3e-8, noise=True, num_decomps=1),
]


def fixed_case(i):
    return _fixed(FIXED[i], i)


def all_cases(n_random):
    """the fixed cases, then n_random seeded ones: -> [(name, planes, kw, size)]"""
    out = [("fixed%d" % i,) + fixed_case(i) for i in range(len(FIXED))]
    out += [("seed%d" % s,) + format_case(s) for s in range(n_random)]
    return out
