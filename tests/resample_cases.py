"""Cases of the resampling recoder's tests (tests/test_cpu_resample.py, tests/test_gpu_recode_resample.py,
tests/golden/make_resample_golden.py): sources of tests/recode_cases.py, the view each is read through, the output with its
chroma format, and cpu_recode_resampled -- the contract of include/ojphgpu.h section 5e ("a resampling recode") stated with
the oracle pipeline (tests/cpu_pipeline.py):

    R(cs, V, out) = encode(fit_frame(resample_frame(crop(decode(cs, skip)))), out)
"""
import numpy as np

from openjph_amd.pipeline import fit_frame, resample_frame
from openjph_amd.plan import Plan, recode_params
from tests import cpu_pipeline as cp
from tests import rate_cases as rc
from tests import recode_cases as rcc

Q150 = rcc.Q150
S422 = [(1, 1), (2, 1), (2, 1)]
S420 = [(1, 1), (2, 2), (2, 2)]

# name -> as recode_cases.CASES; src_kw: make_params keywords a source gets on top of its frame's (an image offset)
CASES = {
    "C422": dict(source=("C", False, rcc.SRC_INDEX), view={}, out=dict(downsampling=S422, qstep=Q150), mode=("plain",)),
    "C420": dict(source=("C", False, rcc.SRC_INDEX), view={}, out=dict(downsampling=S420, qstep=Q150), mode=("plain",)),
    "A420": dict(source=("A", False, rcc.SRC_INDEX), view={}, out=dict(downsampling=S420, bit_depth=10, color_transform=False, qstep=Q150),
                 mode=("plain",)),
}
# what only the GPU test adds: a proxy, an even-origin window, a source with an odd image offset (phase 1 both ways), a
# 4:2:0 source with another factor pair per component (luma halved across, the last chroma to XRsiz 4), and the encoder's search modes
MORE = {
    "proxyC422": dict(source=("C", False, rcc.SRC_INDEX), view=dict(skip_res=1), out=dict(downsampling=S422, qstep=Q150), mode=("plain",)),
    "cropA420": dict(source=("A", False, rcc.SRC_INDEX), view=dict(region=(40, 24, 127, 95)),
                     out=dict(downsampling=S420, color_transform=False, qstep=Q150), mode=("plain",)),
    "offsetB": dict(source=("B", False, rcc.SRC_INDEX), src_kw=dict(image_offset=(3, 5)), view={}, out=dict(downsampling=[(2, 2)], qstep=Q150),
                    mode=("plain",)),
    "Emixed": dict(source=("E", False, rcc.SRC_INDEX), view={}, out=dict(downsampling=[(2, 1), (2, 2), (4, 2)], qstep=Q150), mode=("plain",)),
    "C422cbr": dict(source=("C", False, rcc.SRC_INDEX), view={}, out=dict(downsampling=S422), mode=("max_bytes", rc.budgets("C")[0][1])),
    "C420psnr": dict(source=("C", False, rcc.SRC_INDEX), view={}, out=dict(downsampling=S420), mode=("min_psnr", 40.0)),
}

_sources = {}


def source(case):
    """the oracle pipeline's encode of a case's source (made once)"""
    c = CASES.get(case) or MORE[case]
    key = (c["source"], tuple(sorted(c.get("src_kw", {}).items())))
    if key not in _sources:
        img, size = rc.case_image(c["source"][0])
        kw = dict(rcc.src_kwargs(c["source"]), **c.get("src_kw", {}))
        _sources[key] = cp.encode(img, size=size if isinstance(img, list) else None, **kw)[0]
    return _sources[key]


def factors_and_phases(src, out):
    """per component ((fx, fy), (px, py)) of a view's plan against an output's, from the plans' own component tables: the
    rule of section 5e written out once more (the phase is the parity of the source component's origin; 0 under a view)"""
    view = any(src.skip) or src.region is not None
    f, p = [], []
    for c in range(int(out.params.num_comps)):
        a, b = src.comp_info(c), out.comp_info(c)
        fx, fy = b["dx"] // a["dx"], b["dy"] // a["dy"]
        assert (fx * a["dx"], fy * a["dy"]) == (b["dx"], b["dy"]) and fx in (1, 2) and fy in (1, 2)
        f.append((fx, fy))
        p.append((0 if view or fx == 1 else a["x0"] & 1, 0 if view or fy == 1 else a["y0"] & 1))
    return f, p


def cpu_fitted_resampled(cs, view, out_kw):
    """-> (G as a list of planes, the output's ojphgpu_params, its plan)"""
    src = rcc.view_plan(cs, view)
    skip = src.skip if any(src.skip) else None
    planes = rcc.crop(cp.decode(cs, skip)[0], cs, view)
    params = recode_params(src, **out_kw)
    out = Plan(params)
    nc = int(params.num_comps)
    f, p = factors_and_phases(src, out)
    planes = resample_frame(planes, f, p)
    G = fit_frame(planes, [src.comp_format(c)[0] for c in range(nc)], [out.comp_format(c)[0] for c in range(nc)],
                  [out.comp_format(c)[1] for c in range(nc)])
    assert [q.shape for q in G] == [(out.comp_info(c)["h"], out.comp_info(c)["w"]) for c in range(nc)]
    return G, params, out


def cpu_recode_resampled(cs, view, out_kw):
    """R(cs, V, out) at the output's own step"""
    G, _, out = cpu_fitted_resampled(cs, view, out_kw)
    return rcc.cpu_encode_planes(out, G)
