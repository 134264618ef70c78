"""Cases of the recoder tests (tests/test_cpu_recode.py, tests/test_gpu_recode.py, tests/golden/make_recode_golden.py): frames
of tests/rate_cases.py coded once, the view each codestream is read through, what its output changes, and cpu_recode -- the
contract of include/ojphgpu.h section 5e stated with the oracle pipeline (tests/cpu_pipeline.py):

    R(cs, V, out) = encode(fit_frame(crop(decode(cs, skip))), out)
"""
import hashlib

import numpy as np

from openjph_amd.pipeline import fit_frame
from openjph_amd.plan import Plan, parse_codestream, recode_params
from tests import cpu_pipeline as cp
from tests import rate_cases as rc

SRC_INDEX = 150                                   # irreversible sources are coded at this step of the rate grid
Q150 = rc.grid_qstep(SRC_INDEX)

# name -> source = (frame of rate_cases, reversible, grid index of an irreversible source), view = what codec.Decoder takes,
# out = what plan.recode_params takes, mode = how the encoder half codes: ("plain",), ("max_bytes", [budgets]),
# ("min_psnr", dB), ("capped", dB, [caps]); ref: the fixture holds the reference's encode of the fitted frame
CASES = {
    "rev2irv": dict(source=("A", True, None), view={}, out=dict(reversible=False, qstep=Q150), mode=("plain",), ref=True),
    "rev2cbr": dict(source=("A", True, None), view={}, out=dict(reversible=False), mode=("max_bytes", rc.budgets("A")[0]), ref=False),
    "depthA": dict(source=("A", False, SRC_INDEX), view={}, out=dict(bit_depth=10, qstep=Q150), mode=("plain",), ref=True),
    "depthD": dict(source=("D", True, None), view={}, out=dict(bit_depth=12), mode=("plain",), ref=True),
    "depthB": dict(source=("B", False, SRC_INDEX), view={}, out=dict(bit_depth=10, qstep=Q150), mode=("plain",), ref=True),
    "proxyC": dict(source=("C", False, SRC_INDEX), view=dict(skip_res=1), out=dict(qstep=Q150), mode=("plain",), ref=True),
    "proxyE": dict(source=("E", False, SRC_INDEX), view=dict(skip_res=1), out=dict(qstep=Q150), mode=("plain",), ref=True),
    "cropA": dict(source=("A", False, SRC_INDEX), view=dict(region=(40, 24, 128, 96)), out=dict(qstep=Q150), mode=("plain",), ref=True),
    "cropE": dict(source=("E", False, SRC_INDEX), view=dict(region=(20, 10, 101, 77)), out=dict(qstep=Q150), mode=("plain",), ref=True),
    "proxycropA": dict(source=("A", False, SRC_INDEX), view=dict(skip_res=1, region=(40, 24, 128, 96)), out=dict(qstep=Q150),
                       mode=("plain",), ref=True),
    "rewrapD": dict(source=("D", True, None), view={}, out=dict(block=(32, 32)), mode=("plain",), ref=True),
    "qualityB": dict(source=("B", False, 200), view={}, out=dict(), mode=("min_psnr", 40.0), ref=False),
    # (a cap far above every step's codestream, and one at 0.05 bytes per sample: below what 45 dB takes of a 12-bit frame)
    "cappedA": dict(source=("A", False, SRC_INDEX), view={}, out=dict(), mode=("capped", 45.0, [8 * rc.case_samples("A"), rc.budgets("A")[0][0]]),
                    ref=False),
}
REFUSED = {"cropEodd": dict(source=("E", False, SRC_INDEX), view=dict(region=(21, 10, 100, 76)), out=dict(qstep=Q150))}


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def src_kwargs(source):
    """make_params keywords of a source"""
    name, rev, index = source
    c = rc.CASES[name]
    if rev:
        return dict(c["kw"], bit_depth=c["bd"], reversible=True)
    return rc.case_kwargs(name, rc.grid_qstep(index))


def cpu_source(source):
    """the oracle pipeline's encode of a source's image"""
    img, size = rc.case_image(source[0])
    return cp.encode(img, size=size if isinstance(img, list) else None, **src_kwargs(source))[0]


def view_plan(cs, view, resilient=False):
    """the parsed plan of a source, restricted as codec.Decoder restricts it"""
    src = parse_codestream(cs, resilient)
    skip = view.get("skip_res")
    if skip:
        src.restrict_resolution(*((skip, skip) if isinstance(skip, int) else skip))
    if view.get("region") is not None:
        src.restrict_region(*view["region"])
    return src


def crop(planes, cs, view):
    """the view's window of the planes a whole-frame decode at the view's resolution gives: component c keeps the columns
    [ceil(A0 / fx), ceil(A1 / fx)) of its own grid, fx = XRsiz * 2^skipped resolutions (rows alike)"""
    planes = [np.asarray(q) for q in planes]
    if view.get("region") is None:
        return planes
    whole = view_plan(cs, dict(skip_res=view.get("skip_res")))
    k = whole.skip[1]
    x0, y0, w, h = view["region"]
    ax0, ay0 = int(whole.params.image_x0) + x0, int(whole.params.image_y0) + y0
    out = []
    for c, q in enumerate(planes):
        ci = whole.comp_info(c)
        fx, fy = ci["dx"] << k, ci["dy"] << k
        up = lambda v, f: -(-v // f)
        out.append(np.ascontiguousarray(q[up(ay0, fy) - ci["y0"]:up(ay0 + h, fy) - ci["y0"], up(ax0, fx) - ci["x0"]:up(ax0 + w, fx) - ci["x0"]]))
    return out


def cpu_fitted(cs, view, out_kw, decode=None):
    """-> (G as a list of planes, the output's ojphgpu_params, its plan); decode(cs, skip) -> planes: another decoder than
    the oracle pipeline's (the reference's)"""
    src = view_plan(cs, view)
    skip = src.skip if any(src.skip) else None
    planes = decode(cs, skip) if decode is not None else cp.decode(cs, skip)[0]
    planes = crop(planes, cs, view)
    params = recode_params(src, **out_kw)
    out = Plan(params)
    nc = int(params.num_comps)
    G = fit_frame(planes, [src.comp_format(c)[0] for c in range(nc)], [out.comp_format(c)[0] for c in range(nc)],
                  [out.comp_format(c)[1] for c in range(nc)])
    return G, params, out


def cpu_encode_planes(plan, G):
    """the oracle pipeline's encode of planes with a plan made elsewhere"""
    arena = cp.forward_stages(plan, G)
    data, coded = cp.encode_blocks(plan, arena)
    return plan.t2_write(data, coded)


def cpu_recode(cs, view, out_kw):
    """R(cs, V, out) at the output's own step"""
    G, _, out = cpu_fitted(cs, view, out_kw)
    return cpu_encode_planes(out, G)


def frame_digest(planes):
    """SHA-256 of a frame whatever its container: the planes as little-endian int32, one after the other"""
    return sha(b"".join(np.ascontiguousarray(q).astype("<i4").tobytes() for q in planes))


def out_make_kwargs(case):
    """the output of a case as make_params / the reference binding take it, written out by hand -- (keywords, (W, H) on the
    output's reference grid): what recode_params must amount to"""
    c = CASES[case] if case in CASES else REFUSED[case]
    name = c["source"][0]
    kw = dict(src_kwargs(c["source"]))
    w, h = rc.CASES[name]["w"], rc.CASES[name]["h"]
    skip = c["view"].get("skip_res", 0)
    if c["view"].get("region") is not None:
        w, h = c["view"]["region"][2:]
    if c["view"]:
        w, h = -(-w >> skip), -(-h >> skip)
        kw.pop("tile", None)
        kw["num_decomps"] = kw.get("num_decomps", 5) - skip
    kw.update(c["out"])
    return kw, (w, h)
