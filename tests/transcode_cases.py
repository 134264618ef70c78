"""Cases of the transcoder tests (tests/test_cpu_transcode.py, tests/test_gpu_transcode.py,
tests/golden/make_transcode_golden.py): frames of tests/rate_cases.py coded once, the targets each codestream is recoded to,
and cpu_transcode -- the contract of include/ojphgpu.h section 5d stated with the oracle pipeline (tests/cpu_pipeline.py):

    T(cs, out) = plan(out).t2_write(encode_blocks(plan(out), decode_blocks(parse(cs), cs)))
"""
from openjph_amd.plan import Plan, make_params, parse_codestream
from tests import cpu_pipeline as cp
from tests import rate_cases as rc

SRC_INDEX = 150                                   # irreversible sources are coded at this step of the rate grid
IRV = ("A", "B", "C", "E")                        # A: 64-row blocks (the one-launch block decoder), C: 32 x 32 blocks in four tiles
REV = ("A", "C", "D")                             # (the separate launches), E: 4:2:0, B: 301 x 257, ragged band edges
CASES = [(n, False) for n in IRV] + [(n, True) for n in REV]

# target -> (what changes, as plan.transcode_params / plan.make_params name it; grid index of the output step or None = the
# source's; identity = the result is the direct encode of the original image with the output parameters)
IRV_TARGETS = {
    "blk32": (dict(block=(32, 32)), None, True),
    "blk64x16": (dict(block=(64, 16)), None, True),
    "cprl_tlm": (dict(prog_order="CPRL", tlm=True), None, True),
    "oct1": (dict(), SRC_INDEX - 16, True),       # a whole number of octaves coarser: floor((q + 0.5) / 2^k) = floor(q / 2^k)
    "oct3": (dict(), SRC_INDEX - 48, True),
    "frac": (dict(), SRC_INDEX - 5, False),       # a fraction of an octave, a finer step: codestreams of their own
    "finer": (dict(), SRC_INDEX + 7, False),
}
REV_TARGETS = {
    "blk32": (dict(block=(32, 32)), None, True),
    "blk128x8_pcrl": (dict(block=(128, 8), prog_order="PCRL"), None, True),
}


def case_id(name, rev):
    return name + ("rev" if rev else "irv")


def targets(rev):
    return REV_TARGETS if rev else IRV_TARGETS


def src_kwargs(name, rev, index=SRC_INDEX):
    """make_params keywords of the source of a case (irreversible: coded at grid index `index`)"""
    c = rc.CASES[name]
    if rev:
        return dict(c["kw"], bit_depth=c["bd"], reversible=True)
    return rc.case_kwargs(name, rc.grid_qstep(index))


def out_qstep(rev, target):
    """the base step of a target's output, None for a reversible one"""
    if rev:
        return None
    j = targets(rev)[target][1]
    return rc.grid_qstep(SRC_INDEX if j is None else j)


def out_kwargs(name, rev, target, qstep=None):
    """make_params keywords of a target's output: the source's with the target's changes (qstep: another step than the target's)"""
    kw = dict(src_kwargs(name, rev), **targets(rev)[target][0])
    if not rev:
        kw["qstep"] = out_qstep(rev, target) if qstep is None else float(qstep)
    return kw


def transcode_kwargs(rev, target):
    """what codec.transcode / plan.transcode_params take for a target"""
    kw = dict(targets(rev)[target][0])
    if not rev:
        kw["qstep"] = out_qstep(rev, target)
    return kw


def case_params(name, kw):
    c = rc.CASES[name]
    return make_params(c["w"], c["h"], c["nc"], **kw)


def cpu_encode(name, kw):
    """the oracle pipeline's encode of a case's image"""
    img, size = rc.case_image(name)
    return cp.encode(img, size=size if isinstance(img, list) else None, **kw)[0]


def cpu_source_planes(cs, resilient=False):
    """what the block decoder leaves of a codestream: (parsed plan, arena)"""
    src = parse_codestream(cs, resilient)
    return src, cp.decode_blocks(src, cs, resilient=resilient)


def cpu_failed_blocks(plan, cs):
    """the blocks of a (damaged) codestream the oracle's block decoder refuses -- the ones cp.decode_blocks(resilient=True)
    leaves zero -- counted as it walks them"""
    import numpy as np
    from oracle import oraclebind as ob
    coded = plan.coded_blocks()
    padded = {int(q["block"]): q for q in plan.padded_blocks()}
    buf = np.frombuffer(cs, dtype=np.uint8)
    failed = 0
    for k in range(plan.num_blocks):
        cbk, pad = coded[k], 0
        if k in padded:
            cbk = padded[k]; pad = int(cbk["len1"]) + int(cbk["len2"]) - int(cbk["got"])
        if cbk["len1"] == 0:
            continue
        blk = plan.blocks[k]
        w, h = int(blk["w"]), int(blk["h"])
        o = int(cbk["offset"]); n = int(cbk["len1"]) + int(cbk["len2"])
        ok, _ = ob.ht_decode(buf[o:o + n - pad].tobytes() + bytes(pad), w, h, w, int(cbk["missing_msbs"]), len2=int(cbk["len2"]),
                             num_passes=int(cbk["num_passes"]), stripe_causal=bool(plan.params.reserved[0] & 1))
        failed += not ok
    return failed


def cpu_transcode_planes(arena, params):
    out = Plan(params)
    data, coded = cp.encode_blocks(out, arena)
    return out.t2_write(data, coded)


def cpu_transcode(cs, params, resilient=False):
    """T(cs, out): params = the output's ojphgpu_params (plan.make_params)"""
    _, arena = cpu_source_planes(cs, resilient)
    return cpu_transcode_planes(arena, params)
