"""Encoding to a quality target against what a caller could do without it, device-resident: the C3 8K frame (16-bit
containers in HBM) at 40, 45 and 50 dB.  Per target three contenders take turns, `--runs` rounds after `--warmup`: (a) the
encode with the target, run_device + finish; (b) a plain encode at the fixed step qstep(j*) -- what the target costs over
knowing the answer; (c) what a caller without the feature does: the same search (index 240, index 0, halving) where every
trial is a plain encode (codec.Encoder), an upload and decode of its codestream (codec.Decoder) and an int64 error sum in
torch, then the encode of j*.  Host clock around calls that end in a stream synchronise.  At each target the certificate is
checked once by decoding the codestreams of j* and j* - 1.  Prints one JSON line per target: j*, trials, the medians in ms of
(a) (b) (c), and of (a) the search alone, one trial, the device wait of a trial, and the coding of j* with its download.
  python tools/quality_bench.py [--runs 10] [--warmup 2] [--rows 4320] [--no-caller]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TARGETS_DB = (40, 45, 50)
GRID = 241


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=4320, help="top rows of the frame (rehearsals at a small size)")
    ap.add_argument("--no-caller", action="store_true", help="skip contender (c)")
    a = ap.parse_args()
    import torch
    from openjph_amd import codec
    from openjph_amd import plan as planmod
    from openjph_amd.plan import Plan, make_params
    from tests import synth
    img = synth.survey_c3(rows=a.rows)
    nc, h, w = img.shape
    d_img = torch.from_numpy(img.astype(np.uint16).view(np.int16)).cuda()
    d_wide = d_img.to(torch.int64)                              # (12-bit samples: the int16 view holds them as they are)
    del img

    def params(qstep):
        return make_params(w, h, nc, bit_depth=12, reversible=False, qstep=qstep)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    target = codec.Encoder(params(0.001))
    plain = {}

    def plain_encode(j):
        if j not in plain:                                      # made once (a caller would keep them, or pay for a plan each time)
            plain[j] = codec.Encoder(params(planmod.rate_grid_qstep(j)))
        plain[j].run_device(d_img)
        return plain[j].finish()

    def decoded_sse(cs):
        dec = codec.Decoder(cs)
        got = dec.run_device(dtype=torch.int16)
        assert dec.failed_blocks() == 0
        d = got.to(torch.int64) - d_wide
        return int((d * d).sum().item())

    def caller(T):
        n = [0]

        def sse(j):
            n[0] += 1
            return decoded_sse(plain_encode(j))
        if sse(GRID - 1) > T:
            return None, n[0]
        lo, hi = 0, GRID - 1
        if sse(0) <= T:
            hi = 0
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if sse(mid) <= T:
                hi = mid
            else:
                lo = mid
        plain_encode(hi)
        return hi, n[0]

    pl = Plan(params(0.001))
    for db in TARGETS_DB:
        T = planmod.psnr_to_sse(pl, db)
        target.set_quality(max_sse=T)

        def run_target():
            target.run_device(d_img)
            return target.finish()
        t = {"target": [], "search": [], "final": [], "wait": [], "fixed": [], "caller": []}
        info = trials = None
        for i in range(a.warmup + a.runs):
            ms, cs = timed(run_target)
            info, tm = target.quality_info(), target.quality_timing()
            j = info["grid_index"]
            ms_fixed, cs_fixed = timed(lambda: plain_encode(j))
            assert cs_fixed == cs and info["bytes"] == len(cs)
            if i == 0:                                          # the certificate, from the decodes of j* and j* - 1
                assert decoded_sse(cs) == info["sse"] <= T
                assert j == 0 or decoded_sse(plain_encode(j - 1)) == info["sse_coarser"] > T
            if not a.no_caller:
                ms_caller, (jc, trials) = timed(lambda: caller(T))
                assert jc == j
            if i >= a.warmup:
                t["target"].append(ms); t["fixed"].append(ms_fixed)
                t["search"].append(tm["search_ms"]); t["final"].append(tm["final_ms"]); t["wait"].append(tm["wait_ms"])
                if not a.no_caller:
                    t["caller"].append(ms_caller)
        med = {k: round(float(np.median(v)), 3) if v else None for k, v in t.items()}
        print(json.dumps(dict(
            frame="c3 %dx%dx%d 12-bit, 16-bit containers" % (w, h, nc), min_psnr_db=db, max_sse=T, grid_index=info["grid_index"],
            qstep=info["qstep"], sse=info["sse"], sse_coarser=info["sse_coarser"], pae=info["pae"], bytes=info["bytes"],
            passes=info["passes"], ms_target=med["target"], ms_fixed_step=med["fixed"], ms_caller=med["caller"], caller_trials=trials,
            search_ms=med["search"], trial_ms=round(med["search"] / info["passes"], 3), trial_device_wait_ms=round(med["wait"] / info["passes"], 3),
            code_download_t2_ms=med["final"])), flush=True)


if __name__ == "__main__":
    main()
