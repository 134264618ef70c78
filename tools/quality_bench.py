"""Encoding to a quality target against what a caller could do without it, device-resident: the C3 8K frame (16-bit
containers in HBM) at 40, 45 and 50 dB.  Per target three contenders take turns, `--runs` rounds after `--warmup`: (a) the
encode with the target, run_device + finish; (b) a plain encode at the fixed step qstep(j*) -- what the target costs over
knowing the answer; (c) what a caller without the feature does: the same search (index 240, index 0, halving) where every
trial is a plain encode (codec.Encoder), an upload and decode of its codestream (codec.Decoder) and an int64 error sum in
torch, then the encode of j*.  Host clock around calls that end in a stream synchronise.  At each target the certificate is
checked once by decoding the codestreams of j* and j* - 1.  Prints one JSON line per target: j*, trials, the medians in ms of
(a) (b) (c), and of (a) the search alone, one trial, the device wait of a trial, and the coding of j* with its download.
  python tools/quality_bench.py [--runs 10] [--warmup 2] [--rows 4320] [--no-caller]

--pipe: the target in the encoder pipe instead, from host memory to codestream in host memory: a sequence of identical C3
frames (16-bit containers, depth 4) at the same three targets.  Per target three contenders take turns, `--rounds` rounds
of `--frames` frames each: (a) the pipe with the target; (b) a plain pipe at the fixed step qstep(j*) -- the same bytes,
no search: the difference is what the search costs; (c) codec.Encoder(min_psnr) frame by frame from host memory -- what
there was before the pipe had a target, the full search on every frame; its frames are uploaded from pageable numpy memory
(Encoder.encode), the pipes' from their pinned slots.  Prints one JSON line per target: j*, mean trials per frame, and per
contender the frames/s of every round, their median and their spread (max - min) / median.
  python tools/quality_bench.py --pipe [--rounds 3] [--frames 24] [--rows 4320]

--cap: a target under a byte cap (cap_bench below), single encoder or with --pipe the encoder pipe.
  python tools/quality_bench.py --cap [--pipe] [--rounds 3] [--frames 24] [--rows 4320]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TARGETS_DB = (40, 45, 50)
GRID = 241


def pipe_bench(a):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from e2e_pipeline import run_budget_pipe
    from openjph_amd import codec
    from openjph_amd import plan as planmod
    from openjph_amd.plan import Plan, make_params
    from tests import synth
    img = synth.survey_c3(rows=a.rows)
    nc, h, w = img.shape
    img16 = img.astype(np.uint16)

    def params(qstep):
        return make_params(w, h, nc, bit_depth=12, reversible=False, qstep=qstep)
    searched = Plan(params(0.001))
    single = codec.Encoder(params(0.001))
    for db in TARGETS_DB:
        T = planmod.psnr_to_sse(searched, db)
        single.set_quality(max_sse=T)
        fps = {"pipe_target": [], "pipe_fixed_step": [], "encoder_per_frame": []}
        st = fixed = None
        for r in range(a.rounds + 1):                           # round 0 warms every contender up and is not counted
            dt, st, cs = run_budget_pipe(searched, img16, a.frames, 0, depth=4, max_sse=T)
            if fixed is None:
                fixed = Plan(params(planmod.rate_grid_qstep(st["grid_index"])))
            dt_fixed, _, cs_fixed = run_budget_pipe(fixed, img16, a.frames, 0, depth=4)
            assert cs == cs_fixed and len(cs) == st["bytes"] and st["sse"] <= T
            t0 = time.perf_counter()
            for _ in range(a.frames):
                cs_single = single.encode(img16)
            dt_single = time.perf_counter() - t0
            assert cs_single == cs
            if r:
                fps["pipe_target"].append(a.frames / dt); fps["pipe_fixed_step"].append(a.frames / dt_fixed)
                fps["encoder_per_frame"].append(a.frames / dt_single)
        out = dict(frame="c3 %dx%dx%d 12-bit, 16-bit containers, host memory" % (w, h, nc), depth=4, frames_per_round=a.frames,
                   min_psnr_db=db, max_sse=T, grid_index=st["grid_index"], bytes=st["bytes"], sse=st["sse"], sse_coarser=st["sse_coarser"],
                   mean_trials=st["mean_passes"], single_encoder_trials=single.quality_info()["passes"])
        for k, v in fps.items():
            med = float(np.median(v))
            out[k] = dict(fps=[round(x, 1) for x in v], median_fps=round(med, 1), ms_per_frame=round(1e3 / med, 3),
                          spread=round((max(v) - min(v)) / med, 3))
        print(json.dumps(out), flush=True)


def cap_bench(a):
    """--cap: what a byte cap on the target costs, C3 at 45 dB under three caps -- one above size(q), one at 0.2 bytes per
    sample, one at 3/4 of size(q), which binds.  Three contenders take turns, `--rounds` rounds after one that warms up: (a) the capped run; (b) the plain run at
    qstep(j*); (c) the quality run without a cap.  Single encoder (device-resident frame, ms per frame), or with --pipe the
    encoder pipe from host memory (`--frames` identical frames per round, frames/s).  One JSON line per cap: the outcome,
    both indices, both pass counts (the pipe: of the last frame, its steady state), every round's figure, medians, spread."""
    import torch
    from openjph_amd import codec
    from openjph_amd import plan as planmod
    from openjph_amd.pipeline import EncoderPipe
    from openjph_amd.plan import Plan, make_params
    from tests import synth
    img = synth.survey_c3(rows=a.rows)
    nc, h, w = img.shape
    img16 = img.astype(np.uint16)
    d_img = torch.from_numpy(img16.view(np.int16)).cuda()

    def params(qstep):
        return make_params(w, h, nc, bit_depth=12, reversible=False, qstep=qstep)
    pl = Plan(params(0.001))
    T = planmod.psnr_to_sse(pl, 45)
    quality = codec.Encoder(params(0.001), max_sse=T)
    quality.run_device(d_img)
    size_q = len(quality.finish())
    capped = codec.Encoder(params(0.001))

    def single(enc):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.run_device(d_img)
        cs = enc.finish()
        return (time.perf_counter() - t0) * 1e3, cs

    def piped(**kw):
        pipe = EncoderPipe(Plan(params(kw.pop("qstep", 0.001))), depth=4, **kw)
        t0 = time.perf_counter()
        out = list(pipe.encode_sequence([img16] * a.frames))
        dt = time.perf_counter() - t0
        info = pipe.capped_info() if "cap_bytes" in kw else None
        pipe.close()
        return a.frames / dt, out[-1], info
    # (0.2 bytes per sample lies above this frame's size(q) at 45 dB, 0.17: the third cap is one that binds)
    for label, cap in (("above size(q)", size_q * 5 // 4), ("0.2 bytes per sample", int(0.2 * img.size)), ("3/4 of size(q)", size_q * 3 // 4)):
        capped.set_quality(max_sse=T, cap_bytes=cap)
        v = {"capped": [], "fixed_step": [], "quality": []}
        info = fixed = None
        for r in range(a.rounds + 1):
            if a.pipe:
                x, cs, info = piped(max_sse=T, cap_bytes=cap)
                y, cs_fixed, _ = piped(qstep=planmod.rate_grid_qstep(info["grid_index"]))
                z, _, _ = piped(max_sse=T)
            else:
                x, cs = single(capped)
                info = capped.capped_info()
                fixed = fixed or codec.Encoder(params(planmod.rate_grid_qstep(info["grid_index"])))
                y, cs_fixed = single(fixed)
                z, _ = single(quality)
            assert cs == cs_fixed and len(cs) == info["bytes"] <= cap
            if r:
                v["capped"].append(x); v["fixed_step"].append(y); v["quality"].append(z)
        out = dict(frame="c3 %dx%dx%d 12-bit, 16-bit containers" % (w, h, nc), mode="pipe, frames/s" if a.pipe else "single, ms per frame",
                   min_psnr_db=45, max_sse=T, cap=label, cap_bytes=cap, size_q=size_q,
                   **{k: info[k] for k in ("grid_index", "outcome", "quality_index", "bytes", "sse", "quality_passes", "rate_passes")})
        for k, x in v.items():
            med = float(np.median(x))
            out[k] = dict(rounds=[round(t, 3) for t in x], median=round(med, 3), spread=round((max(x) - min(x)) / med, 3))
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap", action="store_true", help="a target under a byte cap (with --pipe: in the encoder pipe)")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=4320, help="top rows of the frame (rehearsals at a small size)")
    ap.add_argument("--no-caller", action="store_true", help="skip contender (c)")
    ap.add_argument("--pipe", action="store_true", help="the target in the encoder pipe, from host memory")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=24)
    a = ap.parse_args()
    if a.cap:
        return cap_bench(a)
    if a.pipe:
        return pipe_bench(a)
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
