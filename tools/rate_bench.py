"""Encoding to a byte budget against what a caller could do without it, device-resident: the C3 8K frame (16-bit containers
in HBM) at budgets of 0.73, 0.2 and 0.05 bytes per sample.  Per budget three encoders take turns, `--runs` rounds after
`--warmup`: (a) the budgeted encode, run_device + finish; (b) a plain encode at the fixed step qstep(j*) -- what the budget
costs over knowing the answer; (c) a bisection over the grid made of plain encodes (both ends, then halving), each a
run_device + finish at its own step -- what the parent commit offers.  Host clock around calls that end in a stream
synchronise.  Prints one JSON line per budget: j*, passes, first guess, the model's prediction over the true length, median
ms of (a) (b) (c), one pass's device wait and host share, the statistics kernel's time (device events) and its fraction of
the 8 TB/s HBM peak (bytes = 4 x coefficients), beside the level-1 DWT launch of the same run.
  python tools/rate_bench.py [--runs 10] [--warmup 3] [--rows 4320] [--no-bisect]

--pipe: the budget in the encoder pipe instead, from host memory to codestream in host memory: a sequence of identical C3
frames (16-bit containers, depth 4) at the same three budgets.  Per budget three contenders take turns, `--rounds` rounds
of `--frames` frames each: (a) the pipe with the budget; (b) a plain pipe at the fixed step qstep(j*) -- the same bytes,
no search; (c) codec.Encoder(max_bytes) frame by frame from host memory -- what there was before the pipe had a budget;
its frames are uploaded from pageable numpy memory (Encoder.encode), the pipes' from their pinned slots.
Prints one JSON line per budget: j*, mean passes per frame, and per contender the frames/s of every round, their median
and their spread (max - min) / median.
  python tools/rate_bench.py --pipe [--rounds 3] [--frames 24] [--rows 4320]

--batch B: the budgets of a batch encoder (Encoder(frames=B, budgets=...)): B 4K 4:4:4 12-bit frames (the C7 family, seed
1234 + frame; 16-bit containers in HBM), every frame at the same budget of 0.73, 0.2 and 0.05 bytes per sample.  Per budget
three contenders take turns, `--runs` rounds after `--warmup`: (a) the batch with budgets, run_device + finish of every
frame; (b) the same frames through B budgeted single-frame encodes, one after the other -- what a caller has without the
batch form; (c) a plain batch encode at the fixed step of the median j* -- the device and download cost of one coding of
the batch.  The bytes of (a) and (b) are compared.  Prints one JSON line per budget: the j* of the frames, the rounds of
the batch's search and the sum of the frames' passes, median ms of (a) (b) (c), the batch's search / device wait.
  python tools/rate_bench.py --batch 8 [--runs 10] [--warmup 3] [--rows 2160]

--first N: the first budgeted frame of a fresh encoder -- what a one-shot caller (ojph_compress with a byte budget) pays, with
no plan copy of any grid index made yet: per budget N encoders in turn, each made, run once on the C3 frame and timed on
the host clock around finish() alone.  Prints one JSON line per budget: every time and the median.
  python tools/rate_bench.py --first 7 [--rows 4320]

--trunc: a reversible frame under a byte cap (include/ojphgpu.h section 5f): a 4K 4:4:4 16-bit frame (the C7 family scaled
to 16 bits; 16-bit containers in HBM), 5/3 with the RCT, at caps of 0.9, 0.6 and 0.3 of its lossless size.  Per cap two
encoders take turns, `--runs` rounds after `--warmup`: (a) the capped encode, run_device + finish; (b) the plain lossless
encode, which runs none of the new code -- what it costs at the parent commit is bench.py's comparison, not this tool's.
Prints one JSON line per cap: level, passes (trials per search), first guess, the largest number of planes a band drops,
median ms of (a) and (b), the coding inside finish, and the integer statistics kernel's time (device events) with its
fraction of the 8 TB/s HBM peak beside the level-1 DWT launch of the same run.
  python tools/rate_bench.py --trunc [--runs 10] [--warmup 3] [--rows 2160]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
BPS = (0.73, 0.2, 0.05)
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
    for bps in BPS:
        budget = int(img.size * bps)
        single.set_budget(budget)
        fps = {"pipe_budget": [], "pipe_fixed_step": [], "encoder_per_frame": []}
        st = fixed = None
        for r in range(a.rounds + 1):                           # round 0 warms every contender up and is not counted
            dt, st, cs = run_budget_pipe(searched, img16, a.frames, budget, depth=4)
            if fixed is None:
                fixed = Plan(params(planmod.rate_grid_qstep(st["grid_index"])))
            dt_fixed, _, cs_fixed = run_budget_pipe(fixed, img16, a.frames, 0, depth=4)
            assert cs == cs_fixed and len(cs) == st["bytes"] <= budget
            t0 = time.perf_counter()
            for _ in range(a.frames):
                cs_single = single.encode(img16)
            dt_single = time.perf_counter() - t0
            assert cs_single == cs
            if r:
                fps["pipe_budget"].append(a.frames / dt); fps["pipe_fixed_step"].append(a.frames / dt_fixed)
                fps["encoder_per_frame"].append(a.frames / dt_single)
        out = dict(frame="c3 %dx%dx%d 12-bit, 16-bit containers, host memory" % (w, h, nc), depth=4, frames_per_round=a.frames,
                   bytes_per_sample=bps, budget=budget, grid_index=st["grid_index"], bytes=st["bytes"], bytes_finer=st["bytes_finer"],
                   mean_passes=st["mean_passes"], single_encoder_passes=single.rate_info()["passes"])
        for k, v in fps.items():
            med = float(np.median(v))
            out[k] = dict(fps=[round(x, 1) for x in v], median_fps=round(med, 1), ms_per_frame=round(1e3 / med, 3),
                          spread=round((max(v) - min(v)) / med, 3))
        print(json.dumps(out), flush=True)


def batch_bench(a):
    import torch
    from openjph_amd import codec
    from openjph_amd import plan as planmod
    from openjph_amd.plan import make_params
    from tests import synth
    B = a.batch
    rows = min(a.rows, 2160)
    frames = np.stack([synth.survey_c7(seed=1234 + f)[:, :rows].astype(np.uint16) for f in range(B)])
    _, nc, h, w = frames.shape
    samples = frames[0].size
    d_batch = torch.from_numpy(frames.view(np.int16)).cuda()
    del frames

    def params(qstep):
        return make_params(w, h, nc, bit_depth=12, reversible=False, qstep=qstep)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    batch = codec.Encoder(params(0.001), frames=B)
    single = codec.Encoder(params(0.001))
    plain = {}

    def run_batch(enc):
        enc.run_device(d_batch)
        return [enc.finish(f) for f in range(B)]

    def run_singles():
        out, passes = [], 0
        for f in range(B):
            single.run_device(d_batch[f])
            out.append(single.finish())
            passes += single.rate_info()["passes"]
        return out, passes

    for bps in BPS:
        budget = int(samples * bps)
        batch.set_budgets([budget] * B)
        single.set_budget(budget)
        t = {"batch": [], "singles": [], "plain": []}
        for i in range(a.warmup + a.runs):
            ms_batch, cs = timed(lambda: run_batch(batch))
            infos, rounds, timing = batch.rate_info(), batch.rate_rounds(), batch.rate_timing()
            ms_singles, (cs_single, single_passes) = timed(run_singles)
            assert cs == cs_single and all(len(c) <= budget for c in cs)
            jmed = sorted(x["grid_index"] for x in infos)[B // 2]
            if jmed not in plain:
                plain[jmed] = codec.Encoder(params(planmod.rate_grid_qstep(jmed)), frames=B)
            ms_plain, _ = timed(lambda: run_batch(plain[jmed]))
            if i >= a.warmup:
                t["batch"].append(ms_batch); t["singles"].append(ms_singles); t["plain"].append(ms_plain)
        med = {k: round(float(np.median(v)), 3) for k, v in t.items()}
        passes = sum(x["passes"] for x in infos)
        assert passes == single_passes
        print(json.dumps(dict(
            frames="%d x c7 %dx%dx%d 12-bit, 16-bit containers" % (B, w, h, nc), bytes_per_sample=bps, budget=budget,
            grid_index=[x["grid_index"] for x in infos], bytes=[x["bytes"] for x in infos], rounds=rounds, sum_passes=passes,
            ms_batch_budgets=med["batch"], ms_single_encodes=med["singles"], ms_plain_batch_fixed_step=med["plain"], plain_batch_grid_index=jmed,
            singles_over_batch=round(med["singles"] / med["batch"], 3),
            Gsamples_s_batch=round(B * samples / med["batch"] / 1e6, 2), Gsamples_s_singles=round(B * samples / med["singles"] / 1e6, 2),
            search_ms=round(timing["search_ms"], 3), round_ms=round(timing["search_ms"] / rounds, 3),
            round_device_wait_ms=round(timing["wait_ms"] / rounds, 3), round_host_ms=round((timing["search_ms"] - timing["wait_ms"]) / rounds, 3))),
            flush=True)


def trunc_bench(a):
    import torch
    from openjph_amd import codec
    from openjph_amd.plan import make_params
    from tests import synth
    rows = min(a.rows, 2160)
    rng = np.random.default_rng(1234)
    img = synth._noisy(synth._family(2160, 3840, 32768, 14400, 12800, 4800, 197, 161, 23), rng.normal(0, 640, (3, 2160, 3840)), 65535)[:, :rows]
    nc, h, w = img.shape
    d_img = torch.from_numpy(np.ascontiguousarray(img).astype(np.uint16).view(np.int16)).cuda()
    samples = img.size
    del img
    params = make_params(w, h, nc, bit_depth=16, reversible=True, color_transform=True)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def run(enc):
        enc.run_device(d_img)
        return enc.finish()
    plain = codec.Encoder(params)
    capped = codec.Encoder(params)
    lossless = len(run(plain))
    for share in (0.9, 0.6, 0.3):
        cap = int(lossless * share)
        capped.set_truncation(cap)
        t = {"capped": [], "plain": []}
        info = timing = stats = None
        for i in range(a.warmup + a.runs):
            ms, cs = timed(lambda: run(capped))
            info, timing, stats = capped.trunc_info(), capped.trunc_timing(), capped.timing()
            assert len(cs) == info["bytes"] <= cap < info["bytes_finer"]
            ms_plain, cs_plain = timed(lambda: run(plain))
            assert len(cs_plain) == lossless
            if i >= a.warmup:
                t["capped"].append(ms); t["plain"].append(ms_plain)
        med = {k: round(float(np.median(v)), 3) for k, v in t.items()}
        print(json.dumps(dict(
            frame="c7 family x 16, %dx%dx%d 16-bit, 16-bit containers, 5/3 + RCT" % (w, h, nc), lossless_bytes=lossless, share=share, cap=cap,
            level=info["level"], levels=capped.plan.trunc_levels, bytes=info["bytes"], bytes_finer=info["bytes_finer"], passes=info["passes"],
            first_guess=info["first_guess"], max_dropped=info["max_dropped"], ms_capped=med["capped"], ms_plain_lossless=med["plain"],
            capped_over_plain=round(med["capped"] / med["plain"], 3), coding_in_finish_ms=round(timing["search_ms"], 3),
            run_device_ms=round(stats["total_ms"], 3), stats_int_kernel_ms=round(timing["stats_ms"], 4),
            stats_hbm_fraction=round(4.0 * samples / (timing["stats_ms"] * 1e-3) / HBM_PEAK, 3) if timing["stats_ms"] > 0 else None,
            dwt_level1_ms=round(stats["dwt_levels_ms"][0], 4))), flush=True)


def first_frame_bench(a):
    import torch
    from openjph_amd import codec
    from openjph_amd.plan import make_params
    from tests import synth
    img = synth.survey_c3(rows=a.rows)
    nc, h, w = img.shape
    d_img = torch.from_numpy(img.astype(np.uint16).view(np.int16)).cuda()
    params = make_params(w, h, nc, bit_depth=12, reversible=False, qstep=0.001)
    warm = codec.Encoder(params)                               # the runtime's own first-use costs are not the encoder's
    warm.run_device(d_img)
    warm.finish()
    for bps in BPS:
        budget = int(img.size * bps)
        ms = []
        for _ in range(a.first):
            enc = codec.Encoder(params, max_bytes=budget)
            enc.run_device(d_img)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enc.finish()
            ms.append((time.perf_counter() - t0) * 1e3)
            info = enc.rate_info()
            del enc
        print(json.dumps(dict(frame="c3 %dx%dx%d 12-bit, 16-bit containers" % (w, h, nc), bytes_per_sample=bps, budget=budget,
                              grid_index=info["grid_index"], passes=info["passes"], first_frame_finish_ms=[round(x, 3) for x in ms],
                              median=round(float(np.median(ms)), 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4320, help="top rows of the frame (rehearsals at a small size)")
    ap.add_argument("--no-bisect", action="store_true")
    ap.add_argument("--pipe", action="store_true", help="the budget in the encoder pipe, from host memory")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--batch", type=int, default=0, help="B: the budgets of a batch encoder of B 4K frames against B single encodes")
    ap.add_argument("--first", type=int, default=0, help="N: finish() of the first budgeted frame of N fresh encoders per budget")
    ap.add_argument("--trunc", action="store_true", help="a reversible 4K 16-bit frame under caps of 0.9, 0.6 and 0.3 of its lossless size")
    a = ap.parse_args()
    if a.trunc:
        return trunc_bench(a)
    if a.first:
        return first_frame_bench(a)
    if a.pipe:
        return pipe_bench(a)
    if a.batch:
        return batch_bench(a)
    import torch
    from openjph_amd import codec
    from openjph_amd import plan as planmod
    from openjph_amd.plan import make_params
    from tests import synth
    img = synth.survey_c3(rows=a.rows)
    nc, h, w = img.shape
    d_img = torch.from_numpy(img.astype(np.uint16).view(np.int16)).cuda()
    samples = img.size
    del img

    def params(qstep):
        return make_params(w, h, nc, bit_depth=12, reversible=False, qstep=qstep)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    budgeted = codec.Encoder(params(0.001))
    # one plain encoder per grid index a bisection visits, made once (a caller would keep them, or pay for a plan each time)
    plain = {}

    def plain_len(j):
        if j not in plain:
            plain[j] = codec.Encoder(params(planmod.rate_grid_qstep(j)))
        plain[j].run_device(d_img)
        return len(plain[j].finish())

    def bisect(budget):
        n = [0]

        def size(j):
            n[0] += 1
            return plain_len(j)
        if size(0) > budget:
            return None, n[0]
        if size(GRID - 1) <= budget:
            return GRID - 1, n[0]
        lo, hi = 0, GRID - 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if size(mid) <= budget:
                lo = mid
            else:
                hi = mid
        return lo, n[0]

    for bps in BPS:
        budget = int(samples * bps)
        budgeted.set_budget(budget)

        def run_budgeted():
            budgeted.run_device(d_img)
            return budgeted.finish()
        t = {"budget": [], "fixed": [], "bisect": []}
        info = timing = stats = None
        for i in range(a.warmup + a.runs):
            ms, cs = timed(run_budgeted)
            info, timing, stats = budgeted.rate_info(), budgeted.rate_timing(), budgeted.timing()
            j = info["grid_index"]
            ms_fixed, n_fixed = timed(lambda: plain_len(j))
            assert n_fixed == len(cs) == info["bytes"]
            if not a.no_bisect:
                ms_bis, (jb, encodes) = timed(lambda: bisect(budget))
                assert jb == j
            if i >= a.warmup:
                t["budget"].append(ms); t["fixed"].append(ms_fixed)
                if not a.no_bisect:
                    t["bisect"].append(ms_bis)
        coefs = samples                                         # the sub-band planes hold one coefficient per sample
        med = {k: round(float(np.median(v)), 3) if v else None for k, v in t.items()}
        passes = info["passes"]
        print(json.dumps(dict(
            frame="c3 %dx%dx%d 12-bit, 16-bit containers" % (w, h, nc), bytes_per_sample=bps, budget=budget, grid_index=j,
            qstep=info["qstep"], bytes=info["bytes"], bytes_finer=info["bytes_finer"], passes=passes, first_guess=info["first_guess"],
            ms_budgeted=med["budget"], ms_fixed_step=med["fixed"], ms_bisection=med["bisect"],
            bisection_encodes=None if a.no_bisect else encodes,
            search_ms=round(timing["search_ms"], 3), pass_ms=round(timing["search_ms"] / passes, 3),
            pass_device_wait_ms=round(timing["wait_ms"] / passes, 3), pass_host_ms=round((timing["search_ms"] - timing["wait_ms"]) / passes, 3),
            final_download_t2_ms=round(timing["final_ms"], 3), run_device_ms=round(stats["total_ms"], 3),
            stats_kernel_ms=round(timing["stats_ms"], 4), stats_hbm_fraction=round(4.0 * coefs / (timing["stats_ms"] * 1e-3) / HBM_PEAK, 3),
            dwt_level1_ms=round(stats["dwt_levels_ms"][0], 4))), flush=True)


if __name__ == "__main__":
    main()
