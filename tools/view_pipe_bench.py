#!/usr/bin/env python3
"""Sequences played at reduced resolution or through a window: the decoder pipe with the view built in
(DecoderPipe(skip_res=, region=)) against the two ways there were before it -- the plain pipe with the crop taken on the
host, and codec.Decoder(skip_res, region) frame by frame.

    python tools/view_pipe_bench.py [--frames 48] [--depth 4] [--rounds 3] [--threads 2]

Workload: C3 (8K 4:4:4 12-bit, 9/7) in 16-bit containers.  Views: the full frame, skip_res 1 and 2, a 1920 x 1080 window at
the centre, and that window at skip_res 1 (the window is given on the full-size grid, so it comes out 960 x 540).  Per view
the three ways run in alternating rounds, every way the same number of frames per round after a warm-up of its own; frames/s per round, the median and the spread (max - min over the median), and
the bytes over the link per frame in each direction (up: the pipes' view_info staged bytes, plus 24 per run for the view
pipe's run table, the single decoder's region_info upload bytes -- block descriptors, the same for all three, not counted; down: the frame handed out -- int32 samples from the single decoder).  The host crop is one numpy slice copy per frame and component
out of the pinned frame (for skip_res > 0 the plain pipe has no equivalent: it decodes the full size, and the crop is taken
of that -- more samples than the view asks for; the column says so).  Needs a GPU; prints text, one JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fill_and_drain(pipe, cs, depth):
    """every slot once (the warm-up; the slots keep the codestream afterwards) -> the first frame"""
    k = 0
    while k < depth:
        buf = pipe.acquire(len(cs))
        if buf is None:
            break
        buf[:] = np.frombuffer(cs, np.uint8)
        pipe.submit(); k += 1
    first = None
    while pipe.in_flight:
        f = pipe.collect()
        first = f if first is None else first
    return first


def steady(pipe, cs, n, per_frame=None):
    """n frames in steady state -> seconds; per_frame(view of the pinned frame) is the consumer's work"""
    t0 = time.perf_counter()
    sub = col = 0
    while col < n:
        while sub < n and pipe.acquire(len(cs)) is not None:
            pipe.submit(); sub += 1
        f = pipe.collect(copy=False); col += 1
        if per_frame is not None:
            per_frame(f)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("view_pipe_bench: no GPU visible; there is nothing to measure without one")
    from bench import WORKLOADS, workload_image
    from openjph_amd import codec
    from openjph_amd.pipeline import DecoderPipe
    from openjph_amd.plan import Plan, make_params
    name = "c3_8k_444_12b_irv97"
    w, h, nc, bd, rev, ct, qstep, tile = WORKLOADS[name]
    plan = Plan(make_params(w, h, nc, bit_depth=bd, reversible=rev, color_transform=ct, qstep=qstep, tile=tile))
    cs = codec.Encoder(plan=plan).encode(workload_image(name))
    win = ((w - 1920) // 2, (h - 1080) // 2, 1920, 1080)
    views = [("full", None, None), ("skip1", (1, 1), None), ("skip2", (2, 2), None), ("window", None, win), ("window+skip1", (1, 1), win)]
    print("workload %s, codestream %d bytes, depth %d, %d frames per round, %d rounds" % (name, len(cs), args.depth, args.frames, args.rounds))
    results = {}
    for vname, skip, region in views:
        single = codec.Decoder(cs, skip_res=skip, region=region)
        want = single.decode()
        single.upload(cs); single.decode()                   # its warm-up: one more frame through the upload path it is timed on
        up_single = single.region_info()["upload_bytes"]
        view = DecoderPipe(cs, depth=args.depth, host_threads=args.threads, skip_res=skip, region=region)
        first = fill_and_drain(view, cs, args.depth)
        assert np.array_equal(first.astype(np.int64), np.clip(want.astype(np.int64), 0, 65535)), "%s: the view pipe's frame differs" % vname
        info = view.view_info()
        plain = DecoderPipe(cs, depth=args.depth, host_threads=args.threads)
        fill_and_drain(plain, cs, args.depth)
        pinfo = plain.view_info()
        crop = None
        if region is not None:                              # the host's crop of the full-size frame, into a buffer of its own
            x0, y0, cw, ch = region
            dst = np.empty((nc, ch, cw), np.uint16)
            crop = lambda f: np.copyto(dst, f[:, y0:y0 + ch, x0:x0 + cw])
        rows = {"view_pipe": [], "plain_pipe_host_crop": [], "single_decoder": []}
        for _ in range(args.rounds):
            rows["view_pipe"].append(args.frames / steady(view, cs, args.frames))
            rows["plain_pipe_host_crop"].append(args.frames / steady(plain, cs, args.frames, crop))
            t0 = time.perf_counter()
            for _ in range(args.frames):
                single.upload(cs)
                single.decode()
            rows["single_decoder"].append(args.frames / (time.perf_counter() - t0))
        view.close(); plain.close()
        down_view = int(np.prod(want.shape)) * 2
        down_plain = w * h * nc * 2
        link = {"view_pipe": (info["staged_bytes"] + 24 * info["runs"], down_view), "plain_pipe_host_crop": (pinfo["staged_bytes"], down_plain),
                "single_decoder": (up_single, int(np.prod(want.shape)) * 4)}
        print("\n%s  skip_res=%s region=%s  frame %s  blocks %d of %d, runs %d" % (vname, skip, region, tuple(want.shape), info["blocks"],
                                                                                 info["plan_blocks"], info["runs"]))
        results[vname] = {}
        for way, fps in rows.items():
            med = statistics.median(fps)
            spread = (max(fps) - min(fps)) / med
            print("  %-22s frames/s per round %s  median %8.1f  spread %4.1f %%  up %10d B/frame  down %10d B/frame" %
                  (way, " ".join("%8.1f" % v for v in fps), med, spread * 100, link[way][0], link[way][1]))
            results[vname][way] = {"fps": [round(v, 2) for v in fps], "median": round(med, 2), "spread": round(spread, 4),
                                   "up_bytes": link[way][0], "down_bytes": link[way][1]}
        if skip and region is None:
            print("  (the plain pipe decodes and downloads the full-size frame; it has no reduced-resolution output to crop)")
    print(json.dumps({"workload": name, "frames": args.frames, "depth": args.depth, "rounds": args.rounds, "views": results}))


if __name__ == "__main__":
    main()
