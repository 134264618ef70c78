#!/usr/bin/env python3
"""4:2:2 video buffers on an 8K 10-bit frame (7680 x 4320): what the kernels of kernels_video.hip move per second, and what
handing a v210 buffer to the encoder pipe is worth against planar 16-bit containers.

    python tools/video_bench.py [--rounds 5] [--reps 20] [--frames 48] [--depth 4] [--out profiles/video_bench.txt]

1. Every instantiation of ojphgpu_unpack_video / _pack_video (format x container), bytes read plus written per second, beside
   the yardstick: ojphgpu_unpack_pixels / _pack_pixels with 3 components, 16-bit samples into 16-bit containers, on the same
   number of pixels -- the same kind of copy.  All of them alternate inside every round; a kernel runs `reps` launches per
   round between two device events, after a warm-up round that is not counted, and rotates over four sets of buffers so that
   no launch finds its frame in the 256 MiB Infinity Cache.  Per kernel: the rounds, the median and the spread ((max - min) /
   median).  A new kernel whose median stays below its yardstick's by more than the larger of the two spreads is marked.
2. Frames/s of EncoderPipe(video="v210") against the same pipe fed planar 16-bit containers, both without any host
   conversion (the slots are filled once, before the clock starts), alternating rounds, and the bytes per frame over the
   link for both.

Needs a GPU.  Prints the text it also writes to --out, and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, DEPTH = 7680, 4320, 10
NSETS = 4
KERNELS = [(f, c) for f, cs in (("uyvy", (8, 16, 32)), ("yuy2", (8, 16, 32)), ("v210", (16, 32)), ("y210", (16, 32))) for c in cs]


def median_spread(v):
    med = statistics.median(v)
    return med, (max(v) - min(v)) / med


def kernel_rates(torch, rounds, reps, emit):
    from openjph_amd import codec
    from openjph_amd.pipeline import video_layout
    cw = (W + 1) // 2
    n = W * H + 2 * cw * H
    dts = {8: torch.uint8, 16: torch.int16, 32: torch.int32}
    work = {}                                                # name -> (callable(set index), bytes read + written)
    for fmt, cont in KERNELS:
        b = 8 if fmt in ("uyvy", "yuy2") else DEPTH
        total = video_layout(fmt, W, H)[1]
        vid = [torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda") for _ in range(NSETS)]
        pl = [torch.randint(0, 1 << b, (n,), dtype=torch.int32, device="cuda").to(dts[cont]) for _ in range(NSETS)]
        moved = total + n * (cont // 8)
        work["unpack %s -> %d" % (fmt, cont)] = (lambda i, fmt=fmt, b=b, vid=vid, pl=pl: codec.unpack_video(vid[i], fmt, W, H, b, out=pl[i]), moved)
        work["pack %d -> %s" % (cont, fmt)] = (lambda i, fmt=fmt, b=b, vid=vid, pl=pl: codec.pack_video(pl[i], fmt, W, H, b, out=vid[i]), moved)
    L = __import__("openjph_amd.capi", fromlist=["lib"]).lib()
    import ctypes as C
    pix = [torch.randint(0, 1 << 15, (H, W, 3), dtype=torch.int16, device="cuda") for _ in range(NSETS)]
    pla = [torch.empty((3, H, W), dtype=torch.int16, device="cuda") for _ in range(NSETS)]
    st = codec._stream_ptr(torch, 0)

    def y_unpack(i):
        codec.check(L.ojphgpu_unpack_pixels(st, C.c_void_p(pix[i].data_ptr()), C.c_void_p(pla[i].data_ptr()), W, H, 3, 16, 0, 16), "unpack_pixels")

    def y_pack(i):
        codec.check(L.ojphgpu_pack_pixels(st, C.c_void_p(pla[i].data_ptr()), C.c_void_p(pix[i].data_ptr()), W, H, 3, 16, 16, 0, 16), "pack_pixels")

    work["unpack_pixels 3 x 16 -> 16 (yardstick)"] = (y_unpack, 2 * W * H * 3 * 2)
    work["pack_pixels 16 -> 3 x 16 (yardstick)"] = (y_pack, 2 * W * H * 3 * 2)
    rates = {k: [] for k in work}
    for r in range(rounds + 1):                              # round 0: the warm-up
        for name, (fn, moved) in work.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn(0)
            e0.record()
            for k in range(reps):
                fn(k % NSETS)
            e1.record()
            e1.synchronize()
            if r:
                rates[name].append(moved * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    out = {}
    emit("1. kernels, %d x %d, GB/s read + written; %d rounds of %d launches" % (W, H, rounds, reps))
    for name, v in rates.items():
        med, spread = median_spread(v)
        out[name] = {"GBps": [round(x, 1) for x in v], "median": round(med, 1), "spread": round(spread, 4), "bytes": work[name][1]}
    for name, o in out.items():
        yard = out["unpack_pixels 3 x 16 -> 16 (yardstick)" if name.startswith("unpack") else "pack_pixels 16 -> 3 x 16 (yardstick)"]
        below = o["median"] < yard["median"] * (1 - max(o["spread"], yard["spread"]))
        o["below_yardstick"] = bool(below and "yardstick" not in name)
        emit("  %-40s %s  median %7.1f  spread %4.1f %%  %5.1f MB per launch%s" %
             (name, " ".join("%7.1f" % x for x in o["GBps"]), o["median"], o["spread"] * 100, o["bytes"] / 1e6,
              "   BELOW the yardstick by more than the spread" if o["below_yardstick"] else ""))
    return out


def workload_planes():
    """the 8K frame of bench.py's C3 workload, as 10-bit 4:2:2 planes"""
    from bench import workload_image
    img = workload_image("c3_8k_444_12b_irv97")
    assert img.shape == (3, H, W), img.shape
    return [np.ascontiguousarray(img[0] >> 2), np.ascontiguousarray(img[1][:, 0::2] >> 2), np.ascontiguousarray(img[2][:, 0::2] >> 2)]


def fill_and_drain(pipe, frame):
    k = 0
    while True:
        buf = pipe.acquire()
        if buf is None:
            break
        np.copyto(buf, frame.reshape(buf.shape), casting="unsafe")
        pipe.submit(); k += 1
    first = None
    while pipe.in_flight:
        cs = pipe.collect()
        first = cs if first is None else first
    return first


def steady(pipe, n):
    """n frames in steady state, nothing written on the host (the slots keep their frame) -> seconds"""
    t0 = time.perf_counter()
    sub = col = 0
    while col < n:
        while sub < n and pipe.acquire() is not None:
            pipe.submit(); sub += 1
        pipe.collect(copy=False); col += 1
    return time.perf_counter() - t0


def pipe_rates(rounds, frames, depth, emit):
    from openjph_amd.pipeline import EncoderPipe, pack_video
    from openjph_amd.plan import Plan, make_params
    planes = workload_planes()
    mk = lambda: Plan(make_params(W, H, 3, bit_depth=DEPTH, reversible=False, downsampling=[(1, 1), (2, 1), (2, 1)]))
    video = EncoderPipe(plan=mk(), depth=depth, container=16, video="v210")
    planar = EncoderPipe(plan=mk(), depth=depth, container=16)
    a = fill_and_drain(video, pack_video(planes, "v210", DEPTH))
    b = fill_and_drain(planar, planar.plan.pack_frame(planes))
    assert a == b, "the two pipes' codestreams differ"
    link = {"v210": video.acquire().nbytes, "planar16": planar.acquire().nbytes}
    fps = {"v210": [], "planar16": []}
    for _ in range(rounds):
        fps["v210"].append(frames / steady(video, frames))
        fps["planar16"].append(frames / steady(planar, frames))
    video.close(); planar.close()
    out = {}
    emit("2. EncoderPipe, %d x %d 4:2:2 %d-bit 9/7, depth %d, %d frames per round, codestream %d bytes" % (W, H, DEPTH, depth, frames, len(a)))
    for way, v in fps.items():
        med, spread = median_spread(v)
        out[way] = {"fps": [round(x, 1) for x in v], "median": round(med, 1), "spread": round(spread, 4), "link_bytes_per_frame": int(link[way])}
        emit("  %-10s frames/s per round %s  median %7.1f  spread %4.1f %%  %6.1f MB per frame over the link" %
             (way, " ".join("%7.1f" % x for x in v), med, spread * 100, link[way] / 1e6))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "video_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("video_bench: no GPU visible; there is nothing to measure without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("tools/video_bench.py --rounds %d --reps %d --frames %d --depth %d on %s" % (args.rounds, args.reps, args.frames, args.depth,
                                                                                   torch.cuda.get_device_name(0)))
    kernels = kernel_rates(torch, args.rounds, args.reps, emit)
    torch.cuda.empty_cache()
    pipes = pipe_rates(args.rounds, args.frames, args.depth, emit)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"kernels": kernels, "pipes": pipes}))


if __name__ == "__main__":
    main()
