#!/usr/bin/env python3
"""4:2:2 video buffers on an 8K 10-bit frame (7680 x 4320): what the kernels of kernels_video.hip move per second, and what
handing a v210 buffer to the encoder pipe is worth against planar 16-bit containers.

    python tools/video_bench.py [--rounds 5] [--reps 20] [--frames 48] [--depth 4] [--out profiles/video_bench.txt]

--v420 measures the 4:2:0 kernels of kernels_video420.hip instead (NV12 into 8- and 16-bit containers, P010 into 16- and 32-bit
ones, both directions, the tight layout) beside the yardstick and the 4:2:2 kernels of the same containers (UYVY 8, Y210 16),
marks a 4:2:0 kernel whose median stays below that 4:2:2 kernel's by more than the larger of the two spreads, and runs
EncoderPipe(video="p010") on a 4:2:0 plan against the same pipe fed planes; its default --out is profiles/video420_bench.txt.

--v444 measures the 4:4:4 kernels of kernels_video444.hip instead (v410 and r210 into 16- and 32-bit containers, y416 into 16-
and 32-bit ones, bgra into 8-, 16- and 32-bit ones, both directions, the tight layout) beside the yardstick and the P010 kernels,
holds each against the kernel of those with the nearest bytes per launch in its direction, and runs EncoderPipe(video="v410")
against the same pipe fed planes in 16-bit containers and fed the 10-bit string of packed=10; its default --out is
profiles/video444_bench.txt.

--colour measures the two stages of kernels_colour.hip instead (ojphgpu_frame_rgb_to_ycc / _ycc_to_rgb, 16-bit containers, to and
from 4:2:2 and 4:2:0) beside ojphgpu_frame_resample (the same taps: a 4:4:4 int32 frame to 4:2:2 / 4:2:0 in 16-bit containers) and
ojphgpu_unpack_video444 (r210 into 16-bit containers) on the same frame in the same rounds, and runs EncoderPipe(video="r210",
colour="bt709") against EncoderPipe(video="v410") on the same 4:4:4 10-bit plan; its default --out is profiles/colour_bench.txt.

--chroma measures the stage of kernels_chroma.hip instead (ojphgpu_frame_rechroma, 16-bit containers: 4:2:2 -> 4:2:0, 4:2:0 ->
4:2:2, 4:4:4 -> 4:2:2, 4:2:2 -> 4:4:4) beside ojphgpu_frame_resample and the two colour stages with the same factors on the same
frame in the same rounds, and runs EncoderPipe(video="v210", chroma="cosited") on a 4:2:0 plan against EncoderPipe(video="v210") on
a 4:2:2 plan; its default --out is profiles/chroma_bench.txt.

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
KERNELS_420 = [("nv12", 8), ("nv12", 16), ("p010", 16), ("p010", 32)]
KERNELS_444 = [("v410", 16), ("v410", 32), ("r210", 16), ("r210", 32), ("y416", 16), ("y416", 32), ("bgra", 8), ("bgra", 16), ("bgra", 32)]
PEERS_420 = {8: ("uyvy", 8), 16: ("y210", 16)}              # the 4:2:2 kernel a 4:2:0 kernel is held against, by container (32: none measured beside it)


def median_spread(v):
    med = statistics.median(v)
    return med, (max(v) - min(v)) / med


def timed_rounds(torch, work, rounds, reps):
    """work: name -> (callable(set index), bytes read + written); every kernel in every round, `reps` launches between two
    device events, after a warm-up round that is not counted -> name -> GB/s per round"""
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
    return rates


def yardstick_work(torch, work):
    """adds ojphgpu_unpack_pixels / _pack_pixels, 3 components of 16-bit samples into 16-bit containers, to `work`"""
    from openjph_amd import codec
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


def kernel_rates_444(torch, rounds, reps, emit):
    """the 4:4:4 kernels, the yardstick and the P010 kernels, alternating inside every round; each 4:4:4 kernel beside the one of
    the others with the nearest bytes per launch in its direction"""
    from openjph_amd import codec
    from openjph_amd.pipeline import video420_layout, video444_layout
    dts = {8: torch.uint8, 16: torch.int16, 32: torch.int32}
    work, new = {}, []
    for fmt, cont in KERNELS_444:
        b = {"bgra": 8, "y416": 16}.get(fmt, DEPTH)
        total = video444_layout(fmt, W, H)[1]
        vid = [torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda") for _ in range(NSETS)]
        pl = [torch.randint(0, 1 << b, (3 * W * H,), dtype=torch.int32, device="cuda").to(dts[cont]) for _ in range(NSETS)]
        moved = total + 3 * W * H * (cont // 8)
        work["unpack %s -> %d" % (fmt, cont)] = (lambda i, fmt=fmt, b=b, vid=vid, pl=pl: codec.unpack_video444(vid[i], fmt, W, H, b, out=pl[i]), moved)
        work["pack %d -> %s" % (cont, fmt)] = (lambda i, fmt=fmt, b=b, vid=vid, pl=pl: codec.pack_video444(pl[i], fmt, W, H, b, out=vid[i]), moved)
        new += ["unpack %s -> %d" % (fmt, cont), "pack %d -> %s" % (cont, fmt)]
    n420 = W * H + 2 * ((W + 1) // 2) * ((H + 1) // 2)
    for cont in (16, 32):
        total = video420_layout("p010", W, H)[2]
        vid = [torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda") for _ in range(NSETS)]
        pl = [torch.randint(0, 1 << DEPTH, (n420,), dtype=torch.int32, device="cuda").to(dts[cont]) for _ in range(NSETS)]
        moved = total + n420 * (cont // 8)
        work["unpack p010 -> %d" % cont] = (lambda i, vid=vid, pl=pl: codec.unpack_video420(vid[i], "p010", W, H, DEPTH, out=pl[i]), moved)
        work["pack %d -> p010" % cont] = (lambda i, vid=vid, pl=pl: codec.pack_video420(pl[i], "p010", W, H, DEPTH, out=vid[i]), moved)
    yardstick_work(torch, work)
    rates = timed_rounds(torch, work, rounds, reps)
    emit("1. kernels, %d x %d, GB/s read + written; %d rounds of %d launches" % (W, H, rounds, reps))
    out = {}
    for name, v in rates.items():
        med, spread = median_spread(v)
        out[name] = {"GBps": [round(x, 1) for x in v], "median": round(med, 1), "spread": round(spread, 4), "bytes": work[name][1],
                     "us_per_launch": round(work[name][1] / med / 1e3, 2)}
    for name, o in out.items():
        note = ""
        if name in new:                                      # the claim of DESIGN 1.5: the rate of the existing kernel with the nearest bytes per launch
            peers = [k for k in out if k not in new and k.split()[0].split("_")[0] == name.split()[0]]
            peer = min(peers, key=lambda k: abs(out[k]["bytes"] - o["bytes"]))
            o["peer"] = peer
            o["reaches_peer"] = bool(o["median"] >= out[peer]["median"] * (1 - max(o["spread"], out[peer]["spread"])))
            note = "   %s %s (%.1f)" % ("reaches" if o["reaches_peer"] else "BELOW", peer, out[peer]["median"])
        emit("  %-40s %s  median %7.1f  spread %4.1f %%  %5.1f MB, %5.1f us per launch%s" %
             (name, " ".join("%7.1f" % x for x in o["GBps"]), o["median"], o["spread"] * 100, o["bytes"] / 1e6, o["us_per_launch"], note))
    return out


def kernel_rates_colour(torch, rounds, reps, emit):
    """both colour stages to and from 4:2:2 and 4:2:0 in 16-bit containers, the resample stage with the same factors and the
    r210 unpack, alternating inside every round; launches go straight to the C ABI, nothing waits between them"""
    import ctypes as C
    from openjph_amd import capi, codec
    from openjph_amd.pipeline import colour_table, video444_layout
    L, st = capi.lib(), codec._stream_ptr(torch, 0)
    work = {}

    def c_table(t):
        ct = capi.ColourTable()
        for c in range(3):
            for i in range(3):
                ct.m[c][i] = t.m[c][i]
            ct.off[c], ct.lo[c], ct.hi[c] = t.off[c], t.lo[c], t.hi[c]
        ct.k = t.k
        return ct
    fwd, inv = c_table(colour_table("bt709", "forward", DEPTH, DEPTH)), c_table(colour_table("bt709", "inverse", DEPTH, DEPTH))
    rgb = [torch.randint(0, 1 << DEPTH, (3 * W * H,), dtype=torch.int32, device="cuda").to(torch.int16) for _ in range(NSETS)]
    ycc = [torch.randint(0, 1 << DEPTH, (3 * W * H,), dtype=torch.int32, device="cuda").to(torch.int16) for _ in range(NSETS)]
    src32 = [torch.randint(0, 1 << DEPTH, (3 * W * H,), dtype=torch.int32, device="cuda") for _ in range(NSETS)]
    for name, fx, fy in (("4:2:2", 2, 1), ("4:2:0", 2, 2)):
        cw, ch = (W + fx - 1) // fx, (H + fy - 1) // fy
        f = capi.ColourFrame(W, H, fx, fy)
        f.rgb_first[:] = [0, W * H, 2 * W * H]
        f.ycc_first[:] = [0, W * H, W * H + cw * ch]
        moved = (3 * W * H + W * H + 2 * cw * ch) * 2
        work["rgb_to_ycc 16 -> 16 %s" % name] = (lambda i, f=f: codec.check(L.ojphgpu_frame_rgb_to_ycc(st, C.c_void_p(rgb[i].data_ptr()), 16, C.c_void_p(ycc[i].data_ptr()), 16, C.byref(f), C.byref(fwd)), "rgb_to_ycc"), moved)
        work["ycc_to_rgb 16 -> 16 %s" % name] = (lambda i, f=f: codec.check(L.ojphgpu_frame_ycc_to_rgb(st, C.c_void_p(ycc[i].data_ptr()), 16, C.c_void_p(rgb[i].data_ptr()), 16, C.byref(f), C.byref(inv)), "ycc_to_rgb"), moved)
        comps = np.zeros(3, codec.resample_comp_dtype)
        at = 0
        for c, (gx, gy) in enumerate(((1, 1), (fx, fy), (fx, fy))):
            dw, dh = (W + gx - 1) // gx, (H + gy - 1) // gy
            comps[c] = (c * W * H, at, W, H, dw, dh, gx, gy, 0, 0, 0, 0, (1 << DEPTH) - 1, 0)
            at += dw * dh
        d_comps = codec.to_device(comps, 0)
        work["frame_resample 32 -> 16 %s (the same taps)" % name] = (lambda i, d=d_comps: codec.check(L.ojphgpu_frame_resample(st, C.c_void_p(src32[i].data_ptr()), C.c_void_p(ycc[i].data_ptr()), 16, C.c_void_p(d.data_ptr()), 3), "frame_resample"),
                                                                    3 * W * H * 4 + at * 2)
    total = video444_layout("r210", W, H)[1]
    vid = [torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda") for _ in range(NSETS)]
    work["unpack r210 -> 16"] = (lambda i: codec.check(L.ojphgpu_unpack_video444(st, 0x23, C.c_void_p(vid[i].data_ptr()), 4 * W, C.c_void_p(rgb[i].data_ptr()), W, H, DEPTH, 16), "unpack_video444"),
                                 total + 3 * W * H * 2)
    rates = timed_rounds(torch, work, rounds, reps)
    emit("1. kernels, %d x %d, TB/s read + written; %d rounds of %d launches" % (W, H, rounds, reps))
    out = {}
    for name, v in rates.items():
        med, spread = median_spread(v)
        out[name] = {"GBps": [round(x, 1) for x in v], "median": round(med, 1), "spread": round(spread, 4), "bytes": work[name][1],
                     "us_per_launch": round(work[name][1] / med / 1e3, 2)}
        emit("  %-46s %s  median %6.3f TB/s  spread %4.1f %%  %5.1f MB, %6.1f us per launch" %
             (name, " ".join("%6.3f" % (x / 1e3) for x in v), med / 1e3, spread * 100, work[name][1] / 1e6, out[name]["us_per_launch"]))
    return out


def kernel_rates_chroma(torch, rounds, reps, emit):
    """the chroma stage between 4:4:4, 4:2:2 and 4:2:0 in 16-bit containers, the resample stage and both colour stages with the
    same factors, alternating inside every round; launches go straight to the C ABI, nothing waits between them"""
    import ctypes as C
    from openjph_amd import capi, codec
    from openjph_amd.pipeline import colour_table
    L, st = capi.lib(), codec._stream_ptr(torch, 0)
    work = {}

    def c_table(t):
        ct = capi.ColourTable()
        for c in range(3):
            for i in range(3):
                ct.m[c][i] = t.m[c][i]
            ct.off[c], ct.lo[c], ct.hi[c] = t.off[c], t.lo[c], t.hi[c]
        ct.k = t.k
        return ct
    fwd, inv = c_table(colour_table("bt709", "forward", DEPTH, DEPTH)), c_table(colour_table("bt709", "inverse", DEPTH, DEPTH))
    a16 = [torch.randint(0, 1 << DEPTH, (3 * W * H,), dtype=torch.int32, device="cuda").to(torch.int16) for _ in range(NSETS)]
    b16 = [torch.randint(0, 1 << DEPTH, (3 * W * H,), dtype=torch.int32, device="cuda").to(torch.int16) for _ in range(NSETS)]
    src32 = [torch.randint(0, 1 << DEPTH, (3 * W * H,), dtype=torch.int32, device="cuda") for _ in range(NSETS)]
    size = lambda c: ((W + c[0] - 1) // c[0]) * ((H + c[1] - 1) // c[1])
    for name, s, d in (("4:2:2 -> 4:2:0", (2, 1), (2, 2)), ("4:2:0 -> 4:2:2", (2, 2), (2, 1)), ("4:4:4 -> 4:2:2", (1, 1), (2, 1)), ("4:2:2 -> 4:4:4", (2, 1), (1, 1))):
        f = capi.ChromaFrame(W, H, s[0], s[1], d[0], d[1])
        f.src_off[:] = [0, W * H, W * H + size(s)]
        f.dst_off[:] = [0, W * H, W * H + size(d)]
        work["rechroma 16 %s" % name] = (lambda i, f=f: codec.check(L.ojphgpu_frame_rechroma(st, C.c_void_p(a16[i].data_ptr()), C.c_void_p(b16[i].data_ptr()), 16, C.byref(f)), "frame_rechroma"),
                                         (2 * W * H + 2 * size(s) + 2 * size(d)) * 2)
    for name, fx, fy in (("across", 2, 1), ("down", 1, 2)):   # the factors of the four above: chroma halved / doubled in one direction
        cw, ch = (W + fx - 1) // fx, (H + fy - 1) // fy
        f = capi.ColourFrame(W, H, fx, fy)
        f.rgb_first[:] = [0, W * H, 2 * W * H]
        f.ycc_first[:] = [0, W * H, W * H + cw * ch]
        moved = (3 * W * H + W * H + 2 * cw * ch) * 2
        work["rgb_to_ycc 16 -> 16 halved %s" % name] = (lambda i, f=f: codec.check(L.ojphgpu_frame_rgb_to_ycc(st, C.c_void_p(a16[i].data_ptr()), 16, C.c_void_p(b16[i].data_ptr()), 16, C.byref(f), C.byref(fwd)), "rgb_to_ycc"), moved)
        work["ycc_to_rgb 16 -> 16 doubled %s" % name] = (lambda i, f=f: codec.check(L.ojphgpu_frame_ycc_to_rgb(st, C.c_void_p(b16[i].data_ptr()), 16, C.c_void_p(a16[i].data_ptr()), 16, C.byref(f), C.byref(inv)), "ycc_to_rgb"), moved)
        comps = np.zeros(3, codec.resample_comp_dtype)
        at = 0
        for c, (gx, gy) in enumerate(((1, 1), (fx, fy), (fx, fy))):
            dw, dh = (W + gx - 1) // gx, (H + gy - 1) // gy
            comps[c] = (c * W * H, at, W, H, dw, dh, gx, gy, 0, 0, 0, 0, (1 << DEPTH) - 1, 0)
            at += dw * dh
        d_comps = codec.to_device(comps, 0)
        work["frame_resample 32 -> 16 halved %s" % name] = (lambda i, d=d_comps: codec.check(L.ojphgpu_frame_resample(st, C.c_void_p(src32[i].data_ptr()), C.c_void_p(b16[i].data_ptr()), 16, C.c_void_p(d.data_ptr()), 3), "frame_resample"),
                                                            3 * W * H * 4 + at * 2)
    rates = timed_rounds(torch, work, rounds, reps)
    emit("1. kernels, %d x %d, TB/s read + written; %d rounds of %d launches" % (W, H, rounds, reps))
    out = {}
    for name, v in rates.items():
        med, spread = median_spread(v)
        out[name] = {"GBps": [round(x, 1) for x in v], "median": round(med, 1), "spread": round(spread, 4), "bytes": work[name][1],
                     "us_per_launch": round(work[name][1] / med / 1e3, 2)}
        emit("  %-46s %s  median %6.3f TB/s  spread %4.1f %%  %5.1f MB, %6.1f us per launch" %
             (name, " ".join("%6.3f" % (x / 1e3) for x in v), med / 1e3, spread * 100, work[name][1] / 1e6, out[name]["us_per_launch"]))
    return out


def pipe_rates_chroma(rounds, frames, depth, emit):
    """EncoderPipe fed one v210 buffer two ways, alternating rounds: chroma="cosited" on the 8K 10-bit 4:2:0 plan (unpack + the stage
    that halves chroma down) against the plain video="v210" pipe on the 4:2:2 plan (unpack alone; it codes half as many chroma
    samples more)"""
    from openjph_amd.pipeline import EncoderPipe, pack_video
    from openjph_amd.plan import Plan, make_params
    frame = pack_video(workload_planes(), "v210", DEPTH)
    mk = lambda fy: Plan(make_params(W, H, 3, bit_depth=DEPTH, reversible=False, downsampling=[(1, 1), (2, fy), (2, fy)]))
    pipes = {"v210 -> 4:2:0 (chroma)": EncoderPipe(plan=mk(2), depth=depth, container=16, video="v210", chroma="cosited"),
             "v210 -> 4:2:2 (plain)": EncoderPipe(plan=mk(1), depth=depth, container=16, video="v210")}
    first = {way: fill_and_drain(p, frame) for way, p in pipes.items()}
    fps = {way: [] for way in pipes}
    for _ in range(rounds):
        for way, p in pipes.items():
            fps[way].append(frames / steady(p, frames))
    for p in pipes.values():
        p.close()
    out = {}
    emit("2. EncoderPipe, %d x %d %d-bit 9/7, one v210 buffer per frame, depth %d, %d frames per round, codestreams %s bytes" %
         (W, H, DEPTH, depth, frames, " / ".join(str(len(first[w])) for w in pipes)))
    for way, v in fps.items():
        med, spread = median_spread(v)
        out[way] = {"fps": [round(x, 1) for x in v], "median": round(med, 1), "spread": round(spread, 4), "ms_per_frame": round(1e3 / med, 3)}
        emit("  %-23s frames/s per round %s  median %7.1f  spread %4.1f %%  %6.3f ms per frame" %
             (way, " ".join("%7.1f" % x for x in v), med, spread * 100, 1e3 / med))
    return out


def pipe_rates_colour(rounds, frames, depth, emit):
    """EncoderPipe on the 8K 10-bit 4:4:4 plan fed one v410 buffer (no colour stage) against the same plan fed one r210 buffer
    with colour="bt709" (unpack + the forward stage), alternating rounds: the difference is the stage's cost in the overlap"""
    from bench import workload_image
    from openjph_amd.pipeline import EncoderPipe, pack_video444
    from openjph_amd.plan import Plan, make_params
    img = workload_image("c3_8k_444_12b_irv97")
    assert img.shape == (3, H, W), img.shape
    planes = [np.ascontiguousarray(img[c] >> 2) for c in range(3)]
    mk = lambda: Plan(make_params(W, H, 3, bit_depth=DEPTH, reversible=False))
    pipes = {"v410": EncoderPipe(plan=mk(), depth=depth, container=16, video="v410"),
             "r210+bt709": EncoderPipe(plan=mk(), depth=depth, container=16, video="r210", colour="bt709")}
    frame = {"v410": pack_video444(planes, "v410", DEPTH), "r210+bt709": pack_video444(planes, "r210", DEPTH)}
    first = {way: fill_and_drain(p, frame[way]) for way, p in pipes.items()}
    fps = {way: [] for way in pipes}
    for _ in range(rounds):
        for way, p in pipes.items():
            fps[way].append(frames / steady(p, frames))
    for p in pipes.values():
        p.close()
    out = {}
    emit("2. EncoderPipe, %d x %d 4:4:4 %d-bit 9/7, depth %d, %d frames per round, codestreams %s bytes" %
         (W, H, DEPTH, depth, frames, " / ".join(str(len(first[w])) for w in pipes)))
    for way, v in fps.items():
        med, spread = median_spread(v)
        out[way] = {"fps": [round(x, 1) for x in v], "median": round(med, 1), "spread": round(spread, 4), "ms_per_frame": round(1e3 / med, 3)}
        emit("  %-11s frames/s per round %s  median %7.1f  spread %4.1f %%  %6.3f ms per frame" %
             (way, " ".join("%7.1f" % x for x in v), med, spread * 100, 1e3 / med))
    return out


def kernel_rates(torch, rounds, reps, emit, v420=False):
    from openjph_amd import codec
    from openjph_amd.pipeline import video420_layout, video_layout
    cw = (W + 1) // 2
    n = W * H + 2 * cw * H
    dts = {8: torch.uint8, 16: torch.int16, 32: torch.int32}
    work = {}                                                # name -> (callable(set index), bytes read + written)
    for fmt, cont in KERNELS_420 if v420 else ():
        b = 8 if fmt == "nv12" else DEPTH
        n420 = W * H + 2 * cw * ((H + 1) // 2)
        total = video420_layout(fmt, W, H)[2]
        vid = [torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda") for _ in range(NSETS)]
        pl = [torch.randint(0, 1 << b, (n420,), dtype=torch.int32, device="cuda").to(dts[cont]) for _ in range(NSETS)]
        moved = total + n420 * (cont // 8)
        work["unpack %s -> %d" % (fmt, cont)] = (lambda i, fmt=fmt, b=b, vid=vid, pl=pl: codec.unpack_video420(vid[i], fmt, W, H, b, out=pl[i]), moved)
        work["pack %d -> %s" % (cont, fmt)] = (lambda i, fmt=fmt, b=b, vid=vid, pl=pl: codec.pack_video420(pl[i], fmt, W, H, b, out=vid[i]), moved)
    for fmt, cont in sorted(set(PEERS_420.values())) if v420 else KERNELS:
        b = 8 if fmt in ("uyvy", "yuy2") else DEPTH
        total = video_layout(fmt, W, H)[1]
        vid = [torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda") for _ in range(NSETS)]
        pl = [torch.randint(0, 1 << b, (n,), dtype=torch.int32, device="cuda").to(dts[cont]) for _ in range(NSETS)]
        moved = total + n * (cont // 8)
        work["unpack %s -> %d" % (fmt, cont)] = (lambda i, fmt=fmt, b=b, vid=vid, pl=pl: codec.unpack_video(vid[i], fmt, W, H, b, out=pl[i]), moved)
        work["pack %d -> %s" % (cont, fmt)] = (lambda i, fmt=fmt, b=b, vid=vid, pl=pl: codec.pack_video(pl[i], fmt, W, H, b, out=vid[i]), moved)
    yardstick_work(torch, work)
    rates = timed_rounds(torch, work, rounds, reps)
    out = {}
    emit("1. kernels, %d x %d, GB/s read + written; %d rounds of %d launches" % (W, H, rounds, reps))
    floor = None
    if v420:
        # the same loop on a 64 x 2 frame: the pace at which this host issues launches (the device's own fixed cost per launch
        # hides below it).  The kernels here take 20 to 70 us per launch: the loop above stays ahead of the device when this
        # figure is well below that.  --frame tells what a rate owes to the bytes of a launch
        tv, tp = torch.zeros(4096, dtype=torch.uint8, device="cuda"), torch.zeros(4096, dtype=torch.uint8, device="cuda")
        us = []
        for r in range(rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(10 * reps):
                codec.unpack_video420(tv, "nv12", 64, 2, 8, out=tp)
            e1.record()
            e1.synchronize()
            if r:
                us.append(e0.elapsed_time(e1) * 1e3 / (10 * reps))
        floor = statistics.median(us)
        emit("  one launch on a 64 x 2 frame (the host's issue pace), us: %s  median %.2f" % (" ".join("%.2f" % x for x in us), floor))
    for name, v in rates.items():
        med, spread = median_spread(v)
        out[name] = {"GBps": [round(x, 1) for x in v], "median": round(med, 1), "spread": round(spread, 4), "bytes": work[name][1]}
    for name, o in out.items():
        yard = out["unpack_pixels 3 x 16 -> 16 (yardstick)" if name.startswith("unpack") else "pack_pixels 16 -> 3 x 16 (yardstick)"]
        below = o["median"] < yard["median"] * (1 - max(o["spread"], yard["spread"]))
        o["below_yardstick"] = bool(below and "yardstick" not in name)
        note = "   BELOW the yardstick by more than the spread" if o["below_yardstick"] else ""
        words = name.split()
        fmt, cont = (words[1], int(words[3])) if words[0] == "unpack" else (words[3], int(words[1])) if words[0] == "pack" else (None, 0)
        if v420 and (fmt, cont) in KERNELS_420 and cont in PEERS_420:      # the claim of the 4:2:2 finding: at least the 4:2:2 kernel of its container
            peer = out[("unpack %s -> %d" if words[0] == "unpack" else "pack %d -> %s") % (PEERS_420[cont] if words[0] == "unpack" else PEERS_420[cont][::-1])]
            o["peer_422"] = "%s %d" % PEERS_420[cont]
            o["reaches_peer_422"] = bool(o["median"] >= peer["median"] * (1 - max(o["spread"], peer["spread"])))
            note += "   %s %s %d (%.1f)" % ("reaches" if o["reaches_peer_422"] else "BELOW", PEERS_420[cont][0], cont, peer["median"])
        o["us_per_launch"] = round(o["bytes"] / o["median"] / 1e3, 2)
        emit("  %-40s %s  median %7.1f  spread %4.1f %%  %5.1f MB, %5.1f us per launch%s" %
             (name, " ".join("%7.1f" % x for x in o["GBps"]), o["median"], o["spread"] * 100, o["bytes"] / 1e6, o["us_per_launch"], note))
    if floor is not None:
        out["launch_floor_us"] = round(floor, 2)
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


def pipe_rates(rounds, frames, depth, emit, v420=False):
    from openjph_amd.pipeline import EncoderPipe, pack_video, pack_video420
    from openjph_amd.plan import Plan, make_params
    planes = workload_planes()
    fmt = "p010" if v420 else "v210"
    if v420:                                                 # the same frame as 4:2:0 planes
        planes = [planes[0], np.ascontiguousarray(planes[1][0::2]), np.ascontiguousarray(planes[2][0::2])]
    mk = lambda: Plan(make_params(W, H, 3, bit_depth=DEPTH, reversible=False, downsampling=[(1, 1), (2, 2 if v420 else 1), (2, 2 if v420 else 1)]))
    video = EncoderPipe(plan=mk(), depth=depth, container=16, video=fmt)
    planar = EncoderPipe(plan=mk(), depth=depth, container=16)
    a = fill_and_drain(video, pack_video420(planes, fmt, DEPTH) if v420 else pack_video(planes, fmt, DEPTH))
    b = fill_and_drain(planar, planar.plan.pack_frame(planes))
    assert a == b, "the two pipes' codestreams differ"
    link = {fmt: video.acquire().nbytes, "planar16": planar.acquire().nbytes}
    fps = {fmt: [], "planar16": []}
    for _ in range(rounds):
        fps[fmt].append(frames / steady(video, frames))
        fps["planar16"].append(frames / steady(planar, frames))
    video.close(); planar.close()
    out = {}
    emit("2. EncoderPipe, %d x %d %s %d-bit 9/7, depth %d, %d frames per round, codestream %d bytes" % (W, H, "4:2:0" if v420 else "4:2:2", DEPTH, depth, frames, len(a)))
    for way, v in fps.items():
        med, spread = median_spread(v)
        out[way] = {"fps": [round(x, 1) for x in v], "median": round(med, 1), "spread": round(spread, 4), "link_bytes_per_frame": int(link[way])}
        emit("  %-10s frames/s per round %s  median %7.1f  spread %4.1f %%  %6.1f MB per frame over the link" %
             (way, " ".join("%7.1f" % x for x in v), med, spread * 100, link[way] / 1e6))
    return out


def pipe_rates_444(rounds, frames, depth, emit):
    """EncoderPipe on the 8K 10-bit 4:4:4 frame three ways, alternating: one v410 buffer, planes in 16-bit containers, the 10-bit
    string of packed=10"""
    from bench import workload_image
    from openjph_amd.pipeline import EncoderPipe, pack_bits, pack_video444
    from openjph_amd.plan import Plan, make_params
    img = workload_image("c3_8k_444_12b_irv97")
    assert img.shape == (3, H, W), img.shape
    planes = [np.ascontiguousarray(img[c] >> 2) for c in range(3)]
    mk = lambda: Plan(make_params(W, H, 3, bit_depth=DEPTH, reversible=False))
    pipes = {"v410": EncoderPipe(plan=mk(), depth=depth, container=16, video="v410"), "planar16": EncoderPipe(plan=mk(), depth=depth, container=16),
             "packed10": EncoderPipe(plan=mk(), depth=depth, container=16, packed=10)}
    flat = pipes["planar16"].plan.pack_frame(planes).reshape(-1)
    chunk = 1 << 22                                          # (a multiple of 32 samples: the chunks' strings follow each other byte-aligned)
    frame = {"v410": pack_video444(planes, "v410", DEPTH), "planar16": flat,
             "packed10": np.concatenate([pack_bits(flat[i:i + chunk], 10) for i in range(0, flat.size, chunk)])}
    first = {way: fill_and_drain(p, frame[way]) for way, p in pipes.items()}
    assert first["v410"] == first["planar16"] == first["packed10"], "the pipes' codestreams differ"
    link = {way: p.acquire().nbytes for way, p in pipes.items()}
    fps = {way: [] for way in pipes}
    for _ in range(rounds):
        for way, p in pipes.items():
            fps[way].append(frames / steady(p, frames))
    for p in pipes.values():
        p.close()
    out = {}
    emit("2. EncoderPipe, %d x %d 4:4:4 %d-bit 9/7, depth %d, %d frames per round, codestream %d bytes" % (W, H, DEPTH, depth, frames, len(first["v410"])))
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
    ap.add_argument("--v420", action="store_true", help="the 4:2:0 kernels and a p010 pipe beside the yardstick and their 4:2:2 peers")
    ap.add_argument("--v444", action="store_true", help="the 4:4:4 kernels and a v410 pipe beside the yardstick, the P010 kernels, planes and packed=10")
    ap.add_argument("--colour", action="store_true", help="the RGB <-> YCbCr stages beside the resample stage and the r210 unpack; an r210 + colour pipe against a v410 pipe")
    ap.add_argument("--chroma", action="store_true", help="the chroma stage beside the resample stage and the colour stages of the same factors; a v210 + chroma pipe on a 4:2:0 plan against the plain v210 pipe")
    ap.add_argument("--frame", default=None, metavar="WxH", help="another frame size for the kernels (the pipes are then left out): what a rate owes to the bytes of a launch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "chroma_bench.txt" if args.chroma else "colour_bench.txt" if args.colour else "video444_bench.txt" if args.v444 else "video420_bench.txt" if args.v420 else "video_bench.txt")
    global W, H
    if args.frame:
        W, H = (int(v) for v in args.frame.lower().split("x"))
    import torch
    if not torch.cuda.is_available():
        sys.exit("video_bench: no GPU visible; there is nothing to measure without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("tools/video_bench.py%s%s --rounds %d --reps %d --frames %d --depth %d on %s" % (" --chroma" if args.chroma else " --colour" if args.colour else " --v444" if args.v444 else " --v420" if args.v420 else "", " --frame " + args.frame if args.frame else "", args.rounds, args.reps, args.frames,
                                                                                     args.depth, torch.cuda.get_device_name(0)))
    kernels = kernel_rates_chroma(torch, args.rounds, args.reps, emit) if args.chroma else kernel_rates_colour(torch, args.rounds, args.reps, emit) if args.colour else kernel_rates_444(torch, args.rounds, args.reps, emit) if args.v444 else kernel_rates(torch, args.rounds, args.reps, emit, args.v420)
    torch.cuda.empty_cache()
    if args.frame:
        pipes = {}
    else:
        pipes = pipe_rates_chroma(args.rounds, args.frames, args.depth, emit) if args.chroma else pipe_rates_colour(args.rounds, args.frames, args.depth, emit) if args.colour else pipe_rates_444(args.rounds, args.frames, args.depth, emit) if args.v444 else pipe_rates(args.rounds, args.frames, args.depth, emit, args.v420)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"kernels": kernels, "pipes": pipes}))


if __name__ == "__main__":
    main()
