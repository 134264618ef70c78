#!/usr/bin/env python3
"""Steady-state end-to-end throughput of the frame pipelines (host memory -> codestream in host memory
and back), PCIe and host Tier-2 included: the figure a capture / playback process sees.

    python tools/e2e_pipeline.py [--workload c3|c5|c2] [--frames 48] [--depth 4] [--threads 2] [--container 16]

--max-bytes N: the encoder pipe codes every frame to a byte budget of N (irreversible workloads); the result then also
carries the grid index found, the mean number of passes per frame and the codestream length, and the decoder pipe runs on
that codestream.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_budget_pipe(plan, img, n, max_bytes, depth=4, threads=2, container=16, packed=None, max_sse=None):
    """bench.run_encoder_pipe for a pipe with a byte budget (max_bytes = 0: a plain pipe through the same loop) or, with
    max_sse, a quality target: every slot filled once, then n frames in steady state -> (seconds, stats with the rate or
    quality figures, the codestream)"""
    from openjph_amd.pipeline import EncoderPipe, pack_bits
    pipe = EncoderPipe(plan=plan, depth=depth, container=container, host_threads=threads, packed=packed, max_bytes=max_bytes or None,
                       max_sse=max_sse)
    filled = pack_bits(img, packed) if packed else None
    for _ in range(depth):
        buf = pipe.acquire()
        buf[:] = filled if packed else img.astype(buf.dtype)
        pipe.submit()
    first = None
    while pipe.in_flight:
        c = pipe.collect()
        first = c if first is None else first
    t0 = time.perf_counter()
    sub = col = nbytes = passes = 0
    info = None
    while col < n:
        while sub < n and pipe.acquire() is not None:
            pipe.submit(); sub += 1
        nbytes += len(pipe.collect(copy=False)); col += 1
        if max_bytes or max_sse is not None:
            info = pipe.rate_info() if max_bytes else pipe.quality_info()
            passes += info["passes"]
    dt = time.perf_counter() - t0
    st = pipe.stats()
    pipe.close()
    assert nbytes == n * len(first)
    if max_bytes:
        st.update(max_bytes=max_bytes, grid_index=info["grid_index"], qstep=info["qstep"], bytes=info["bytes"],
                  bytes_finer=info["bytes_finer"], mean_passes=round(passes / n, 3))
    elif max_sse is not None:
        st.update(max_sse=max_sse, grid_index=info["grid_index"], qstep=info["qstep"], bytes=info["bytes"], sse=info["sse"],
                  sse_coarser=info["sse_coarser"], mean_passes=round(passes / n, 3))
    return dt, st, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--threads", type=int, default=2)
    ap.add_argument("--container", type=int, default=16, help="bits per sample in host memory: 8, 16 or 32")
    ap.add_argument("--packed", type=int, default=0, help="frames cross PCIe as bit-packed planes: 10, 12 or 14 bits per sample")
    ap.add_argument("--max-bytes", type=int, default=0, help="code every frame to this byte budget")
    args = ap.parse_args()
    import torch
    from bench import WORKLOADS, workload_image, pcie_bandwidth, run_encoder_pipe, run_decoder_pipe
    from openjph_amd import codec
    from openjph_amd.plan import Plan, make_params
    name = [k for k in WORKLOADS if k.startswith(args.workload)][0]
    w, h, nc, bd, rev, ct, qstep, tile = WORKLOADS[name]
    plan = Plan(make_params(w, h, nc, bit_depth=bd, reversible=rev, color_transform=ct, qstep=qstep, tile=tile))
    img = workload_image(name)
    nsamp = img.size
    res = {"workload": name, "frames": args.frames, "depth": args.depth, "host_threads": args.threads, "pcie_GBps": pcie_bandwidth(torch)}
    want = codec.Encoder(plan=plan).encode(img)
    if args.max_bytes:
        dt, st, want = run_budget_pipe(plan, img, args.frames, args.max_bytes, args.depth, args.threads, args.container, args.packed or None)
        assert len(want) == st["bytes"] <= args.max_bytes
    else:
        dt, st = run_encoder_pipe(plan, img, args.frames, args.depth, args.threads, container=args.container, want=want, packed=args.packed or None)
    res["encode"] = {"Msamples_s": round(nsamp * args.frames / dt / 1e6, 1), "ms_per_frame": round(dt * 1e3 / args.frames, 3), **st,
                     "h2d_GBps": round(img.size * ((args.packed or args.container) / 8) * args.frames / dt / 1e9, 1)}
    ref = codec.decode(want)
    dt, st = run_decoder_pipe(want, args.frames, args.depth, args.threads, container=args.container, want=ref, packed=args.packed or None)
    res["decode"] = {"Msamples_s": round(nsamp * args.frames / dt / 1e6, 1), "ms_per_frame": round(dt * 1e3 / args.frames, 3), **st,
                     "d2h_GBps": round(img.size * ((args.packed or args.container) / 8) * args.frames / dt / 1e9, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
