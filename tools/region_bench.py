"""Region decoding against the whole-frame decode of the same codestream, device-resident (the codestream bytes are uploaded
once per decoder, before timing): the C3 8K frame whole and as regions of 256^2, 1024^2 and 4096^2, the C4 16K tiled image
whole and as a 2048^2 region.  Each decoder runs `--warmup` times, then the decoders take turns, `--runs` rounds; a run is
timed by the decoder's own device events (total_ms).  Prints one JSON line per case: median / min ms, blocks decoded, bytes
uploaded, tiles touched, and the ratio to the whole decode.
  python tools/region_bench.py [--runs 20] [--warmup 5] [--only c3-1024]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cases():
    from openjph_amd import codec
    from openjph_amd.plan import Plan, make_params
    from tests import synth
    img = synth.survey_c3()
    cs3 = codec.Encoder(bit_depth=12, width=7680, height=4320, num_comps=3, reversible=False, qstep=0.001).encode(img)
    del img
    yield "c3", cs3, [("c3-full", None), ("c3-256", (3701, 2001, 256, 256)), ("c3-1024", (3001, 1501, 1024, 1024)),
                      ("c3-4096", (1799, 111, 4096, 4096))]
    img = synth.survey_c4()
    cs4 = codec.Encoder(plan=Plan(make_params(16384, 16384, 1, bit_depth=16, tile=(1024, 1024)))).encode(img)
    del img
    yield "c4", cs4, [("c4-full", None), ("c4-2048", (7001, 5001, 2048, 2048))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="run the whole decode and this one case (e.g. c3-1024)")
    a = ap.parse_args()
    import torch
    from openjph_amd import codec
    for frame, cs, regs in cases():
        if a.only and not a.only.startswith(frame):
            continue
        regs = [r for r in regs if r[1] is None or not a.only or r[0] == a.only]
        decs = []
        for name, reg in regs:
            dec = codec.Decoder(cs, region=reg)
            dec.set_timing(False)
            out = dec.run_device(dtype=torch.int16)
            assert dec.failed_blocks() == 0
            decs.append((name, reg, dec, out))
        times = {name: [] for name, *_ in decs}
        for i in range(a.warmup + a.runs):
            for name, reg, dec, out in decs:                 # alternated: every decoder sees the same chip state
                dec.run_device(out)
                dec.failed_blocks()
                if i >= a.warmup:
                    times[name].append(dec.timing()["total_ms"])
        full = float(np.median(times[decs[0][0]]))
        for name, reg, dec, out in decs:
            t = np.asarray(times[name])
            info = dec.region_info()
            print(json.dumps(dict(case=name, region=reg, ms_median=round(float(np.median(t)), 4), ms_min=round(float(t.min()), 4),
                                  vs_full=round(float(np.median(t)) / full, 3), blocks=info["blocks"], plan_blocks=info["plan_blocks"],
                                  upload_bytes=info["upload_bytes"], codestream_bytes=len(cs), tiles=info["tiles"])), flush=True)
        del decs


if __name__ == "__main__":
    main()
