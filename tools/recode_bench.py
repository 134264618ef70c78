"""The recoder against what a caller has without it: the C3 8K frame (tests/synth.py survey_c3, 12-bit) coded REVERSIBLY --
the archive form codec.transcode refuses to recode -- taken to the 9/7 at a byte budget of 0.2 bytes per sample and at a fixed
step (0.001).  Per target the contenders take turns, `--runs` rounds after `--warmup`, host clock from the call to a stream
synchronise:

  recoder               codec.Recoder: submit (parse, upload, decode into the int32 frame, the fit, the encoder's run) +
                        finish (verdicts; with a budget the search; download, Tier-2); submit and finish are also given
                        apart, and the object's own timing() of the last round
  new_decoder_encode    a Decoder made from the codestream in every round (parse, create, upload), run_device into an int32
                        frame, failed_blocks, the clamp in torch into a 16-bit frame, then a resident Encoder's run_device +
                        finish: what a caller has for a SEQUENCE of codestreams -- a Decoder's block descriptors are its first
                        codestream's
  resident_pair         the same with one resident Decoder handed the same bytes again (upload, run_device): what the pair
                        costs where it can be used at all

All three write the same bytes (asserted).  Beside the table: the fit kernel's time (device events, Recoder.timing) and its
share of the HBM peak from the bytes it moves, 4 read + 2 written per sample.  One JSON line per target: medians, spread =
(max - min) / median.
  python tools/recode_bench.py [--runs 10] [--warmup 2] [--rows 4320]
  python tools/recode_bench.py --resample [...]: the resampling stage beside the fit (resample_rounds below)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OUT_QSTEP = 0.001
BPS = 0.2
HBM_PEAK = 8e12                                   # bytes per second (MI355X, specification)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=4320, help="top rows of the frame (rehearsals at a small size)")
    ap.add_argument("--resample", action="store_true", help="the resampling stage beside the fit: 4:4:4 / 4:2:2 / 4:2:0 at 10 bits")
    a = ap.parse_args()
    import torch
    from openjph_amd import codec
    from openjph_amd.plan import make_params
    from tests import synth
    img = synth.survey_c3(rows=a.rows)
    nc, h, w = img.shape
    samples = img.size
    cs = codec.Encoder(make_params(w, h, nc, bit_depth=12, reversible=True)).encode(img.astype(np.uint16))
    del img

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    if a.resample:
        return resample_rounds(a, codec, cs, (nc, h, w))
    dec = codec.Decoder(cs)
    d32 = torch.empty(dec.shape, dtype=torch.int32, device="cuda")
    targets = [("budget %.2f B/sample" % BPS, dict(max_bytes=int(samples * BPS))), ("qstep %.3f" % OUT_QSTEP, dict(qstep=OUT_QSTEP))]
    for label, kw in targets:
        rec = codec.Recoder(cs, reversible=False, **kw)
        enc = codec.Encoder(make_params(w, h, nc, bit_depth=12, reversible=False, qstep=kw.get("qstep", -1.0)), max_bytes=kw.get("max_bytes", 0))

        def pair(d, upload):
            if upload:
                d.upload(cs)
            d.run_device(d32)
            assert d.failed_blocks() == 0
            enc.run_device(d32.clamp(0, 4095).to(torch.int16))
            return enc.finish()
        t = {"recoder": [], "submit": [], "finish": [], "new_decoder_encode": [], "resident_pair": []}
        fit = []
        for i in range(a.warmup + a.runs):
            ms_sub, _ = timed(lambda: rec.submit(cs))
            ms_fin, out_r = timed(rec.finish)
            ms_new, out_n = timed(lambda: pair(codec.Decoder(cs), False))
            ms_res, out_p = timed(lambda: pair(dec, True))
            assert out_r == out_n == out_p
            if i >= a.warmup:
                t["recoder"].append(ms_sub + ms_fin); t["submit"].append(ms_sub); t["finish"].append(ms_fin)
                t["new_decoder_encode"].append(ms_new); t["resident_pair"].append(ms_res)
                fit.append(rec.timing()["fit_ms"])
        out = dict(frame="c3 %dx%dx%d 12-bit reversible, %d bytes" % (w, h, nc, len(cs)), target=label, runs=a.runs, bytes_out=len(out_r))
        if "max_bytes" in kw:
            out.update(budget=kw["max_bytes"], grid_index=rec.rate_info()["grid_index"], passes=rec.rate_info()["passes"])
        for k, v in t.items():
            med = float(np.median(v))
            out[k] = dict(median_ms=round(med, 3), spread=round((max(v) - min(v)) / med, 3))
        out["recoder_ahead_of_new_decoder_ms"] = round(out["new_decoder_encode"]["median_ms"] - out["recoder"]["median_ms"], 3)
        fit_ms = float(np.median(fit))
        out["fit_kernel"] = dict(median_ms=round(fit_ms, 4), spread=round((max(fit) - min(fit)) / fit_ms, 3), bytes=samples * 6,
                                 share_of_hbm_peak=round(samples * 6 / (fit_ms * 1e-3) / HBM_PEAK, 3))
        out["recoder_timing_ms"] = {k: round(float(v), 3) for k, v in rec.timing().items()}
        print(json.dumps(out), flush=True)
        del rec, enc


def resample_rounds(a, codec, cs, shape):
    """--resample: the frame taken to 10 bits at the fixed step as 4:4:4 (the fit: ojphgpu_frame_fit), 4:2:2 and 4:2:0 (the
    resampling stage: ojphgpu_frame_resample), the three recoders taking turns in every round; per format the stage's time
    from the recoder's own device events (timing()["fit_ms"]), the bytes it moves -- 4 read per source sample, 2 written per
    output sample -- and what that makes per second.  One JSON line with every round and the medians."""
    nc, h, w = shape
    formats = [("444", [(1, 1)] * 3, None), ("422", [(1, 1), (2, 1), (2, 1)], "cosited"), ("420", [(1, 1), (2, 2), (2, 2)], "cosited")]
    recs, rounds, sizes = {}, {}, {}
    for name, ds, rs in formats:
        recs[name] = codec.Recoder(cs, resample=rs, reversible=False, qstep=OUT_QSTEP, bit_depth=10, color_transform=False, downsampling=ds)
        rounds[name] = dict(stage_ms=[], recode_ms=[])
    for i in range(a.warmup + a.runs):
        for name, _, _ in formats:
            t0 = time.perf_counter()
            out = recs[name].recode(cs)
            ms = (time.perf_counter() - t0) * 1e3
            sizes[name] = len(out)
            if i >= a.warmup:
                rounds[name]["stage_ms"].append(round(float(recs[name].timing()["fit_ms"]), 4))
                rounds[name]["recode_ms"].append(round(ms, 3))
    out = dict(frame="c3 %dx%dx%d 12-bit reversible, %d bytes" % (w, h, nc, len(cs)), target="10 bits, qstep %.3f" % OUT_QSTEP, runs=a.runs)
    for name, _, _ in formats:
        moved = 4 * nc * h * w + 2 * recs[name].plan.frame_elems
        st = rounds[name]["stage_ms"]
        med = float(np.median(st))
        out[name] = dict(stage="ojphgpu_frame_fit" if name == "444" else "ojphgpu_frame_resample", bytes_out=sizes[name], bytes_moved=moved,
                         stage_median_ms=round(med, 4), stage_spread=round((max(st) - min(st)) / med, 3), TB_per_s=round(moved / (med * 1e-3) / 1e12, 3),
                         share_of_hbm_peak=round(moved / (med * 1e-3) / HBM_PEAK, 3), recode_median_ms=round(float(np.median(rounds[name]["recode_ms"])), 3),
                         rounds=rounds[name])
    for name in ("422", "420"):
        out[name]["stage_over_fit"] = round(out[name]["stage_median_ms"] / out["444"]["stage_median_ms"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
