"""The transcoder against what a caller has without it: the C3 8K frame (tests/synth.py survey_c3, 12-bit, coded at qstep
0.001) recoded to byte budgets of 0.2 and 0.05 bytes per sample and to a fixed step one octave coarser (0.002).  Per
target the contenders take turns, `--runs` rounds after `--warmup`, host clock from the call to a stream synchronise:

  transcoder        codec.Transcoder: submit (parse, upload of the block bytes, block decoder, with a budget the band
                    statistics) + finish (with a budget the search; coding, download, Tier-2); submit and finish are also
                    given apart, and the object's own timing() of the last round
  decode_encode     Decoder.run_device into a frame in HBM (16-bit containers), then Encoder(max_bytes=) / Encoder(qstep)
                    .run_device + finish on that frame -- the same build, the codestream resident in HBM from the decoder's
                    construction: neither parse nor upload is in its time
  upload_decode_encode   the same with Decoder.upload(codestream) in front: the host-to-device traffic the transcoder's submit
                    carries (still without the parse)
  new_decoder_encode     a Decoder made from the codestream in every round (parse, create, upload), then run_device and the
                    encoder as above: what a caller has for a SEQUENCE of codestreams -- a Decoder's block descriptors are
                    its first codestream's, so the two contenders above can only be handed the same bytes again, while the
                    transcoder parses whatever it is given
  parse             plan.parse_codestream alone, host only: the part of submit that is Tier-2 reading

The two paths do not write the same bytes (the second rounds and clamps to samples in between); the lengths are reported.
Prints one JSON line per target: medians, spread = (max - min) / median.
  python tools/transcode_bench.py [--runs 10] [--warmup 2] [--rows 4320]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SRC_QSTEP = 0.001
BPS = (0.2, 0.05)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=4320, help="top rows of the frame (rehearsals at a small size)")
    a = ap.parse_args()
    import torch
    from openjph_amd import codec
    from openjph_amd.plan import make_params, parse_codestream
    from tests import synth
    img = synth.survey_c3(rows=a.rows)
    nc, h, w = img.shape
    samples = img.size

    def params(qstep):
        return make_params(w, h, nc, bit_depth=12, reversible=False, qstep=qstep)
    cs = codec.Encoder(params(SRC_QSTEP)).encode(img.astype(np.uint16))
    del img

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    dec = codec.Decoder(cs)
    d_frame = torch.empty(dec.shape, dtype=torch.int16, device="cuda")
    targets = [("budget %.2f B/sample" % b, dict(max_bytes=int(samples * b))) for b in BPS] + [("qstep %.3f" % (2 * SRC_QSTEP), dict(qstep=2 * SRC_QSTEP))]
    for label, kw in targets:
        tr = codec.Transcoder(cs, **kw)
        enc = codec.Encoder(params(kw.get("qstep", SRC_QSTEP)), max_bytes=kw.get("max_bytes", 0))

        def decode_encode(upload):
            if upload:
                dec.upload(cs)
            dec.run_device(d_frame)
            enc.run_device(d_frame)
            return enc.finish()

        def new_decoder_encode():
            d = codec.Decoder(cs)
            d.run_device(d_frame)
            enc.run_device(d_frame)
            return enc.finish()
        t = {"transcoder": [], "submit": [], "finish": [], "decode_encode": [], "upload_decode_encode": [], "new_decoder_encode": [], "parse": []}
        for i in range(a.warmup + a.runs):
            ms_sub, _ = timed(lambda: tr.submit(cs))
            ms_fin, out_t = timed(tr.finish)
            ms_de, out_d = timed(lambda: decode_encode(False))
            ms_ude, _ = timed(lambda: decode_encode(True))
            ms_nde, _ = timed(new_decoder_encode)
            ms_parse, _ = timed(lambda: parse_codestream(cs))
            if i >= a.warmup:
                t["transcoder"].append(ms_sub + ms_fin); t["submit"].append(ms_sub); t["finish"].append(ms_fin)
                t["decode_encode"].append(ms_de); t["upload_decode_encode"].append(ms_ude)
                t["new_decoder_encode"].append(ms_nde); t["parse"].append(ms_parse)
        out = dict(frame="c3 %dx%dx%d 12-bit at qstep %g, %d bytes" % (w, h, nc, SRC_QSTEP, len(cs)), target=label, runs=a.runs,
                   bytes_transcoder=len(out_t), bytes_decode_encode=len(out_d))
        if "max_bytes" in kw:
            it, ie = tr.rate_info(), enc.rate_info()
            out.update(budget=kw["max_bytes"], grid_index_transcoder=it["grid_index"], passes_transcoder=it["passes"],
                       grid_index_decode_encode=ie["grid_index"], passes_decode_encode=ie["passes"])
        for k, v in t.items():
            med = float(np.median(v))
            out[k] = dict(median_ms=round(med, 3), spread=round((max(v) - min(v)) / med, 3))
        out["transcoder_timing_ms"] = {k: round(float(v), 3) for k, v in tr.timing().items()}
        dt = dec.timing()
        out["decoder_timing_ms"] = dict(ht_ms=round(dt["ht_ms"], 3), dwt_ms=round(dt["dwt_ms"], 3), total_ms=round(dt["total_ms"], 3))
        print(json.dumps(out), flush=True)
        del tr, enc


if __name__ == "__main__":
    main()
