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
  python tools/transcode_bench.py [--runs 10] [--warmup 2] [--rows 4320]

--pipe: a SEQUENCE of sources instead, host memory to host memory: `--frames` identical C3 codestreams per round at the same
three targets.  Per target three contenders take turns, `--rounds` rounds after one that warms every contender up:
  pipe              pipeline.TranscoderPipe, depth 4: every slot's pinned source filled once, then acquire / submit / collect
                    (copy=False) in steady state, as tools/e2e_pipeline.py drives the other two pipes
  transcoder        codec.Transcoder.transcode called codestream by codestream on the bytes object (pageable memory in, a
                    bytes object out): the same build's single call
  dec_enc_pipes     a DecoderPipe (16-bit containers, slots filled once) feeding an EncoderPipe with the target's step or
                    budget: the sample-domain route a caller has today; the frame goes from the decoder's pinned output into
                    the encoder's pinned input by one host copy, which is part of the route
Prints one JSON line per target: per contender the frames/s of every round, their median and spread (max - min) / median, and
whether the pipe's median exceeds the single transcoder's by more than the larger of the two round-to-round spreads.
  python tools/transcode_bench.py --pipe [--rounds 3] [--frames 24] [--rows 4320]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SRC_QSTEP = 0.001
BPS = (0.2, 0.05)


def run_tc_pipe(cs, n, kw, depth=4):
    """every slot filled once, then n sources in steady state -> (seconds, the output, mean passes or None, stats)"""
    from openjph_amd.pipeline import TranscoderPipe
    pipe = TranscoderPipe(cs, depth=depth, **kw)
    src = np.frombuffer(cs, dtype=np.uint8)
    for _ in range(depth):
        pipe.acquire(len(cs))[:] = src
        pipe.submit()
    first = None
    while pipe.in_flight:
        c = pipe.collect()
        first = c if first is None else first
    t0 = time.perf_counter()
    sub = col = nbytes = passes = 0
    while col < n:
        while sub < n and pipe.acquire(len(cs)) is not None:
            pipe.submit(); sub += 1
        nbytes += len(pipe.collect(copy=False)); col += 1
        if "max_bytes" in kw:
            passes += pipe.rate_info()["passes"]
    dt = time.perf_counter() - t0
    st = pipe.stats()
    pipe.close()
    assert nbytes == n * len(first)
    return dt, first, (passes / n if "max_bytes" in kw else None), st


def run_dec_enc_pipes(cs, n, params, max_bytes, depth=4):
    """a DecoderPipe feeding an EncoderPipe, n frames in steady state -> (seconds, the output)"""
    from openjph_amd.pipeline import DecoderPipe, EncoderPipe
    from openjph_amd.plan import Plan
    dec = DecoderPipe(cs, depth=depth, container=16)
    enc = EncoderPipe(plan=Plan(params), depth=depth, container=16, max_bytes=max_bytes or None)
    src = np.frombuffer(cs, dtype=np.uint8)
    out = [None]

    def run(count, refill):
        dsub = dcol = ecol = 0
        while dcol < count:
            while dsub < count:
                buf = dec.acquire(len(cs))
                if buf is None:
                    break
                if refill:
                    buf[:] = src
                dec.submit(); dsub += 1
            frame = dec.collect(copy=False); dcol += 1
            buf = enc.acquire()
            while buf is None:
                out[0] = enc.collect(copy=False); ecol += 1
                buf = enc.acquire()
            np.copyto(buf, frame.reshape(buf.shape))
            enc.submit()
        while enc.in_flight:
            out[0] = enc.collect(copy=True); ecol += 1
        assert ecol == count
    run(depth, True)
    t0 = time.perf_counter()
    run(n, False)
    dt = time.perf_counter() - t0
    dec.close(); enc.close()
    return dt, out[0]


def pipe_bench(a):
    from openjph_amd import codec
    from openjph_amd.plan import make_params
    from tests import synth
    img = synth.survey_c3(rows=a.rows)
    nc, h, w = img.shape
    samples = img.size

    def params(qstep):
        return make_params(w, h, nc, bit_depth=12, reversible=False, qstep=qstep)
    cs = codec.Encoder(params(SRC_QSTEP)).encode(img.astype(np.uint16))
    del img
    targets = [("budget %.2f B/sample" % b, dict(max_bytes=int(samples * b))) for b in BPS] + [("qstep %.3f" % (2 * SRC_QSTEP), dict(qstep=2 * SRC_QSTEP))]
    for label, kw in targets:
        single = codec.Transcoder(cs, **kw)
        fps = {"pipe": [], "transcoder": [], "dec_enc_pipes": []}
        passes = st = out_de = None
        for r in range(a.rounds + 1):                           # round 0 warms every contender up and is not counted
            dt_pipe, out_pipe, passes, st = run_tc_pipe(cs, a.frames, kw)
            t0 = time.perf_counter()
            for _ in range(a.frames):
                out_single = single.transcode(cs)
            dt_single = time.perf_counter() - t0
            assert out_single == out_pipe
            dt_de, out_de = run_dec_enc_pipes(cs, a.frames, params(kw.get("qstep", SRC_QSTEP)), kw.get("max_bytes", 0))
            if r:
                fps["pipe"].append(a.frames / dt_pipe); fps["transcoder"].append(a.frames / dt_single); fps["dec_enc_pipes"].append(a.frames / dt_de)
        out = dict(frame="c3 %dx%dx%d 12-bit at qstep %g, %d bytes, host memory" % (w, h, nc, SRC_QSTEP, len(cs)), target=label, depth=4,
                   frames_per_round=a.frames, bytes_pipe=len(out_pipe), bytes_dec_enc_pipes=len(out_de), mean_passes=passes,
                   pipe_host_parse_ms=round(st["host_parse_ms"], 3), pipe_host_tier2_ms=round(st["host_tier2_ms"], 3),
                   pipe_latency_ms=round(st["latency_ms"], 3))
        if "max_bytes" in kw:
            out.update(budget=kw["max_bytes"], grid_index=single.rate_info()["grid_index"], single_passes=single.rate_info()["passes"])
        for k, v in fps.items():
            med = float(np.median(v))
            out[k] = dict(fps=[round(x, 1) for x in v], median_fps=round(med, 1), ms_per_frame=round(1e3 / med, 3),
                          spread=round((max(v) - min(v)) / med, 3))
        gap = float(np.median(fps["pipe"])) - float(np.median(fps["transcoder"]))
        need = max(max(fps[k]) - min(fps[k]) for k in ("pipe", "transcoder"))
        out["pipe_minus_transcoder_fps"] = round(gap, 1)
        out["larger_spread_fps"] = round(need, 1)
        out["margin_met"] = bool(gap > need)
        print(json.dumps(out), flush=True)
        del single


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=4320, help="top rows of the frame (rehearsals at a small size)")
    ap.add_argument("--pipe", action="store_true", help="a sequence: the transcode pipe against the single transcoder and a DecoderPipe feeding an EncoderPipe")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=24)
    a = ap.parse_args()
    if a.pipe:
        return pipe_bench(a)
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
