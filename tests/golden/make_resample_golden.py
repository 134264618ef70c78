#!/usr/bin/env python3
"""Generates tests/golden/recode_resample.json from the REAL reference's generic build (oracle/_ref/libojph_refgen.so) and
the oracle pipeline.  Run where the reference has been built only:

    python tests/golden/make_resample_golden.py

Per case of tests/resample_cases.py CASES: the SHA-256 and length of the reference's source codestream; the SHA-256 of G --
the REFERENCE's decode of the source, resampled and fitted in numpy (pipeline.resample_frame, pipeline.fit_frame: the
reference has no resampler, the numpy statement is the arbiter) --; and the SHA-256 and length of the REFERENCE's encode of G
with the output's parameters written out by hand.  The script asserts that the oracle pipeline agrees at every step: its
source, its G, and cpu_recode_resampled's output.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from openjph_amd.pipeline import fit_frame, resample_frame    # noqa: E402
from oracle import refbind                                    # noqa: E402
from tests import rate_cases as rc                            # noqa: E402
from tests import recode_cases as rcc                         # noqa: E402
from tests import resample_cases as rsc                       # noqa: E402

OUT = os.path.join(HERE, "recode_resample.json")


def main():
    refgen = refbind.Ref(generic=True)
    out = {"reference": "aous72/OpenJPH 0.31.0, generic build (oracle/_ref/libojph_refgen.so)", "cases": {}}
    for case, c in rsc.CASES.items():
        name = c["source"][0]
        img, size = rc.case_image(name)
        cs = refgen.encode(img, size=size if isinstance(img, list) else None, **rcc.src_kwargs(c["source"]))
        assert cs == rsc.source(case), (case, "the oracle pipeline does not write the reference's source")
        # G from the reference's decode, with the factors written out by hand: the source is 4:4:4 without an offset
        planes, _ = refgen.decode(cs, skip=(0, 0))
        ds = c["out"]["downsampling"]
        bs, bo = rc.CASES[name]["bd"], c["out"].get("bit_depth", rc.CASES[name]["bd"])
        nc = len(ds)
        G = fit_frame(resample_frame(list(planes), ds), [bs] * nc, [bo] * nc, [False] * nc)
        G_cpu, _, _ = rsc.cpu_fitted_resampled(cs, c["view"], c["out"])
        assert rcc.frame_digest(G) == rcc.frame_digest(G_cpu), (case, "the oracle pipeline's frame is not the reference's")
        kw = dict(rcc.src_kwargs(c["source"]))
        kw.update(c["out"])
        want = refgen.encode([q.astype("int32") for q in G], size=(rc.CASES[name]["w"], rc.CASES[name]["h"]), **kw)
        got = rsc.cpu_recode_resampled(cs, c["view"], c["out"])
        assert got == want, (case, "cpu_recode_resampled is not the reference's encode of the frame", len(got), len(want))
        out["cases"][case] = {"source": {"sha256": rcc.sha(cs), "len": len(cs)},
                              "frame": {"sha256": rcc.frame_digest(G), "shapes": [list(q.shape) for q in G]},
                              "output": {"sha256": rcc.sha(want), "len": len(want)}}
        print(case, len(cs), out["cases"][case]["frame"]["shapes"], len(want), flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
