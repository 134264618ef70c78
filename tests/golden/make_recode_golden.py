#!/usr/bin/env python3
"""Generates tests/golden/recode.json from the REAL reference's generic build (oracle/_ref/libojph_refgen.so) and the oracle
pipeline.  Run where the reference has been built only:

    python tests/golden/make_recode_golden.py

Per case of tests/recode_cases.py: the SHA-256 and length of the reference's source codestream; the SHA-256 of G -- the
REFERENCE's decode of the source at the view's resolution, cropped to the view's window and fitted in numpy
(recode_cases.frame_digest); and, where the output has a step of its own or is reversible, the SHA-256 and length of the
REFERENCE's encode of G with the output's parameters written out by hand (recode_cases.out_make_kwargs).  The script
asserts that the oracle pipeline agrees at every step: its source, its G, and cpu_recode's output.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import refbind                      # noqa: E402
from tests import rate_cases as rc              # noqa: E402
from tests import recode_cases as rcc           # noqa: E402

OUT = os.path.join(HERE, "recode.json")


def main():
    refgen = refbind.Ref(generic=True)
    out = {"reference": "aous72/OpenJPH 0.31.0, generic build (oracle/_ref/libojph_refgen.so)", "cases": {}}
    sources = {}

    def ref_decode(cs, skip):
        planes, _ = refgen.decode(cs, skip=skip or (0, 0))
        return list(planes)

    for case, c in rcc.CASES.items():
        src = c["source"]
        if src not in sources:
            img, size = rc.case_image(src[0])
            cs = refgen.encode(img, size=size if isinstance(img, list) else None, **rcc.src_kwargs(src))
            assert cs == rcc.cpu_source(src), (case, "the oracle pipeline does not write the reference's source")
            sources[src] = cs
        cs = sources[src]
        G, params, plan = rcc.cpu_fitted(cs, c["view"], c["out"], decode=ref_decode)
        G_cpu, _, _ = rcc.cpu_fitted(cs, c["view"], c["out"])
        assert rcc.frame_digest(G) == rcc.frame_digest(G_cpu), (case, "the oracle pipeline's fitted frame is not the reference's")
        entry = {"source": {"sha256": rcc.sha(cs), "len": len(cs)}, "frame": {"sha256": rcc.frame_digest(G), "shapes": [list(q.shape) for q in G]}}
        if c["ref"]:
            kw, size = rcc.out_make_kwargs(case)
            want = refgen.encode([q.astype("int32") for q in G], size=size, **kw)
            got = rcc.cpu_recode(cs, c["view"], c["out"])
            assert got == want, (case, "cpu_recode is not the reference's encode of the fitted frame", len(got), len(want))
            entry["output"] = {"sha256": rcc.sha(want), "len": len(want)}
        out["cases"][case] = entry
        print(case, entry["source"]["len"], entry["frame"]["shapes"], entry.get("output", {}).get("len"), flush=True)
    # rewrap: a reversible source through the sample domain is the direct encode of the original image
    img, _ = rc.case_image("D")
    direct = refgen.encode(img, **rcc.out_make_kwargs("rewrapD")[0])
    assert rcc.sha(direct) == out["cases"]["rewrapD"]["output"]["sha256"]
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
