#!/usr/bin/env python3
"""Generates tests/golden/rate_sizes.json from the REAL reference's generic build (oracle/_ref/libojph_refgen.so).  Run where
the reference has been built only:

    python tests/golden/make_rate_golden.py [--no-survey]

Per case of tests/rate_cases.py: the codestream length at every one of the 241 steps of the rate grid, and for every budget
the index j* the grid certifies with the SHA-256 of the reference's codestreams at j* and j* + 1.  For the 8K frame of
tools/rate_bench.py (tests/synth.py survey_c3) only the lengths and digests at j* and j* + 1 of its three budgets, found
by bisection over reference encodes (--no-survey keeps the entry the file already has).
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import refbind                      # noqa: E402
from tests import rate_cases as rc              # noqa: E402
from tests.synth import survey_c3               # noqa: E402

OUT = os.path.join(HERE, "rate_sizes.json")


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def certified(sizes, budget):
    """the largest j with size(j) <= budget (the table is monotone: any certified index is this one)"""
    ok = [j for j in range(rc.GRID) if sizes[j] <= budget]
    return ok[-1] if ok else None


def main():
    refgen = refbind.Ref(generic=True)
    old = json.load(open(OUT)) if os.path.exists(OUT) else {}
    out = {"reference": "aous72/OpenJPH 0.31.0, generic build (oracle/_ref/libojph_refgen.so)", "cases": {}}
    for name in rc.CASES:
        img, size = rc.case_image(name)
        streams = {}

        def enc(j):
            if j not in streams:
                kw = rc.case_kwargs(name, rc.grid_qstep(j))
                streams[j] = refgen.encode(img, size=size if isinstance(img, list) else None, **kw)
            return streams[j]
        sizes = [len(enc(j)) for j in range(rc.GRID)]
        assert all(sizes[j] <= sizes[j + 1] for j in range(rc.GRID - 1)), "%s: the lengths are not monotone" % name
        inr, below, above = rc.budgets(name)
        assert below < sizes[0] and above > sizes[-1]
        assert all(sizes[0] < b < sizes[-1] for b in inr), (name, sizes[0], sizes[-1], inr)
        entry = {"sizes": sizes, "budgets": {}}
        for b in inr + [above]:
            j = certified(sizes, b)
            entry["budgets"][str(b)] = {"j": j, "sha256": sha(enc(j)), "sha256_finer": sha(enc(j + 1)) if j + 1 < rc.GRID else None}
        out["cases"][name] = entry
        print(name, "headers only", sizes[0], "finest", sizes[-1], {b: v["j"] for b, v in entry["budgets"].items()}, flush=True)
    if "--no-survey" in sys.argv:
        out["survey_c3"] = old.get("survey_c3", {})
    else:
        img = survey_c3()
        lens, digs = {}, {}

        def size(j):
            if j not in lens:
                cs = refgen.encode(img, 12, reversible=False, qstep=rc.grid_qstep(j))
                lens[j], digs[j] = len(cs), sha(cs)
                print("survey_c3 j", j, "bytes", lens[j], flush=True)
            return lens[j]
        sv = {}
        for bps in rc.SURVEY_BPS:
            b = int(img.size * bps)
            j, _ = rc.bisect_passes(size, b)
            size(j + 1)
            assert lens[j] <= b < lens[j + 1]
            sv[str(b)] = {"bps": bps, "j": j, "bytes": lens[j], "bytes_finer": lens[j + 1], "sha256": digs[j], "sha256_finer": digs[j + 1]}
        out["survey_c3"] = sv
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
