#!/usr/bin/env python3
"""Generates tests/golden/quality_sse.json from the REAL reference's generic build (oracle/_ref/libojph_refgen.so).  Run where
the reference has been built only, on the CPU:

    python tests/golden/make_quality_golden.py

Per case of tests/rate_cases.py: the squared error and the peak absolute error, per component, between the frame and the
reference's decode of the reference's encode at every one of the 241 steps of the rate grid; and for every target of
tests/quality_cases.py the max_sse the formula gives, the set of indices that carry the certificate (SSE(j) <= T and j == 0
or SSE(j - 1) > T) -- which this script asserts to have exactly one member -- and the SHA-256 of the reference's codestream
there.
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
from tests import quality_cases as qc           # noqa: E402
from tests import rate_cases as rc              # noqa: E402

OUT = os.path.join(HERE, "quality_sse.json")


def main():
    refgen = refbind.Ref(generic=True)
    out = {"reference": "aous72/OpenJPH 0.31.0, generic build (oracle/_ref/libojph_refgen.so)", "cases": {}}
    for name in rc.CASES:
        img, size = rc.case_image(name)
        planes = img if isinstance(img, list) else [img[c] for c in range(img.shape[0])]
        digests, sse, pae = [], [], []
        for j in range(rc.GRID):
            cs = refgen.encode(img, size=size if isinstance(img, list) else None, **rc.case_kwargs(name, rc.grid_qstep(j)))
            dec, _ = refgen.decode(cs)
            s, p = qc.frame_error(planes, dec if isinstance(dec, list) else [dec[c] for c in range(len(planes))])
            digests.append(hashlib.sha256(cs).hexdigest()); sse.append(s); pae.append(p)
        total = [sum(s) for s in sse]
        entry = {"sse": sse, "pae": pae, "targets": {}}
        for db in qc.TARGETS_DB:
            T = qc.psnr_to_sse(name, db)
            cert = qc.certified(total, T)
            assert len(cert) == 1, (name, db, T, cert)
            entry["targets"][str(db)] = {"max_sse": T, "certified": cert, "sha256": digests[cert[0]]}
        out["cases"][name] = entry
        rises = [j for j in range(1, rc.GRID) if total[j] > total[j - 1]]
        zero = [j for j in range(rc.GRID) if total[j] == 0]
        print(name, "SSE(0)", total[0], "SSE(240)", total[-1], "first zero", zero[0] if zero else None, "rises at", rises,
              {db: (v["certified"][0], v["max_sse"]) for db, v in entry["targets"].items()}, flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
